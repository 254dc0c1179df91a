// SmokePhysNet.input_encoder + pooling as ONE fused kernel per precision (gfx950).
//
// Reference: /root/reference/src/models/smokephys_net.py:24-32 (Conv7x7 1->64, BN, ReLU, Conv3x3 64->128, BN, ReLU,
// AdaptiveAvgPool2d(input_dim)) and :90-91 (adaptive_avg_pool2d -> 32x32).  Eval-mode BN is folded to a per-channel
// scale/shift; for H a multiple of 32 and input_dim a multiple/divisor of H the two adaptive pools compose to an
// (H/32)^2 block mean.
//
// Nothing but the frame is read from HBM and nothing but the pooled features is written: the conv1 activations of a
// tile (+1 halo) live only in LDS, conv2 is an implicit GEMM  D[pixel][o] = sum_k A[pixel][k] B[k][o]  with
// k = (tap, channel) whose A fragments are shifted reads of that LDS tile (no im2col), BN2 + ReLU + the block-mean pool
// run in the epilogue.  One kernel per arithmetic (SMK_BF16X3, the default, runs k_encoder_b16):
//   k_encoder_f32   tile 8x32, 512 threads; conv1 on VALU, conv2 on v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chain),
//                   weights [tap][c][o] double-buffered through LDS.
//   k_encoder_bf16  persistent, tile 8x16, 256 threads; both convs on v_mfma_f32_32x32x16_bf16; X3 = split-bf16
//                   (hi*hi + hi*lo + lo*hi: fp32-class accuracy), weights as register fragments straight from L2.
//   k_encoder_b16   the headline kernel: split-bf16 as k_encoder_bf16<X3>, conv2 on v_mfma_f32_16x16x32_bf16 (same cycles per
//                   flop, higher sustained clock under the power limit), XOR-swizzled a1 image, one-xor fragment addressing,
//                   product-major MFMA emission, pinned read / ring-load placement (-22 % time vs k_encoder_bf16<X3>).
//   k_encoder_i8    same structure as k_encoder_bf16; conv2 on v_mfma_i32_32x32x32_i8 with 16-bit fixed-point operands as two
//                   int8 limbs.
// The three persistent kernels (bf16, b16, i8) share one scaffold, written once ahead of them: conv1 staging, the work-list walk
// (TileWalk), the x halo fetch (TileSrc), conv1's MFMA units and the pooled store of the 32x32 layout; one launcher template
// (launch_persistent) launches all three.  Also here: weight folding (k_fold_weights, k_quant_w2), the conv1 parity hook and the
// tile skip (k_encoder_tile_scan, skip_prepare).  The convolutions under autograd are in encoder_train.hip.
#include "encoder.h"

#include <stdlib.h>

#include "encoder_tile.h"
#include "encoder_cells.h"

namespace smk {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int ENC_TH = 8, ENC_TW = 32;          // output tile
constexpr int ENC_AH = ENC_TH + 2, ENC_AW = ENC_TW + 2;   // a1 halo tile (conv2 3x3)
constexpr int ENC_XH = ENC_TH + 8, ENC_XW = ENC_TW + 8;   // x halo tile (+ conv1 7x7)
constexpr int ENC_ACS = ENC_AH * ENC_AW;        // a1 channel stride in LDS (floats)

// ---------------------------------------------------------------- weight folding / re-layout
// s = bn_w / sqrt(var + eps), t = (conv_b - mean) * s + bn_b       (BN eval, eps = 1e-5)
__global__ void k_fold_weights(smk_encoder_weights w, EncoderDev e) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 64) {
        float s = w.bn1_w[t] / sqrtf(w.bn1_var[t] + 1e-5f);
        e.s1[t] = s;
        e.t1[t] = (w.conv1_b[t] - w.bn1_mean[t]) * s + w.bn1_b[t];
    }
    if (t < 128) {
        float s = w.bn2_w[t] / sqrtf(w.bn2_var[t] + 1e-5f);
        e.s2[t] = s;
        e.t2[t] = (w.conv2_b[t] - w.bn2_mean[t]) * s + w.bn2_b[t];
    }
    if (t < 64 * 49) e.w1[t] = w.conv1_w[t];                       // [c][49]
    if (t < 9 * 64 * 128) {                                         // conv2_w [o][c][3][3] -> w2t [tap][c][o]
        int o = t % 128, c = (t / 128) % 64, tap = t / (128 * 64);
        e.w2t[t] = w.conv2_w[((size_t)o * 64 + c) * 9 + tap];
    }
    __bf16 *w1p = reinterpret_cast<__bf16 *>(e.w1p), *w2q = reinterpret_cast<__bf16 *>(e.w2q);
    if (t < 64 * 64) {                                              // w1p [hi|lo][c][k = 8*ki + kj] (ki = 7, kj = 7: zero)
        int c = t / 64, k = t % 64, ki = k >> 3, kj = k & 7;
        float v = (ki < 7 && kj < 7) ? w.conv1_w[c * 49 + ki * 7 + kj] : 0.f;
        __bf16 hi = (__bf16)v;
        w1p[t] = hi;
        w1p[64 * 64 + t] = (__bf16)(v - (float)hi);
    }
    if (t < 36 * 128 * 16) {                                        // w2q [k-step = tap*4 + c/16][hi|lo][o][16 c]
        int cc = t % 16, o = (t / 16) % 128, ks = t / (16 * 128);
        int tap = ks >> 2, c = (ks & 3) * 16 + cc;
        float v = w.conv2_w[((size_t)o * 64 + c) * 9 + tap];
        __bf16 hi = (__bf16)v;
        w2q[((size_t)(ks * 2 + 0) * 128 + o) * 16 + cc] = hi;
        w2q[((size_t)(ks * 2 + 1) * 128 + o) * 16 + cc] = (__bf16)(v - (float)hi);
        // the same weights for the 16x16x32 shape: [k-step = tap*2 + c/32][hi|lo][o][32 c]
        __bf16 *w2s = reinterpret_cast<__bf16 *>(e.w2s);
        const int ks2 = tap * 2 + (c >> 5), c32 = c & 31;
        w2s[((size_t)(ks2 * 2 + 0) * 128 + o) * 32 + c32] = hi;
        w2s[((size_t)(ks2 * 2 + 1) * 128 + o) * 32 + c32] = (__bf16)(v - (float)hi);
    }
}

// conv2 weights as two balanced int8 limbs per output channel: w ~= sw2[o] * (256*h + l), |256h + l| <= 32512.
__global__ __launch_bounds__(256) void k_quant_w2(smk_encoder_weights w, EncoderDev e) {
    __shared__ float red[256];
    __shared__ int sh_h, sh_l;
    const int o = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { sh_h = 0; sh_l = 0; }
    float m = 0.f;
    for (int k = tid; k < 576; k += 256) m = fmaxf(m, fabsf(w.conv2_w[(size_t)o * 576 + k]));
    red[tid] = m;
    __syncthreads();
    for (int sft = 128; sft > 0; sft >>= 1) {
        if (tid < sft) red[tid] = fmaxf(red[tid], red[tid + sft]);
        __syncthreads();
    }
    const float wmax = red[0];
    const float sw = wmax > 0.f ? wmax / 32512.0f : 1.0f;
    if (tid == 0) e.sw2[o] = sw;
    int sum_h = 0, sum_l = 0;
    for (int k = tid; k < 576; k += 256) {
        const int c = k / 9, tap = k - 9 * c;                      // conv2_w [o][c][3][3]
        const int q = (int)rintf(w.conv2_w[(size_t)o * 576 + k] / sw);
        const int h = (q + 128) >> 8, l = q - (h << 8);              // arithmetic shift = floor: l in [-128, 127]
        const int ks = tap * 2 + (c >> 5), cc = c & 31;
        e.w2i[((size_t)(ks * 2 + 0) * 128 + o) * 32 + cc] = (signed char)h;
        e.w2i[((size_t)(ks * 2 + 1) * 128 + o) * 32 + cc] = (signed char)l;
        sum_h += h; sum_l += l;
    }
    atomicAdd(&sh_h, sum_h);
    atomicAdd(&sh_l, sum_l);
    __syncthreads();
    if (tid == 0) { e.wsum[o] = 128 * sh_h; e.wsum[128 + o] = 128 * sh_l; }
}

hipError_t launch_fold_weights(const smk_encoder_weights &w, const EncoderDev &e, hipStream_t st) {
    hipLaunchKernelGGL(k_quant_w2, dim3(128), dim3(256), 0, st, w, e);
    int n = 9 * 64 * 128;    // largest of the index spaces above
    hipLaunchKernelGGL(k_fold_weights, dim3((n + 255) / 256), dim3(256), 0, st, w, e);
    return hipGetLastError();
}

// conv1 + BN + ReLU for one pixel and NC consecutive channels starting at c0 (wave-uniform), from a 7x7 patch in regs.
template <int NC>
__device__ __forceinline__ void conv1_pixel(const float (&patch)[49], const float *__restrict__ w1,
                                            const float *__restrict__ s1, const float *__restrict__ t1, int c0,
                                            float (&out)[NC]) {
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
        const float *wc = w1 + (c0 + cc) * 49;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 49; ++t) acc = fmaf(patch[t], wc[t], acc);
        float y = fmaf(acc, s1[c0 + cc], t1[c0 + cc]);
        out[cc] = y > 0.f ? y : 0.f;
    }
}

// ---------------------------------------------------------------- parity hook: conv1 activations to HBM
__global__ __launch_bounds__(256) void k_conv1_only(const float *frames, int64_t fstride, int H, int W, EncoderDev e, float *act) {
    int b = blockIdx.z;
    int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (i >= H || j >= W) return;
    const float *x = frames + (size_t)b * fstride;
    float patch[49];
#pragma unroll
    for (int ki = 0; ki < 7; ++ki)
#pragma unroll
        for (int kj = 0; kj < 7; ++kj) {
            int ii = i + ki - 3, jj = j + kj - 3;
            patch[ki * 7 + kj] = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? x[(size_t)ii * W + jj] : 0.f;
        }
#pragma unroll 1
    for (int c0 = 0; c0 < 64; c0 += 4) {                      // 4 channels at a time: 49-tap patch + 4 sums stay in registers
        float o[4];
        conv1_pixel<4>(patch, e.w1, e.s1, e.t1, c0, o);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) act[(((size_t)b * 64 + c0 + cc) * H + i) * W + j] = o[cc];
    }
}

hipError_t launch_conv1_only(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e, float *act,
                             hipStream_t st) {
    dim3 grid(cdiv(W, 64), cdiv(H, 4), B), block(64, 4);
    hipLaunchKernelGGL(k_conv1_only, grid, block, 0, st, frames, fstride, H, W, e, act);
    return hipGetLastError();
}

// ---------------------------------------------------------------- frames beyond 256^2: per-tile partial sums, pooled by a second kernel
// The epilogues pool inside one 8 x 16 tile, which holds whole cells up to PS = H/32 = 8.  At 512^2 (PS = 16) a pooled cell spans
// 2 x 1 tiles, at 1024^2 (PS = 32) 4 x 2.  There every main kernel (instantiated once as PS = 16: a tile's sum does not depend on the
// cell size) writes, per tile and channel, the un-normalised fp32 sum of the tile's 128 bn_relu values into the handle's partial
// buffer [B][H/8][W/16][128] -- a tile is 512 contiguous bytes, whichever output layout the call asked for -- and
// k_encoder_pool_partials, launched behind it on the same stream, adds a cell's partials in ascending (tile row, tile column) order,
// multiplies by 1/PS^2 once and stores the feature in the call's layout.  No atomics: two addends commute exactly, the eight of a
// 1024^2 cell do not, and both layouts as well as skip-on and skip-off must stay bit-equal.  The pooling kernel does not know which
// tiles ran: on the skip path skip_fill copies an empty tile's 128 partials from the zero-response table (the same kernel form's
// partials of one all-zero frame) into the buffer, so skipping is invisible by construction.
constexpr int POOL_THREADS = 256;

// One thread per (cell, V channels): token-major stores are contiguous over channels (V = 4 when `features` is 16-byte aligned).
template <int V>
__global__ __launch_bounds__(POOL_THREADS) void k_encoder_pool_partials_tokens(const float *__restrict__ partials, float *__restrict__ features,
                                                                               int ncells, int lg_tr, int lg_tc, float inv) {
    typedef float vec_t __attribute__((ext_vector_type(V)));
    constexpr int PER = 128 / V;
    const int idx = blockIdx.x * POOL_THREADS + threadIdx.x, cell = idx / PER, o = (idx - cell * PER) * V;
    if (cell >= ncells) return;
    const int b = cell >> 10, pi = (cell >> 5) & 31, pj = cell & 31, tiles_x = 32 << lg_tc;
    const float *p = partials + (((size_t)b * (32 << lg_tr) + ((size_t)pi << lg_tr)) * tiles_x + (pj << lg_tc)) * 128 + o;
    vec_t sum = *reinterpret_cast<const vec_t *>(p);
    for (int tr = 0; tr < (1 << lg_tr); ++tr)
        for (int tc = (tr == 0); tc < (1 << lg_tc); ++tc) sum += *reinterpret_cast<const vec_t *>(p + ((size_t)tr * tiles_x + tc) * 128);
    *reinterpret_cast<vec_t *>(features + (size_t)cell * 128 + o) = sum * inv;
}

// NCHW: one workgroup per cell row (b, pi): the same sums, one thread per (cell, 4 channels) with 16-byte loads, turned through LDS
// so that a channel's 32 cells go out as one 128-byte row.
__global__ __launch_bounds__(POOL_THREADS) void k_encoder_pool_partials(const float *__restrict__ partials, float *__restrict__ features,
                                                                        int lg_tr, int lg_tc, float inv) {
    __shared__ float cells[32][129];
    const int tid = threadIdx.x, b = blockIdx.x >> 5, pi = blockIdx.x & 31, tiles_x = 32 << lg_tc;
    const float *row = partials + ((size_t)b * (32 << lg_tr) + ((size_t)pi << lg_tr)) * tiles_x * 128;
    for (int i = tid; i < 32 * 32; i += POOL_THREADS) {
        const int pj = i >> 5, o = (i & 31) * 4;
        const float *p = row + (size_t)(pj << lg_tc) * 128 + o;
        float4 sum = *reinterpret_cast<const float4 *>(p);
        for (int tr = 0; tr < (1 << lg_tr); ++tr)
            for (int tc = (tr == 0); tc < (1 << lg_tc); ++tc) {
                const float4 v = *reinterpret_cast<const float4 *>(p + ((size_t)tr * tiles_x + tc) * 128);
                sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
            }
        cells[pj][o] = sum.x * inv; cells[pj][o + 1] = sum.y * inv; cells[pj][o + 2] = sum.z * inv; cells[pj][o + 3] = sum.w * inv;
    }
    __syncthreads();
    for (int i = tid; i < 128 * 32; i += POOL_THREADS) {
        const int o = i >> 5, pj = i & 31;
        features[((size_t)b * 128 + o) * 1024 + pi * 32 + pj] = cells[pj][o];
    }
}

// features [B][128][32][32] or [B][1024][128] from the partials of B frames of H x H, H = 512 or 1024
static hipError_t launch_pool_partials(const float *partials, float *features, int B, int H, bool tokens, hipStream_t st) {
    const int PS = H / 32, lg_tr = PS == 16 ? 1 : 2, lg_tc = lg_tr - 1;       // a cell is PS/8 x PS/16 tiles
    const float inv = 1.0f / (float)(PS * PS);
    if (!tokens) {
        hipLaunchKernelGGL(k_encoder_pool_partials, dim3(B * 32), dim3(POOL_THREADS), 0, st, partials, features, lg_tr, lg_tc, inv);
    } else if ((reinterpret_cast<uintptr_t>(features) & 15) == 0) {
        hipLaunchKernelGGL(k_encoder_pool_partials_tokens<4>, dim3(B * 1024 * 32 / POOL_THREADS), dim3(POOL_THREADS), 0, st, partials,
                           features, B * 1024, lg_tr, lg_tc, inv);
    } else {
        hipLaunchKernelGGL(k_encoder_pool_partials_tokens<1>, dim3(B * 1024 * 128 / POOL_THREADS), dim3(POOL_THREADS), 0, st, partials,
                           features, B * 1024, lg_tr, lg_tc, inv);
    }
    return hipGetLastError();
}

void EncoderPartials::release() {
    if (buf) (void)hipFree(buf);
    for (void *p : retired) (void)hipFree(p);
    retired.clear();
    buf = nullptr;
    floats = 0;
}

hipError_t EncoderPartials::acquire(int B, int H, int W, hipStream_t st, float **out) {
    *out = nullptr;
    if (H / 32 < 16) return hipSuccess;
    const size_t need = (size_t)B * (H / B3_TH) * (W / B3_TW) * 128;
    std::lock_guard<std::mutex> lk(mu);
    if (floats < need) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
        if (cs != hipStreamCaptureStatusNone) return hipErrorStreamCaptureUnsupported;
        float *p = nullptr;
        const hipError_t err = hipMalloc((void **)&p, need * sizeof(float));
        if (err != hipSuccess) return err;
        if (buf) retired.push_back(buf);
        buf = p;
        floats = need;
    }
    *out = buf;
    return hipSuccess;
}

// ---------------------------------------------------------------- fused encoder, fp32 MFMA
// LDS carve (floats): xs [16][40] | a1s [64][10][34] | w2s 2 x [64][128]  (= 2560 + 87040 + 65536 B = 155,136 B)
// The epilogue reuses the a1s/w2s region as a2s [256 pixels][128+1 channels... see below].
constexpr int LDS_XS = ENC_XH * ENC_XW;                  // 640
constexpr int LDS_A1 = 64 * ENC_ACS;                     // 21760
constexpr int LDS_W2 = 64 * 128;                         // 8192 per buffer
constexpr int LDS_F32_TOTAL = LDS_XS + LDS_A1 + 2 * LDS_W2;
constexpr int A2_PITCH = 129;                            // a2s [pixel][o], +1 pad

template <int PS>
__global__ __launch_bounds__(512) void k_encoder_f32(const float *__restrict__ frames, int64_t fstride, int H, int W,
                                                     EncoderDev e, float *__restrict__ features) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *xs = lds, *a1s = lds + LDS_XS, *w2s = lds + LDS_XS + LDS_A1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z, r0 = blockIdx.y * ENC_TH, c0 = blockIdx.x * ENC_TW;
    const float *x = frames + (size_t)b * fstride;

    // ---- stage the x halo tile (zero outside the image = conv1's padding)
    for (int k = tid; k < LDS_XS; k += 512) {
        int ii = r0 - 4 + k / ENC_XW, jj = c0 - 4 + k % ENC_XW;
        xs[k] = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? x[(size_t)ii * W + jj] : 0.f;
    }
    // prefetch tap-0 weights into registers (4 x float4 per thread = 32 KB per workgroup)
    float4 wreg[4];
    {
        const float4 *src = reinterpret_cast<const float4 *>(e.w2t);
#pragma unroll
        for (int q = 0; q < 4; ++q) wreg[q] = src[q * 512 + tid];
    }
    __syncthreads();

    // ---- conv1 + BN + ReLU into a1s: 6 pixel chunks of 64 x 8 channel eighths = 48 wave tasks over 8 waves
    for (int task = wave; task < 48; task += 8) {
        const int chunk = task % 6, cq = task / 6;            // wave-uniform
        const int pix = chunk * 64 + lane;
        if (pix < ENC_ACS) {
            const int ar = pix / ENC_AW, ac = pix % ENC_AW;     // a1 halo coords; image coords (r0-1+ar, c0-1+ac)
            const int ii = r0 - 1 + ar, jj = c0 - 1 + ac;
            float o[8];
            if (ii >= 0 && ii < H && jj >= 0 && jj < W) {
                float patch[49];
#pragma unroll
                for (int ki = 0; ki < 7; ++ki)
#pragma unroll
                    for (int kj = 0; kj < 7; ++kj) patch[ki * 7 + kj] = xs[(ar + ki) * ENC_XW + ac + kj];
                conv1_pixel<8>(patch, e.w1, e.s1, e.t1, cq * 8, o);
            } else {
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) o[cc] = 0.f;       // conv2's zero padding
            }
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) a1s[(cq * 8 + cc) * ENC_ACS + pix] = o[cc];
        }
    }
    // tap-0 weights -> LDS buffer 0
    {
        float4 *dst = reinterpret_cast<float4 *>(w2s);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q * 512 + tid] = wreg[q];
    }
    __syncthreads();

    // ---- conv2 implicit GEMM: wave -> tile row `wave`, 32 pixels x 128 channels = 4 accumulators of 32x32
    f32x16 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    const int l31 = lane & 31, hi = lane >> 5;
    for (int tap = 0; tap < 9; ++tap) {
        if (tap + 1 < 9) {
            const float4 *src = reinterpret_cast<const float4 *>(e.w2t + (size_t)(tap + 1) * LDS_W2);
#pragma unroll
            for (int q = 0; q < 4; ++q) wreg[q] = src[q * 512 + tid];
        }
        const int ki = tap / 3, kj = tap % 3;
        const float *ap = a1s + hi * ENC_ACS + (wave + ki) * ENC_AW + l31 + kj;
        const float *bp = w2s + (tap & 1) * LDS_W2 + hi * 128 + l31;
#pragma unroll 4
        for (int cp = 0; cp < 32; ++cp) {
            float a = ap[cp * 2 * ENC_ACS];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                float bv = bp[cp * 2 * 128 + n * 32];
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[n], 0, 0, 0);
            }
        }
        if (tap + 1 < 9) {
            float4 *dst = reinterpret_cast<float4 *>(w2s + ((tap + 1) & 1) * LDS_W2);
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q * 512 + tid] = wreg[q];
        }
        __syncthreads();
    }

    // ---- epilogue: BN2 + ReLU, stage a2 [pixel][o] in LDS (a1s/w2s are dead), block-mean pool, store
    float *a2s = lds;                                        // 256 x 129 floats = 132,096 B
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int o = n * 32 + l31;
        const float s = e.s2[o], t = e.t2[o];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = (r & 3) + 8 * (r >> 2) + 4 * hi;   // C/D map of 32x32 MFMA: row = pixel
            float y = fmaf(acc[n][r], s, t);
            a2s[(wave * ENC_TW + col) * A2_PITCH + o] = y > 0.f ? y : 0.f;
        }
    }
    __syncthreads();
    if constexpr (PS >= 16) {
        // frames beyond 256^2 (see below): `features` is the partial buffer [B][H/8][W/16][128]; this 8 x 32 tile is two of its
        // 8 x 16 tiles, each the plain sum of its 128 activations, rows then columns
        if (tid < 256) {
            const int o = tid & 127, half = tid >> 7;
            float sum = 0.f;
            for (int rr = 0; rr < ENC_TH; ++rr)
                for (int q = 0; q < B3_TW; ++q) sum += a2s[(rr * ENC_TW + half * B3_TW + q) * A2_PITCH + o];
            const size_t tile = ((size_t)b * (H / B3_TH) + blockIdx.y) * (W / B3_TW) + 2 * blockIdx.x + half;
            features[tile * 128 + o] = sum;
        }
    } else {
        constexpr int CELLS_R = ENC_TH / PS, CELLS_C = ENC_TW / PS;   // pooled cells in this tile
        const int OW = 32, OHW = 32 * 32;
        for (int k = tid; k < CELLS_R * CELLS_C * 128; k += 512) {
            const int o = k & 127, cell = k >> 7, cr = cell / CELLS_C, cc = cell % CELLS_C;
            float sum = 0.f;
            for (int rr = 0; rr < PS; ++rr)
                for (int q = 0; q < PS; ++q) sum += a2s[((cr * PS + rr) * ENC_TW + cc * PS + q) * A2_PITCH + o];
            const int pi = r0 / PS + cr, pj = c0 / PS + cc;
            features[((size_t)b * 128 + o) * OHW + pi * OW + pj] = sum * (1.0f / (PS * PS));
        }
    }
}

hipError_t launch_encoder_f32(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e,
                              float *features, hipStream_t st, float *partials) {
    const int PS = H / 32;
    if (PS >= 16 && !partials) return hipErrorInvalidValue;
    dim3 grid(W / ENC_TW, H / ENC_TH, B), block(512);
    size_t lds_bytes = sizeof(float) * (size_t)(LDS_F32_TOTAL > 256 * A2_PITCH ? LDS_F32_TOTAL : 256 * A2_PITCH);
    once_per_device((const void *)k_encoder_f32<8>, [&] {
        (void)hipFuncSetAttribute((const void *)k_encoder_f32<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        (void)hipFuncSetAttribute((const void *)k_encoder_f32<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        (void)hipFuncSetAttribute((const void *)k_encoder_f32<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        (void)hipFuncSetAttribute((const void *)k_encoder_f32<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    });
    switch (PS) {
        case 2: hipLaunchKernelGGL(k_encoder_f32<2>, grid, block, lds_bytes, st, frames, fstride, H, W, e, features); break;
        case 4: hipLaunchKernelGGL(k_encoder_f32<4>, grid, block, lds_bytes, st, frames, fstride, H, W, e, features); break;
        case 8: hipLaunchKernelGGL(k_encoder_f32<8>, grid, block, lds_bytes, st, frames, fstride, H, W, e, features); break;
        case 16:
        case 32: {                                            // per-tile partials, then the pooling kernel
            hipLaunchKernelGGL(k_encoder_f32<16>, grid, block, lds_bytes, st, frames, fstride, H, W, e, partials);
            const hipError_t err = hipGetLastError();
            return err != hipSuccess ? err : launch_pool_partials(partials, features, B, H, false, st);
        }
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------- fused encoder, bf16 MFMA (single-pass or split "x3")
// Both convolutions on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; output tile 8 rows x 16 cols x 128 channels per
// 256-thread workgroup (4 waves, wave = one 32-channel block).  LDS 54 KB (x3) / 28 KB: >= 2 workgroups per CU, so the
// VALU/LDS-heavy conv1 phase of one tile overlaps the MFMA-bound conv2 loop of another.
//   x3: every operand is split v = hi + lo (two bf16) and a product is hi*hi + hi*lo + lo*hi (lo*lo ~ 2^-18 dropped):
//       fp32-class accuracy (features within 1e-4 of the fp32 reference) at 3 bf16 MFMAs per fp32 MFMA-equivalent.
// conv1: D[ch][pix] = W1[ch][k] * X[k][pix], M = 32 channels, N = 32 halo pixels, K = 64 with k = 8*ki + kj (kj = 7 and
//        ki = 7 carry zero weights): a lane's 8 k-values are 8 consecutive pixels of one row of the x tile, read with
//        immediate-offset ds_read_b32 (no address arithmetic); C/D gives each lane 4 consecutive channels of a pixel ->
//        8-byte packed stores into a1s[pix][ch].
// conv2: D[pix][o] = a1[pix + tap][c] * W2[tap][c][o], M block = 2 rows x 16 cols of the tile, K = 16 c per step;
//        A fragments = 16-byte reads of a1s (pixel pitch 144 B = 9*16); B fragments straight from L2 as coalesced
//        1 KiB loads into a 3-deep register ring (layout [k-step][hi|lo][o][16 c]); no barrier inside the K loop.
// epilogue: BN2 + ReLU + block-mean pool in registers (+ one wave shuffle for PS = 8); NCHW or token-major stores.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int B3_XH = B3_TH + 9, B3_XW = B3_TW + 9;      // x tile 16 x 24 (+1 zero row, +1 pad column) = 17 x 25
constexpr int B3_XS_BYTES = ((B3_XH * B3_XW * 4 + 15) / 16) * 16;   // 1712
constexpr int B3_A1_PITCH = 144;                         // bytes per halo pixel: 64 ch * 2 B + 16 pad (9 x 16 B: odd)
constexpr int B3_A1_ROW = B3_AW * B3_A1_PITCH + 32;      // 2624 B per halo row: 4 rows = 656 x 16 B = 0 mod 16 units, so
                                                         // an M block of rows (m, m+4) x 16 cols reads conflict-free
constexpr int B3_A1_BYTES = (B3_TH + 2) * B3_A1_ROW;     // 26240
template <bool X3> constexpr int b3_lds_bytes() { return B3_XS_BYTES + (X3 ? 2 : 1) * B3_A1_BYTES; }   // 54,192 (x3): 3 per CU

template <bool X3>
__device__ __forceinline__ void mma3(f32x16 &acc, const bf16x8 &ah, const bf16x8 &al, const bf16x8 &bh, const bf16x8 &bl) {
    if (X3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

__device__ __forceinline__ float bn_relu(float a, float s, float t) {
    float y = fmaf(a, s, t);
    return y > 0.f ? y : 0.f;
}

constexpr int B3_W1_PITCH = 144;                         // conv1 weights in LDS: [hi|lo][64 ch][64 k] bf16, row pitch 9 x 16 B
constexpr int B3_W1_BYTES = 64 * B3_W1_PITCH;            // 9216 per part
constexpr int B3_ST_BYTES = 2 * 64 * 4;                  // BN1 scale | shift
template <bool X3> constexpr int b3_lds_total() { return b3_lds_bytes<X3>() + (X3 ? 2 : 1) * B3_W1_BYTES + B3_ST_BYTES; }   // 73,136 (x3)

// Work list of the persistent kernels.  Direct path (sa.masks == nullptr): entry k is tile k, all ntiles tiles run.  Skip path:
// entry k is the k-th non-empty tile in ascending order, found by every workgroup itself from the band masks that
// k_encoder_tile_scan wrote before on the same stream (a kernel boundary orders them; bit i of mask j = tile j * band_tiles + i).
//   tiles_to_run  once per workgroup: thread c sums the popcounts of chunk c of the masks (SKIP_CHUNKS chunks of
//                 ceil(nbands / SKIP_CHUNKS) bands each, so the array is fixed and the band count is not), an exclusive scan over
//                 the chunks stays in LDS for the whole kernel, the total is the number of tiles to run.
//   skip_lookup   rank k -> tile: binary search for the chunk that holds rank k, walk its masks, select the n-th set bit.
//   skip_slate    the first SKIP_SLATE lanes look up the workgroup's next SKIP_SLATE rounds (k = blockIdx.x + round * gridDim.x) at
//                 once: one lookup's latency per SKIP_SLATE tiles, paid in the prologue beside the weight loads; inside the tile loop
//                 tile_at is one LDS word.  A launch of more rounds refills the slate every SKIP_SLATE rounds.
// All masks full (dense input): the list is the identity, nothing is looked up.
// Per pooled cell (CELLS: k_encoder_b16 at PS == 8, where a tile is two 8 x 8 cells with a 16 x 16 window each; encoder_cells.h): the
// scan also writes, per band, which tiles have a live left cell and which a live right cell (tile live = left | right).  The list is
// then two segments, walked as one: every tile with both cells live in ascending order, then every tile with exactly one, in ascending
// order; an entry carries the tile and which cell to run (enc_entry).  A one-cell tile costs about half a tile, and a launch ends with its
// slowest workgroup: in a mixed list some workgroups would draw whole tiles only.  Segmented, every workgroup also changes bodies in
// the same round.  Each segment has its own popcount prefix array; nothing else changes, and a kernel without CELLS reads the tile
// masks as before.
struct SkipArgs {
    const unsigned long long *masks = nullptr;              // null: direct path
    const unsigned long long *cell_l = nullptr, *cell_r = nullptr;   // CELLS kernels: the bands' cell words (both = masks: whole tiles)
    int *count = nullptr;                                     // workgroup 0 stores the number of tiles run (smk_encoder_skip_stats)
    const float *table = nullptr;                             // the call's zero-response table: what an empty tile's cells hold
    int nbands = 0, lg_band_tiles = 0, bands_per_frame = 0;
};
// Tile rows per band: a band is one 64-bit mask, so 64 / tiles_x rows, capped at 4: 4 for W <= 256, 2 at 512, 1 at 1024.
constexpr int scan_rows_for(int tiles_x) { return tiles_x <= 16 ? 4 : 64 / tiles_x; }
constexpr int ENC_FRAME_FEATS = 128 * 1024;                   // features per frame, either layout
constexpr int SKIP_CHUNKS = 256, SKIP_SLATE = 16;
template <bool CELLS>
struct SkipLds {
    static constexpr int SEGS = CELLS ? 2 : 1;
    int cpre[SEGS][SKIP_CHUNKS + 1];                          // entries of segment s before chunk c; [SKIP_CHUNKS] = all of them
    int wsum[SEGS][4];
    int slate[SKIP_SLATE];                                    // entry of round (r0 + i), r0 a multiple of SKIP_SLATE
};
// Band j's mask of segment seg: the tile mask, or with CELLS the both-cells (seg 0) and exactly-one-cell (seg 1) masks.
template <bool CELLS>
__device__ __forceinline__ unsigned long long skip_mask(const SkipArgs &sa, int seg, int j) {
    if (!CELLS) return sa.masks[j];
    const unsigned long long l = sa.cell_l[j], r = sa.cell_r[j];
    return seg ? enc_cells_one(l, r) : enc_cells_both(l, r);
}

template <bool CELLS>
__device__ __forceinline__ int skip_lookup(const SkipLds<CELLS> &s, const SkipArgs &sa, int k) {
    const int seg = CELLS && k >= s.cpre[0][SKIP_CHUNKS];     // ranks beyond the first segment index the second
    if (seg) k -= s.cpre[0][SKIP_CHUNKS];
    const int *cpre = s.cpre[seg];
    int c = 0;                                                // the largest c with cpre[c] <= k: chunk c holds rank k (k < total)
#pragma unroll
    for (int step = SKIP_CHUNKS / 2; step >= 1; step >>= 1)
        if (cpre[c + step] <= k) c += step;
    int n = k - cpre[c];
    int j = c * ((sa.nbands + SKIP_CHUNKS - 1) / SKIP_CHUNKS);
    unsigned long long m = skip_mask<CELLS>(sa, seg, j);
    for (int pc = __popcll(m); n >= pc; pc = __popcll(m)) {   // ends inside the chunk: it holds rank k
        n -= pc;
        m = skip_mask<CELLS>(sa, seg, ++j);
    }
    int pos = 0;                                              // the n-th set bit of m (n < popcount)
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const int cnt = __popcll((m >> pos) & ((1ull << w) - 1));
        if (n >= cnt) {
            n -= cnt;
            pos += w;
        }
    }
    const int tile = (j << sa.lg_band_tiles) + pos;
    if (!CELLS) return tile;
    return enc_entry(tile, seg, (int)(~sa.cell_l[j] >> pos) & 1);   // one cell: the right one iff the left is dead
}

// rounds r0 .. r0 + SKIP_SLATE - 1 of this workgroup -> s.slate (the caller's barrier publishes it)
template <bool CELLS>
__device__ __forceinline__ void skip_slate(SkipLds<CELLS> &s, const SkipArgs &sa, int r0, int nrun) {
    const int i = threadIdx.x;
    if (i < SKIP_SLATE) {
        const long long k = (long long)blockIdx.x + (long long)(r0 + i) * gridDim.x;
        if (k < nrun) s.slate[i] = skip_lookup(s, sa, (int)k);
    }
}

// Number of work-list entries (workgroup-uniform; all 256 threads call it, it holds barriers); leaves the chunk sums and, unless
// the list is the identity (`listed`), the slate of rounds 0 .. SKIP_SLATE - 1 in LDS.
template <bool CELLS>
__device__ __forceinline__ int tiles_to_run(SkipLds<CELLS> &s, const SkipArgs &sa, int ntiles, bool &listed) {
    listed = false;
    if (!sa.masks) return ntiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cs = (sa.nbands + SKIP_CHUNKS - 1) / SKIP_CHUNKS;
    int c[SkipLds<CELLS>::SEGS], inc[SkipLds<CELLS>::SEGS];
#pragma unroll
    for (int seg = 0; seg < SkipLds<CELLS>::SEGS; ++seg) {
        c[seg] = 0;
        for (int j = tid * cs, je = min(j + cs, sa.nbands); j < je; ++j) c[seg] += __popcll(skip_mask<CELLS>(sa, seg, j));
        inc[seg] = c[seg];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc[seg], d);
            if (lane >= d) inc[seg] += v;
        }
        if (lane == 63) s.wsum[seg][wave] = inc[seg];
    }
    __syncthreads();
#pragma unroll
    for (int seg = 0; seg < SkipLds<CELLS>::SEGS; ++seg) {
        int base = 0;
        for (int w = 0; w < wave; ++w) base += s.wsum[seg][w];
        s.cpre[seg][tid] = base + inc[seg] - c[seg];
        if (tid == SKIP_CHUNKS - 1) s.cpre[seg][SKIP_CHUNKS] = base + inc[seg];
    }
    __syncthreads();
    const int nfirst = __builtin_amdgcn_readfirstlane(s.cpre[0][SKIP_CHUNKS]);
    const int nrun = CELLS ? nfirst + __builtin_amdgcn_readfirstlane(s.cpre[SkipLds<CELLS>::SEGS - 1][SKIP_CHUNKS]) : nfirst;
    if (blockIdx.x == 0 && tid == 0) *sa.count = nrun;
    listed = nfirst != ntiles;                                // a complete first segment is ascending, i.e. the identity: no lookups
    if (listed) {
        skip_slate(s, sa, 0, nrun);
        __syncthreads();
    }
    return nrun;
}
// Entry k = blockIdx.x + round * gridDim.x of the list (k < nrun).  Workgroup-uniform; at a multiple of SKIP_SLATE > 0 it refills
// the slate behind a barrier, so every thread of the workgroup calls it at the same place.
template <bool CELLS>
__device__ __forceinline__ int tile_at(SkipLds<CELLS> &s, const SkipArgs &sa, bool listed, int round, int k, int nrun) {
    if (!listed) return k;
    if (round > 0 && (round & (SKIP_SLATE - 1)) == 0) {
        skip_slate(s, sa, round, nrun);                       // the slate's last reader is one barrier back at least
        __syncthreads();
    }
    return __builtin_amdgcn_readfirstlane(s.slate[round & (SKIP_SLATE - 1)]);
}

// The empty tiles' pooled cells, copied from the zero-response table (same offsets within the frame).  Partitioned by band straight
// from the masks: workgroup g takes bands g, g + gridDim.x, ...  Empty and non-empty tiles are disjoint words of the features, so the
// copy needs no ordering against the tile loop; it runs outside it (four loads in flight per thread, nothing live across a tile).
// The stores are non-temporal: 31 MB per headline launch that nothing in the launch reads again, beside a K loop whose weight
// fragments come from L2.
// CELLS (PS == 8: CR = 1, CC = 2): the dead cell of a one-cell tile is copied too.  Token-major a vector lies inside one cell; NCHW a
// vector is a channel's two cells, of which a one-cell tile gets the dead one as a single word.
template <int PS, bool TOKENS, bool CELLS>
__device__ __forceinline__ void skip_fill(const SkipArgs &sa, int lg_tiles_x, float *__restrict__ features) {
    static_assert(!CELLS || PS == 8, "cells are the two halves of a tile at PS == 8 only");
    constexpr bool PART = PS >= 16;                           // frames beyond 256^2: `features` and the table hold per-tile partials
    constexpr int CR = PART ? 1 : B3_TH / PS, CC = PART ? 1 : B3_TW / PS;   // cells per tile: rows x columns
    // token-major: a cell row of a tile is CC cells x 128 channels, contiguous (float4).  NCHW: a channel's CC cells of one row.
    // Partials: a tile's 128 sums, contiguous (32 x float4).
    constexpr int VW = TOKENS || PART ? 4 : (CC < 4 ? CC : 4), VPR = TOKENS || PART ? 1 : CC / VW, ROWV = CC * 32;
    constexpr int UPT = TOKENS || PART ? CR * ROWV : 128 * CR * VPR;  // vectors per tile
    constexpr int UNR = 4;
    typedef float vec_t __attribute__((ext_vector_type(VW)));
    const int tid = threadIdx.x, tiles_x = 1 << lg_tiles_x, band_tiles = 1 << sa.lg_band_tiles, total = band_tiles * UPT;
    const unsigned long long full = band_tiles == 64 ? ~0ull : (1ull << band_tiles) - 1;
    auto uniform = [](unsigned long long mv) -> unsigned long long {
        return ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned int)(mv >> 32)) << 32) |
               (unsigned int)__builtin_amdgcn_readfirstlane((unsigned int)mv);
    };
    for (int band = blockIdx.x; band < sa.nbands; band += gridDim.x) {
        // ml, mr: tiles whose left / right cell the tile loop writes (without CELLS both are the tile mask)
        const unsigned long long ml = uniform(CELLS ? sa.cell_l[band] : sa.masks[band]), mr = CELLS ? uniform(sa.cell_r[band]) : ml;
        const unsigned long long m = ml & mr;
        if (m == full) continue;
        const int lg_rows = PART ? sa.lg_band_tiles - lg_tiles_x : 2;      // tile rows per band (scan_rows_for)
        const int b = band / sa.bands_per_frame, ty0 = (band - b * sa.bands_per_frame) << lg_rows;
        float *out = features + (size_t)b * (PART ? (size_t)sa.bands_per_frame << (sa.lg_band_tiles + 7) : (size_t)ENC_FRAME_FEATS);
        for (int i0 = tid; i0 < total; i0 += 256 * UNR) {
            vec_t v[UNR];
            int off[UNR], word[UNR];                          // word: -1 the whole vector, else the one word of it to copy (CELLS, NCHW)
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                const int i = i0 + 256 * j, tl = i / UPT, u = i - tl * UPT;
                off[j] = -1;
                word[j] = -1;
                if (i >= total || ((m >> tl) & 1)) continue;
                const int ty = ty0 + (tl >> lg_tiles_x), tx = tl & (tiles_x - 1);
                const bool lrun = CELLS && ((ml >> tl) & 1), rrun = CELLS && ((mr >> tl) & 1);   // at most one of them
                if (PART) {
                    off[j] = ((ty << lg_tiles_x) + tx) * 128 + u * 4;
                } else if (TOKENS) {
                    const int a = u / ROWV, q = u - a * ROWV;
                    if (CELLS && (q >= 32 ? rrun : lrun)) continue;       // this vector is of the cell the tile loop writes
                    off[j] = ((ty * CR + a) * 32 + tx * CC) * 128 + q * 4;
                } else {
                    const int vv = u % VPR, a = (u / VPR) % CR, o = u / (VPR * CR);
                    off[j] = o * 1024 + (ty * CR + a) * 32 + tx * CC + vv * VW;
                    if (CELLS && (lrun || rrun)) word[j] = lrun ? 1 : 0;
                }
                v[j] = *reinterpret_cast<const vec_t *>(sa.table + off[j]);
            }
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                if (off[j] < 0) continue;
                if (CELLS && !TOKENS && word[j] >= 0)
                    __builtin_nontemporal_store(word[j] ? v[j][VW - 1] : v[j][0], out + off[j] + word[j]);
                else __builtin_nontemporal_store(v[j], reinterpret_cast<vec_t *>(out + off[j]));
            }
        }
    }
}
// When a workgroup copies.  The second dispatch round (the workgroups that share a CU with one of the first round) copies before
// its first tile, in place of the start delay that takes it out of phase with its partner (see the stagger below); the first round
// copies after its last tile, while the partner, started later, is still in its K loop.  Either way the copy of one workgroup runs
// beside the matrix work of the other.  Measured against "all after", "all before" and "only workgroups with a round to spare":
// DESIGN.md 3.2.
__device__ __forceinline__ bool skip_fill_first() { return (blockIdx.x / 256) & 1; }

// ---------------------------------------------------------------- what the three persistent kernels share
// k_encoder_bf16, k_encoder_b16 and k_encoder_i8 are one design: stage the conv1 weights, walk the work list of 8 x 16 tiles,
// conv1 on MFMA into an LDS image, prefetch the next tile's input under the conv2 K loop, pool, store.  The parts below exist
// once; a kernel keeps its conv2 K loop, its a1 image and what it does with conv1's results.

// BN1 scale | shift and the conv1 weights [part][ch][64 k] -> LDS with a 144-byte row pitch (16-byte chunks: 8 per row); once
// per workgroup.  PARTS = 2: hi and lo.
template <int PARTS>
__device__ __forceinline__ void conv1_stage(const EncoderDev &e, unsigned char *w1s, float *st1) {
    const int tid = threadIdx.x;
    if (tid < 128) st1[tid] = tid < 64 ? e.s1[tid] : e.t1[tid - 64];
    const uint4 *src = reinterpret_cast<const uint4 *>(e.w1p);
    for (int c = tid; c < PARTS * 64 * 8; c += 256) {
        const int row = c >> 3, u = c & 7;                     // row = part*64 + ch
        *reinterpret_cast<uint4 *>(w1s + row * B3_W1_PITCH + u * 16) = src[c];
    }
}

// The frames of a call and their grid of tiles (tile counts are 2^n).
struct TileSrc {
    const float *frames;
    int64_t fstride;
    int H, W, lg_tiles_x, lg_tiles_per_frame;
    // tile id -> frame, first row, first column
    __device__ __forceinline__ void decode(int t, int &b, int &r0, int &c0) const {
        b = t >> lg_tiles_per_frame;
        const int rem = t & ((1 << lg_tiles_per_frame) - 1);
        r0 = (rem >> lg_tiles_x) * B3_TH;
        c0 = (rem & ((1 << lg_tiles_x) - 1)) * B3_TW;
    }
    // x halo element k of tile t (2 per thread): value or 0 outside the image / in the pad row and column
    __device__ __forceinline__ float fetch(int t, int k) const {
        if (k >= B3_XH * B3_XW) return 0.f;
        int bb, rr0, cc0;
        decode(t, bb, rr0, cc0);
        const int row = k / B3_XW, col = k - row * B3_XW;
        const int ii = rr0 - 4 + row, jj = cc0 - 4 + col;
        const bool ok = row < B3_XH - 1 && col < B3_XW - 1 && ii >= 0 && ii < H && jj >= 0 && jj < W;
        return ok ? frames[(size_t)bb * fstride + (size_t)ii * W + jj] : 0.f;
    }
};

// A thread's two x halo elements -> the LDS tile; word(v) is what a kernel keeps per element (the float, or b16's split pair).
template <class T, class Word>
__device__ __forceinline__ void halo_to_lds(T *xs, float v0, float v1, Word word) {
    const int tid = threadIdx.x;
    xs[tid] = word(v0);
    if (tid + 256 < B3_XH * B3_XW) xs[tid + 256] = word(v1);
}

// The walk of a workgroup over the work list: entries k = blockIdx.x, + gridDim.x, ...; t is the tile of entry k.
//   begin   list length, first tile, the fill or the start delay, first halo -> LDS, barrier
//   next    rank and tile of the following round, its halo into registers (lands under the K loop); after the a1 barrier
//   the kernel's loop tail puts those registers into LDS (halo_to_lds), holds its barrier and sets t = tn
//   end     the trailing fill
// tiles_to_run and tile_at hold barriers: every thread of the workgroup calls begin and next, at the same place.
// CELLS: the list's entries say which cells of the tile to run (cell / celln, as enc_entry_cell gives them; 0 = the whole tile).
template <bool CELLS = false>
struct TileWalk {
    int k, nrun, round, t, tn, cell, celln;
    bool listed;

    __device__ __forceinline__ int entry(SkipLds<CELLS> &skl, const SkipArgs &sa, int kk, int &what) {
        const int e = tile_at(skl, sa, listed, round, kk, nrun);
        what = CELLS && listed ? enc_entry_cell(e) : 0;
        return CELLS && listed ? enc_entry_tile(e) : e;
    }
    template <int PS, bool TOKENS, class T, class Word>
    __device__ __forceinline__ void begin(SkipLds<CELLS> &skl, const SkipArgs &sa, const TileSrc &src, int ntiles, int stagger,
                                          float *__restrict__ features, T *xs, Word word) {
        k = blockIdx.x;
        nrun = tiles_to_run(skl, sa, ntiles, listed);
        round = 0;
        cell = 0;
        t = k < nrun ? entry(skl, sa, k, cell) : 0;
        // Workgroups that share a CU run the same program with the same period; started together they stay in lockstep
        // (both in the VALU-heavy conv1 phase, then both in the MFMA loop).  Delay every other dispatch round by about
        // half a tile so that one workgroup's conv1 overlaps the other's K loop (speed only, never correctness).
        // On the skip path that round copies its share of the empty tiles' cells instead (skip_fill_first): the same shift, not idle.
        if (listed && skip_fill_first()) skip_fill<PS, TOKENS, CELLS>(sa, src.lg_tiles_x, features);
        else if (stagger > 0 && ((blockIdx.x / 256) & 1))
            for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);
        const int tid = threadIdx.x;
        if (k < nrun) halo_to_lds(xs, src.fetch(t, tid), src.fetch(t, tid + 256), word);
        __syncthreads();
    }
    __device__ __forceinline__ void next(SkipLds<CELLS> &skl, const SkipArgs &sa, const TileSrc &src, float &xr0, float &xr1) {
        const int kn = k + gridDim.x;
        ++round;
        celln = 0;
        tn = kn < nrun ? entry(skl, sa, kn, celln) : 0;
        xr0 = 0.f;
        xr1 = 0.f;
        if (kn < nrun) {
            int tid = threadIdx.x;
            // CELLS: the element's row and column are formed here, per tile, instead of living through both tile bodies' K loops
            // (k_encoder_b16's whole-tile loop has no registers to spare)
            if (CELLS) asm volatile("" : "+v"(tid));
            xr0 = src.fetch(tn, tid);
            xr1 = src.fetch(tn, tid + 256);
        }
    }
    template <int PS, bool TOKENS>
    __device__ __forceinline__ void end(const SkipArgs &sa, const TileSrc &src, float *__restrict__ features) const {
        if (listed && !skip_fill_first()) {
            __builtin_amdgcn_s_setprio(0);
            skip_fill<PS, TOKENS, CELLS>(sa, src.lg_tiles_x, features);
        }
    }
    // the loop tail's step to the next entry
    __device__ __forceinline__ void advance() {
        t = tn;
        cell = celln;
    }
};

// conv1's B fragments for pixel block pb of the a1 halo tile (32 halo pixels, lane r = one pixel), from the fp32 x tile: a lane's
// 8 k-values are 8 consecutive pixels of one row, split into hi and lo.  aoff = the pixel's byte offset in an a1 image of the
// given row and pixel pitch; valid = the pixel exists (pixel block 5 is partial); inimg = it lies inside the image.
template <int A1_ROW, int A1_PITCH>
__device__ __forceinline__ void x_frags(const float *xs, int pb, int r0, int c0, int H, int W, bf16x8 (&xh)[4], bf16x8 (&xl)[4],
                                        int &aoff, bool &valid, bool &inimg) {
    const int r = threadIdx.x & 31, hi = (threadIdx.x >> 5) & 1;
    const int pix = pb * 32 + r;
    valid = pix < B3_APIX;
    const int pc = valid ? pix : B3_APIX - 1;
    const int ar = pc / B3_AW, ac = pc - ar * B3_AW;
    const int ii = r0 - 1 + ar, jj = c0 - 1 + ac;
    inimg = valid && ii >= 0 && ii < H && jj >= 0 && jj < W;
    aoff = ar * A1_ROW + ac * A1_PITCH;
    const float *xp = xs + (ar + hi) * B3_XW + ac;                          // row ar + 2s + hi, cols ac .. ac+7
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 vh, vl;
            split_bf16(xp[s * 2 * B3_XW + j], vh, vl);
            xh[s][j] = vh; xl[s][j] = vl;
        }
}

// conv1 on MFMA: 6 blocks of 32 halo pixels x 2 blocks of 32 channels.  Wave w takes pixel block w for BOTH channel blocks (x
// fragments built once, two independent accumulator chains: conv1_both) and one half of a shared block (pixel block 4 + w/2,
// channel block w&1: conv1_one): 3 (block, channel-block) units per wave.
template <bool X3>
__device__ __forceinline__ void conv1_both(const unsigned char *w1s, const bf16x8 (&xh)[4], const bf16x8 (&xl)[4], f32x16 &acc0,
                                           f32x16 &acc1) {
    const int r = threadIdx.x & 31, hi = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int g = 0; g < 16; ++g) { acc0[g] = 0.f; acc1[g] = 0.f; }
    const unsigned char *wrow = w1s + r * B3_W1_PITCH + 8 * hi * 2;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bf16x8 a0h = *reinterpret_cast<const bf16x8 *>(wrow + s * 32);
        const bf16x8 a1hh = *reinterpret_cast<const bf16x8 *>(wrow + 32 * B3_W1_PITCH + s * 32);
        const bf16x8 a0l = X3 ? *reinterpret_cast<const bf16x8 *>(wrow + B3_W1_BYTES + s * 32) : a0h;
        const bf16x8 a1l_ = X3 ? *reinterpret_cast<const bf16x8 *>(wrow + B3_W1_BYTES + 32 * B3_W1_PITCH + s * 32) : a1hh;
        mma3<X3>(acc0, a0h, a0l, xh[s], xl[s]);
        mma3<X3>(acc1, a1hh, a1l_, xh[s], xl[s]);
    }
}
template <bool X3>
__device__ __forceinline__ void conv1_one(const unsigned char *w1s, int cb, const bf16x8 (&xh)[4], const bf16x8 (&xl)[4],
                                          f32x16 &acc) {
    const int r = threadIdx.x & 31, hi = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    const unsigned char *wrow = w1s + (cb * 32 + r) * B3_W1_PITCH + 8 * hi * 2;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(wrow + s * 32);
        const bf16x8 al = X3 ? *reinterpret_cast<const bf16x8 *>(wrow + B3_W1_BYTES + s * 32) : ah;
        mma3<X3>(acc, ah, al, xh[s], xl[s]);
    }
}

// Block-mean pool + store for the 32x32 accumulator layout (k_encoder_bf16, k_encoder_i8); val(mi, g) is the finished activation
// of register g of M block mi: pixel p = (g&3) + 8(g>>2) + 4hi of the block -> tile row mi + 4(p>>4), col p & 15,
// i.e. q = g>>2 = 2qr + qc: row mi + 4qr, cols 8qc + 4hi + (g&3).  o = the lane's output channel.
// PS >= 16 (frames beyond 256^2): `features` is the partial buffer and the store is tile `tile`'s sum for channel o.
template <int PS, bool TOKENS, class Val>
__device__ __forceinline__ void pool_store_32(float *__restrict__ features, int b, int o, int r0, int c0, int tile, Val val) {
    const int hi = (threadIdx.x >> 5) & 1;
    auto out_index = [&](int pi, int pj) -> size_t {
        return TOKENS ? ((size_t)b * 1024 + pi * 32 + pj) * 128 + o : ((size_t)b * 128 + o) * 1024 + pi * 32 + pj;
    };
    if (PS == 2) {          // cell rows (mi, mi+1) for even mi, cell cols = column pairs
#pragma unroll
        for (int mp = 0; mp < 2; ++mp)
#pragma unroll
            for (int qr = 0; qr < 2; ++qr)
#pragma unroll
                for (int qc = 0; qc < 2; ++qc)
#pragma unroll
                    for (int cg = 0; cg < 2; ++cg) {
                        float sum = 0.f;
#pragma unroll
                        for (int mi = 2 * mp; mi < 2 * mp + 2; ++mi)
#pragma unroll
                            for (int i = 2 * cg; i < 2 * cg + 2; ++i) sum += val(mi, 4 * (2 * qr + qc) + i);
                        features[out_index((r0 + 2 * mp + 4 * qr) / 2, (c0 + 8 * qc + 4 * hi + 2 * cg) / 2)] = sum * 0.25f;
                    }
    } else if (PS == 4) {   // cell row = qr (rows 4qr .. 4qr+3 = all mi), cell col = 2qc + hi
#pragma unroll
        for (int qr = 0; qr < 2; ++qr)
#pragma unroll
            for (int qc = 0; qc < 2; ++qc) {
                float sum = 0.f;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int i = 0; i < 4; ++i) sum += val(mi, 4 * (2 * qr + qc) + i);
                features[out_index((r0 + 4 * qr) / 4, (c0 + 8 * qc + 4 * hi) / 4)] = sum * (1.0f / 16);
            }
    } else if (PS >= 16) {   // the PS == 8 sums, the two 8-column halves added, then the two lane halves: one sum per tile
        float cell[2];
#pragma unroll
        for (int qc = 0; qc < 2; ++qc) {
            float sum = 0.f;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int qr = 0; qr < 2; ++qr)
#pragma unroll
                    for (int i = 0; i < 4; ++i) sum += val(mi, 4 * (2 * qr + qc) + i);
            cell[qc] = sum;
        }
        const float mine = cell[0] + cell[1];
        const float total = mine + __shfl_xor(mine, 32);     // a+b == b+a: both halves agree bitwise
        if (hi == 0) features[(size_t)tile * 128 + o] = total;
    } else {   // PS == 8: two cells (qc); each is split over the two lane halves (hi)
        float cell[2];
#pragma unroll
        for (int qc = 0; qc < 2; ++qc) {
            float sum = 0.f;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int qr = 0; qr < 2; ++qr)
#pragma unroll
                    for (int i = 0; i < 4; ++i) sum += val(mi, 4 * (2 * qr + qc) + i);
            cell[qc] = sum;
        }
        const float other0 = __shfl_xor(cell[0], 32), other1 = __shfl_xor(cell[1], 32);
        const float total = hi == 0 ? cell[0] + other0 : cell[1] + other1;   // a+b == b+a: both halves agree bitwise
        features[out_index(r0 / 8, c0 / 8 + hi)] = total * (1.0f / 64);
    }
}

// Persistent: each workgroup walks work-list entries k = blockIdx.x, +gridDim.x, ... (t = tile_at(..., k)).  Per-workgroup
// costs (conv1 weights -> LDS, BN2 scale/shift, B-ring fill) are paid once; the next tile's x halo is prefetched into registers under the K loop and
// the B-fragment ring simply keeps running across tiles (the weights do not depend on the tile).
template <bool X3, int PS, bool TOKENS>
__global__ __launch_bounds__(256, 2) void k_encoder_bf16(const float *__restrict__ frames, int64_t fstride, int H, int W,
                                                      EncoderDev e, float *__restrict__ features, int lg_tiles_x,
                                                      int lg_tiles_per_frame, int ntiles, int stagger,
                                                      SkipArgs sa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);
    unsigned char *a1h = smem + B3_XS_BYTES, *a1l = a1h + B3_A1_BYTES;
    unsigned char *w1s = a1h + (X3 ? 2 : 1) * B3_A1_BYTES;
    float *st1 = reinterpret_cast<float *>(w1s + (X3 ? 2 : 1) * B3_W1_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    conv1_stage<X3 ? 2 : 1>(e, w1s, st1);                     // once per workgroup
    const int o = wave * 32 + r;
    const float s2 = e.s2[o], t2 = e.t2[o];
    // w2q: [k-step 36][hi|lo][o 128][16 c] bf16 = 4 KiB per (k-step, part); this lane reads 16 bytes at a constant
    // per-lane offset from a wave-uniform (scalar) base: no per-load VGPR address arithmetic
    // (buffer_load with the descriptor in SGPRs: voffset = lane bytes, soffset = fragment bytes).
    const int lane_b = (o * 2 + hi) * 16;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(e.w2q), 0, 36 * 2 * 4096, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto load_b = [&](int kn, int part) -> uint4 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane_b, (kn * 2 + part) * 4096, 0);
        return make_uint4(v[0], v[1], v[2], v[3]);
    };
    constexpr int RING = 6;                      // B fragments in flight: RING-1 k-steps ahead (L2 latency under load);
                                                          // the ring stays live through conv1, so x3 (2 regs sets) keeps it shorter
    uint4 bqh[RING], bql[RING];
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) {
        bqh[k] = load_b(k, 0);
        if (X3) bql[k] = load_b(k, 1);
    }
    const int lane_off = (r >> 4) * 4 * B3_A1_ROW + (r & 15) * B3_A1_PITCH + 8 * hi * 2;

    const TileSrc src{frames, fstride, H, W, lg_tiles_x, lg_tiles_per_frame};
    __shared__ SkipLds<false> skl;
    TileWalk<> wk;
    wk.begin<PS, TOKENS>(skl, sa, src, ntiles, stagger, features, xs, [](float v) { return v; });

    for (; wk.k < wk.nrun; wk.k += gridDim.x) {
        int b, r0, c0;
        src.decode(wk.t, b, r0, c0);

        __builtin_amdgcn_s_setprio(0);
        // ---- conv1 on MFMA (x_frags, conv1_both, conv1_one): results split and stored into the a1 image
        auto conv1_store = [&](const f32x16 &acc, int cb, int aoff, bool valid, bool inimg) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ch0 = cb * 32 + 8 * q + 4 * hi;
                const float4 sc = *reinterpret_cast<const float4 *>(st1 + ch0);
                const float4 sh = *reinterpret_cast<const float4 *>(st1 + 64 + ch0);
                const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
                bf16x4 vh, vl;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float y = inimg ? bn_relu(acc[4 * q + i], scv[i], shv[i]) : 0.f;   // outside the image: conv2's zero pad
                    __bf16 a, bb;
                    split_bf16(y, a, bb);
                    vh[i] = a; vl[i] = bb;
                }
                if (valid) {
                    *reinterpret_cast<bf16x4 *>(a1h + aoff + ch0 * 2) = vh;
                    if (X3) *reinterpret_cast<bf16x4 *>(a1l + aoff + ch0 * 2) = vl;
                }
            }
        };
        {
            bf16x8 xh[4], xl[4];
            int aoff; bool valid, inimg;
            x_frags<B3_A1_ROW, B3_A1_PITCH>(xs, wave, r0, c0, H, W, xh, xl, aoff, valid, inimg);
            f32x16 acc0, acc1;
            conv1_both<X3>(w1s, xh, xl, acc0, acc1);
            conv1_store(acc0, 0, aoff, valid, inimg);
            conv1_store(acc1, 1, aoff, valid, inimg);
        }
        {
            bf16x8 xh[4], xl[4];
            int aoff; bool valid, inimg;
            const int cb = wave & 1;
            x_frags<B3_A1_ROW, B3_A1_PITCH>(xs, 4 + (wave >> 1), r0, c0, H, W, xh, xl, aoff, valid, inimg);
            f32x16 acc;
            conv1_one<X3>(w1s, cb, xh, xl, acc);
            conv1_store(acc, cb, aoff, valid, inimg);
        }
        __syncthreads();                                      // a1s complete; xs is free again
        // The MFMA-bound K loop runs at raised priority: while the co-resident workgroup is in its VALU-heavy conv1 phase
        // the matrix pipe is the resource to keep fed.  Interleaved A/B, 5 rounds: 1.439 -> 1.358 ms median (-5.7 %);
        // raising it before the barrier or to priority 3 gives -4 %.
        __builtin_amdgcn_s_setprio(1);

        float xr0, xr1;                                       // next tile's x halo -> registers (lands under the K loop)
        wk.next(skl, sa, src, xr0, xr1);

        // ---- conv2: wave = channel block; 4 M blocks (rows mi and mi+4, 16 cols each)
        f32x16 acc[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[mi][g] = 0.f;
        auto load_a = [&](int k, bf16x8 (&ah)[4], bf16x8 (&al)[4]) {
            const int tap = k >> 2, ks = k & 3, ki = tap / 3, kj = tap - 3 * ki;
            const int abase = lane_off + ki * B3_A1_ROW + kj * B3_A1_PITCH + ks * 32;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                ah[mi] = *reinterpret_cast<const bf16x8 *>(a1h + abase + mi * B3_A1_ROW);
                if (X3) al[mi] = *reinterpret_cast<const bf16x8 *>(a1l + abase + mi * B3_A1_ROW);
            }
        };
        bf16x8 ahA[4], alA[4], ahB[4], alB[4];
        load_a(0, ahA, alA);
        constexpr int UNR = 6;               // multiple of RING and of 2: ring / buffer indices are constants
#pragma unroll 1
        for (int k0 = 0; k0 < 36; k0 += UNR) {                // (a full unroll needs 352 registers: 1 wave/SIMD, slower)
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int k = k0 + u;
                {   // refill the slot consumed one step ago with k-step k + RING - 1 (wraps into the next tile's k-steps)
                    int kn = k + RING - 1;
                    kn = kn >= 36 ? kn - 36 : kn;
                    kn = __builtin_amdgcn_readfirstlane(kn);
                    bqh[(u + RING - 1) % RING] = load_b(kn, 0);
                    if (X3) bql[(u + RING - 1) % RING] = load_b(kn, 1);
                }
                if (k + 1 < 36) {
                    if (u & 1) load_a(k + 1, ahA, alA); else load_a(k + 1, ahB, alB);
                }
                const bf16x8 bh = __builtin_bit_cast(bf16x8, bqh[u % RING]);
                const bf16x8 bl = X3 ? __builtin_bit_cast(bf16x8, bql[u % RING]) : bh;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    if (u & 1) mma3<X3>(acc[mi], ahB[mi], alB[mi], bh, bl); else mma3<X3>(acc[mi], ahA[mi], alA[mi], bh, bl);
                }
                // Schedule of one k-step: the loads of step k+1 (LDS) and k+RING-1 (L2) are issued INSIDE the gaps of step
                // k's MFMAs, one per MFMA (hipcc otherwise either sinks each ds_read to just before its consumer or, with
                // the blocks pinned, issues all loads while the matrix pipe idles).
                constexpr int NMF = X3 ? 12 : 4, NDS = X3 ? 8 : 4, NVM = X3 ? 2 : 1;
#pragma unroll
                for (int i = 0; i < NMF; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                    // 1 MFMA
                    if (i < NDS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);       // 1 DS read
                    else if (i < NDS + NVM) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // 1 VMEM read
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- epilogue: BN2 + ReLU + block-mean pool
        pool_store_32<PS, TOKENS>(features, b, o, r0, c0, wk.t, [&](int mi, int g) { return bn_relu(acc[mi][g], s2, t2); });

        // next tile's x halo -> LDS (xs has been free since the barrier above); one barrier then covers both
        // "every wave is done reading a1" and "xs is visible"
        halo_to_lds(xs, xr0, xr1, [](float v) { return v; });
        __syncthreads();
        wk.advance();
    }
    wk.end<PS, TOKENS>(sa, src, features);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_encoder_b16: the split-bf16 encoder on v_mfma_f32_16x16x32_bf16.  Same tiles, same arithmetic (x3), same conv1 as
// k_encoder_bf16<true>; only conv2's MFMA shape changes.  Why: the K loop is power-limited (about 1.5 GHz); at equal cycles
// per flop the 16x16x32 shape sustains a higher clock (MI355X_MICROARCH.md, "Shape": 1.12-1.14x in LDS-fed loops).
//   conv2: D[pix][o], M tile = one tile row of 16 pixels (8 per workgroup tile), N tile = 16 channels (2 per wave), K = 32 c per
//          k-step (18 = 9 taps x 2).  A lane reads pixel (lane & 15), channel group 4*half + (lane >> 4) (8 c = 16 B).
//   a1 image: [180 halo pixels][8 groups of 8 c] without padding, group g of pixel p stored at unit g ^ (p & 7).
//          No linear pitch is conflict-free for this operand (ds_read_b128 serves lanes {0-3,12-15,20-27} together: 8 pixels
//          of one channel group with 8 of the next); with the XOR every lane group hits 16 distinct 16-byte units for every tap
//          shift, and conv1's 8-byte stores stay at their inherent 2-way (an exhaustive search over pitches 8..16 units and
//          shift/mask swizzles: DESIGN.md 3.2; the first swizzle tried, (p >> 1 & 3) << 1, read conflict-free but stored 4-way).
//   loop:  unit = half a k-step (M tiles 4hm..4hm+3: 24 MFMAs = 384 cycles, the same unit as k_encoder_bf16's k-step), so the
//          skeleton -- A fragments of the next unit read under this unit's MFMAs, B ring from L2 -- and the register budget
//          (64 acc + 64 A + 48 B) carry over.
constexpr int S16_LDS = B3_XS_BYTES + 2 * S16_A1_BYTES + 2 * B3_W1_BYTES + B3_ST_BYTES;   // 66,736 -> 2 workgroups per CU

template <int PS, bool TOKENS>
__global__ __launch_bounds__(256, 2) void k_encoder_b16(const float *__restrict__ frames, int64_t fstride, int H, int W,
                                                     EncoderDev e, float *__restrict__ features, int lg_tiles_x,
                                                     int lg_tiles_per_frame, int ntiles, int stagger,
                                                     SkipArgs sa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // x tile kept already split: one word per pixel, hi bf16 in the low half, lo bf16 in the high half (split once by the staging
    // thread; every wave's fragment builder then needs one v_perm_b32 per element pair instead of two 3-instruction splits)
    constexpr bool CELLS = PS == 8;                           // a tile is two pooled cells: one-cell tiles run the second body below
    unsigned int *xs = reinterpret_cast<unsigned int *>(smem);
    unsigned char *a1h = smem + B3_XS_BYTES, *a1l = a1h + S16_A1_BYTES;
    unsigned char *w1s = a1l + S16_A1_BYTES;
    float *st1 = reinterpret_cast<float *>(w1s + 2 * B3_W1_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    conv1_stage<2>(e, w1s, st1);
    // conv2 operand lanes: pixel / channel px = lane & 15, channel group kg = lane >> 4
    const int px = lane & 15, kg = lane >> 4;
    const int o0 = wave * 32 + px;                                            // N tile 0; tile 1 = + 16
    const float s2a = e.s2[o0], t2a = e.t2[o0], s2b = e.s2[o0 + 16], t2b = e.t2[o0 + 16];
    // w2s: [k-step 18][hi|lo][o 128][32 c]: 8 KiB per (k-step, part); lane offset = (o * 32 + kg * 8) * 2 B
    const int lane_b = o0 * 64 + kg * 16;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(e.w2s), 0, 18 * 2 * 8192, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto load_b = [&](int ks, int part, int nt) -> uint4 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane_b, (ks * 2 + part) * 8192 + nt * 1024, 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    };
    // B ring in k-steps: slot = [nt][part]; 3 slots = two k-steps ahead
    constexpr int RING = 2;                                   // two k-steps = one tap: the slot of k-step (tap, half) is `half`
                                                              // (3-deep with a 3-tap body: 43 spilled registers, +12 % time)
    uint4 bq[RING][2][2];
#pragma unroll
    for (int k = 0; k < RING - 1; ++k)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            bq[k][nt][0] = load_b(k, 0, nt);
            bq[k][nt][1] = load_b(k, 1, nt);
        }
    // A addressing: pixel p = (mt + ki) * 18 + px + kj; unit = g ^ (p & 7), g = 4 half + kg.  p & 7 = (px + kj + 2 (mt + ki)) & 7
    // because 18 = 2 (mod 8): tq[kj] is the lane part, the row part is added per read.

    auto pack_split = [](float v) -> unsigned int {
        __bf16 vh, vl;
        split_bf16(v, vh, vl);
        return (unsigned int)__builtin_bit_cast(unsigned short, vh) | ((unsigned int)__builtin_bit_cast(unsigned short, vl) << 16);
    };
    const TileSrc src{frames, fstride, H, W, lg_tiles_x, lg_tiles_per_frame};
    __shared__ SkipLds<CELLS> skl;
    TileWalk<CELLS> wk;
    wk.template begin<PS, TOKENS>(skl, sa, src, ntiles, stagger, features, xs, pack_split);

    for (; wk.k < wk.nrun; wk.k += gridDim.x) {
        int b, r0, c0;
        src.decode(wk.t, b, r0, c0);
        // CELLS: conv1's lane constants (pixel, halo coordinates, a1 store offsets of every unit) are formed per tile from an opaque copy of
        // the lane's pixel index: kept across tiles they would live through both K loops, and the whole-tile loop has no registers to spare
        int rt = r;
        if (CELLS) asm volatile("" : "+v"(rt));

        __builtin_amdgcn_s_setprio(S16_PRIO_CONV1);
#ifdef SMK_ENC_ABLATE      // timing ablations (tools/enc_ablate.sh; never a product build): 1 conv1 only on a workgroup's first tile,
                           // 2 no BN/ReLU/pool epilogue, 4 no workgroup barriers, 8 no conv2 MFMAs -- results are wrong by construction
        const bool abl_conv1 = !((SMK_ENC_ABLATE & 1) && wk.k != (int)blockIdx.x);
#else
        constexpr bool abl_conv1 = true;
#endif
        // ---- conv1 on MFMA (32x32x16, as k_encoder_bf16): results stored into the swizzled a1 image
        // the B fragments of the a1 halo pixel at (ar, ac): 8 rows x 8 columns of the x tile from there on, this lane's 4 rows
        // K = 64 holds the 7 x 7 patch as 8 x 8: row 7 and column 7 carry zero weights.  Their x operands are zeros too, not the pixels
        // that lie there (the column is not read, the row is the tile's zero row): 0 x NaN and 0 x Inf are NaN, and a pixel must not reach
        // an activation 4 columns to its left or 4 rows above, outside the window the tile skip tests.  Finite frames: the same bits.
        auto x_build = [&](int ar, int ac, bf16x8 (&xh)[4], bf16x8 (&xl)[4]) {
            const unsigned int *xp = xs + (ar + hi) * B3_XW + ac;
            const unsigned int *xz = hi ? xs + (B3_XH - 1) * B3_XW + ac : xp + 6 * B3_XW;      // patch row 6 (hi 0) or 7 (hi 1: zeros)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                unsigned int wh[4], wl[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const unsigned int *row = s == 3 ? xz : xp + s * 2 * B3_XW;
                    const unsigned int e0 = row[2 * jj], e1 = jj == 3 ? 0u : row[2 * jj + 1];
                    wh[jj] = __builtin_amdgcn_perm(e1, e0, 0x05040100u);          // low halves: the two hi parts
                    wl[jj] = __builtin_amdgcn_perm(e1, e0, 0x07060302u);          // high halves: the two lo parts
                }
                xh[s] = __builtin_bit_cast(bf16x8, make_uint4(wh[0], wh[1], wh[2], wh[3]));
                xl[s] = __builtin_bit_cast(bf16x8, make_uint4(wl[0], wl[1], wl[2], wl[3]));
            }
        };
        auto x_frags = [&](int pb, bf16x8 (&xh)[4], bf16x8 (&xl)[4], int &pix, bool &valid, bool &inimg) {
            const int pp = pb * 32 + rt;
            valid = pp < B3_APIX;
            pix = valid ? pp : B3_APIX - 1;
            const int ar = pix / B3_AW, ac = pix - ar * B3_AW;
            const int ii = r0 - 1 + ar, jj = c0 - 1 + ac;
            inimg = valid && ii >= 0 && ii < H && jj >= 0 && jj < W;
            x_build(ar, ac, xh, xl);
        };
        auto conv1_store = [&](const f32x16 &acc, int cb, int pix, bool valid, bool inimg) {
            const int sw = pix & 7;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ch0 = cb * 32 + 8 * q + 4 * hi;                      // 4 consecutive channels: half of group cb*4 + q
                const float4 sc = *reinterpret_cast<const float4 *>(st1 + ch0);
                const float4 sh = *reinterpret_cast<const float4 *>(st1 + 64 + ch0);
                const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
                bf16x4 vh, vl;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float y = inimg ? bn_relu(acc[4 * q + i], scv[i], shv[i]) : 0.f;
                    __bf16 a, bb;
                    split_bf16(y, a, bb);
                    vh[i] = a; vl[i] = bb;
                }
                if (valid) {
                    const int off = pix * 128 + (((cb * 4 + q) ^ sw) * 16) + 8 * hi;
                    *reinterpret_cast<bf16x4 *>(a1h + off) = vh;
                    *reinterpret_cast<bf16x4 *>(a1l + off) = vl;
                }
            }
        };
        auto out_index = [&](int pi, int pj, int o) -> size_t {
            return TOKENS ? ((size_t)b * 1024 + pi * 32 + pj) * 128 + o : ((size_t)b * 128 + o) * 1024 + pi * 32 + pj;
        };
        float xr0, xr1;                                       // the next tile's x halo (TileWalk::next)
        if (CELLS && wk.cell != 0) {
            // ---- a one-cell tile (encoder_cells.h): only cell `side` has a non-zero window; skip_fill writes the other one.  The same
            // a1 image, swizzle and K order per output as below, over half the pixels: every accumulator holds the bits the whole
            // tile would give it.
            //   conv1: the 10 x 10 a1 pixels the cell's conv2 reads, 4 pixel blocks of 32 (one per wave, both channel blocks) for 6.
            //   conv2: 4 M blocks (block m = cell rows 2m, 2m + 1 x 8 columns) for 8; a unit is a whole k-step, 24 MFMAs as below.
            //          The rows of a block are 18 pixels = 2 (mod 8) apart, so in a ds_read_b128 lane group two lane pairs share a
            //          16-byte unit (2-way) where the whole tile's 16 consecutive pixels are conflict-free: half the reads at twice
            //          the cost each.
            //   B ring: the same 18 k-steps, consumed twice as fast.  A third slot (its registers are free: half the accumulators)
            //          keeps the loads two units ahead as below; it enters and leaves with slot 0 = k-step 0 like the whole tile.
            const int side = wk.cell & 1;
            // This body's lane constants are formed per tile from opaque copies: hoisted out of the tile loop they would stay live
            // through the whole tile's K loop, which has no registers to spare (scratch 0 there is worth more than these few adds).
            int cpx = px, ckg = kg;
            asm volatile("" : "+v"(cpx), "+v"(ckg));
            uint4 bqx[2][2];
            auto ring_load = [&](uint4 (&slot)[2][2], int ks) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    slot[nt][0] = load_b(ks, 0, nt);
                    slot[nt][1] = load_b(ks, 1, nt);
                }
            };
            ring_load(bq[1], 1);                              // lands under conv1
            if (abl_conv1) {
                bf16x8 xh[4], xl[4];
                const int pp = wave * 32 + rt;
                const bool valid = pp < ENC_CELL_A1_PIX;
                int ar, ac;
                enc_cell_conv1_pixel(valid ? pp : ENC_CELL_A1_PIX - 1, side, ar, ac);
                const int pix = ar * B3_AW + ac, ii = r0 - 1 + ar, jj = c0 - 1 + ac;
                const bool inimg = valid && ii >= 0 && ii < H && jj >= 0 && jj < W;
                x_build(ar, ac, xh, xl);
                f32x16 acc0, acc1;
                conv1_both<true>(w1s, xh, xl, acc0, acc1);
                conv1_store(acc0, 0, pix, valid, inimg);
                conv1_store(acc1, 1, pix, valid, inimg);
            }
            __syncthreads();                                  // a1 complete; xs is free again
            __builtin_amdgcn_s_setprio(S16_PRIO_KLOOP);
            wk.next(skl, sa, src, xr0, xr1);

            // acc[m][nt][reg] = D(cell row 2m + (ckg >> 1), cell column 4 (ckg & 1) + reg; channel 16 nt + cpx of the wave's 32)
            f32x4v acc[4][2];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[m][nt][g] = 0.f;
            // A addressing as below with p = pl + kj + (2m + ki) * 18: the swizzle term (p & 7) depends on m & 1 only
            const int c16[2] = {ckg << 4, (4 + ckg) << 4};
            const int pl = enc_cell_a1_pixel(0, cpx, 0, 0, side);
            auto tap_consts = [&](int ki, int kj, int (&om)[2]) {
#pragma unroll
                for (int m = 0; m < 2; ++m) om[m] = ((pl + kj) << 7) ^ (((pl + kj + 2 * (2 * m + ki)) & 7) << 4);
            };
            auto load_a = [&](int ki, int half, const int (&om)[2], bf16x8 (&ah)[4], bf16x8 (&al)[4]) {
                const unsigned char *ph = a1h + ki * (B3_AW * 128), *pw = a1l + ki * (B3_AW * 128);      // wave-uniform part
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int off = om[m & 1] ^ c16[half];
                    ah[m] = *reinterpret_cast<const bf16x8 *>(ph + off + 2 * m * (B3_AW * 128));
                    al[m] = *reinterpret_cast<const bf16x8 *>(pw + off + 2 * m * (B3_AW * 128));
                }
            };
            bf16x8 ahA[4], alA[4], ahB[4], alB[4];
            int om[2];
            tap_consts(0, 0, om);
            load_a(0, 0, om, ahA, alA);
            // unit u of tap row ki = k-step ks = 6 ki + u: tap (ki, kj = u >> 1), channel half u & 1, ring slot u % 3
#pragma unroll 1
            for (int ki = 0; ki < 3; ++ki) {
#pragma unroll
                for (int u = 0; u < 6; ++u) {
                    const int kj = u >> 1, half = u & 1;
                    uint4 (&bs)[2][2] = u % 3 == 0 ? bq[0] : u % 3 == 1 ? bq[1] : bqx;
                    uint4 (&bn)[2][2] = (u + 2) % 3 == 0 ? bq[0] : (u + 2) % 3 == 1 ? bq[1] : bqx;
                    // refill: k-step ks + 2 into the slot consumed one unit ago; the tile's last two units leave k-step 0 in slot 0
                    if (u < 4) ring_load(bn, __builtin_amdgcn_readfirstlane(6 * ki + u + 2));
                    else if (u == 4) ring_load(bn, __builtin_amdgcn_readfirstlane(ki < 2 ? 6 * ki + 6 : 0));
                    else if (ki < 2) ring_load(bn, __builtin_amdgcn_readfirstlane(6 * ki + 7));
                    if (u < 5) {                               // next unit: same tap row
                        if (u & 1) {
                            tap_consts(ki, kj + 1, om);
                            load_a(ki, 0, om, ahA, alA);
                        } else {
                            load_a(ki, 1, om, ahB, alB);
                        }
                    } else if (ki < 2) {                       // first unit of the next tap row (u = 5 is odd: set A)
                        tap_consts(ki + 1, 0, om);
                        load_a(ki + 1, 0, om, ahA, alA);
                    }
#pragma unroll
                    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                        for (int m = 0; m < 4; ++m)
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt) {
                                const bf16x8 bh = __builtin_bit_cast(bf16x8, bs[nt][0]);
                                const bf16x8 bl = __builtin_bit_cast(bf16x8, bs[nt][1]);
                                f32x4v &c = acc[m][nt];
                                const bf16x8 ah = half ? ahB[m] : ahA[m], al = half ? alB[m] : alA[m];
                                if (pr == 0) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
                                else if (pr == 1) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
                                else c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
                            }
#pragma unroll
                    for (int i = 0; i < 24; ++i) {             // the whole tile's placement of the 8 fragment reads and 4 ring loads
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (i % 3 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        else if (i == 1 || i == 2 || i == 4 || i == 5) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }

            // epilogue.  The whole tile's lane sums rows 0 .. 7 x its 4 columns in order, then adds lane ^ 16.  Here lanes ckg 0/1 hold
            // the even rows and ckg 2/3 the odd rows of those columns: bn_relu where the value lives, then one v_permlane32_swap per
            // register pair (nt 0, nt 1) leaves the low half-wave with both row parities of channel o0 and the high one with those
            // of o0 + 16 -- ev = rows 2m, od = rows 2m + 1 -- and the adds run in the whole tile's order.
            float sum = 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                float ev[4], od[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned int va = __builtin_bit_cast(unsigned int, bn_relu(acc[m][0][i], s2a, t2a));
                    const unsigned int vb = __builtin_bit_cast(unsigned int, bn_relu(acc[m][1][i], s2b, t2b));
                    const auto sw = __builtin_amdgcn_permlane32_swap(va, vb, false, false);   // va's high lanes <-> vb's low lanes
                    ev[i] = __builtin_bit_cast(float, (unsigned int)sw[0]);
                    od[i] = __builtin_bit_cast(float, (unsigned int)sw[1]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) sum += ev[i];
#pragma unroll
                for (int i = 0; i < 4; ++i) sum += od[i];
            }
            const float other = __shfl_xor(sum, 16);
            const float total = (ckg & 1) == 0 ? sum + other : other + sum;       // a+b == b+a: both lanes agree bitwise
            if ((ckg & 1) == 0) features[out_index(r0 / 8, c0 / 8 + side, o0 + 16 * (ckg >> 1))] = total * (1.0f / 64);
        } else {
            if (abl_conv1) {
                bf16x8 xh[4], xl[4];
                int pix; bool valid, inimg;
                x_frags(wave, xh, xl, pix, valid, inimg);
                f32x16 acc0, acc1;
                conv1_both<true>(w1s, xh, xl, acc0, acc1);
                conv1_store(acc0, 0, pix, valid, inimg);
                conv1_store(acc1, 1, pix, valid, inimg);
            }
            if (abl_conv1) {
                bf16x8 xh[4], xl[4];
                int pix; bool valid, inimg;
                const int cb = wave & 1;
                x_frags(4 + (wave >> 1), xh, xl, pix, valid, inimg);
                f32x16 acc;
                conv1_one<true>(w1s, cb, xh, xl, acc);
                conv1_store(acc, cb, pix, valid, inimg);
            }
#if !defined(SMK_ENC_ABLATE) || !(SMK_ENC_ABLATE & 4)
            __syncthreads();                                      // a1 complete; xs is free again
#endif
            __builtin_amdgcn_s_setprio(S16_PRIO_KLOOP);

            wk.next(skl, sa, src, xr0, xr1);                      // next tile's x halo -> registers (lands under the K loop)

            // ---- conv2: acc[mt][nt][reg] = D(pixel row mt, column 4 kg + reg; channel 16 nt + px of the wave's 32)
            f32x4v acc[8][2];
#pragma unroll
            for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[mt][nt][g] = 0.f;
            // unit k (0..35) = tap * 4 + half * 2 + hm: M tiles 4hm .. 4hm+3 of k-step ks = k >> 1 = tap * 2 + half.  The loop runs over
            // the 9 taps (runtime) x 4 unrolled units.  Per tap four lane registers om[m] = pixel base ^ swizzle term of row m + ki
            // are formed once (the base is a multiple of 128 and the term < 128, so base + (c ^ t) = base ^ t ^ c): a fragment pair then
            // costs ONE xor, and the row offsets ki * 2304 (scalar) and 4hm * 2304 + m * 2304 (ds_read immediate) are free.
            const int c16[2] = {kg << 4, (4 + kg) << 4};
            auto tap_consts = [&](int ki, int kj, int (&om)[4]) {
#pragma unroll
                for (int m = 0; m < 4; ++m) om[m] = ((px + kj) << 7) ^ (((px + kj + 2 * (m + ki)) & 7) << 4);
            };
            auto load_a = [&](int ki, int half, int hm, const int (&om)[4], bf16x8 (&ah)[4], bf16x8 (&al)[4]) {
                const unsigned char *ph = a1h + ki * (B3_AW * 128), *pl = a1l + ki * (B3_AW * 128);      // wave-uniform part
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int off = om[m] ^ c16[half];
                    ah[m] = *reinterpret_cast<const bf16x8 *>(ph + off + (4 * hm + m) * (B3_AW * 128));
                    al[m] = *reinterpret_cast<const bf16x8 *>(pl + off + (4 * hm + m) * (B3_AW * 128));
                }
            };
            bf16x8 ahA[4], alA[4], ahB[4], alB[4];
            int om[4];
            tap_consts(0, 0, om);
            load_a(0, 0, 0, om, ahA, alA);
            int ki = 0, kj = 0;
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int half = u >> 1, hm = u & 1, slot = half % RING;
                    if (hm == 0) {
                        // refill: k-step ks + 1 into the slot consumed one k-step ago.  All four fragments (both N tiles, hi and lo) are
                        // requested in the FIRST unit of the k-step, right at its start: two units (768 cycles) before their first use.
                        // Measured placements of the ring loads within a unit: early 1.06 ms, middle 1.075, late 1.11.
                        int kn = tap * 2 + half + RING - 1;
                        kn = kn >= 18 ? kn - 18 : kn;
                        kn = __builtin_amdgcn_readfirstlane(kn);
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) {
                            bq[(slot + RING - 1) % RING][nt][0] = load_b(kn, 0, nt);
                            bq[(slot + RING - 1) % RING][nt][1] = load_b(kn, 1, nt);
                        }
                    }
                    if (u < 3) {                                   // next unit: same tap
                        if (u & 1) load_a(ki, (u + 1) >> 1, (u + 1) & 1, om, ahA, alA);
                        else load_a(ki, (u + 1) >> 1, (u + 1) & 1, om, ahB, alB);
                    } else if (tap < 8) {                          // first unit of the next tap (u = 3 is odd: set A)
                        kj = kj == 2 ? 0 : kj + 1;
                        ki = kj == 0 ? ki + 1 : ki;
                        tap_consts(ki, kj, om);
                        load_a(ki, 0, 0, om, ahA, alA);
                    }
                    // product-major emission: consecutive MFMAs go to different accumulators (dependency distance 8 instead of 1); each
                    // accumulator still sums lo*hi, hi*lo, hi*hi in that order, so results are bitwise those of the chain-major form
#pragma unroll
                    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                        for (int m = 0; m < 4; ++m)
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt) {
                                const bf16x8 bh = __builtin_bit_cast(bf16x8, bq[slot][nt][0]);
                                const bf16x8 bl = __builtin_bit_cast(bf16x8, bq[slot][nt][1]);
                                f32x4v &c = acc[4 * hm + m][nt];
                                const bf16x8 ah = (u & 1) ? ahB[m] : ahA[m], al = (u & 1) ? alB[m] : alA[m];
#if defined(SMK_ENC_ABLATE) && (SMK_ENC_ABLATE & 8)
                                asm volatile("" :: "v"(al), "v"(ah), "v"(bh), "v"(bl), "v"(c));      // operands stay live, no MFMA
#else
                                if (pr == 0) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
                                else if (pr == 1) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
                                else c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
#endif
                            }
                    // 24 MFMAs of 16 cycles.  The next unit's 8 fragment reads are spread evenly, one after every third MFMA; the ring loads
                    // go right behind the first MFMAs.  (One read per second MFMA in the first 16 -- what hipcc also does unpinned -- is
                    // 4 % slower; see DESIGN.md 3.2 for the placements measured.)
#pragma unroll
                    for (int i = 0; i < 24; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (i % 3 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        else if (hm == 0 && (i == 1 || i == 2 || i == 4 || i == 5)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }

            // ---- epilogue: BN2 + ReLU + block-mean pool.  Lane: channel o0 (nt 0) / o0 + 16 (nt 1), pixels (row mt, cols 4kg .. 4kg+3)
#if defined(SMK_ENC_ABLATE) && (SMK_ENC_ABLATE & 2)
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) asm volatile("" :: "v"(acc[mt][0]), "v"(acc[mt][1]));
            if (false)
#endif
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const float s2 = nt ? s2b : s2a, t2 = nt ? t2b : t2a;
                const int o = o0 + 16 * nt;
                if (PS == 2) {          // cells: rows (mt, mt+1), column pairs (reg 0,1), (reg 2,3)
#pragma unroll
                    for (int mp = 0; mp < 4; ++mp)
#pragma unroll
                        for (int cg = 0; cg < 2; ++cg) {
                            float sum = 0.f;
#pragma unroll
                            for (int mt = 2 * mp; mt < 2 * mp + 2; ++mt)
#pragma unroll
                                for (int i = 2 * cg; i < 2 * cg + 2; ++i) sum += bn_relu(acc[mt][nt][i], s2, t2);
                            features[out_index((r0 + 2 * mp) / 2, (c0 + 4 * kg + 2 * cg) / 2, o)] = sum * 0.25f;
                        }
                } else if (PS == 4) {   // cells: rows 4mq .. 4mq+3, columns 4kg .. 4kg+3 (all four registers)
#pragma unroll
                    for (int mq = 0; mq < 2; ++mq) {
                        float sum = 0.f;
#pragma unroll
                        for (int mt = 4 * mq; mt < 4 * mq + 4; ++mt)
#pragma unroll
                            for (int i = 0; i < 4; ++i) sum += bn_relu(acc[mt][nt][i], s2, t2);
                        features[out_index((r0 + 4 * mq) / 4, (c0 + 4 * kg) / 4, o)] = sum * (1.0f / 16);
                    }
                } else if (PS >= 16) {  // frames beyond 256^2: the PS == 8 sum, then one more step over kg for the whole tile's partial
                    float sum = 0.f;
#pragma unroll
                    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) sum += bn_relu(acc[mt][nt][i], s2, t2);
                    const float half8 = sum + __shfl_xor(sum, 16);             // a+b == b+a at each step: all four lanes agree bitwise
                    const float total = half8 + __shfl_xor(half8, 32);
                    if (kg == 0) features[(size_t)wk.t * 128 + o] = total;
                } else {                // PS == 8: all 8 rows; columns 0-7 = kg 0,1, columns 8-15 = kg 2,3 (lane ^ 16 holds the other half)
                    float sum = 0.f;
#pragma unroll
                    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) sum += bn_relu(acc[mt][nt][i], s2, t2);
                    const float other = __shfl_xor(sum, 16);
                    const float total = (kg & 1) == 0 ? sum + other : other + sum;   // a+b == b+a: both lanes agree bitwise
                    if ((kg & 1) == 0) features[out_index(r0 / 8, c0 / 8 + (kg >> 1), o)] = total * (1.0f / 64);
                }
            }
        }

        halo_to_lds(xs, xr0, xr1, pack_split);
#if !defined(SMK_ENC_ABLATE) || !(SMK_ENC_ABLATE & 4)
        __syncthreads();
#endif
        wk.advance();
    }
    wk.template end<PS, TOKENS>(sa, src, features);
}

// Diagnostic switches, read once per process: SMK_ENC_STAGGER (s_sleep units of the second workgroup wave, default 1),
// SMK_ENC_WGS_PER_CU (override the occupancy query), SMK_ENC_SHAPE=32 (split-bf16 on the 32x32x16 kernel instead of 16x16x32),
// SMK_ENC_SKIP=0 (every tile runs: no tile scan, see below), SMK_ENC_CELLS=0 (the skip decides per tile only: a live tile runs whole).
struct EncoderKnobs {
    int stagger, wgs_per_cu, shape;
    bool skip, cells;
    EncoderKnobs() {
        const char *sv = getenv("SMK_ENC_STAGGER"), *ov = getenv("SMK_ENC_WGS_PER_CU"), *sh = getenv("SMK_ENC_SHAPE");
        const char *sk = getenv("SMK_ENC_SKIP"), *ce = getenv("SMK_ENC_CELLS");
        cells = !(ce && atoi(ce) == 0);
        stagger = sv ? atoi(sv) : 1;
        wgs_per_cu = ov && atoi(ov) > 0 ? atoi(ov) : 0;
        shape = sh && atoi(sh) == 32 ? 32 : 16;
        skip = !(sk && atoi(sk) == 0);
    }
};
static const EncoderKnobs &enc_knobs() {
    static const EncoderKnobs k;
    return k;
}

// ---------------------------------------------------------------- tile skip: input windows that are all zero
// A tile's result depends on its 16 x 24 input window (tile + 4 pixels each way, outside the image = zero) and on its position in the
// frame, nothing else.  A tile whose window is all zero therefore equals the same tile of an all-zero frame, bit for bit, and the
// simulator's frames are mostly background.  Two launches per call:
//   k_encoder_tile_scan       one workgroup per band of ROWS = scan_rows_for(tiles_x) tile rows of a frame.  Reads the band's 8 ROWS + 8 image rows once
//          (16-byte loads when the frames allow), keeps one flag per 4 x 4 pixel block in LDS (window edges fall on multiples of 4),
//          ORs 4 x 6 flags per tile.  EMPTY means every 32-bit word of the window inside the image is 0x00000000: bits are compared,
//          so -0.0, denormals, NaN and Inf all keep a tile on the normal path.  The band's non-empty tiles go out as one 64-bit
//          mask, beside two more words of the same form: the tiles whose left 4 x 4 flags are not all empty, and those whose right
//          4 x 4 are not (the two overlap by two flag columns; at 256^2 they are the windows of the tile's two pooled cells, and
//          k_encoder_b16 runs a tile with one live cell at half size: "per pooled cell" above).  That is all it writes.
//   the main kernel (k_encoder_b16, k_encoder_bf16, k_encoder_i8) reads the masks: tiles_to_run / tile_at turn them into "my k-th
//          tile" inside every workgroup (no list in memory, no pack launch), skip_fill copies the empty tiles' pooled cells from the
//          handle's zero-response table (the same kernel form's output for one all-zero frame, in the layout of the call) outside the
//          tile loop, and workgroup 0 stores the number of tiles run for smk_encoder_skip_stats.
// Every word the main kernel reads is rewritten by the scan of the same call, so nothing needs a reset, nothing is read back by the
// host, the walk is the same on every run, and both launches are capturable.  No workgroup waits for another one; the kernel
// boundary orders scan and main kernel.
template <bool VEC, int ROWS>
__global__ __launch_bounds__(256) void k_encoder_tile_scan(const float *__restrict__ frames, int64_t fstride, int H, int W, int lg_tiles_x,
                                                           int bands_per_frame, unsigned long long *__restrict__ masks,
                                                           unsigned long long *__restrict__ cell_l, unsigned long long *__restrict__ cell_r) {
    constexpr int SCAN_ROWS = ROWS;
    constexpr int SCAN_BR = 2 * ROWS + 2;                     // 4-row flag blocks per band (the band's rows + 4 each way)
    constexpr int SCAN_FW = 1024 / ROWS / 4 + 2;              // flag columns: the 4-pixel blocks of the widest frame with ROWS rows per
                                                              // band (W = 256, 512, 1024 for ROWS = 4, 2, 1) + one pad each side
    __shared__ unsigned int flag[SCAN_BR][SCAN_FW];
    const int tid = threadIdx.x;
    const int band = blockIdx.x, b = band / bands_per_frame, bi = band - b * bands_per_frame;
    const int tiles_x = 1 << lg_tiles_x, band_tiles = SCAN_ROWS * tiles_x;
    for (int i = tid; i < SCAN_BR * SCAN_FW; i += 256) (&flag[0][0])[i] = 0;
    __syncthreads();
    const int W4 = W >> 2, row0 = bi * (SCAN_ROWS * B3_TH) - 4;
    const unsigned int *src = reinterpret_cast<const unsigned int *>(frames) + (size_t)b * fstride;
    for (int i = tid; i < SCAN_BR * 4 * W4; i += 256) {
        const int rr = i / W4, c4 = i - rr * W4, row = row0 + rr;
        if (row < 0 || row >= H) continue;
        const unsigned int *p = src + (size_t)row * W + 4 * c4;
        unsigned int any;
        if (VEC) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            any = v.x | v.y | v.z | v.w;
        } else {
            any = p[0] | p[1] | p[2] | p[3];
        }
        if (any) flag[rr >> 2][c4 + 1] = 1;                   // racing writers all store the same value
    }
    __syncthreads();
    if (tid < 64) {                                           // wave 0: one lane per tile of the band
        unsigned int any[2] = {0, 0};                         // the tile's two 16-column halves with 4 more each way (encoder_cells.h):
        if (tid < band_tiles) {                               // at 256^2 its two cells' windows; their union is the tile's at any size
            const int tyl = tid >> lg_tiles_x, tx = tid & (tiles_x - 1);
#pragma unroll
            for (int side = 0; side < 2; ++side)
#pragma unroll
                for (int br = 0; br < 4; ++br)
#pragma unroll
                    for (int bc = 0; bc < ENC_CELL_FLAG_COLS; ++bc) any[side] |= flag[2 * tyl + br][enc_cell_flag_col(tx, side) + bc];
        }
        const unsigned long long l = __ballot(any[0] != 0), r = __ballot(any[1] != 0);
        if (tid == 0) {
            masks[band] = enc_cells_tile(l, r);
            cell_l[band] = l;
            cell_r[band] = r;
        }
    }
}

void EncoderSkip::release() {
    for (auto &f : table)
        for (auto &h : f)
            for (float *&t : h) {
                if (t) (void)hipFree(t);
                t = nullptr;
            }
    if (ws) (void)hipFree(ws);
    for (void *p : retired) (void)hipFree(p);
    retired.clear();
    ws = nullptr;
    ws_bands = 0;
    last_count = nullptr;
}

hipError_t encoder_skip_stats(EncoderSkip &sk, int64_t *tiles_total, int64_t *tiles_run, hipStream_t st) {
    std::lock_guard<std::mutex> lk(sk.mu);
    hipError_t err = hipStreamSynchronize(st);
    if (err != hipSuccess) return err;
    int n = 0;
    if (sk.last_count && (err = hipMemcpy(&n, sk.last_count, sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) return err;
    *tiles_total = sk.last_total;
    *tiles_run = sk.last_count ? n : sk.last_total;
    return hipSuccess;
}

// Decides between the direct and the skip path of one forward call and, for the skip path, launches the scan.  FORM: 0 split-bf16,
// 1 single-pass bf16, 2 int8 limbs (one zero-response table each, per frame size and layout).  zero_launch(zero_frame, table) runs
// the call's own kernel form on the direct path over one all-zero frame.  Direct when the call has no more tiles than workgroups (one
// round either way: the scan could only cost), when SMK_ENC_SKIP=0, when `features` is not 16-byte aligned, and while the stream is
// capturing unless table and workspace already exist (nothing is allocated inside a capture).  Outgrown workspaces are kept until the
// handle is destroyed: a captured graph may still name them.
template <int FORM, bool TOKENS, class ZeroLaunch>
static hipError_t skip_prepare(EncoderSkip *sk, const float *frames, int64_t fstride, int B, int H, int W, float *features, int lg_tx,
                               int ntiles, int nwg, hipStream_t st, ZeroLaunch zero_launch, SkipArgs &plan) {
    if (!sk) return hipSuccess;
    std::lock_guard<std::mutex> lk(sk->mu);
    sk->last_total = ntiles;
    sk->last_count = nullptr;
    if (!enc_knobs().skip || ntiles <= nwg || (reinterpret_cast<uintptr_t>(features) & 15)) return hipSuccess;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return hipSuccess;
    }
    const bool capturing = cs != hipStreamCaptureStatusNone;
    hipError_t err;
    const bool part = H / 32 >= 16;                           // `features` is the partial buffer: one table layout
    const int hidx = H == 64 ? 0 : H == 128 ? 1 : H == 256 ? 2 : H == 512 ? 3 : 4;
    if (H != 64 && H != 128 && H != 256 && H != 512 && H != 1024) return hipErrorInvalidValue;
    float *&tab = sk->table[FORM][hidx][TOKENS && !part ? 1 : 0];
    if (!tab) {
        if (capturing) return hipSuccess;
        // [table: 1024 x 128 features, or the frame's per-tile partials][zero frame H x W]
        const size_t tfloats = part ? (size_t)(H / B3_TH) * (W / B3_TW) * 128 : (size_t)ENC_FRAME_FEATS;
        float *p = nullptr;
        if ((err = hipMalloc((void **)&p, (tfloats + (size_t)H * W) * sizeof(float))) != hipSuccess) return err;
        err = hipMemsetAsync(p + tfloats, 0, (size_t)H * W * sizeof(float), st);
        if (err == hipSuccess) err = zero_launch(p + tfloats, p);
        if (err != hipSuccess) {
            (void)hipFree(p);
            return err;
        }
        tab = p;
    }
    const int scan_rows = scan_rows_for(1 << lg_tx);
    const int bands_per_frame = H / B3_TH / scan_rows, nbands = B * bands_per_frame;
    if (sk->ws_bands < (size_t)nbands) {
        if (capturing) return hipSuccess;
        int *p = nullptr;                                     // [tiles run + pad: 4][band masks, left-cell words, right-cell words: 2 per band each]
        if ((err = hipMalloc((void **)&p, (4 + 6 * (size_t)nbands) * sizeof(int))) != hipSuccess) return err;
        if (sk->ws) sk->retired.push_back(sk->ws);
        sk->ws = p;
        sk->ws_bands = nbands;
    }
    int *count = sk->ws;
    // three arrays of the call's band count each: scan and main kernel of one call (or of one captured graph) get the same pointers
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(sk->ws + 4);
    unsigned long long *cell_l = masks + nbands, *cell_r = cell_l + nbands;
    const bool vec = (reinterpret_cast<uintptr_t>(frames) & 15) == 0 && (fstride & 3) == 0;
    dim3 grid(nbands), block(256);
    auto scan = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, st, frames, fstride, H, W, lg_tx, bands_per_frame, masks, cell_l, cell_r);
    };
    switch (scan_rows) {
        case 4: vec ? scan(k_encoder_tile_scan<true, 4>) : scan(k_encoder_tile_scan<false, 4>); break;
        case 2: vec ? scan(k_encoder_tile_scan<true, 2>) : scan(k_encoder_tile_scan<false, 2>); break;
        default: vec ? scan(k_encoder_tile_scan<true, 1>) : scan(k_encoder_tile_scan<false, 1>); break;
    }
    if ((err = hipGetLastError()) != hipSuccess) return err;
    plan.masks = masks;
    // SMK_ENC_CELLS=0: both cell words are the tile mask, i.e. every live tile has two live cells and runs whole
    plan.cell_l = enc_knobs().cells ? cell_l : masks;
    plan.cell_r = enc_knobs().cells ? cell_r : masks;
    plan.count = count;
    plan.nbands = nbands;
    plan.lg_band_tiles = lg_tx + 2 < 6 ? lg_tx + 2 : 6;      // scan_rows x tiles_x tiles, at most one mask word
    plan.table = tab;
    plan.bands_per_frame = bands_per_frame;
    sk->last_count = count;
    return hipSuccess;
}

// ---------------------------------------------------------------- fused encoder, int8 fixed-point MFMA ("i8x3")
// conv1 as in the split-bf16 kernel; its fp32 outputs stay in registers until the tile's maximum is known, then every
// a1 value (>= 0 after the ReLU) is quantised to UNSIGNED 16-bit fixed point with the TILE's scale,
// q = rint(y * 65024 / max) = 256 (h + 128) + l with int8 limbs h, l in [-128, 127]; the offset is undone exactly in the
// epilogue by adding 128 * sum_k w[o][k] (precomputed integers) to the accumulators.  Limbs are stored as
// [halo row][pixel][64 ch] bytes (pixel pitch 80 B, row pitch 1472 B: conflict-free b128 reads).
// conv2 runs on v_mfma_i32_32x32x32_i8 (2x the bf16 rate, K = 32 channels per instruction) with EXACT i32 accumulation
// in two weight classes: acc_hh += ah*wh (x 2^16), acc_mid += ah*wl + al*wh (x 2^8); the l*l class (2^-16 relative) is
// dropped.  Result = ((hh + Ch[o])*65536 + (mid + Cl[o])*256) * s_tile * sw2[o].  216 MFMAs per wave-tile instead of 432, half the LDS and
// L2 operand bytes.  Accuracy is fixed-point (absolute error ~ tile max * 2^-16): features within 1e-4 of the reference
// on every fixture (2e-5 .. 7e-5), tighter than bf16 but looser than bf16x3 (3e-6) -- opt-in.
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int I8_A1_PITCH = 80;                           // bytes per halo pixel: 64 ch + 16 pad (5 x 16 B: odd)
constexpr int I8_A1_ROW = B3_AW * I8_A1_PITCH + 32;       // 1472 B: 4 rows = 368 x 16 B = 0 mod 16 units
constexpr int I8_A1_BYTES = (B3_TH + 2) * I8_A1_ROW;      // 14720 per limb
constexpr int I8_LDS_BYTES = B3_XS_BYTES + 2 * I8_A1_BYTES + 2 * B3_W1_BYTES + B3_ST_BYTES + 64;   // ~50.2 KB

template <int PS, bool TOKENS>
__global__ __launch_bounds__(256, 2) void k_encoder_i8(const float *__restrict__ frames, int64_t fstride, int H, int W,
                                                    EncoderDev e, float *__restrict__ features, int lg_tiles_x,
                                                    int lg_tiles_per_frame, int ntiles,
                                                    SkipArgs sa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);
    unsigned char *a1h = smem + B3_XS_BYTES, *a1l = a1h + I8_A1_BYTES;
    unsigned char *w1s = a1l + I8_A1_BYTES;
    float *st1 = reinterpret_cast<float *>(w1s + 2 * B3_W1_BYTES);
    float *wmx = st1 + 128;                                 // per-wave maxima (4 floats) + padding
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    conv1_stage<2>(e, w1s, st1);
    const int o = wave * 32 + r;
    const float t2 = e.t2[o];
    const float scale_o = e.sw2[o] * e.s2[o];               // weight scale x BN2 scale (tile scale multiplies in later)
    const int corr_h = e.wsum[o], corr_l = e.wsum[128 + o];   // 128 * sum of the weight limbs: undoes the activation offset
    const int lane_b = (o * 2 + hi) * 16;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<signed char *>(e.w2i), 0, 18 * 2 * 4096, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto load_b = [&](int kn, int part) -> i32x4 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane_b, (kn * 2 + part) * 4096, 0);
        return __builtin_bit_cast(i32x4, v);
    };
    constexpr int RING = 3;
    i32x4 bqh[RING], bql[RING];
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) {
        bqh[k] = load_b(k, 0);
        bql[k] = load_b(k, 1);
    }
    const int lane_off = (r >> 4) * 4 * I8_A1_ROW + (r & 15) * I8_A1_PITCH + 16 * hi;

    const TileSrc src{frames, fstride, H, W, lg_tiles_x, lg_tiles_per_frame};
    __shared__ SkipLds<false> skl;
    TileWalk<> wk;
    wk.begin<PS, TOKENS>(skl, sa, src, ntiles, 0, features, xs, [](float v) { return v; });   // this kernel does not stagger

    // [stamp:begin]
    for (; wk.k < wk.nrun; wk.k += gridDim.x) {
        // [stamp:T0]
        int b, r0, c0;
        src.decode(wk.t, b, r0, c0);

        __builtin_amdgcn_s_setprio(0);
        // ---- conv1 (split-bf16 MFMA): 3 (pixel block, channel block) units per wave, fp32 results kept in registers
        float yv[3][16];
        int aoffs[2];
        bool valids[2];
        float vmax = 0.f;
        bool inimgs[2];
        auto bn1 = [&](const f32x16 &acc, int cb, bool inimg, float (&y)[16]) {
            float umax = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ch0 = cb * 32 + 8 * q + 4 * hi;
                const float4 sc = *reinterpret_cast<const float4 *>(st1 + ch0);
                const float4 sh = *reinterpret_cast<const float4 *>(st1 + 64 + ch0);
                const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = bn_relu(acc[4 * q + i], scv[i], shv[i]);
                    y[4 * q + i] = v;
                    umax = fmaxf(umax, v);
                }
            }
            vmax = fmaxf(vmax, inimg ? umax : 0.f);           // pixels outside the image are conv2's zero padding
        };
        {
            bf16x8 xh[4], xl[4];
            bool inimg;
            x_frags<I8_A1_ROW, I8_A1_PITCH>(xs, wave, r0, c0, H, W, xh, xl, aoffs[0], valids[0], inimg);
            inimgs[0] = inimg;
            f32x16 acc0, acc1;
            conv1_both<true>(w1s, xh, xl, acc0, acc1);
            bn1(acc0, 0, inimg, yv[0]);
            bn1(acc1, 1, inimg, yv[1]);
        }
        const int cbs = wave & 1;
        {
            bf16x8 xh[4], xl[4];
            bool inimg;
            x_frags<I8_A1_ROW, I8_A1_PITCH>(xs, 4 + (wave >> 1), r0, c0, H, W, xh, xl, aoffs[1], valids[1], inimg);
            inimgs[1] = inimg;
            f32x16 acc;
            conv1_one<true>(w1s, cbs, xh, xl, acc);
            bn1(acc, cbs, inimg, yv[2]);
        }
        // [stamp:T1]
        // ---- tile maximum -> fixed-point scale
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off));
        if (lane == 0) wmx[wave] = vmax;
        __syncthreads();
        // [stamp:T2]
        const float tmax = fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3]));
        // q' = rint(y * 65024 / max) + 128 as packed u16 (v_cvt_pknorm_u16_f32: round(x * 65535) of x in [0,1]);
        // q' = 256 hu + lo, stored limbs h = hu - 128 and l = lo - 128 are the bytes XOR 0x80 (v_perm_b32 gathers them)
        const float invn = tmax > 0.f ? 65024.0f / (tmax * 65535.0f) : 0.f;
        const float s_tile = tmax > 0.f ? tmax / 65024.0f : 0.f;
        constexpr float OFFN = 128.0f / 65535.0f;
        auto quant_store = [&](const float (&y)[16], int cb, int aoff, bool valid, bool inimg) {
            if (!valid) return;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ch0 = cb * 32 + 8 * q + 4 * hi;
                const unsigned int d0 = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_pknorm_u16(
                    fmaf(y[4 * q + 0], invn, OFFN), fmaf(y[4 * q + 1], invn, OFFN)));
                const unsigned int d1 = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_pknorm_u16(
                    fmaf(y[4 * q + 2], invn, OFFN), fmaf(y[4 * q + 3], invn, OFFN)));
                unsigned int ph = __builtin_amdgcn_perm(d1, d0, 0x07050301) ^ 0x80808080u;   // high bytes of the 4 u16
                unsigned int pl = __builtin_amdgcn_perm(d1, d0, 0x06040200) ^ 0x80808080u;   // low bytes
                ph = inimg ? ph : 0x80808080u;                                               // q = 0 (zero padding)
                pl = inimg ? pl : 0u;
                *reinterpret_cast<unsigned int *>(a1h + aoff + ch0) = ph;
                *reinterpret_cast<unsigned int *>(a1l + aoff + ch0) = pl;
            }
        };
        quant_store(yv[0], 0, aoffs[0], valids[0], inimgs[0]);
        quant_store(yv[1], 1, aoffs[0], valids[0], inimgs[0]);
        quant_store(yv[2], cbs, aoffs[1], valids[1], inimgs[1]);
        // [stamp:T3]
        __syncthreads();                                      // a1 limbs complete; xs is free again
        __builtin_amdgcn_s_setprio(1);                        // K loop at raised priority (see k_encoder_bf16)
        // [stamp:T4]

        float xr0, xr1;                                       // next tile's x halo -> registers (lands under the K loop)
        wk.next(skl, sa, src, xr0, xr1);

        // ---- conv2 on int8 MFMA: 18 k-steps (tap, channel half) x 4 M blocks x 3 limb products
        i32x16 hh[4], mid[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int g = 0; g < 16; ++g) { hh[mi][g] = corr_h; mid[mi][g] = corr_l; }   // offset correction pre-added
        auto load_a = [&](int k, int pair, i32x4 (&ah)[2], i32x4 (&al)[2]) {
            const int tap = k >> 1, half = k & 1, ki = tap / 3, kj = tap - 3 * ki;
            const int abase = lane_off + ki * I8_A1_ROW + kj * I8_A1_PITCH + half * 32 + pair * 2 * I8_A1_ROW;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                ah[m] = *reinterpret_cast<const i32x4 *>(a1h + abase + m * I8_A1_ROW);
                al[m] = *reinterpret_cast<const i32x4 *>(a1l + abase + m * I8_A1_ROW);
            }
        };
        i32x4 ahA[2], alA[2], ahB[2], alB[2];
        load_a(0, 0, ahA, alA);
#pragma unroll 1
        for (int k0 = 0; k0 < 18; k0 += 6) {
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int k = k0 + u;
                {
                    int kn = k + RING - 1;
                    kn = kn >= 18 ? kn - 18 : kn;
                    kn = __builtin_amdgcn_readfirstlane(kn);
                    bqh[(u + RING - 1) % RING] = load_b(kn, 0);
                    bql[(u + RING - 1) % RING] = load_b(kn, 1);
                }
                const i32x4 bh = bqh[u % RING], bl = bql[u % RING];
                // half-step 0: M blocks 0,1 from buffer A while buffer B loads M blocks 2,3 of this k-step
                load_a(k, 1, ahB, alB);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    mid[m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(alA[m], bh, mid[m], 0, 0, 0);
                    mid[m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ahA[m], bl, mid[m], 0, 0, 0);
                    hh[m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ahA[m], bh, hh[m], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (i < 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    else __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // half-step 1: M blocks 2,3 from buffer B while buffer A loads M blocks 0,1 of the next k-step
                if (k + 1 < 18) load_a(k + 1, 0, ahA, alA);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    mid[2 + m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(alB[m], bh, mid[2 + m], 0, 0, 0);
                    mid[2 + m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ahB[m], bl, mid[2 + m], 0, 0, 0);
                    hh[2 + m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ahB[m], bh, hh[2 + m], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (i < 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // [stamp:T5]
        // ---- epilogue: (hh*2^16 + mid*2^8) * s_tile * sw2[o] -> BN2 + ReLU + block mean
        const float sc = s_tile * scale_o * 256.0f;
        auto val = [&](int mi, int g) -> float {
            const float v = fmaf((float)hh[mi][g], 256.0f, (float)mid[mi][g]);        // (hh*2^16 + mid*2^8) / 2^8
            const float y = fmaf(v, sc, t2);
            return y > 0.f ? y : 0.f;
        };
        pool_store_32<PS, TOKENS>(features, b, o, r0, c0, wk.t, val);

        halo_to_lds(xs, xr0, xr1, [](float v) { return v; });
        // [stamp:T6]
        __syncthreads();
        // [stamp:T7]
        // [stamp:accumulate]
        wk.advance();
    }
    // [stamp:end]
    wk.end<PS, TOKENS>(sa, src, features);
}

// ---------------------------------------------------------------- launching the persistent kernels
// A kernel family for the launcher: its instantiation for <PS, TOKENS>, its dynamic LDS, its skip_prepare FORM (the zero-response
// table it fills) and whether it takes the stagger argument.
struct FormB16 {
    static constexpr int FORM = 0, LDS = S16_LDS;
    static constexpr bool STAGGERS = true;
    template <int PS, bool TOKENS> static constexpr auto kernel = &k_encoder_b16<PS, TOKENS>;
};
template <bool X3>
struct FormBf16 {
    static constexpr int FORM = X3 ? 0 : 1, LDS = b3_lds_total<X3>();
    static constexpr bool STAGGERS = true;
    template <int PS, bool TOKENS> static constexpr auto kernel = &k_encoder_bf16<X3, PS, TOKENS>;
};
struct FormI8 {
    static constexpr int FORM = 2, LDS = I8_LDS_BYTES;
    static constexpr bool STAGGERS = false;
    template <int PS, bool TOKENS> static constexpr auto kernel = &k_encoder_i8<PS, TOKENS>;
};

template <class F, bool TOKENS>
static hipError_t launch_persistent(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e, float *features,
                                    hipStream_t st, EncoderSkip *skip, float *partials) {
    const int PS = H / 32;
    const int tiles_x = W / B3_TW, tiles_per_frame = tiles_x * (H / B3_TH), ntiles = B * tiles_per_frame;
    int lg_tx = 0, lg_tpf = 0;
    while ((1 << lg_tx) < tiles_x) ++lg_tx;
    while ((1 << lg_tpf) < tiles_per_frame) ++lg_tpf;
    if ((1 << lg_tx) != tiles_x || (1 << lg_tpf) != tiles_per_frame || (PS != 2 && PS != 4 && PS != 8 && PS != 16 && PS != 32))
        return hipErrorInvalidValue;                          // H = W in {64,128,256,512,1024}
    const bool part = PS >= 16;                               // the main kernel writes per-tile partials, the pooling kernel the features
    if (part && !partials) return hipErrorInvalidValue;
    const int stagger = enc_knobs().stagger;
    const int num_cu = device_num_cu();
    const int wgs_per_cu = device_cached_int((const void *)F::template kernel<8, TOKENS>, [] {
        (void)hipFuncSetAttribute((const void *)F::template kernel<8, TOKENS>, hipFuncAttributeMaxDynamicSharedMemorySize, F::LDS);
        (void)hipFuncSetAttribute((const void *)F::template kernel<4, TOKENS>, hipFuncAttributeMaxDynamicSharedMemorySize, F::LDS);
        (void)hipFuncSetAttribute((const void *)F::template kernel<2, TOKENS>, hipFuncAttributeMaxDynamicSharedMemorySize, F::LDS);
        (void)hipFuncSetAttribute((const void *)F::template kernel<16, false>, hipFuncAttributeMaxDynamicSharedMemorySize, F::LDS);
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)F::template kernel<8, TOKENS>, 256, F::LDS) != hipSuccess || n < 1) n = 2;
        return enc_knobs().wgs_per_cu ? enc_knobs().wgs_per_cu : n;
    });
    // the fixed persistent grid, capped by the tile count of the call (never by the device-side list length)
    auto run = [&](const float *fr, int64_t fs, int nt, float *out, const SkipArgs &sa) -> hipError_t {
        int nwg = num_cu * wgs_per_cu;
        if (nwg > nt) nwg = nt;
        dim3 grid(nwg), block(256);
        auto go = [&](auto kern) {
            if constexpr (F::STAGGERS) hipLaunchKernelGGL(kern, grid, block, F::LDS, st, fr, fs, H, W, e, out, lg_tx, lg_tpf, nt, stagger, sa);
            else hipLaunchKernelGGL(kern, grid, block, F::LDS, st, fr, fs, H, W, e, out, lg_tx, lg_tpf, nt, sa);
        };
        switch (PS) {
            case 2: go(F::template kernel<2, TOKENS>); break;
            case 4: go(F::template kernel<4, TOKENS>); break;
            case 8: go(F::template kernel<8, TOKENS>); break;
            default: go(F::template kernel<16, false>); break;   // partials have one layout and do not depend on the cell size
        }
        return hipGetLastError();
    };
    SkipArgs plan;
    hipError_t err = skip_prepare<F::FORM, TOKENS>(
        skip, frames, fstride, B, H, W, part ? partials : features, lg_tx, ntiles, num_cu * wgs_per_cu, st,
        [&](const float *zero_frame, float *table) { return run(zero_frame, (int64_t)H * W, tiles_per_frame, table, SkipArgs()); },
        plan);
    if (err != hipSuccess) return err;
    if (!part) return run(frames, fstride, ntiles, features, plan);
    if ((err = run(frames, fstride, ntiles, partials, plan)) != hipSuccess) return err;
    return launch_pool_partials(partials, features, B, H, TOKENS, st);
}

hipError_t launch_encoder_b16(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e, float *features,
                              bool tokens, hipStream_t st, EncoderSkip *skip, float *partials) {
    return tokens ? launch_persistent<FormB16, true>(frames, fstride, B, H, W, e, features, st, skip, partials)
                  : launch_persistent<FormB16, false>(frames, fstride, B, H, W, e, features, st, skip, partials);
}

hipError_t launch_encoder_bf16(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e,
                               float *features, bool x3, bool tokens, hipStream_t st, EncoderSkip *skip, float *partials) {
    // split-bf16 runs on the 16x16x32 shape (k_encoder_b16: -7 % time, interleaved A/B); SMK_ENC_SHAPE=32 selects the
    // 32x32x16 kernel (k_encoder_bf16<true>) for comparison
    const int shape = enc_knobs().shape;
    if (x3 && shape == 16) return launch_encoder_b16(frames, fstride, B, H, W, e, features, tokens, st, skip, partials);
    if (x3) return tokens ? launch_persistent<FormBf16<true>, true>(frames, fstride, B, H, W, e, features, st, skip, partials)
                          : launch_persistent<FormBf16<true>, false>(frames, fstride, B, H, W, e, features, st, skip, partials);
    return tokens ? launch_persistent<FormBf16<false>, true>(frames, fstride, B, H, W, e, features, st, skip, partials)
                  : launch_persistent<FormBf16<false>, false>(frames, fstride, B, H, W, e, features, st, skip, partials);
}

hipError_t launch_encoder_i8(const float *frames, int64_t fstride, int B, int H, int W, const EncoderDev &e, float *features,
                             bool tokens, hipStream_t st, EncoderSkip *skip, float *partials) {
    return tokens ? launch_persistent<FormI8, true>(frames, fstride, B, H, W, e, features, st, skip, partials)
                  : launch_persistent<FormI8, false>(frames, fstride, B, H, W, e, features, st, skip, partials);
}

}  // namespace smk
