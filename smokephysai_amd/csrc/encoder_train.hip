// The encoder's two convolutions under autograd: forward, data and weight gradients (declared in encoder_train.h).  BatchNorm, ReLU and
// the pools between them stay with PyTorch / norm.hip; the fused inference kernels are in encoder.hip.
#include "encoder_train.h"

#include "encoder_tile.h"

namespace smk {

// ---------------------------------------------------------------------------------------------------------------------
// The encoder's FIRST convolution for training (smokephys_net.py:25, Conv2d(1, 64, 7, padding=3) under autograd), in plain fp32 on the
// vector ALUs -- 26 GFLOP per batch of 64 x 256^2, nothing for the matrix cores to win, and its output feeds train-mode BatchNorm +
// ReLU, so it has to be as exact as an fp32 convolution (see k_conv2_fwd_b16).  Having both convolutions here also takes MIOpen's
// find pass (20-50 s on a fresh machine for these two layers) out of the first training step.
// k_conv1_train_fwd: z1[b][c][i][j] = bias[c] + sum over the 49 taps (ki-major, one fma chain) of x[b][i+ki-3][j+kj-3] * w[c][ki][kj].
//   A workgroup = 4 rows x 256 columns; a thread = 4 consecutive pixels of one row, their 7 x 10 window of x in registers; the 64
//   channels in turn, each channel's 49 weights as 13 broadcast ds_read_b128 for 196 fmas; z1 stored as float4.
constexpr int C1_WP = 52;                                     // weights per channel in LDS (49 + 3 pad: 13 float4)
__global__ __launch_bounds__(256) void k_conv1_train_fwd(const float *__restrict__ x, int H, int W, const float *__restrict__ w,
                                                        const float *__restrict__ bias, float *__restrict__ z1) {
    __shared__ __attribute__((aligned(16))) float ws[64 * C1_WP];
    __shared__ float xs[10][264];                             // rows i0-3 .. i0+6, columns j0-3 .. j0+258 (+ pad)
    const int tid = threadIdx.x, b = blockIdx.z, i0 = blockIdx.y * 4, j0 = blockIdx.x * 256;
    for (int k = tid; k < 64 * C1_WP; k += 256) {
        const int c = k / C1_WP, t = k - c * C1_WP;
        ws[k] = t < 49 ? w[c * 49 + t] : 0.f;
    }
    const float *xb = x + (size_t)b * H * W;
    // (addresses clamped into the image, values zeroed afterwards: a load under a condition is waited for before the next one is issued)
    for (int k = tid; k < 10 * 262; k += 256) {
        const int r = k / 262, cc = k - r * 262, ii = i0 - 3 + r, jj = j0 - 3 + cc;
        const int ci = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii), cj = jj < 0 ? 0 : (jj > W - 1 ? W - 1 : jj);
        const float v = xb[(size_t)ci * W + cj];
        xs[r][cc] = (ii == ci && jj == cj) ? v : 0.f;
    }
    __syncthreads();
    const int jq = tid & 63, row = tid >> 6;
    float win[7][10];
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int cc = 0; cc < 10; ++cc) win[r][cc] = xs[row + r][4 * jq + cc];
    const int i = i0 + row, j = j0 + 4 * jq;
    if (i >= H || j >= W) return;                             // (W % 4 == 0: a quad is inside or outside as a whole)
    float *dst = z1 + ((size_t)b * 64 * H + i) * W + j;
#pragma unroll 1
    for (int c = 0; c < 64; ++c) {
        float wv[C1_WP];
#pragma unroll
        for (int q = 0; q < C1_WP / 4; ++q) {
            const float4 t4 = *reinterpret_cast<const float4 *>(&ws[c * C1_WP + 4 * q]);
            wv[4 * q] = t4.x; wv[4 * q + 1] = t4.y; wv[4 * q + 2] = t4.z; wv[4 * q + 3] = t4.w;
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ki = 0; ki < 7; ++ki)
#pragma unroll
            for (int kj = 0; kj < 7; ++kj)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p] = fmaf(win[ki][kj + p], wv[ki * 7 + kj], acc[p]);
        const float bb = bias ? bias[c] : 0.f;
        *reinterpret_cast<float4 *>(dst + (size_t)c * H * W) = make_float4(acc[0] + bb, acc[1] + bb, acc[2] + bb, acc[3] + bb);
    }
}

// k_conv1_train_wgrad: dW[c][ki][kj] = sum over b, i, j of dz[b][c][i][j] * x[b][i+ki-3][j+kj-3] (and db[c] = sum of dz): an outer-product
// accumulation over 4.2 M pixels.  A persistent workgroup walks tiles of 4 rows x 64 columns; dz of the tile sits in LDS as float4 per
// (4-channel group, pixel), x as a 10 x 70 halo; a thread owns 4 channels x one kernel row (28 accumulators + 4 for db) for half of the
// tile's rows: per pixel one ds_read_b128 of dz, one new x value into a 7-wide sliding window, 28 fmas.  Partials per workgroup, added in
// workgroup order by k_conv1_wgrad_finish (deterministic).
constexpr int C1G_PX = 4 * 64;                                // pixels per tile
constexpr int C1G_ZP = C1G_PX * 4 + 4;                        // floats per channel group in LDS (+ 4: the 16 groups start on different banks)
__global__ __launch_bounds__(256) void k_conv1_train_wgrad(const float *__restrict__ dz, const float *__restrict__ x, int H, int W, int tiles_x,
                                                          int tiles_per_frame, int ntiles, float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smemf[];
    float *zs = smemf;                                        // [16 groups][C1G_ZP]
    float *xs = smemf + 16 * C1G_ZP;                          // [10][72]
    const int tid = threadIdx.x;
    const int st = tid / 112, rem = tid - st * 112, cg = rem / 7, ky = rem - cg * 7;      // tid >= 224: staging only
    float acc[4][7], dbs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[c][k] = 0.f;
    const size_t plane = (size_t)H * W;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int b = t / tiles_per_frame, rm = t - b * tiles_per_frame;
        const int i0 = (rm / tiles_x) * 4, j0 = (rm % tiles_x) * 64;
        // stage dz: (group g, pixel p) -> float4 of channels 4g .. 4g+3; 16 x 256 items, 16 per thread, lanes along the pixels
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int it = tid + 256 * k, g = it >> 8, p = it & 255, r = p >> 6, cc = p & 63;
            const float *src = dz + ((size_t)b * 64 + 4 * g) * plane + (size_t)(i0 + r) * W + j0 + cc;
            *reinterpret_cast<float4 *>(&zs[g * C1G_ZP + 4 * p]) = make_float4(src[0], src[plane], src[2 * plane], src[3 * plane]);
        }
        const float *xb = x + (size_t)b * plane;
        for (int k = tid; k < 10 * 70; k += 256) {
            const int r = k / 70, cc = k - r * 70, ii = i0 - 3 + r, jj = j0 - 3 + cc;
            const int ci = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii), cj = jj < 0 ? 0 : (jj > W - 1 ? W - 1 : jj);
            const float v = xb[(size_t)ci * W + cj];            // (clamped address, value zeroed: no load under a condition)
            xs[r * 72 + cc] = (ii == ci && jj == cj) ? v : 0.f;
        }
        __syncthreads();
        if (tid < 224) {
#pragma unroll 1
            for (int r = 2 * st; r < 2 * st + 2; ++r) {
                const float *xr = xs + (r + ky) * 72;         // x row i0 + r + ky - 3
                float xv[7];
#pragma unroll
                for (int k = 0; k < 6; ++k) xv[k + 1] = xr[k];
#pragma unroll 4
                for (int cc = 0; cc < 64; ++cc) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) xv[k] = xv[k + 1];
                    xv[6] = xr[cc + 6];
                    const float4 d = *reinterpret_cast<const float4 *>(&zs[cg * C1G_ZP + 4 * (r * 64 + cc)]);
                    const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
#pragma unroll
                        for (int k = 0; k < 7; ++k) acc[c][k] = fmaf(dv[c], xv[k], acc[c][k]);
                        if (ky == 0) dbs[c] += dv[c];
                    }
                }
            }
        }
        __syncthreads();
    }
    // the two row-halves of the workgroup: half 1 hands its sums to half 0 through LDS, half 0 stores the workgroup's partial
    float *ex = smemf;                                        // [112][32]
    if (st == 1 && tid < 224) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int k = 0; k < 7; ++k) ex[rem * 32 + c * 7 + k] = acc[c][k];
            ex[rem * 32 + 28 + c] = dbs[c];
        }
    }
    __syncthreads();
    if (st == 0) {
        float *dst = part + (size_t)blockIdx.x * (64 * 49 + 64);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int k = 0; k < 7; ++k) dst[(4 * cg + c) * 49 + ky * 7 + k] = acc[c][k] + ex[rem * 32 + c * 7 + k];
            if (ky == 0) dst[64 * 49 + 4 * cg + c] = dbs[c] + ex[rem * 32 + 28 + c];
        }
    }
}

__global__ __launch_bounds__(256) void k_conv1_wgrad_finish(const float *__restrict__ part, int nparts, float *__restrict__ dw, float *__restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 64 * 49 + 64) return;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s += part[(size_t)k * (64 * 49 + 64) + i];
    if (i < 64 * 49) dw[i] = s;
    else if (db) db[i - 64 * 49] = s;
}

// k_conv1_train_dgrad: dx[b][i][j] = sum over c (ascending) and the 49 taps of dz[b][c][i+3-ki][j+3-kj] * w[c][ki][kj], zeros outside the
// plane: the 7x7 correlation of the 64 dz planes with the flipped kernels, summed over the channels -- for a caller that differentiates
// with respect to the frame (PGD, saliency).  Plain fp32: per channel one fma chain per output (window rows top to bottom, taps in
// memory order within a row), the 64 chains added in channel order.  No atomics, no workspace: every dx element is written exactly once.
//   A workgroup = 32 rows x 64 columns of dx; a thread = 2 rows x 4 consecutive pixels (8 accumulators).  dz is staged 4 channels at a
//   time as a 38 x 72 halo image per channel (columns j0-4 .. j0+67: whole aligned float4s, 1.30x the tile's bytes instead of the
//   forward tile's 2.5x); the next 4 channels' global loads are issued before the barrier that ends the current ones.  Per channel a
//   thread reads its 8 x 12 window (consecutive lanes, consecutive 16 bytes) for 392 fmas, which the compiler pairs along the pixels into
//   196 v_pk_fma_f32 (and reads the window as 8-byte pieces, the odd-aligned pairs a second time); the channel's 49 weights are
//   wave-uniform and come through scalar loads.  LDS 43,776 B, 245 VGPRs (two workgroups per CU), no scratch.
//   Measured 0.715 ms at 64 x 256^2 (4.3x the 0.17 ms byte / flop floors; aten.convolution_backward's dX: 2.60 ms), DESIGN 3.7.
constexpr int C1D_TH = 32, C1D_TW = 64, C1D_R = 2, C1D_CH = 4;
constexpr int C1D_ROWS = C1D_TH + 6, C1D_PITCH = C1D_TW + 8, C1D_Q = C1D_PITCH / 4;
__global__ __launch_bounds__(256) void k_conv1_train_dgrad(const float *__restrict__ dz, const float *__restrict__ w, int H, int W,
                                                          float *__restrict__ dx) {
    __shared__ __attribute__((aligned(16))) float zs[C1D_CH][C1D_ROWS * C1D_PITCH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int b = blockIdx.z, i0 = blockIdx.y * C1D_TH, j0 = blockIdx.x * C1D_TW;
    const size_t plane = (size_t)H * W;
    const float *zb = dz + (size_t)b * 64 * plane;
    constexpr int ITEMS = C1D_CH * C1D_ROWS * C1D_Q, NIT = (ITEMS + 255) / 256;        // 2,736 float4 per stage, 11 per thread
    float acc[C1D_R][4];
#pragma unroll
    for (int o = 0; o < C1D_R; ++o)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[o][p] = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < 64; c0 += C1D_CH) {
        // (addresses clamped into the plane, values zeroed afterwards; W % 4 == 0: a float4 is inside or outside as a whole)
        float4 v[NIT];
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            int idx = tid + 256 * k;
            idx = idx < ITEMS ? idx : ITEMS - 1;
            const int ch = idx / (C1D_ROWS * C1D_Q), rm = idx - ch * (C1D_ROWS * C1D_Q), r = rm / C1D_Q, q = rm - r * C1D_Q;
            const int ii = i0 - 3 + r, jj = j0 - 4 + 4 * q;
            const int ci = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii), cj = jj < 0 ? 0 : (jj > W - 4 ? W - 4 : jj);
            v[k] = *reinterpret_cast<const float4 *>(zb + (size_t)(c0 + ch) * plane + (size_t)ci * W + cj);
        }
        __syncthreads();                                      // every wave is done reading the previous channels
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int idx = tid + 256 * k;
            if (idx < ITEMS) {
                const int ch = idx / (C1D_ROWS * C1D_Q), rm = idx - ch * (C1D_ROWS * C1D_Q), r = rm / C1D_Q, q = rm - r * C1D_Q;
                const int ii = i0 - 3 + r, jj = j0 - 4 + 4 * q;
                const bool in = ii >= 0 && ii < H && jj >= 0 && jj < W;
                *reinterpret_cast<float4 *>(&zs[ch][r * C1D_PITCH + 4 * q]) = in ? v[k] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int ch = 0; ch < C1D_CH; ++ch) {
            const float *wc = w + (c0 + ch) * 49;             // wave-uniform: scalar loads
            const float *zt = &zs[ch][(ty * C1D_R) * C1D_PITCH + 4 * tx];
            float t[C1D_R][4];
#pragma unroll
            for (int o = 0; o < C1D_R; ++o)
#pragma unroll
                for (int p = 0; p < 4; ++p) t[o][p] = 0.f;
#pragma unroll
            for (int r = 0; r < C1D_R + 6; ++r) {             // window row r = dz row i0 + 2 ty + r - 3
                float m[12];                                  // columns j0 + 4 tx - 4 .. + 7; the window is m[1] .. m[10]
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float4 t4 = *reinterpret_cast<const float4 *>(zt + r * C1D_PITCH + 4 * q);
                    m[4 * q] = t4.x; m[4 * q + 1] = t4.y; m[4 * q + 2] = t4.z; m[4 * q + 3] = t4.w;
                }
#pragma unroll
                for (int o = 0; o < C1D_R; ++o) {
                    const int ki = o + 6 - r;                 // dz row = (output row) + 3 - ki
                    if (ki < 0 || ki > 6) continue;
#pragma unroll
                    for (int kj = 0; kj < 7; ++kj)
#pragma unroll
                        for (int p = 0; p < 4; ++p) t[o][p] = fmaf(m[p + 7 - kj], wc[ki * 7 + kj], t[o][p]);     // dz column = j + 3 - kj
                }
            }
#pragma unroll
            for (int o = 0; o < C1D_R; ++o)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[o][p] += t[o][p];
        }
    }
    const int j = j0 + 4 * tx;
    if (j >= W) return;
#pragma unroll
    for (int o = 0; o < C1D_R; ++o) {
        const int i = i0 + ty * C1D_R + o;
        if (i < H) *reinterpret_cast<float4 *>(dx + (size_t)b * plane + (size_t)i * W + j) = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
    }
}

constexpr int C1G_LDS = (16 * C1G_ZP + 10 * 72) * 4;          // 68,672 B
int conv1_wgrad_parts() { return device_num_cu() * 2; }
size_t conv1_wgrad_workspace_bytes() { return (size_t)conv1_wgrad_parts() * (64 * 49 + 64) * sizeof(float); }

hipError_t launch_conv1_train_forward(const float *x, const float *weight, const float *bias, int B, int H, int W, float *z1, hipStream_t st) {
    if (W % 4 != 0 || B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_conv1_train_fwd, dim3(cdiv(W, 256), cdiv(H, 4), B), dim3(256), 0, st, x, H, W, weight, bias, z1);
    return hipGetLastError();
}

hipError_t launch_conv1_train_dgrad(const float *dz, const float *weight, int B, int H, int W, float *dx, hipStream_t st) {
    if (W % 4 != 0 || W < 4 || H < 1 || B < 1 || B > 65535 || cdiv(H, C1D_TH) > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_conv1_train_dgrad, dim3(cdiv(W, C1D_TW), cdiv(H, C1D_TH), B), dim3(256), 0, st, dz, weight, H, W, dx);
    return hipGetLastError();
}

hipError_t launch_conv1_train_wgrad(const float *dz, const float *x, int B, int H, int W, float *dw, float *db, void *workspace, hipStream_t st) {
    if (H % 4 != 0 || W % 64 != 0 || B < 1) return hipErrorInvalidValue;
    const int tiles_x = W / 64, tiles_per_frame = tiles_x * (H / 4), ntiles = B * tiles_per_frame;
    int nparts = conv1_wgrad_parts();
    once_per_device((const void *)k_conv1_train_wgrad, [&] {
        (void)hipFuncSetAttribute((const void *)k_conv1_train_wgrad, hipFuncAttributeMaxDynamicSharedMemorySize, C1G_LDS);
    });
    const int grid = nparts < ntiles ? nparts : ntiles;
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(k_conv1_train_wgrad, dim3(grid), dim3(256), C1G_LDS, st, dz, x, H, W, tiles_x, tiles_per_frame, ntiles, part);
    hipLaunchKernelGGL(k_conv1_wgrad_finish, dim3(cdiv(64 * 49 + 64, 256)), dim3(256), 0, st, part, grid, dw, db);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// k_conv2_fwd_b16: the encoder's second convolution alone, for TRAINING (smokephys_net.py:28, Conv2d(64, 128, 3, padding=1) under
// autograd): z2 = conv(a1, w) + bias with a1 the activated first block [B, 64, H, W] and z2 [B, 128, H, W], both NCHW fp32 in HBM
// (train-mode BatchNorm needs the whole z2 before it can normalise, so nothing fuses across it).  The tile (8 x 16 pixels, 180-pixel
// halo image in LDS as swizzled bf16 planes) and the tap-loop skeleton are k_encoder_b16's; the prologue stages the halo tile from
// HBM (a thread owns one pixel and one group of 8 channels: 8 loads whose lanes run along a row, one split, one 16-byte store per
// plane) instead of computing it, and the epilogue stores the raw accumulators (+ bias) as 16-byte row pieces.
// ARITHMETIC: three bf16 terms per operand (v = h + m + l, 24 bits) and the six products h*h, h*m, m*h, m*m, h*l, l*h -- not the eval
// encoder's two terms / three products: this output feeds train-mode BatchNorm + ReLU, whose masks turn a 5e-6 forward error into a
// 1e-2 error of conv2.weight.grad (in fp64, noise of relative size 5e-7 / 5e-6 on z2 moves that gradient by 4e-3 / 1.7e-2), so the
// training forward has to be as exact as an fp32 convolution.  Per MFMA it moves LESS operand data than the three-product loop (12 A
// fragments and 6 B fragments per 96 MFMAs against 8 and 4 per 48).
constexpr int C2F_LDS = 3 * S16_A1_BYTES;                     // 69,120 -> 2 workgroups per CU
__device__ __forceinline__ void split3_bf16(float v, __bf16 &h, __bf16 &m, __bf16 &l) {
    h = (__bf16)v;
    const float r1 = v - (float)h;
    m = (__bf16)r1;
    l = (__bf16)(r1 - (float)m);
}

__global__ __launch_bounds__(256, 2) void k_conv2_fwd_b16(const float *__restrict__ a1, int H, int W, const unsigned short *__restrict__ w2s,
                                                       const float *__restrict__ bias, float *__restrict__ z2, int tiles_x,
                                                       int tiles_per_frame, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *a1p[3] = {smem, smem + S16_A1_BYTES, smem + 2 * S16_A1_BYTES};
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int px = lane & 15, kg = lane >> 4;
    const int o0 = wave * 32 + px;                                            // N tile 0; tile 1 = + 16
    const float b2a = bias ? bias[o0] : 0.f, b2b = bias ? bias[o0 + 16] : 0.f;
    const int lane_b = o0 * 64 + kg * 16;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(w2s), 0, 18 * 3 * 8192, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto load_b = [&](int ks, int part, int nt) -> uint4 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane_b, (ks * 3 + part) * 8192 + nt * 1024, 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    };
    uint4 bq[2][2][3];                                        // [slot][nt][h | m | l]
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int part = 0; part < 3; ++part) bq[0][nt][part] = load_b(0, part, nt);
    const size_t plane = (size_t)H * W;
    constexpr int ITEMS = (B3_TH + 2) * 8 * B3_AW;            // 10 rows x 8 channel groups x 18 pixels = 1,440 (pixel fastest)
    constexpr int NIT = (ITEMS + 255) / 256;                  // 6 per thread

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int b = t / tiles_per_frame, rem = t - b * tiles_per_frame;
        const int r0 = (rem / tiles_x) * B3_TH, c0 = (rem % tiles_x) * B3_TW;
        __builtin_amdgcn_s_setprio(S16_PRIO_CONV1);
        // ---- stage the halo tile: all of a thread's loads first (addresses clamped into the image, values zeroed afterwards), then split + store
        {
            const float *ab = a1 + (size_t)b * 64 * plane;
            float v[NIT][8];
#pragma unroll
            for (int j = 0; j < NIT; ++j) {
                int idx = tid + 256 * j;
                idx = idx < ITEMS ? idx : ITEMS - 1;
                const int row = idx / (8 * B3_AW), rm = idx - row * (8 * B3_AW), g = rm / B3_AW, pc = rm - g * B3_AW;
                const int ii = r0 - 1 + row, jj = c0 - 1 + pc;
                const int ci = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii), cj = jj < 0 ? 0 : (jj > W - 1 ? W - 1 : jj);
                const float *src = ab + (size_t)(8 * g) * plane + (size_t)ci * W + cj;
#pragma unroll
                for (int c = 0; c < 8; ++c) v[j][c] = src[(size_t)c * plane];
            }
#pragma unroll
            for (int j = 0; j < NIT; ++j) {
                const int idx = tid + 256 * j;
                if (idx < ITEMS) {
                    const int row = idx / (8 * B3_AW), rm = idx - row * (8 * B3_AW), g = rm / B3_AW, pc = rm - g * B3_AW;
                    const int ii = r0 - 1 + row, jj = c0 - 1 + pc;
                    const bool in = ii >= 0 && ii < H && jj >= 0 && jj < W;
                    const int p = row * B3_AW + pc;
                    bf16x8 vh, vm, vl;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        __bf16 hh, mm, ll;
                        split3_bf16(in ? v[j][c] : 0.f, hh, mm, ll);
                        vh[c] = hh; vm[c] = mm; vl[c] = ll;
                    }
                    const int off = p * 128 + ((g ^ (p & 7)) * 16);
                    *reinterpret_cast<bf16x8 *>(a1p[0] + off) = vh;
                    *reinterpret_cast<bf16x8 *>(a1p[1] + off) = vm;
                    *reinterpret_cast<bf16x8 *>(a1p[2] + off) = vl;
                }
            }
        }
        __syncthreads();                                      // a1 complete
        __builtin_amdgcn_s_setprio(S16_PRIO_KLOOP);

        // ---- conv2: acc[mt][nt][reg] = D(pixel row mt, column 4 kg + reg; channel 16 nt + px of the wave's 32); units as in k_encoder_b16
        f32x4v acc[8][2];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[mt][nt][g] = 0.f;
        const int c16[2] = {kg << 4, (4 + kg) << 4};
        auto tap_consts8 = [&](int ki, int kj, int (&om8)[8]) {
#pragma unroll
            for (int m = 0; m < 8; ++m) om8[m] = ((px + kj) << 7) ^ (((px + kj + 2 * (m + ki)) & 7) << 4);
        };
        auto load_a = [&](int ki, int half, int mq, const int (&om8)[8], bf16x8 (&af)[3][2]) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int m = 2 * mq + j;
                const int off = (om8[m] ^ c16[half]) + (ki + m) * (B3_AW * 128);
#pragma unroll
                for (int part = 0; part < 3; ++part) af[part][j] = *reinterpret_cast<const bf16x8 *>(a1p[part] + off);
            }
        };
        // unit u = half * 4 + mq of a tap: pixel rows 2mq, 2mq+1 of k-step (tap, half): 24 MFMAs on 6 A fragments and the k-step's 6 B fragments
        bf16x8 afA[3][2], afB[3][2];
        int om8[8];
        tap_consts8(0, 0, om8);
        load_a(0, 0, 0, om8, afA);
        int ki = 0, kj = 0;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int half = u >> 2, mq = u & 3, slot = half;
                if (mq == 0) {                                 // refill the other slot with k-step ks + 1: six fragments, at the k-step's start
                    int kn = tap * 2 + half + 1;
                    kn = kn >= 18 ? kn - 18 : kn;
                    kn = __builtin_amdgcn_readfirstlane(kn);
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int part = 0; part < 3; ++part) bq[slot ^ 1][nt][part] = load_b(kn, part, nt);
                }
                if (u < 7) {
                    if (u & 1) load_a(ki, (u + 1) >> 2, (u + 1) & 3, om8, afA);
                    else load_a(ki, (u + 1) >> 2, (u + 1) & 3, om8, afB);
                } else if (tap < 8) {                          // u = 7 is odd: the next tap's first unit goes to set A
                    kj = kj == 2 ? 0 : kj + 1;
                    ki = kj == 0 ? ki + 1 : ki;
                    tap_consts8(ki, kj, om8);
                    load_a(ki, 0, 0, om8, afA);
                }
                // six products, smallest first, product-major (consecutive MFMAs go to different accumulators: dependency distance 4)
#pragma unroll
                for (int pr = 0; pr < 6; ++pr)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) {
                            constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};       // l*h, h*l, m*m, m*h, h*m, h*h
                            const bf16x8 av = (u & 1) ? afB[PA[pr]][j] : afA[PA[pr]][j];
                            const bf16x8 bv = __builtin_bit_cast(bf16x8, bq[slot][nt][PB[pr]]);
                            f32x4v &c = acc[2 * mq + j][nt];
                            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
                        }
                // 24 MFMAs: the next unit's 6 fragment reads one per four MFMAs, a k-step's six weight loads behind the first MFMAs of its first unit
#pragma unroll
                for (int i = 0; i < 24; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (i % 4 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    else if (mq == 0 && i < 9) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- epilogue: z2 = acc + bias.  Lane: channel o0 (nt 0) / o0 + 16 (nt 1), pixels (row mt, cols 4kg .. 4kg+3): 16-byte stores
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float bb = nt ? b2b : b2a;
            float *dst = z2 + ((size_t)b * 128 + o0 + 16 * nt) * plane + (size_t)r0 * W + c0 + 4 * kg;
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
                const f32x4v c = acc[mt][nt];
                *reinterpret_cast<float4 *>(dst + (size_t)mt * W) = make_float4(c[0] + bb, c[1] + bb, c[2] + bb, c[3] + bb);
            }
        }
        __syncthreads();                                      // every wave is done reading a1
    }
}

// k_conv2_dgrad_b16: the data gradient of the same convolution, dX[b][c] = sum over o, taps of dZ[b][o][y + ky' - 1][x + kx' - 1] * W[o][c][2 - ky'][2 - kx']
// -- a 3x3 convolution from 128 channels to 64 with the flipped kernel.  Same tile, halo image and swizzle; the 128 input channels
// go through the 64-channel LDS image as two passes (stage half, 18 k-steps, stage the other half, 18 more) into the same accumulators.
// With only 64 outputs the waves split the tile's rows as well as the channels: wave = (4 M-tiles, 2 N-tiles), so every unit of 24
// MFMAs is a k-step of its own (8 A-fragment reads as in the forward, 4 weight-fragment loads: twice the forward's weight stream).
// w2d: [pass 2][k-step 18 = tap' * 2 + o_local / 32][hi|lo][c 64][32 o]: 4 KiB per (k-step, part).
__global__ __launch_bounds__(256, 2) void k_conv2_dgrad_b16(const float *__restrict__ dz, int H, int W, const unsigned short *__restrict__ w2d,
                                                         float *__restrict__ dx, int tiles_x, int tiles_per_frame, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *a1h = smem, *a1l = a1h + S16_A1_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int px = lane & 15, kg = lane >> 4;
    const int mh = wave & 1, nh = wave >> 1;
    const int c0o = nh * 32 + px;                                             // output channel of N tile 0; tile 1 = + 16
    const int lane_b = c0o * 64 + kg * 16;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(w2d), 0, 2 * 18 * 2 * 4096, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    auto load_b = [&](int ks36, int part, int nt) -> uint4 {                  // ks36 = pass * 18 + k-step
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane_b, (ks36 * 2 + part) * 4096 + nt * 1024, 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    };
    uint4 bq[2][2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        bq[0][nt][0] = load_b(0, 0, nt);
        bq[0][nt][1] = load_b(0, 1, nt);
    }
    const size_t plane = (size_t)H * W;
    constexpr int ITEMS = (B3_TH + 2) * 8 * B3_AW, NIT = (ITEMS + 255) / 256;
    const unsigned char *a1h_w = a1h + mh * 4 * (B3_AW * 128), *a1l_w = a1l + mh * 4 * (B3_AW * 128);
    const int c16[2] = {kg << 4, (4 + kg) << 4};

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int b = t / tiles_per_frame, rem = t - b * tiles_per_frame;
        const int r0 = (rem / tiles_x) * B3_TH, c0 = (rem % tiles_x) * B3_TW;
        f32x4v acc[4][2];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[m][nt][g] = 0.f;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            __builtin_amdgcn_s_setprio(S16_PRIO_CONV1);
            {   // stage the halo tile of dZ's channels 64 pass .. 64 pass + 63 (as k_conv2_fwd_b16 stages a1)
                const float *ab = dz + ((size_t)b * 128 + 64 * pass) * plane;
                float v[NIT][8];
#pragma unroll
                for (int j = 0; j < NIT; ++j) {
                    int idx = tid + 256 * j;
                    idx = idx < ITEMS ? idx : ITEMS - 1;
                    const int row = idx / (8 * B3_AW), rm = idx - row * (8 * B3_AW), g = rm / B3_AW, pc = rm - g * B3_AW;
                    const int ii = r0 - 1 + row, jj = c0 - 1 + pc;
                    const int ci = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii), cj = jj < 0 ? 0 : (jj > W - 1 ? W - 1 : jj);
                    const float *src = ab + (size_t)(8 * g) * plane + (size_t)ci * W + cj;
#pragma unroll
                    for (int c = 0; c < 8; ++c) v[j][c] = src[(size_t)c * plane];
                }
#pragma unroll
                for (int j = 0; j < NIT; ++j) {
                    const int idx = tid + 256 * j;
                    if (idx < ITEMS) {
                        const int row = idx / (8 * B3_AW), rm = idx - row * (8 * B3_AW), g = rm / B3_AW, pc = rm - g * B3_AW;
                        const int ii = r0 - 1 + row, jj = c0 - 1 + pc;
                        const bool in = ii >= 0 && ii < H && jj >= 0 && jj < W;
                        const int p = row * B3_AW + pc;
                        bf16x8 vh, vl;
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            __bf16 hh, ll;
                            split_bf16(in ? v[j][c] : 0.f, hh, ll);
                            vh[c] = hh; vl[c] = ll;
                        }
                        const int off = p * 128 + ((g ^ (p & 7)) * 16);
                        *reinterpret_cast<bf16x8 *>(a1h + off) = vh;
                        *reinterpret_cast<bf16x8 *>(a1l + off) = vl;
                    }
                }
            }
            __syncthreads();                                  // the image is complete
            __builtin_amdgcn_s_setprio(S16_PRIO_KLOOP);
            auto tap_consts = [&](int ki, int kj, int (&om)[4]) {
#pragma unroll
                for (int m = 0; m < 4; ++m) om[m] = ((px + kj) << 7) ^ (((px + kj + 2 * (m + ki)) & 7) << 4);
            };
            auto load_a = [&](int ki, int half, const int (&om)[4], bf16x8 (&ah)[4], bf16x8 (&al)[4]) {
                const unsigned char *ph = a1h_w + ki * (B3_AW * 128), *pl = a1l_w + ki * (B3_AW * 128);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int off = om[m] ^ c16[half];
                    ah[m] = *reinterpret_cast<const bf16x8 *>(ph + off + m * (B3_AW * 128));
                    al[m] = *reinterpret_cast<const bf16x8 *>(pl + off + m * (B3_AW * 128));
                }
            };
            bf16x8 ahA[4], alA[4], ahB[4], alB[4];
            int om[4];
            tap_consts(0, 0, om);
            load_a(0, 0, om, ahA, alA);
            int ki = 0, kj = 0;
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int slot = half;
                    {   // refill the other slot with the next k-step (the ring runs through both passes and on into the next tile)
                        int kn = pass * 18 + tap * 2 + half + 1;
                        kn = kn >= 36 ? kn - 36 : kn;
                        kn = __builtin_amdgcn_readfirstlane(kn);
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) {
                            bq[slot ^ 1][nt][0] = load_b(kn, 0, nt);
                            bq[slot ^ 1][nt][1] = load_b(kn, 1, nt);
                        }
                    }
                    if (half == 0) {
                        load_a(ki, 1, om, ahB, alB);
                    } else if (tap < 8) {
                        kj = kj == 2 ? 0 : kj + 1;
                        ki = kj == 0 ? ki + 1 : ki;
                        tap_consts(ki, kj, om);
                        load_a(ki, 0, om, ahA, alA);
                    }
#pragma unroll
                    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                        for (int m = 0; m < 4; ++m)
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt) {
                                const bf16x8 bh = __builtin_bit_cast(bf16x8, bq[slot][nt][0]);
                                const bf16x8 bl = __builtin_bit_cast(bf16x8, bq[slot][nt][1]);
                                f32x4v &c = acc[m][nt];
                                const bf16x8 ah = half ? ahB[m] : ahA[m], al = half ? alB[m] : alA[m];
                                if (pr == 0) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
                                else if (pr == 1) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
                                else c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
                            }
#pragma unroll
                    for (int i = 0; i < 24; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (i % 3 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        else if (i == 1 || i == 2 || i == 4 || i == 5) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();                                  // every wave is done reading the image
        }
        // ---- epilogue: dX rows 4 mh + m, columns 4kg .. 4kg+3 of channel c0o (+ 16): 16-byte stores
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            float *dst = dx + ((size_t)b * 64 + c0o + 16 * nt) * plane + (size_t)(r0 + 4 * mh) * W + c0 + 4 * kg;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x4v c = acc[m][nt];
                *reinterpret_cast<float4 *>(dst + (size_t)m * W) = make_float4(c[0], c[1], c[2], c[3]);
            }
        }
    }
}

// w [128 o][64 c][3][3] -> w2d [pass = o / 64][k-step = tap' * 2 + (o % 64) / 32][hi|lo][c 64][32 o], tap' = the flipped tap (2 - ky, 2 - kx)
__global__ void k_split_conv2_weights_dgrad(const float *__restrict__ w, unsigned short *__restrict__ w2d_) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 9 * 64 * 128) return;
    const int o = t % 128, c = (t / 128) % 64, tap = t / (64 * 128);
    const float v = w[((size_t)o * 64 + c) * 9 + tap];
    const int ky = tap / 3, kx = tap - 3 * ky, tapf = (2 - ky) * 3 + (2 - kx);
    __bf16 *w2d = reinterpret_cast<__bf16 *>(w2d_);
    const __bf16 hi = (__bf16)v;
    const int pass = o >> 6, ol = o & 63, ks = tapf * 2 + (ol >> 5), o32 = ol & 31;
    const size_t base = ((size_t)(pass * 18 + ks) * 2) * 64 * 32;
    w2d[base + (size_t)c * 32 + o32] = hi;
    w2d[base + (size_t)64 * 32 + (size_t)c * 32 + o32] = (__bf16)(v - (float)hi);
}

hipError_t launch_conv2_train_dgrad(const float *dz, const float *weight, int B, int H, int W, float *dx, void *workspace, hipStream_t st) {
    if (H % B3_TH != 0 || W % B3_TW != 0 || B < 1) return hipErrorInvalidValue;
    unsigned short *w2d = static_cast<unsigned short *>(workspace);
    hipLaunchKernelGGL(k_split_conv2_weights_dgrad, dim3(cdiv(9 * 64 * 128, 256)), dim3(256), 0, st, weight, w2d);
    const int tiles_x = W / B3_TW, tiles_per_frame = tiles_x * (H / B3_TH), ntiles = B * tiles_per_frame;
    constexpr int lds = 2 * S16_A1_BYTES;
    const int wgs_per_cu = device_cached_int((const void *)k_conv2_dgrad_b16, [] {
        (void)hipFuncSetAttribute((const void *)k_conv2_dgrad_b16, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)k_conv2_dgrad_b16, 256, lds) != hipSuccess || n < 1) n = 2;
        return n;
    });
    int nwg = device_num_cu() * wgs_per_cu;
    if (nwg > ntiles) nwg = ntiles;
    hipLaunchKernelGGL(k_conv2_dgrad_b16, dim3(nwg), dim3(256), lds, st, dz, H, W, w2d, dx, tiles_x, tiles_per_frame, ntiles);
    return hipGetLastError();
}

// k_conv2_wgrad_b16: the weight gradient of the same convolution, dW[o][c][ky][kx] = sum over b, y, x of dZ[b][o][y][x] * a1[b][c][y+ky-1][x+kx-1]:
// per 8 x 16 tile a GEMM D[o][(tap, c)] += A[o][pixel] * B[(tap, c)][pixel] with the PIXELS as the MFMA k dimension -- both operands are
// pixel-contiguous in NCHW already, so staging is a copy + split (16 bytes of bf16 per 8 pixels of a row).
//   workgroup: 32 output channels (2 M-tiles) x all 576 (tap, c) columns (36 N-tiles) for its stream of tiles; wave w: channels 16w .. 16w+15
//              of a1 and all 9 taps (9 N-tiles): 72 accumulator registers, kept for the whole launch.
//   k-step:    32 pixels = tile rows 2s, 2s+1; a lane's k-group kg = 8 consecutive x of one row (row 2s + (kg >> 1), x0 = 8 (kg & 1)).
//   LDS:       dZ tile [hi|lo][32 o][128 px] (row pitch 272 B), a1 tile [hi|lo][64 c][10 rows][16 px] (c pitch 336 B: 16 lanes of one
//              k-group read conflict-free) + the two halo columns [hi|lo][64 c][10 rows][2].
//   taps:      ky moves the row (an address), kx = 1 reads the aligned 16-byte chunk, kx = 0 / 2 need the chunk shifted by one bf16: the
//              neighbouring element comes from the other chunk of the row or from the halo column (one ds_read_u16 at a per-lane address)
//              and four v_alignbit_b32 build the fragment.
//   output:    every workgroup adds its tiles into registers and stores ONE partial [32 o][9 taps][64 c]; k_conv2_wgrad_finish adds the
//              partials of a channel group in stream order (deterministic) and writes dW [128][64][3][3] (and db from the staged dZ).
constexpr int WG_OG = 32;                                     // output channels per workgroup
constexpr int WG_ZP = 272;                                    // dZ row pitch (bytes): 128 px * 2 B + 16
constexpr int WG_AC = 336;                                    // a1 channel pitch (bytes): 10 rows * 32 B + 16
constexpr int WG_Z_BYTES = WG_OG * WG_ZP;                     // 8,704 per plane
constexpr int WG_A_BYTES = 64 * WG_AC;                        // 21,504 per plane
constexpr int WG_H_BYTES = 64 * 10 * 2 * 2;                   // 2,560 per plane: [c][row][left|right] bf16
constexpr int WG_LDS = 2 * (WG_Z_BYTES + WG_A_BYTES + WG_H_BYTES);   // 65,536

__global__ __launch_bounds__(256, 2) void k_conv2_wgrad_b16(const float *__restrict__ dz, const float *__restrict__ a1, int H, int W, int tiles_x,
                                                         int tiles_per_frame, int ntiles, int nstreams, float *__restrict__ part,
                                                         float *__restrict__ dbpart) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *zh = smem, *zl = zh + WG_Z_BYTES, *ah = zl + WG_Z_BYTES, *al = ah + WG_A_BYTES, *hh = al + WG_A_BYTES, *hl = hh + WG_H_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n15 = lane & 15, kg = lane >> 4;
    // blocks i and i + 8 share an XCD: the four channel groups of one tile stream sit on one XCD (a1 is fetched into that L2 once)
    const int xcd = blockIdx.x & 7, og = (blockIdx.x >> 3) & 3, stream = (blockIdx.x >> 5) * 8 + xcd;
    const size_t plane = (size_t)H * W;
    f32x4v acc[2][9];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[m][t9][g] = 0.f;
    float dbsum = 0.f;                                        // this thread's share of db: channel og*32 + tid / 8, pixels 16 (tid % 8) ..

    for (int t = stream; t < ntiles; t += nstreams) {
        const int b = t / tiles_per_frame, rem = t - b * tiles_per_frame;
        const int r0 = (rem / tiles_x) * B3_TH, c0 = (rem % tiles_x) * B3_TW;
        // ---- stage dZ: 32 o x 8 rows x 16 px; thread: o = tid / 8, row = tid % 8 (16 px = 4 x float4)
        {
            const int o = tid >> 3, row = tid & 7;
            const float *src = dz + ((size_t)b * 128 + og * WG_OG + o) * plane + (size_t)(r0 + row) * W + c0;
            float4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4 *>(src + 4 * q);
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const float f[8] = {v[2 * hlf].x, v[2 * hlf].y, v[2 * hlf].z, v[2 * hlf].w, v[2 * hlf + 1].x, v[2 * hlf + 1].y, v[2 * hlf + 1].z, v[2 * hlf + 1].w};
                bf16x8 vh, vl;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    __bf16 a_, b_;
                    split_bf16(f[c], a_, b_);
                    vh[c] = a_; vl[c] = b_;
                    dbsum += f[c];
                }
                const int off = o * WG_ZP + (row * 16 + 8 * hlf) * 2;
                *reinterpret_cast<bf16x8 *>(zh + off) = vh;
                *reinterpret_cast<bf16x8 *>(zl + off) = vl;
            }
        }
        // ---- stage a1: 64 c x 10 rows x 16 px (+ 2 halo columns); items (c, row): 640 -> 3 per thread (the last partly)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int it = tid + 256 * j;
            if (it < 640) {
                const int c = it / 10, row = it - c * 10;
                const int ii = r0 - 1 + row;
                const bool rin = ii >= 0 && ii < H;
                const float *src = a1 + ((size_t)b * 64 + c) * plane + (size_t)(rin ? ii : 0) * W + c0;
                float4 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4 *>(src + 4 * q);
                const float lft = (rin && c0 > 0) ? src[-1] : 0.f, rgt = (rin && c0 + 16 < W) ? src[16] : 0.f;
#pragma unroll
                for (int hlf = 0; hlf < 2; ++hlf) {
                    const float f[8] = {v[2 * hlf].x, v[2 * hlf].y, v[2 * hlf].z, v[2 * hlf].w, v[2 * hlf + 1].x, v[2 * hlf + 1].y, v[2 * hlf + 1].z, v[2 * hlf + 1].w};
                    bf16x8 vh, vl;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        __bf16 a_, b_;
                        split_bf16(rin ? f[e] : 0.f, a_, b_);
                        vh[e] = a_; vl[e] = b_;
                    }
                    const int off = c * WG_AC + row * 32 + 16 * hlf;
                    *reinterpret_cast<bf16x8 *>(ah + off) = vh;
                    *reinterpret_cast<bf16x8 *>(al + off) = vl;
                }
                __bf16 lh_, ll_, rh_, rl_;
                split_bf16(lft, lh_, ll_);
                split_bf16(rgt, rh_, rl_);
                __bf16 *ph = reinterpret_cast<__bf16 *>(hh) + (c * 10 + row) * 2, *pl = reinterpret_cast<__bf16 *>(hl) + (c * 10 + row) * 2;
                ph[0] = lh_; ph[1] = rh_;
                pl[0] = ll_; pl[1] = rl_;
            }
        }
        __syncthreads();
        // ---- 4 k-steps of 32 pixels: A = dZ (2 M-tiles), B = a1 of the wave's 16 channels at the 9 taps
        const int cw = wave * 16 + n15;                       // the lane's a1 channel (B row)
        const int x0 = 8 * (kg & 1);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int prow = 2 * s4 + (kg >> 1);              // the lane's tile row in this k-step
            bf16x8 azh[2], azl[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int off = (m * 16 + n15) * WG_ZP + (prow * 16 + x0) * 2;
                azh[m] = *reinterpret_cast<const bf16x8 *>(zh + off);
                azl[m] = *reinterpret_cast<const bf16x8 *>(zl + off);
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int arow = prow + ky;                   // row of the 10-row halo tile (tile row + ky - 1, + 1 for the halo)
                const int rbase = cw * WG_AC + arow * 32;
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 ch = *reinterpret_cast<const u32x4 *>(ah + rbase + 2 * x0), cl = *reinterpret_cast<const u32x4 *>(al + rbase + 2 * x0);
                // the element left of the chunk (x0 - 1) and right of it (x0 + 8): the row's other chunk, or the halo column
                const int lo_off = x0 ? rbase + 14 : -1, ro_off = x0 ? -1 : rbase + 16;
                const int hidx = ((cw * 10 + arow) * 2) * 2;
                const unsigned int leh = lo_off >= 0 ? *reinterpret_cast<const unsigned short *>(ah + lo_off) : *reinterpret_cast<const unsigned short *>(hh + hidx);
                const unsigned int lel = lo_off >= 0 ? *reinterpret_cast<const unsigned short *>(al + lo_off) : *reinterpret_cast<const unsigned short *>(hl + hidx);
                const unsigned int reh = ro_off >= 0 ? *reinterpret_cast<const unsigned short *>(ah + ro_off) : *reinterpret_cast<const unsigned short *>(hh + hidx + 2);
                const unsigned int rel = ro_off >= 0 ? *reinterpret_cast<const unsigned short *>(al + ro_off) : *reinterpret_cast<const unsigned short *>(hl + hidx + 2);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    u32x4 fh, fl;
                    if (kx == 1) {
                        fh = ch; fl = cl;
                    } else if (kx == 0) {                     // elements x0-1 .. x0+6
                        fh[0] = leh | (ch[0] << 16); fl[0] = lel | (cl[0] << 16);
#pragma unroll
                        for (int i = 1; i < 4; ++i) {
                            fh[i] = __builtin_amdgcn_alignbit(ch[i], ch[i - 1], 16);
                            fl[i] = __builtin_amdgcn_alignbit(cl[i], cl[i - 1], 16);
                        }
                    } else {                                  // elements x0+1 .. x0+8
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            fh[i] = __builtin_amdgcn_alignbit(ch[i + 1], ch[i], 16);
                            fl[i] = __builtin_amdgcn_alignbit(cl[i + 1], cl[i], 16);
                        }
                        fh[3] = (ch[3] >> 16) | (reh << 16); fl[3] = (cl[3] >> 16) | (rel << 16);
                    }
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, fh), bl = __builtin_bit_cast(bf16x8, fl);
                    const int t9 = ky * 3 + kx;
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        f32x4v &c = acc[m][t9];
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(azl[m], bh, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(azh[m], bl, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(azh[m], bh, c, 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                                      // every wave is done reading the tiles
    }
    // ---- this workgroup's partial: part[stream][og][o_local 32][tap 9][c 64]; D layout: lane (n15 = column = c, kg) holds rows 4kg .. 4kg+3 (= o)
    float *dst = part + ((size_t)stream * 4 + og) * (WG_OG * 9 * 64);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
            for (int g = 0; g < 4; ++g) dst[((size_t)(m * 16 + 4 * kg + g) * 9 + t9) * 64 + wave * 16 + n15] = acc[m][t9][g];
    // db partial: 8 threads per channel (tid % 8 = the tile row they staged), added in lane order
    float sdb = dbsum;
    sdb += __shfl_xor(sdb, 1); sdb += __shfl_xor(sdb, 2); sdb += __shfl_xor(sdb, 4);
    if ((tid & 7) == 0) dbpart[((size_t)stream * 4 + og) * WG_OG + (tid >> 3)] = sdb;
}

// dW[o][c][tap] = sum over streams (in stream order) of part[stream][o / 32][o % 32][tap][c]; db[o] likewise
__global__ __launch_bounds__(256) void k_conv2_wgrad_finish(const float *__restrict__ part, const float *__restrict__ dbpart, int nstreams,
                                                          float *__restrict__ dw, float *__restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;             // over [o 128][tap 9][c 64]
    if (i < 128 * 9 * 64) {
        const int c = i & 63, t9 = (i >> 6) % 9, o = i / (9 * 64);
        const float *src = part + ((size_t)(o >> 5) * (WG_OG * 9 * 64)) + ((size_t)(o & 31) * 9 + t9) * 64 + c;
        float s = 0.f;
        for (int st = 0; st < nstreams; ++st) s += src[(size_t)st * 4 * (WG_OG * 9 * 64)];
        dw[((size_t)o * 64 + c) * 9 + t9] = s;
    }
    if (db && i < 128) {
        float s = 0.f;
        for (int st = 0; st < nstreams; ++st) s += dbpart[((size_t)st * 4 + (i >> 5)) * WG_OG + (i & 31)];
        db[i] = s;
    }
}

size_t conv2_wgrad_workspace_bytes(int nstreams) { return ((size_t)nstreams * 4 * (WG_OG * 9 * 64) + (size_t)nstreams * 4 * WG_OG) * sizeof(float); }
int conv2_wgrad_streams() { return (device_num_cu() * 2 / 32) * 8; }     // two workgroups per CU, four channel groups per stream, 8 XCD slots

hipError_t launch_conv2_train_wgrad(const float *dz, const float *a1, int B, int H, int W, float *dw, float *db, void *workspace, hipStream_t st) {
    if (H % B3_TH != 0 || W % B3_TW != 0 || B < 1) return hipErrorInvalidValue;
    const int tiles_x = W / B3_TW, tiles_per_frame = tiles_x * (H / B3_TH), ntiles = B * tiles_per_frame;
    const int nstreams = conv2_wgrad_streams();
    if (nstreams < 8) return hipErrorInvalidValue;
    float *part = static_cast<float *>(workspace), *dbpart = part + (size_t)nstreams * 4 * (WG_OG * 9 * 64);
    once_per_device((const void *)k_conv2_wgrad_b16, [&] {
        (void)hipFuncSetAttribute((const void *)k_conv2_wgrad_b16, hipFuncAttributeMaxDynamicSharedMemorySize, WG_LDS);
    });
    hipLaunchKernelGGL(k_conv2_wgrad_b16, dim3(nstreams * 4), dim3(256), WG_LDS, st, dz, a1, H, W, tiles_x, tiles_per_frame, ntiles, nstreams, part, dbpart);
    hipLaunchKernelGGL(k_conv2_wgrad_finish, dim3(cdiv(128 * 9 * 64, 256)), dim3(256), 0, st, part, dbpart, nstreams, dw, db);
    return hipGetLastError();
}

// w [128 o][64 c][3][3] -> w2s [k-step = tap*2 + c/32][h|m|l][o][32 c] (the B fragments of the training forward's tap loop: three bf16 terms)
__global__ void k_split_conv2_weights(const float *__restrict__ w, unsigned short *__restrict__ w2s_) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 9 * 64 * 128) return;
    const int c = t % 64, o = (t / 64) % 128, tap = t / (64 * 128);
    const float v = w[((size_t)o * 64 + c) * 9 + tap];
    __bf16 *w2s = reinterpret_cast<__bf16 *>(w2s_);
    __bf16 h, m, l;
    split3_bf16(v, h, m, l);
    const int ks2 = tap * 2 + (c >> 5), c32 = c & 31;
    w2s[((size_t)(ks2 * 3 + 0) * 128 + o) * 32 + c32] = h;
    w2s[((size_t)(ks2 * 3 + 1) * 128 + o) * 32 + c32] = m;
    w2s[((size_t)(ks2 * 3 + 2) * 128 + o) * 32 + c32] = l;
}

size_t conv2_train_workspace_bytes() { return (size_t)18 * 3 * 128 * 32 * sizeof(unsigned short); }     // (the data gradient uses 2/3 of it)

hipError_t launch_conv2_train_forward(const float *a1, const float *weight, const float *bias, int B, int H, int W, float *z2, void *workspace,
                                      hipStream_t st) {
    if (H % B3_TH != 0 || W % B3_TW != 0 || B < 1) return hipErrorInvalidValue;
    unsigned short *w2s = static_cast<unsigned short *>(workspace);
    hipLaunchKernelGGL(k_split_conv2_weights, dim3(cdiv(9 * 64 * 128, 256)), dim3(256), 0, st, weight, w2s);
    const int tiles_x = W / B3_TW, tiles_per_frame = tiles_x * (H / B3_TH), ntiles = B * tiles_per_frame;
    constexpr int lds = C2F_LDS;
    const int wgs_per_cu = device_cached_int((const void *)k_conv2_fwd_b16, [] {
        (void)hipFuncSetAttribute((const void *)k_conv2_fwd_b16, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)k_conv2_fwd_b16, 256, lds) != hipSuccess || n < 1) n = 2;
        return n;
    });
    int nwg = device_num_cu() * wgs_per_cu;
    if (nwg > ntiles) nwg = ntiles;
    hipLaunchKernelGGL(k_conv2_fwd_b16, dim3(nwg), dim3(256), lds, st, a1, H, W, w2s, bias, z2, tiles_x, tiles_per_frame, ntiles);
    return hipGetLastError();
}

}  // namespace smk
