// Training kernels of the 3-D encoder (SPEC_3D.md section 11), channels-last [B][D][H][W][C] throughout -- no transposes to NCDHW.
//
// Arithmetic.  Every convolution pass here runs on the exact fp32-input MFMA (v_mfma_f32_16x16x4_f32: an fmaf chain, bit for bit), not on
// split bf16.  The forward passes must be fp32-class (they feed train-mode BatchNorm + ReLU, whose masks turn forward noise of 5e-6 into
// gradient error of 1e-2: models/conv.py); the two gradients of conv2 MAY use two bf16 terms and would then run up to 5 x faster at peak --
// that form is the next step and not built here.  One MFMA = A [16][4] x B [4][16]: lane (px = lane & 15, kg = lane >> 4)
// holds A[px][kg] and B[kg][px]; the result's register i is D[4 kg + i][px].
//
//   k_c3t_conv<CIN, COUT>   3 x 3 x 3 convolution CIN -> COUT of an 8 x 16 tile of one plane per workgroup: <64, 128> is conv2's forward,
//                           <128, 64> with the flipped kernel its data gradient.  One input plane's 10 x 18 halo tile (64 channels) lies in
//                           LDS at a time (48,960 B: three workgroups per CU); M = the tile's 128 voxels (8 rows of 16), wave w = COUT / 4
//                           output channels, K = 9 taps x 64 channels per staged plane.  Weights come from L2 in the layout [tap][cin][cout]
//                           that k_c3t_prep_w2 writes in the same call (so an optimizer step needs no other notification).
//   k_c3t_conv1             7 x 7 x 7 convolution 1 -> 64 of a scalar volume, same tiling: the 7 x 14 x 24 halo block in LDS, K = 49 window
//                           rows x 8 kx slots (slot 7 carries zero weights).
//   k_c3t_conv1_dgrad       the data gradient of conv1 (64 -> 1 with the flipped 7 x 7 x 7 kernel): Toeplitz in y, two output planes per
//                           workgroup, one dz1 halo plane in LDS at a time (its own section below).
//   k_c3t_wgrad             dW2[o][tap][c] = sum over voxels of dz2[voxel][o] a1[voxel + tap][c] with the VOXELS as the MFMA k dimension.
//                           A workgroup owns 32 output channels x one kz slice (9 taps x 64 channels: 72 accumulator registers per lane) and
//                           one of S voxel streams (tiles s, s + S, ...: a function of the shape alone); per tile the dz2 rows and the a1
//                           halo plane are staged once and all nine taps read from there.  Each stream writes one partial;
//                           k_c3t_wgrad_finish adds the partials in stream order.  No atomics: a repeated call is bit-identical.
//   k_bncl_*                train-mode BatchNorm + ReLU phases on [M][C], C in {64, 128}: float4 per lane, rows strided over the grid,
//                           per-channel sums in fp64 through a two-stage reduction in a fixed order (one finishing workgroup per channel).
#include "conv3d_train.h"

namespace smk {

typedef float c3t_f32x4 __attribute__((ext_vector_type(4)));

constexpr int C3T_AW = C3T_TW + 2, C3T_APIX = (C3T_TH + 2) * C3T_AW;      // halo tile 10 x 18 = 180 voxels
constexpr int C3T_VS = 68;                                    // floats per staged voxel (64 + 4: a wave's 16-byte reads fall on 64 distinct banks)

__global__ void k_c3t_prep_w2(const float *__restrict__ w2, float *__restrict__ wk, int dgrad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // index into w2 [128][64][27]
    if (i >= 128 * 64 * 27) return;
    const int tap = i % 27, c = (i / 27) % 64, o = i / (27 * 64);
    if (dgrad) wk[((26 - tap) * 128 + o) * 64 + c] = w2[i];   // flipped kernel, reduction over o
    else wk[(tap * 64 + c) * 128 + o] = w2[i];
}

__global__ void k_c3t_prep_w1(const float *__restrict__ w1, float *__restrict__ wk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // index into wk [49][8][64]
    if (i >= 49 * 8 * 64) return;
    const int o = i & 63, kx = (i >> 6) & 7, row = i >> 9;
    wk[i] = kx < 7 ? w1[o * 343 + row * 7 + kx] : 0.f;
}

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void k_c3t_conv(const float *__restrict__ src, const float *__restrict__ wk, const float *__restrict__ bias,
                                                  float *__restrict__ dst, int D, int H, int W, int tiles_x, int tiles_plane) {
    __shared__ __attribute__((aligned(16))) float sm[C3T_APIX * C3T_VS];
    constexpr int NT = COUT / 64;                             // 16-channel N tiles per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 15, kg = lane >> 4;
    const int t = blockIdx.x % tiles_plane, bz = blockIdx.x / tiles_plane, z = bz % D, b = bz / D;
    const int ty = t / tiles_x, tx = t - ty * tiles_x, r0 = ty * C3T_TH, c0 = tx * C3T_TW;
    const int ob = wave * 16 * NT + px;
    const size_t plane = (size_t)H * W;

    c3t_f32x4 acc[8][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float bb = bias ? bias[ob + 16 * nt] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) acc[mt][nt] = c3t_f32x4{bb, bb, bb, bb};
    }
    for (int kz = 0; kz < 3; ++kz) {
        const int zz = z + kz - 1;
        if (zz < 0 || zz >= D) continue;                      // block-uniform: a plane outside the volume adds nothing
        const float *sp = src + ((size_t)b * D + zz) * plane * CIN;
        for (int h = 0; h < CIN / 64; ++h) {
            __syncthreads();                                  // the previous plane's readers are done
            for (int idx = tid; idx < C3T_APIX * 16; idx += 256) {
                const int q = idx & 15, p = idx >> 4, row = p / C3T_AW, col = p - row * C3T_AW;
                const int yy = r0 - 1 + row, xx = c0 - 1 + col;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = *reinterpret_cast<const float4 *>(sp + ((size_t)yy * W + xx) * CIN + h * 64 + 4 * q);
                *reinterpret_cast<float4 *>(sm + p * C3T_VS + 4 * q) = v;
            }
            __syncthreads();
            const float *wp = wk + ((size_t)(kz * 9) * CIN + h * 64 + 4 * kg) * COUT + ob;
            // a fresh accumulator per window row (ky: 3 taps x 64 channels = 192 terms), added to the running sum once: the rounding error
            // of the fp32 chain grows with the length of a chain (1,728 terms in one chain measured 1.7e-6 of the output's range)
#pragma unroll 1
            for (int ky = 0; ky < 3; ++ky) {
                c3t_f32x4 part[8][NT];
#pragma unroll
                for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) part[mt][nt] = c3t_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
                for (int kx = 0; kx < 3; ++kx) {
                    const float *wt = wp + (size_t)(ky * 3 + kx) * CIN * COUT;
                    const float *ap = sm + (ky * C3T_AW + px + kx) * C3T_VS + 4 * kg;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {             // 16 channels: lane group kg holds channels 16 j + 4 kg + s, MFMA s takes element s
                        float bw[NT][4];
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt) bw[nt][s] = wt[(16 * j + s) * COUT + 16 * nt];
                        float av[8][4];
#pragma unroll
                        for (int mt = 0; mt < 8; ++mt) {
                            const float4 a = *reinterpret_cast<const float4 *>(ap + mt * (C3T_AW * C3T_VS) + 16 * j);
                            av[mt][0] = a.x; av[mt][1] = a.y; av[mt][2] = a.z; av[mt][3] = a.w;
                        }
                        // consecutive MFMAs go to different accumulators (a dependent one waits 40 cycles, an independent one issues after 32)
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                                for (int nt = 0; nt < NT; ++nt)
                                    part[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][s], bw[nt][s], part[mt][nt], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] += part[mt][nt];
            }
        }
    }
    float *dp = dst + (((size_t)b * D + z) * plane) * COUT;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) dp[((size_t)(r0 + mt) * W + c0 + 4 * kg + i) * COUT + ob + 16 * nt] = acc[mt][nt][i];
}

constexpr int C1T_ROWS = C3T_TH + 6, C1T_RW = 24, C1T_PLANE = C1T_ROWS * C1T_RW;     // 14 rows of 24 (22 used; the rest zero)

__global__ __launch_bounds__(256) void k_c3t_conv1(const float *__restrict__ vol, const float *__restrict__ wk, const float *__restrict__ bias,
                                                   float *__restrict__ z1, int D, int H, int W, int tiles_x, int tiles_plane) {
    __shared__ float sm[7 * C1T_PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 15, kg = lane >> 4;
    const int t = blockIdx.x % tiles_plane, bz = blockIdx.x / tiles_plane, z = bz % D, b = bz / D;
    const int ty = t / tiles_x, tx = t - ty * tiles_x, r0 = ty * C3T_TH, c0 = tx * C3T_TW;
    const int o = wave * 16 + px;
    const size_t plane = (size_t)H * W;
    for (int idx = tid; idx < 7 * C1T_PLANE; idx += 256) {
        const int pz = idx / C1T_PLANE, rem = idx - pz * C1T_PLANE, row = rem / C1T_RW, col = rem - row * C1T_RW;
        const int zz = z - 3 + pz, yy = r0 - 3 + row, xx = c0 - 3 + col;
        float v = 0.f;
        if (col < C3T_TW + 6 && zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W) v = vol[((size_t)b * D + zz) * plane + (size_t)yy * W + xx];
        sm[idx] = v;
    }
    __syncthreads();
    const float bo = bias ? bias[o] : 0.f;
    c3t_f32x4 acc[8];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) acc[mt] = c3t_f32x4{bo, bo, bo, bo};
#pragma unroll 1
    for (int kz = 0; kz < 7; ++kz) {
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const float *wr = wk + ((kz * 7 + ky) * 8 + kg) * 64 + o;
            const float *ap = sm + kz * C1T_PLANE + ky * C1T_RW + px + kg;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {                  // kx = 4 hh + kg
                const float bw = wr[hh * 4 * 64];
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[mt * C1T_RW + 4 * hh], bw, acc[mt], 0, 0, 0);
            }
        }
    }
    float *dp = z1 + (((size_t)b * D + z) * plane) * 64;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) dp[((size_t)(r0 + mt) * W + c0 + 4 * kg + i) * 64 + o] = acc[mt][i];
}

// ------------------------------------------------------------------------------------------------------------------ conv1 data gradient
// dvol[z][y][x] = sum over c, kz, ky, kx of dz1[z + 3 - kz][y + 3 - ky][x + 3 - kx][c] w[c][kz][ky][kx] (out-of-volume terms zero): one output
// channel, so a plain implicit GEMM would have N = 1.  The MFMA is filled instead with a Toeplitz operand in y and a pair of output planes:
// a workgroup owns the 8 x 16 tile of the planes z0, z0 + 1 and marches over the eight dz1 planes zz = z0 - 3 .. z0 + 4 that reach them.  Per
// staged plane (its 14 x 22 halo tile, 64 channels, in LDS) and per kx
//     M = the 16 output columns x          A[x][(hr, c)]      = dz1[zz][halo row hr][halo column x + 6 - kx][c]
//     N = 8 output rows r x 2 planes dp     B[(hr, c)][(r, dp)] = w[c][kz = z0 + dp + 3 - zz][ky = r + 6 - hr][kx], zero outside the kernel
//     K = 14 halo rows x 64 channels
// i.e. 8 x 7 x 14 x 16 = 12,544 MFMAs per 256 voxels, 2.3 x the counted FLOP (the zeros of B).  B is never stored expanded: a lane reads the one
// weight row its (r, dp, hr) selects from the plane's two kz slices in LDS, or takes zero.  Wave w owns channels 16 w .. 16 w + 15 (lane group kg:
// 16 w + 4 kg + s, MFMA s takes element s of one 16-byte read); the four waves' partial tiles are added in wave order through LDS.  Every plane's
// products go to fresh accumulators (four, one per s: independent MFMA chains) that join the running sum once, as in k_c3t_conv.  No atomics;
// every dvol element is written once; the order of every sum is fixed by the shape alone.
constexpr int D1_ROWS = C3T_TH + 6, D1_COLS = C3T_TW + 6, D1_PIX = D1_ROWS * D1_COLS;        // halo tile 14 x 22 = 308 voxels
constexpr int D1_WROWS = 2 * 49;                              // staged weight rows: [dp][ky * 7 + kx], 64 channels each
constexpr int D1_SM_FLOATS = (D1_PIX + D1_WROWS) * C3T_VS;    // 110,432 B: one workgroup per CU

__global__ void k_c3t_prep_w1_dgrad(const float *__restrict__ w1, float *__restrict__ wk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // index into wk [343 taps][64]
    if (i >= 343 * 64) return;
    wk[i] = w1[(i & 63) * 343 + (i >> 6)];
}

__global__ __launch_bounds__(256) void k_c3t_conv1_dgrad(const float *__restrict__ dz1, const float *__restrict__ wk, float *__restrict__ dvol, int D,
                                                         int H, int W, int tiles_x, int tiles_plane, int zpairs) {
    __shared__ __attribute__((aligned(16))) float sm[D1_SM_FLOATS];
    float *wl = sm + D1_PIX * C3T_VS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 15, kg = lane >> 4;
    const int t = blockIdx.x % tiles_plane, bz = blockIdx.x / tiles_plane, z0 = 2 * (bz % zpairs), b = bz / zpairs;
    const int ty = t / tiles_x, tx = t - ty * tiles_x, r0 = ty * C3T_TH, c0 = tx * C3T_TW;
    const int r = px & 7, dp = px >> 3, ch = 16 * wave + 4 * kg;
    const size_t plane = (size_t)H * W;

    // the planes that exist (block-uniform: a plane outside the volume adds nothing); plane p + 1 is loaded into registers under plane p's MFMAs
    const int p_lo = z0 < 3 ? 3 - z0 : 0, p_hi = D + 2 - z0 < 7 ? D + 2 - z0 : 7;
    constexpr int NA = (D1_PIX * 16 + 255) / 256, NW = (D1_WROWS * 16 + 255) / 256;
    float4 pre[NA], wpre[NW];
    auto fetch = [&](int p) {
        const float *sp = dz1 + ((size_t)b * D + (z0 - 3 + p)) * plane * 64;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + 256 * i, q = idx & 15, v = idx >> 4, row = v / D1_COLS, col = v - row * D1_COLS;
            const int yy = r0 - 3 + row, xx = c0 - 3 + col;
            pre[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (v < D1_PIX && yy >= 0 && yy < H && xx >= 0 && xx < W) pre[i] = *reinterpret_cast<const float4 *>(sp + ((size_t)yy * W + xx) * 64 + 4 * q);
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {                        // the two kz slices this plane carries: kz = 6 - p (plane z0), 7 - p (z0 + 1)
            const int idx = tid + 256 * i, q = idx & 15, row = idx >> 4, kz = 6 - p + row / 49;
            wpre[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < D1_WROWS && kz >= 0 && kz < 7) wpre[i] = *reinterpret_cast<const float4 *>(wk + ((size_t)kz * 49 + row % 49) * 64 + 4 * q);
        }
    };
    c3t_f32x4 acc = c3t_f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(p_lo);
    for (int p = p_lo; p <= p_hi; ++p) {
        __syncthreads();                                      // the previous plane's readers are done
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + 256 * i;
            if (idx < D1_PIX * 16) *reinterpret_cast<float4 *>(sm + (idx >> 4) * C3T_VS + 4 * (idx & 15)) = pre[i];
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + 256 * i;
            if (idx < D1_WROWS * 16) *reinterpret_cast<float4 *>(wl + (idx >> 4) * C3T_VS + 4 * (idx & 15)) = wpre[i];
        }
        __syncthreads();
        if (p < p_hi) fetch(p + 1);                           // in flight until the next plane's LDS writes: no barrier in between
        c3t_f32x4 part[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) part[s] = c3t_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int hr = 0; hr < D1_ROWS; ++hr) {
            const int ky = r + 6 - hr;
            const bool in = ky >= 0 && ky < 7;                // outside: this lane's B column is zero for the whole halo row
            const float *ap = sm + (hr * D1_COLS + px + 6) * C3T_VS + ch;
            const float *bp = wl + ((dp * 49 + (in ? ky : 0) * 7)) * C3T_VS + ch;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float4 a = *reinterpret_cast<const float4 *>(ap - kx * C3T_VS);
                float4 w = *reinterpret_cast<const float4 *>(bp + kx * C3T_VS);
                if (!in) w = make_float4(0.f, 0.f, 0.f, 0.f);
                part[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, part[0], 0, 0, 0);
                part[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, part[1], 0, 0, 0);
                part[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, part[2], 0, 0, 0);
                part[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, part[3], 0, 0, 0);
            }
        }
        acc += (part[0] + part[1]) + (part[2] + part[3]);
    }
    __syncthreads();                                          // the last plane's readers are done: its space takes the four waves' tiles
    *reinterpret_cast<float4 *>(sm + (wave * 64 + lane) * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    if (tid < 64 && z0 + dp < D) {                            // lane (px, kg) holds dvol[z0 + dp][r0 + r][c0 + 4 kg .. + 3]
        float4 o = *reinterpret_cast<const float4 *>(sm + tid * 4);
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            const float4 v = *reinterpret_cast<const float4 *>(sm + (wv * 64 + tid) * 4);
            o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
        }
        *reinterpret_cast<float4 *>(dvol + ((size_t)b * D + z0 + dp) * plane + (size_t)(r0 + r) * W + c0 + 4 * kg) = o;
    }
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
constexpr int WG_DZS = 48, WG_AS = 80;                        // floats per staged dz2 row (32 + 16) and a1 voxel (64 + 16): the four k groups of a read fall on disjoint banks
constexpr int WG_PART = 128 * 27 * 64;                        // one stream's partial [o][tap][c]

__global__ __launch_bounds__(256) void k_c3t_wgrad(const float *__restrict__ dz, const float *__restrict__ a1, float *__restrict__ part,
                                                   float *__restrict__ dbpart, int D, int H, int W, int tiles_x, int tiles_plane, int total, int S) {
    __shared__ __attribute__((aligned(16))) float dzs[128 * WG_DZS];
    __shared__ __attribute__((aligned(16))) float as[C3T_APIX * WG_AS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 15, kg = lane >> 4;
    const int s = blockIdx.x, og = blockIdx.y & 3, kz = blockIdx.y >> 2;
    const size_t plane = (size_t)H * W;
    c3t_f32x4 acc[2][9];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9) acc[m][t9] = c3t_f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;
    for (int tile = s; tile < total; tile += S) {
        const int t = tile % tiles_plane, bz = tile / tiles_plane, z = bz % D, b = bz / D;
        const int zz = z + kz - 1;
        if (zz < 0 || zz >= D) continue;                      // block-uniform
        const int ty = t / tiles_x, tx = t - ty * tiles_x, r0 = ty * C3T_TH, c0 = tx * C3T_TW;
        __syncthreads();                                      // the previous tile's readers are done
        const float *dzp = dz + (((size_t)b * D + z) * plane) * 128 + og * 32;
        for (int idx = tid; idx < 128 * 8; idx += 256) {
            const int q = idx & 7, v = idx >> 3;
            *reinterpret_cast<float4 *>(dzs + v * WG_DZS + 4 * q) =
                *reinterpret_cast<const float4 *>(dzp + ((size_t)(r0 + (v >> 4)) * W + c0 + (v & 15)) * 128 + 4 * q);
        }
        const float *ap = a1 + (((size_t)b * D + zz) * plane) * 64;
        for (int idx = tid; idx < C3T_APIX * 16; idx += 256) {
            const int q = idx & 15, p = idx >> 4, row = p / C3T_AW, col = p - row * C3T_AW;
            const int yy = r0 - 1 + row, xx = c0 - 1 + col;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = *reinterpret_cast<const float4 *>(ap + ((size_t)yy * W + xx) * 64 + 4 * q);
            *reinterpret_cast<float4 *>(as + p * WG_AS + 4 * q) = v;
        }
        __syncthreads();
        if (kz == 1) {                                        // the bias gradient: column sums of dz2, voxels in order within this thread's 16
            const int o = tid & 31, p0 = (tid >> 5) * 16;
#pragma unroll
            for (int v = 0; v < 16; ++v) dbacc += dzs[(p0 + v) * WG_DZS + o];
        }
#pragma unroll 2
        for (int ks = 0; ks < 32; ++ks) {                     // 4 voxels per step: row ks >> 2, columns 4 (ks & 3) + kg
            const int r = ks >> 2, x = 4 * (ks & 3) + kg;
            const float d0 = dzs[(r * 16 + x) * WG_DZS + px], d1 = dzs[(r * 16 + x) * WG_DZS + 16 + px];
            const float *bp = as + (r * C3T_AW + x) * WG_AS + 16 * wave + px;
#pragma unroll
            for (int t9 = 0; t9 < 9; ++t9) {
                const float bv = bp[((t9 / 3) * C3T_AW + t9 % 3) * WG_AS];
                acc[0][t9] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0, bv, acc[0][t9], 0, 0, 0);
                acc[1][t9] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1, bv, acc[1][t9], 0, 0, 0);
            }
        }
    }
    float *pp = part + (size_t)s * WG_PART;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
            for (int i = 0; i < 4; ++i) pp[((og * 32 + m * 16 + 4 * kg + i) * 27 + kz * 9 + t9) * 64 + 16 * wave + px] = acc[m][t9][i];
    if (kz == 1) {
        __syncthreads();
        dzs[tid] = dbacc;
        __syncthreads();
        if (tid < 32) {
            float sum = 0.f;
#pragma unroll
            for (int p = 0; p < 8; ++p) sum += dzs[p * 32 + tid];
            dbpart[s * 128 + og * 32 + tid] = sum;
        }
    }
}

__global__ void k_c3t_wgrad_finish(const float *__restrict__ part, const float *__restrict__ dbpart, float *__restrict__ dw, float *__restrict__ db,
                                   int S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // index into a partial [o][tap][c]
    if (i < WG_PART) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += part[(size_t)s * WG_PART + i];
        const int c = i & 63, tap = (i >> 6) % 27, o = i / (27 * 64);
        dw[(o * 64 + c) * 27 + tap] = sum;
    }
    if (db && i < 128) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += dbpart[s * 128 + i];
        db[i] = sum;
    }
}

int conv3d_wgrad_streams(long long tiles) { return (int)(tiles < 64 ? tiles : 64); }
size_t conv3d_wgrad_workspace_bytes(int B, int D, int H, int W) {
    const long long tiles = (long long)B * D * (H / C3T_TH) * (W / C3T_TW);
    return (size_t)conv3d_wgrad_streams(tiles) * (WG_PART + 128) * sizeof(float);
}

hipError_t launch_conv3d_cl_train_forward(const float *a1, const float *w2, const float *bias, int B, int D, int H, int W, float *z2, void *ws,
                                          hipStream_t st) {
    if (!conv3d_train_shape_ok(B, D, H, W)) return hipErrorInvalidValue;
    float *wk = static_cast<float *>(ws);
    hipLaunchKernelGGL(k_c3t_prep_w2, dim3((128 * 64 * 27 + 255) / 256), dim3(256), 0, st, w2, wk, 0);
    const int tiles_x = W / C3T_TW, tiles_plane = tiles_x * (H / C3T_TH);
    hipLaunchKernelGGL((k_c3t_conv<64, 128>), dim3((unsigned)((long long)B * D * tiles_plane)), dim3(256), 0, st, a1, wk, bias, z2, D, H, W, tiles_x,
                       tiles_plane);
    return hipGetLastError();
}

hipError_t launch_conv3d_cl_dgrad(const float *dz2, const float *w2, int B, int D, int H, int W, float *da1, void *ws, hipStream_t st) {
    if (!conv3d_train_shape_ok(B, D, H, W)) return hipErrorInvalidValue;
    float *wk = static_cast<float *>(ws);
    hipLaunchKernelGGL(k_c3t_prep_w2, dim3((128 * 64 * 27 + 255) / 256), dim3(256), 0, st, w2, wk, 1);
    const int tiles_x = W / C3T_TW, tiles_plane = tiles_x * (H / C3T_TH);
    hipLaunchKernelGGL((k_c3t_conv<128, 64>), dim3((unsigned)((long long)B * D * tiles_plane)), dim3(256), 0, st, dz2, wk, (const float *)nullptr, da1, D,
                       H, W, tiles_x, tiles_plane);
    return hipGetLastError();
}

hipError_t launch_conv3d_cl_wgrad(const float *dz2, const float *a1, int B, int D, int H, int W, float *dw, float *db, void *ws, hipStream_t st) {
    if (!conv3d_train_shape_ok(B, D, H, W)) return hipErrorInvalidValue;
    const int tiles_x = W / C3T_TW, tiles_plane = tiles_x * (H / C3T_TH);
    const long long total = (long long)B * D * tiles_plane;
    const int S = conv3d_wgrad_streams(total);
    float *part = static_cast<float *>(ws), *dbpart = part + (size_t)S * WG_PART;
    hipLaunchKernelGGL(k_c3t_wgrad, dim3(S, 12), dim3(256), 0, st, dz2, a1, part, dbpart, D, H, W, tiles_x, tiles_plane, (int)total, S);
    hipLaunchKernelGGL(k_c3t_wgrad_finish, dim3((WG_PART + 255) / 256), dim3(256), 0, st, part, dbpart, dw, db, S);
    return hipGetLastError();
}

hipError_t launch_conv3d_s7_train_forward(const float *vol, const float *w1, const float *bias, int B, int D, int H, int W, float *z1, void *ws,
                                          hipStream_t st) {
    if (!conv3d_train_shape_ok(B, D, H, W)) return hipErrorInvalidValue;
    float *wk = static_cast<float *>(ws);
    hipLaunchKernelGGL(k_c3t_prep_w1, dim3((49 * 8 * 64 + 255) / 256), dim3(256), 0, st, w1, wk);
    const int tiles_x = W / C3T_TW, tiles_plane = tiles_x * (H / C3T_TH);
    hipLaunchKernelGGL(k_c3t_conv1, dim3((unsigned)((long long)B * D * tiles_plane)), dim3(256), 0, st, vol, wk, bias, z1, D, H, W, tiles_x, tiles_plane);
    return hipGetLastError();
}

hipError_t launch_conv3d_s7_dgrad(const float *dz1, const float *w1, int B, int D, int H, int W, float *dvol, void *ws, hipStream_t st) {
    if (!conv3d_train_shape_ok(B, D, H, W)) return hipErrorInvalidValue;
    float *wk = static_cast<float *>(ws);
    hipLaunchKernelGGL(k_c3t_prep_w1_dgrad, dim3((343 * 64 + 255) / 256), dim3(256), 0, st, w1, wk);
    const int tiles_x = W / C3T_TW, tiles_plane = tiles_x * (H / C3T_TH), zpairs = (D + 1) / 2;
    hipLaunchKernelGGL(k_c3t_conv1_dgrad, dim3((unsigned)((long long)B * zpairs * tiles_plane)), dim3(256), 0, st, dz1, wk, dvol, D, H, W, tiles_x,
                       tiles_plane, zpairs);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ BatchNorm phases
constexpr int BNCL_MAXG = 1024;                               // workgroups (= partial rows) of a reduction pass

struct BnGeom {
    long long M;                                              // rows = B * D * H * W
    int D, H, W, bh, bw;                                      // token block (H / 32) x (W / 32)
    float inv_n;                                              // 1 / (D * bh * bw)
};

// token-gradient row of voxel row m (pooled): [b][(y / bh) * 32 + x / bw]
__device__ __forceinline__ long long bncl_token_row(const BnGeom &g, long long m) {
    const int x = (int)(m % g.W);
    const long long r = m / g.W;
    const int y = (int)(r % g.H);
    const long long b = r / g.H / g.D;
    return b * 1024 + (y / g.bh) * 32 + x / g.bw;
}

// MODE 0: sum z, sum z^2.  MODE 1: sum dy [y > 0], sum dy [y > 0] zhat.  Partials ws [G][2][C] fp64.
template <int C, int MODE, int POOLED>
__global__ __launch_bounds__(256) void k_bncl_reduce(const float *__restrict__ z, const float *__restrict__ dout, BnGeom g,
                                                     const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                                     const float *__restrict__ rstd, double *__restrict__ ws) {
    constexpr int L = C / 4, R = 256 / L;
    __shared__ double red[256][8];
    const int tid = threadIdx.x, q = tid % L, rr = tid / L;
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    float mu[4], rs[4], sc[4], be[4];
    if (MODE == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mu[i] = mean[4 * q + i]; rs[i] = rstd[4 * q + i]; sc[i] = gamma[4 * q + i] * rs[i]; be[i] = beta[4 * q + i];
        }
    }
    for (long long m = (long long)blockIdx.x * R + rr; m < g.M; m += (long long)gridDim.x * R) {
        const float4 zv = *reinterpret_cast<const float4 *>(z + m * C + 4 * q);
        const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s0[i] += (double)zz[i];
                s1[i] += (double)zz[i] * (double)zz[i];
            }
        } else {
            const float4 dv = *reinterpret_cast<const float4 *>(dout + (POOLED ? bncl_token_row(g, m) : m) * C + 4 * q);
            const float dd[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dy = ((zz[i] - mu[i]) * sc[i] + be[i] > 0.f) ? (POOLED ? dd[i] * g.inv_n : dd[i]) : 0.f;
                s0[i] += (double)dy;
                s1[i] += (double)dy * (double)((zz[i] - mu[i]) * rs[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        red[tid][i] = s0[i];
        red[tid][4 + i] = s1[i];
    }
    __syncthreads();
    if (tid < C) {                                            // channel tid: its lane group's R row slots in order
        const int qq = tid >> 2, i = tid & 3;
        double a = 0, b2 = 0;
        for (int r = 0; r < R; ++r) {
            a += red[r * L + qq][i];
            b2 += red[r * L + qq][4 + i];
        }
        ws[((size_t)blockIdx.x * 2) * C + tid] = a;
        ws[((size_t)blockIdx.x * 2 + 1) * C + tid] = b2;
    }
}

// MODE 0 -> mean / var (biased) / rstd; MODE 1 -> dbeta, dgamma.  One workgroup of 64 lanes per channel: lane l adds the partials l, l + 64, ...
// in order, lane 0 then adds the 64 lane sums in lane order -- a fixed order (one thread walking 1,024 partials was 0.27 ms of latency).
__global__ __launch_bounds__(64) void k_bncl_finish(const double *__restrict__ ws, int G, int C, int mode, double count, double eps,
                                                    float *__restrict__ o0, float *__restrict__ o1, float *__restrict__ o2) {
    __shared__ double red[2][64];
    const int c = blockIdx.x, l = threadIdx.x;
    double a = 0, b = 0;
    for (int gI = l; gI < G; gI += 64) {
        a += ws[((size_t)gI * 2) * C + c];
        b += ws[((size_t)gI * 2 + 1) * C + c];
    }
    red[0][l] = a;
    red[1][l] = b;
    __syncthreads();
    if (l != 0) return;
    a = b = 0;
    for (int i = 0; i < 64; ++i) {
        a += red[0][i];
        b += red[1][i];
    }
    if (mode == 0) {
        const double mu = a / count;
        double var = b / count - mu * mu;
        var = var > 0 ? var : 0;
        o0[c] = (float)mu;
        o1[c] = (float)var;
        o2[c] = (float)(1.0 / sqrt(var + eps));
    } else {
        o0[c] = (float)a;                                     // dbeta
        o1[c] = (float)b;                                     // dgamma
    }
}

// MODE 0: out = relu(bn(z)).  MODE 1: dz = gamma rstd (dy [y > 0] - dbeta / count - zhat dgamma / count).
template <int C, int MODE, int POOLED>
__global__ __launch_bounds__(256) void k_bncl_rows(const float *__restrict__ z, const float *__restrict__ dout, BnGeom g,
                                                   const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                                   const float *__restrict__ rstd, const float *__restrict__ dgamma, const float *__restrict__ dbeta,
                                                   float inv_count, float *__restrict__ out) {
    constexpr int L = C / 4, R = 256 / L;
    const int tid = threadIdx.x, q = tid % L, rr = tid / L;
    float mu[4], rs[4], sc[4], be[4], k0[4], k1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mu[i] = mean[4 * q + i]; rs[i] = rstd[4 * q + i]; sc[i] = gamma[4 * q + i] * rs[i]; be[i] = beta[4 * q + i];
        k0[i] = MODE ? dbeta[4 * q + i] * inv_count : 0.f;
        k1[i] = MODE ? dgamma[4 * q + i] * inv_count : 0.f;
    }
    for (long long m = (long long)blockIdx.x * R + rr; m < g.M; m += (long long)gridDim.x * R) {
        const float4 zv = *reinterpret_cast<const float4 *>(z + m * C + 4 * q);
        const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
        float o[4];
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = __builtin_fmaxf((zz[i] - mu[i]) * sc[i] + be[i], 0.f);
        } else {
            const float4 dv = *reinterpret_cast<const float4 *>(dout + (POOLED ? bncl_token_row(g, m) : m) * C + 4 * q);
            const float dd[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dy = ((zz[i] - mu[i]) * sc[i] + be[i] > 0.f) ? (POOLED ? dd[i] * g.inv_n : dd[i]) : 0.f;
                o[i] = sc[i] * (dy - k0[i] - (zz[i] - mu[i]) * rs[i] * k1[i]);
            }
        }
        *reinterpret_cast<float4 *>(out + m * C + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// token sums [B][1024][C] of relu(bn(z)): one thread per (b, token, four channels), its D x bh x bw voxels added in memory order in fp64
template <int C>
__global__ __launch_bounds__(256) void k_bncl_apply_tokens(const float *__restrict__ z, BnGeom g, int B, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ mean,
                                                           const float *__restrict__ rstd, float *__restrict__ out) {
    constexpr int L = C / 4;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)B * 1024 * L) return;
    const int q = (int)(id % L), tok = (int)(id / L % 1024);
    const long long b = id / L / 1024;
    const int ty = tok >> 5, tx = tok & 31;
    float mu[4], sc[4], be[4];
    double acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mu[i] = mean[4 * q + i]; sc[i] = gamma[4 * q + i] * rstd[4 * q + i]; be[i] = beta[4 * q + i];
    }
    for (int zI = 0; zI < g.D; ++zI)
        for (int y = ty * g.bh; y < (ty + 1) * g.bh; ++y) {
            const float *row = z + (((b * g.D + zI) * g.H + y) * g.W + (long long)tx * g.bw) * C + 4 * q;
            for (int x = 0; x < g.bw; ++x) {
                const float4 zv = *reinterpret_cast<const float4 *>(row + (long long)x * C);
                const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += (double)__builtin_fmaxf((zz[i] - mu[i]) * sc[i] + be[i], 0.f);
            }
        }
    *reinterpret_cast<float4 *>(out + id * 4) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
}

static int bncl_groups(long long M, int C) {
    const int R = 256 / (C / 4);
    const long long need = (M + R - 1) / R;
    return (int)(need < BNCL_MAXG ? need : BNCL_MAXG);
}
size_t bn_cl_workspace_bytes(long long M, int C) { return (size_t)bncl_groups(M, C) * 2 * C * sizeof(double); }

template <int C>
static hipError_t bncl_phase(int phase, const float *z, const float *dout, int B, const BnGeom &g, int pooled, const float *gamma, const float *beta,
                             double eps, float *mean, float *var, float *rstd, float *out, float *dz, float *dgamma, float *dbeta, double count,
                             void *ws, hipStream_t st) {
    const int G = bncl_groups(g.M, C);
    double *wsd = static_cast<double *>(ws);
    const dim3 blk(256);
    switch (phase) {
    case SMK_BN_STATS:
        hipLaunchKernelGGL((k_bncl_reduce<C, 0, 0>), dim3(G), blk, 0, st, z, dout, g, gamma, beta, mean, rstd, wsd);
        hipLaunchKernelGGL(k_bncl_finish, dim3(C), dim3(64), 0, st, wsd, G, C, 0, (double)g.M, eps, mean, var, rstd);
        break;
    case SMK_BN_APPLY:
        if (pooled) hipLaunchKernelGGL(k_bncl_apply_tokens<C>, dim3((unsigned)(((long long)B * 1024 * (C / 4) + 255) / 256)), blk, 0, st, z, g, B, gamma, beta, mean, rstd, out);
        else hipLaunchKernelGGL((k_bncl_rows<C, 0, 0>), dim3(G), blk, 0, st, z, dout, g, gamma, beta, mean, rstd, dgamma, dbeta, 0.f, out);
        break;
    case SMK_BN_BWD_SUMS:
        if (pooled) hipLaunchKernelGGL((k_bncl_reduce<C, 1, 1>), dim3(G), blk, 0, st, z, dout, g, gamma, beta, mean, rstd, wsd);
        else hipLaunchKernelGGL((k_bncl_reduce<C, 1, 0>), dim3(G), blk, 0, st, z, dout, g, gamma, beta, mean, rstd, wsd);
        hipLaunchKernelGGL(k_bncl_finish, dim3(C), dim3(64), 0, st, wsd, G, C, 1, 1.0, eps, dbeta, dgamma, (float *)nullptr);
        break;
    case SMK_BN_BWD_DZ:
        if (pooled) hipLaunchKernelGGL((k_bncl_rows<C, 1, 1>), dim3(G), blk, 0, st, z, dout, g, gamma, beta, mean, rstd, dgamma, dbeta, (float)(1.0 / count), dz);
        else hipLaunchKernelGGL((k_bncl_rows<C, 1, 0>), dim3(G), blk, 0, st, z, dout, g, gamma, beta, mean, rstd, dgamma, dbeta, (float)(1.0 / count), dz);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_bn_cl_phase(int phase, const float *z, const float *dout, int B, int D, int H, int W, int C, int pooled, const float *gamma,
                              const float *beta, double eps, float *mean, float *var, float *rstd, float *out, float *dz, float *dgamma,
                              float *dbeta, double count, void *ws, hipStream_t st) {
    BnGeom g;
    g.M = (long long)B * D * H * W;
    g.D = D; g.H = H; g.W = W;
    g.bh = pooled ? H / 32 : 1; g.bw = pooled ? W / 32 : 1;
    g.inv_n = 1.f / (float)((long long)D * g.bh * g.bw);
    if (C == 64) return bncl_phase<64>(phase, z, dout, B, g, pooled, gamma, beta, eps, mean, var, rstd, out, dz, dgamma, dbeta, count, ws, st);
    if (C == 128) return bncl_phase<128>(phase, z, dout, B, g, pooled, gamma, beta, eps, mean, var, rstd, out, dz, dgamma, dbeta, count, ws, st);
    return hipErrorInvalidValue;
}

}  // namespace smk
