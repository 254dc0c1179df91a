// SmokePhysNet.reconstruction_head (smokephys_net.py:57-66,117-118) in TRAINING mode: the three convolutions under autograd, plain fp32 FMAs
// on the vector ALUs.  The BatchNorms between them run on the training-mode kernels of norm.hip (batch statistics), so nothing folds here:
//   ConvTranspose2d(CIN, COUT, 4, 2, 1):  forward z = conv + bias (raw), data gradient, weight / bias gradients
//   Conv2d(16, 1, 3, padding 1) + Sigmoid: forward y, and from dY and y the data, weight and bias gradients
// No float atomics anywhere: every reduction is per-workgroup partials in a workspace, added in a fixed order by a second launch, so
// repeated calls are bit-identical.  The eval kernels (decoder.hip, BatchNorm folded) are separate and unchanged.
#include "decoder_train.h"

namespace smk {

// ---------------------------------------------------------------------------------------------------------------------------------------
// ConvT forward: the 2 x 2-phase tap decomposition of k_convt4s2 (decoder.hip).  y = 2 iy - 1 + ky, so output row parity 0 takes
// (ky 1, iy i) and (ky 3, iy i-1), parity 1 takes (ky 0, iy i+1) and (ky 2, iy i); columns likewise.  The thread that owns input position
// (i, j) writes the output quad (2i + py, 2j + px) for OG output channels; weights are wave-uniform (scalar loads).
constexpr int TT = 16;                                        // input positions per tile side (forward, data gradient)
constexpr int TF_CC = 16;                                     // input channels staged per chunk
constexpr int TF_PW = TT + 3;                                 // LDS row pitch (18 used + 1 pad)

template <int COUT, int OG, bool TOK>
__global__ __launch_bounds__(256) void k_convt4s2_train_fwd(const float *__restrict__ in, const float *__restrict__ wt, const float *__restrict__ bias,
                                                           float *__restrict__ z, int CIN, int H, int W) {
    __shared__ float tile[TF_CC][TT + 2][TF_PW];
    const int tid = threadIdx.x, tj = tid & 15, ti = tid >> 4;
    const int tiles_x = W / TT;
    const int i0 = (blockIdx.x / tiles_x) * TT, j0 = (blockIdx.x % tiles_x) * TT;
    const int og = blockIdx.y, b = blockIdx.z;
    const float *inb = in + (size_t)b * CIN * H * W;
    float acc[OG][4];
#pragma unroll
    for (int o = 0; o < OG; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[o][q] = 0.f;

    for (int c0 = 0; c0 < CIN; c0 += TF_CC) {
        __syncthreads();
        if (TOK) {   // 18 x 18 positions x 4 float4 (16 channels): position-major reads, channel-major LDS image
            for (int e = tid; e < (TT + 2) * (TT + 2) * (TF_CC / 4); e += 256) {
                const int c4 = e & 3, p = e >> 2, pr = p / (TT + 2), pc = p - pr * (TT + 2);
                const int ii = i0 - 1 + pr, jj = j0 - 1 + pc;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ii >= 0 && ii < H && jj >= 0 && jj < W)
                    v = *reinterpret_cast<const float4 *>(inb + ((size_t)ii * W + jj) * CIN + c0 + 4 * c4);
                tile[4 * c4 + 0][pr][pc] = v.x; tile[4 * c4 + 1][pr][pc] = v.y;
                tile[4 * c4 + 2][pr][pc] = v.z; tile[4 * c4 + 3][pr][pc] = v.w;
            }
        } else {
            for (int e = tid; e < TF_CC * (TT + 2) * (TT + 2); e += 256) {
                const int pc = e % (TT + 2), rest = e / (TT + 2), pr = rest % (TT + 2), c = rest / (TT + 2);
                const int ii = i0 - 1 + pr, jj = j0 - 1 + pc;
                tile[c][pr][pc] = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? inb[((size_t)(c0 + c) * H + ii) * W + jj] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < TF_CC; ++c) {
            float n[3][3];                                    // n[a][d] = in(i - 1 + a, j - 1 + d)
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int d = 0; d < 3; ++d) n[a][d] = tile[c][ti + a][tj + d];
            const float *wc = wt + ((size_t)(c0 + c) * COUT + og * OG) * 16;
#pragma unroll
            for (int o = 0; o < OG; ++o) {
                const float *k = wc + o * 16;                 // k[ky * 4 + kx]
                acc[o][0] = fmaf(n[1][1], k[5], fmaf(n[1][0], k[7], fmaf(n[0][1], k[13], fmaf(n[0][0], k[15], acc[o][0]))));
                acc[o][1] = fmaf(n[1][2], k[4], fmaf(n[1][1], k[6], fmaf(n[0][2], k[12], fmaf(n[0][1], k[14], acc[o][1]))));
                acc[o][2] = fmaf(n[2][1], k[1], fmaf(n[2][0], k[3], fmaf(n[1][1], k[9], fmaf(n[1][0], k[11], acc[o][2]))));
                acc[o][3] = fmaf(n[2][2], k[0], fmaf(n[2][1], k[2], fmaf(n[1][2], k[8], fmaf(n[1][1], k[10], acc[o][3]))));
            }
        }
    }
    const int i = i0 + ti, j = j0 + tj, OH = 2 * H, OW = 2 * W;
#pragma unroll
    for (int o = 0; o < OG; ++o) {
        const int oc = og * OG + o;
        const float t = bias ? bias[oc] : 0.f;
        float *op = z + (((size_t)b * COUT + oc) * OH + 2 * i) * OW + 2 * j;
        *reinterpret_cast<float2 *>(op) = make_float2(acc[o][0] + t, acc[o][1] + t);
        *reinterpret_cast<float2 *>(op + OW) = make_float2(acc[o][2] + t, acc[o][3] + t);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// ConvT data gradient, gather form: dX[c][i][j] = sum_o sum_{ky,kx} dZ[o][2i-1+ky][2j-1+kx] W[c][o][ky][kx] (taps outside dZ are zero).
// A 16 x 16 tile of input positions reads a 34 x 34 window of dZ, staged TD_CC channels at a time; the thread of position (i, j) takes its
// 4 x 4 window as eight 8-byte LDS reads (even pitch, even column 2 tj) and runs 16 FMAs per (o, c) for OG input channels c.
constexpr int TD_CC = 8;                                      // dZ channels staged per chunk
constexpr int TD_R = 2 * TT + 2;                              // 34 rows / columns of dZ behind a tile
constexpr int TD_PW = TD_R + 2;                               // 36: even, for the float2 reads

template <int COUT, int OG, bool TOK>
__global__ __launch_bounds__(256) void k_convt4s2_train_dgrad(const float *__restrict__ dz, const float *__restrict__ wt, float *__restrict__ dx,
                                                             int CIN, int H, int W) {
    __shared__ __attribute__((aligned(16))) float zs[TD_CC][TD_R][TD_PW];
    const int tid = threadIdx.x, tj = tid & 15, ti = tid >> 4;
    const int tiles_x = W / TT;
    const int i0 = (blockIdx.x / tiles_x) * TT, j0 = (blockIdx.x % tiles_x) * TT;
    const int og = blockIdx.y, b = blockIdx.z, OH = 2 * H, OW = 2 * W;
    const float *dzb = dz + (size_t)b * COUT * OH * OW;
    float acc[OG];
#pragma unroll
    for (int c = 0; c < OG; ++c) acc[c] = 0.f;
    for (int o0 = 0; o0 < COUT; o0 += TD_CC) {
        __syncthreads();
        for (int e = tid; e < TD_CC * TD_R * TD_R; e += 256) {
            const int cc = e % TD_R, rest = e / TD_R, rr = rest % TD_R, oc = rest / TD_R;
            const int y = 2 * i0 - 1 + rr, x = 2 * j0 - 1 + cc;
            zs[oc][rr][cc] = (y >= 0 && y < OH && x >= 0 && x < OW) ? dzb[((size_t)(o0 + oc) * OH + y) * OW + x] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int oc = 0; oc < TD_CC; ++oc) {
            float d[4][4];                                    // d[ky][kx] = dZ[o][2i - 1 + ky][2j - 1 + kx]
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const float2 l = *reinterpret_cast<const float2 *>(&zs[oc][2 * ti + ky][2 * tj]);
                const float2 r = *reinterpret_cast<const float2 *>(&zs[oc][2 * ti + ky][2 * tj + 2]);
                d[ky][0] = l.x; d[ky][1] = l.y; d[ky][2] = r.x; d[ky][3] = r.y;
            }
            const float *wo = wt + ((size_t)(og * OG) * COUT + o0 + oc) * 16;        // wave-uniform: scalar loads
#pragma unroll
            for (int c = 0; c < OG; ++c) {
                const float *k = wo + (size_t)c * COUT * 16;
                float s = acc[c];
#pragma unroll
                for (int q = 0; q < 16; ++q) s = fmaf(d[q >> 2][q & 3], k[q], s);
                acc[c] = s;
            }
        }
    }
    const int i = i0 + ti, j = j0 + tj;
    if (TOK) {
        float *op = dx + ((size_t)b * H * W + (size_t)i * W + j) * CIN + og * OG;
#pragma unroll
        for (int q = 0; q < OG / 4; ++q)
            *reinterpret_cast<float4 *>(op + 4 * q) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < OG; ++c) dx[(((size_t)b * CIN + og * OG + c) * H + i) * W + j] = acc[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// ConvT weight / bias gradients: dW[c][o][ky][kx] = sum_{b,i,j} X[b][c][i][j] dZ[b][o][2i-1+ky][2j-1+kx], db[o] = sum dZ[b][o].
// A GEMM over input positions: a workgroup owns CB input channels and all COUT output channels (thread = 4 channels c x one o x 16 taps,
// 64 accumulators) and walks tiles of 2 x 16 positions, chunk k taking tiles k, k + nchunks, ... in order.  Per tile: the 6 x 34 dZ window
// of every o and X of the tile's 32 positions in LDS; per position one 16-byte X read (a broadcast) and eight 8-byte dZ reads for 64 FMAs.
// db rides along: the taps ky, kx in {1, 2} of all positions cover every dZ pixel exactly once.  Each workgroup stores its partial sums;
// k_train_partials_finish adds them in chunk order.
constexpr int TW_R = 2, TW_C = 16, TW_P = TW_R * TW_C;       // input positions per tile
constexpr int TW_ZR = 2 * TW_R + 2, TW_ZC = 2 * TW_C + 2;    // 6 x 34 dZ window behind a tile
constexpr int TW_ZP = 36;                                     // row pitch (even: float2 reads)
constexpr int TW_PL = 226;                                    // plane pitch >= 6 x 36; 226 = 34 mod 64: lanes o = 0..31 read distinct bank pairs

template <int COUT>
constexpr int convt_wgrad_cb() { return COUT == 32 ? 16 : 32; }   // 128 threads either way

template <int COUT, bool TOK>
__global__ __launch_bounds__(convt_wgrad_cb<COUT>() / 4 * COUT) void k_convt4s2_train_wgrad(const float *__restrict__ dz, const float *__restrict__ x,
                                                                                            int CIN, int H, int W, int tiles_x, int tiles_per_frame,
                                                                                            int ntiles, float *__restrict__ part) {
    constexpr int CB = convt_wgrad_cb<COUT>(), NT = CB / 4 * COUT;
    __shared__ __attribute__((aligned(16))) float zs[COUT * TW_PL];
    __shared__ __attribute__((aligned(16))) float xs[TW_P * CB];
    const int tid = threadIdx.x, o = tid % COUT, cg = tid / COUT, c0 = blockIdx.y * CB;
    const int OH = 2 * H, OW = 2 * W;
    const size_t plane = (size_t)OH * OW;
    float acc[4][16], dbs = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[c][k] = 0.f;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int b = t / tiles_per_frame, rm = t - b * tiles_per_frame;
        const int i0 = (rm / tiles_x) * TW_R, j0 = (rm % tiles_x) * TW_C;
        __syncthreads();
        const float *dzb = dz + (size_t)b * COUT * plane;
        for (int e = tid; e < COUT * TW_ZR * TW_ZC; e += NT) {
            const int cc = e % TW_ZC, rest = e / TW_ZC, rr = rest % TW_ZR, oc = rest / TW_ZR;
            const int y = 2 * i0 - 1 + rr, xx = 2 * j0 - 1 + cc;
            zs[oc * TW_PL + rr * TW_ZP + cc] = (y >= 0 && y < OH && xx >= 0 && xx < OW) ? dzb[(size_t)oc * plane + (size_t)y * OW + xx] : 0.f;
        }
        if (TOK) {
            for (int e = tid; e < TW_P * (CB / 4); e += NT) {
                const int q = e % (CB / 4), p = e / (CB / 4), i = i0 + p / TW_C, j = j0 + p % TW_C;
                *reinterpret_cast<float4 *>(&xs[p * CB + 4 * q]) =
                    *reinterpret_cast<const float4 *>(x + ((size_t)b * H * W + (size_t)i * W + j) * CIN + c0 + 4 * q);
            }
        } else {
            for (int e = tid; e < TW_P * CB; e += NT) {
                const int p = e % TW_P, c = e / TW_P, i = i0 + p / TW_C, j = j0 + p % TW_C;
                xs[p * CB + c] = x[(((size_t)b * CIN + c0 + c) * H + i) * W + j];
            }
        }
        __syncthreads();
        const float *zo = zs + o * TW_PL;
#pragma unroll 2
        for (int p = 0; p < TW_P; ++p) {
            const int r = p / TW_C, cc = p % TW_C;
            const float4 xv = *reinterpret_cast<const float4 *>(&xs[p * CB + 4 * cg]);
            const float xa[4] = {xv.x, xv.y, xv.z, xv.w};
            float d[4][4];
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const float2 l = *reinterpret_cast<const float2 *>(zo + (2 * r + ky) * TW_ZP + 2 * cc);
                const float2 rr = *reinterpret_cast<const float2 *>(zo + (2 * r + ky) * TW_ZP + 2 * cc + 2);
                d[ky][0] = l.x; d[ky][1] = l.y; d[ky][2] = rr.x; d[ky][3] = rr.y;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[c][q] = fmaf(xa[c], d[q >> 2][q & 3], acc[c][q]);
            dbs += (d[1][1] + d[1][2]) + (d[2][1] + d[2][2]);
        }
    }
    const size_t ps = (size_t)CIN * COUT * 16 + COUT;
    float *dst = part + (size_t)blockIdx.x * ps;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float *dc = dst + ((size_t)(c0 + 4 * cg + c) * COUT + o) * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4 *>(dc + 4 * q) = make_float4(acc[c][4 * q], acc[c][4 * q + 1], acc[c][4 * q + 2], acc[c][4 * q + 3]);
    }
    if (blockIdx.y == 0 && cg == 0) dst[(size_t)CIN * COUT * 16 + o] = dbs;
}

// out[i] = sum over k = 0 .. nparts-1 (in that order) of part[k][i]; the first ndw go to dw, the next ndb to db (skipped when db is NULL)
__global__ __launch_bounds__(256) void k_train_partials_finish(const float *__restrict__ part, int nparts, int ndw, int ndb, float *__restrict__ dw,
                                                              float *__restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ndw + ndb) return;
    const size_t ps = (size_t)ndw + ndb;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s += part[(size_t)k * ps + i];
    if (i < ndw) {
        if (dw) dw[i] = s;
    } else if (db) {
        db[i - ndw] = s;
    }
}

bool convt_train_shape_ok(int B, int CIN, int COUT, int H, int W) {
    const int cb = COUT == 32 ? 16 : 32;
    return B >= 1 && B <= 65535 && (COUT == 16 || COUT == 32) && CIN >= cb && CIN % cb == 0 && CIN <= 4096 && H >= 16 && W >= 16 &&
           H % 16 == 0 && W % 16 == 0 && (int64_t)B * COUT * 4 * H * W < (1ll << 31) && (int64_t)B * CIN * H * W < (1ll << 31);
}

static int convt_wgrad_chunks(int B, int CIN, int COUT, int H, int W) {
    const int64_t ntiles = (int64_t)B * (H / TW_R) * (W / TW_C);
    const int cblocks = CIN / (COUT == 32 ? 16 : 32);
    int cap = 1024 / cblocks;
    if (cap < 64) cap = 64;
    return (int)(ntiles < cap ? ntiles : cap);
}

size_t convt_train_wgrad_workspace_bytes(int B, int CIN, int COUT, int H, int W) {
    if (!convt_train_shape_ok(B, CIN, COUT, H, W)) return 0;
    return (size_t)convt_wgrad_chunks(B, CIN, COUT, H, W) * ((size_t)CIN * COUT * 16 + COUT) * sizeof(float);
}

template <int COUT, bool TOK>
static void convt_fwd(const float *x, const float *w, const float *bias, int B, int CIN, int H, int W, float *z, hipStream_t st) {
    const int tiles = (H / TT) * (W / TT);
    if ((int64_t)tiles * (COUT / 8) * B < 1024)             // few workgroups: two output channels each
        hipLaunchKernelGGL((k_convt4s2_train_fwd<COUT, 2, TOK>), dim3(tiles, COUT / 2, B), dim3(256), 0, st, x, w, bias, z, CIN, H, W);
    else
        hipLaunchKernelGGL((k_convt4s2_train_fwd<COUT, 8, TOK>), dim3(tiles, COUT / 8, B), dim3(256), 0, st, x, w, bias, z, CIN, H, W);
}

hipError_t launch_convt_train_forward(const float *x, const float *w, const float *bias, int B, int CIN, int COUT, int H, int W, bool tok,
                                      float *z, hipStream_t st) {
    if (!convt_train_shape_ok(B, CIN, COUT, H, W)) return hipErrorInvalidValue;
    if (COUT == 32) tok ? convt_fwd<32, true>(x, w, bias, B, CIN, H, W, z, st) : convt_fwd<32, false>(x, w, bias, B, CIN, H, W, z, st);
    else tok ? convt_fwd<16, true>(x, w, bias, B, CIN, H, W, z, st) : convt_fwd<16, false>(x, w, bias, B, CIN, H, W, z, st);
    return hipGetLastError();
}

template <int COUT, bool TOK>
static void convt_dgrad(const float *dz, const float *w, int B, int CIN, int H, int W, float *dx, hipStream_t st) {
    const int tiles = (H / TT) * (W / TT);
    if ((int64_t)tiles * (CIN / 16) * B < 1024)             // few workgroups: four input channels each
        hipLaunchKernelGGL((k_convt4s2_train_dgrad<COUT, 4, TOK>), dim3(tiles, CIN / 4, B), dim3(256), 0, st, dz, w, dx, CIN, H, W);
    else
        hipLaunchKernelGGL((k_convt4s2_train_dgrad<COUT, 16, TOK>), dim3(tiles, CIN / 16, B), dim3(256), 0, st, dz, w, dx, CIN, H, W);
}

hipError_t launch_convt_train_dgrad(const float *dz, const float *w, int B, int CIN, int COUT, int H, int W, bool tok, float *dx,
                                    hipStream_t st) {
    if (!convt_train_shape_ok(B, CIN, COUT, H, W)) return hipErrorInvalidValue;
    if (COUT == 32) tok ? convt_dgrad<32, true>(dz, w, B, CIN, H, W, dx, st) : convt_dgrad<32, false>(dz, w, B, CIN, H, W, dx, st);
    else tok ? convt_dgrad<16, true>(dz, w, B, CIN, H, W, dx, st) : convt_dgrad<16, false>(dz, w, B, CIN, H, W, dx, st);
    return hipGetLastError();
}

template <int COUT, bool TOK>
static void convt_wgrad(const float *dz, const float *x, int B, int CIN, int H, int W, int nchunks, float *part, hipStream_t st) {
    constexpr int CB = convt_wgrad_cb<COUT>();
    const int tiles_x = W / TW_C, tiles_per_frame = tiles_x * (H / TW_R);
    hipLaunchKernelGGL((k_convt4s2_train_wgrad<COUT, TOK>), dim3(nchunks, CIN / CB), dim3(CB / 4 * COUT), 0, st, dz, x, CIN, H, W, tiles_x,
                       tiles_per_frame, B * tiles_per_frame, part);
}

hipError_t launch_convt_train_wgrad(const float *dz, const float *x, int B, int CIN, int COUT, int H, int W, bool tok, float *dw, float *db,
                                    void *workspace, hipStream_t st) {
    if (!convt_train_shape_ok(B, CIN, COUT, H, W)) return hipErrorInvalidValue;
    const int nchunks = convt_wgrad_chunks(B, CIN, COUT, H, W);
    float *part = static_cast<float *>(workspace);
    if (COUT == 32) tok ? convt_wgrad<32, true>(dz, x, B, CIN, H, W, nchunks, part, st) : convt_wgrad<32, false>(dz, x, B, CIN, H, W, nchunks, part, st);
    else tok ? convt_wgrad<16, true>(dz, x, B, CIN, H, W, nchunks, part, st) : convt_wgrad<16, false>(dz, x, B, CIN, H, W, nchunks, part, st);
    const int ndw = CIN * COUT * 16;
    hipLaunchKernelGGL(k_train_partials_finish, dim3(cdiv(ndw + COUT, 256)), dim3(256), 0, st, part, nchunks, ndw, COUT, dw, db);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Conv2d(16, 1, 3, padding 1) + Sigmoid.  Tiles of 8 x 32 pixels, one thread per pixel (the lanes of an LDS access group read one row).
constexpr int T3_H = 8, T3_W = 32, T3_PW = T3_W + 3;

__global__ __launch_bounds__(256) void k_conv3_sigmoid_train_fwd(const float *__restrict__ in, const float *__restrict__ w3, const float *__restrict__ b3,
                                                                float *__restrict__ out, int H, int W) {
    __shared__ float tile[16][T3_H + 2][T3_PW];
    const int tid = threadIdx.x, tj = tid % T3_W, ti = tid / T3_W;
    const int tiles_x = W / T3_W;
    const int i0 = (blockIdx.x / tiles_x) * T3_H, j0 = (blockIdx.x % tiles_x) * T3_W, b = blockIdx.z;
    const float *inb = in + (size_t)b * 16 * H * W;
    for (int e = tid; e < 16 * (T3_H + 2) * (T3_W + 2); e += 256) {
        const int pc = e % (T3_W + 2), rest = e / (T3_W + 2), pr = rest % (T3_H + 2), c = rest / (T3_H + 2);
        const int ii = i0 - 1 + pr, jj = j0 - 1 + pc;
        tile[c][pr][pc] = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? inb[((size_t)c * H + ii) * W + jj] : 0.f;
    }
    __syncthreads();
    float acc = b3 ? b3[0] : 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int d = 0; d < 3; ++d) acc = fmaf(tile[c][ti + a][tj + d], w3[c * 9 + a * 3 + d], acc);
    out[((size_t)b * H + i0 + ti) * W + j0 + tj] = 1.0f / (1.0f + expf(-acc));
}

// Backward, first launch: g = dY y (1 - y) on the tile and its halo (zero outside the image) in LDS; g of the tile is stored for the weight
// gradient, and dX[c][i][j] = sum_{a,d} g[i + 1 - a][j + 1 - d] w[c][a][d] for the 16 channels.
__global__ __launch_bounds__(256) void k_conv3_sigmoid_train_dgrad(const float *__restrict__ dy, const float *__restrict__ y, const float *__restrict__ w3,
                                                                  float *__restrict__ g, float *__restrict__ dx, int H, int W) {
    __shared__ float gt[T3_H + 2][T3_PW];
    const int tid = threadIdx.x, tj = tid % T3_W, ti = tid / T3_W;
    const int tiles_x = W / T3_W;
    const int i0 = (blockIdx.x / tiles_x) * T3_H, j0 = (blockIdx.x % tiles_x) * T3_W, b = blockIdx.z;
    for (int e = tid; e < (T3_H + 2) * (T3_W + 2); e += 256) {
        const int pc = e % (T3_W + 2), pr = e / (T3_W + 2), ii = i0 - 1 + pr, jj = j0 - 1 + pc;
        float v = 0.f;
        if (ii >= 0 && ii < H && jj >= 0 && jj < W) {
            const size_t k = ((size_t)b * H + ii) * W + jj;
            const float yv = y[k];
            v = dy[k] * yv * (1.0f - yv);
        }
        gt[pr][pc] = v;
    }
    __syncthreads();
    const int i = i0 + ti, j = j0 + tj;
    g[((size_t)b * H + i) * W + j] = gt[ti + 1][tj + 1];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int d = 0; d < 3; ++d) s = fmaf(gt[ti + 2 - a][tj + 2 - d], w3[c * 9 + a * 3 + d], s);
        dx[(((size_t)b * 16 + c) * H + i) * W + j] = s;
    }
}

// Backward, second launch: dW[c][a][d] = sum_{b,i,j} g[b][i][j] x[b][c][i+a-1][j+d-1], db = sum g.  Thread = (channel c, a run of 16 pixels
// of one tile row): 9 accumulators over its runs of every tile of its chunk; the 16 threads of a channel are added in thread order through
// LDS, one partial of 145 values per workgroup, and k_train_partials_finish adds those in chunk order.
__global__ __launch_bounds__(256) void k_conv3_train_wgrad(const float *__restrict__ g, const float *__restrict__ x, int H, int W, int tiles_x,
                                                          int tiles_per_frame, int ntiles, float *__restrict__ part) {
    __shared__ float xs[16][T3_H + 2][T3_PW];
    __shared__ float gs[T3_H][T3_W + 1];
    __shared__ float red[256][11];
    const int tid = threadIdx.x, c = tid >> 4, s = tid & 15, row = s >> 1, cb = (s & 1) * 16;
    float acc[9], dbs = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.f;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int b = t / tiles_per_frame, rm = t - b * tiles_per_frame;
        const int i0 = (rm / tiles_x) * T3_H, j0 = (rm % tiles_x) * T3_W;
        __syncthreads();
        const float *xb = x + (size_t)b * 16 * H * W;
        for (int e = tid; e < 16 * (T3_H + 2) * (T3_W + 2); e += 256) {
            const int pc = e % (T3_W + 2), rest = e / (T3_W + 2), pr = rest % (T3_H + 2), cc = rest / (T3_H + 2);
            const int ii = i0 - 1 + pr, jj = j0 - 1 + pc;
            xs[cc][pr][pc] = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? xb[((size_t)cc * H + ii) * W + jj] : 0.f;
        }
        gs[tid / T3_W][tid % T3_W] = g[((size_t)b * H + i0 + tid / T3_W) * W + j0 + tid % T3_W];
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const float gv = gs[row][cb + k];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int d = 0; d < 3; ++d) acc[a * 3 + d] = fmaf(gv, xs[c][row + a][cb + k + d], acc[a * 3 + d]);
            dbs += gv;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) red[tid][k] = acc[k];
    red[tid][9] = dbs;
    __syncthreads();
    if (tid < 145) {
        float sum = 0.f;
        if (tid < 144) {
            const int cc = tid / 9, k = tid - cc * 9;
            for (int q = 0; q < 16; ++q) sum += red[cc * 16 + q][k];
        } else {
            for (int q = 0; q < 16; ++q) sum += red[q][9];   // channel 0's threads: every pixel of the chunk once
        }
        part[(size_t)blockIdx.x * 145 + tid] = sum;
    }
}

bool conv3_train_shape_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= T3_H && W >= T3_W && H % T3_H == 0 && W % T3_W == 0 && (int64_t)B * 16 * H * W < (1ll << 31);
}

static int conv3_wgrad_chunks(int B, int H, int W) {
    const int64_t ntiles = (int64_t)B * (H / T3_H) * (W / T3_W);
    return (int)(ntiles < 1024 ? ntiles : 1024);
}

static size_t conv3_g_floats(int B, int H, int W) { return ((size_t)B * H * W + 3) / 4 * 4; }

size_t conv3_sigmoid_train_workspace_bytes(int B, int H, int W) {
    if (!conv3_train_shape_ok(B, H, W)) return 0;
    return (conv3_g_floats(B, H, W) + (size_t)conv3_wgrad_chunks(B, H, W) * 145) * sizeof(float);
}

hipError_t launch_conv3_sigmoid_train_forward(const float *x, const float *w, const float *bias, int B, int H, int W, float *y, hipStream_t st) {
    if (!conv3_train_shape_ok(B, H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_conv3_sigmoid_train_fwd, dim3((H / T3_H) * (W / T3_W), 1, B), dim3(256), 0, st, x, w, bias, y, H, W);
    return hipGetLastError();
}

hipError_t launch_conv3_sigmoid_train_backward(const float *dy, const float *y, const float *x, const float *w, int B, int H, int W, float *dx,
                                               float *dw, float *db, void *workspace, hipStream_t st) {
    if (!conv3_train_shape_ok(B, H, W)) return hipErrorInvalidValue;
    float *g = static_cast<float *>(workspace), *part = g + conv3_g_floats(B, H, W);
    const int tiles_x = W / T3_W, tiles_per_frame = tiles_x * (H / T3_H), nchunks = conv3_wgrad_chunks(B, H, W);
    hipLaunchKernelGGL(k_conv3_sigmoid_train_dgrad, dim3(tiles_per_frame, 1, B), dim3(256), 0, st, dy, y, w, g, dx, H, W);
    if (dw || db) {
        hipLaunchKernelGGL(k_conv3_train_wgrad, dim3(nchunks), dim3(256), 0, st, g, x, H, W, tiles_x, tiles_per_frame, B * tiles_per_frame, part);
        hipLaunchKernelGGL(k_train_partials_finish, dim3(1), dim3(256), 0, st, part, nchunks, 144, 1, dw, db);
    }
    return hipGetLastError();
}

}  // namespace smk
