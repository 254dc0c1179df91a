// Optical-flow baselines of the reference's benchmark.py (benchmark.py:21-94): Farneback dense flow, Shi-Tomasi corners with
// pyramidal Lucas-Kanade tracking, and the bilinear warp with its per-pair squared error, over n uint8 frame pairs [n][H][W].
// The rules (taps, borders, summation order) are the specification in DESIGN.md "Optical-flow baselines"; every kernel does its
// arithmetic in fp32 in the order written there (the Makefile sets -ffp-contract=off), so results repeat bit for bit.
//   * no allocation, no host synchronisation: scratch comes from the caller's workspace, every launch goes to the caller's stream
//   * every gather clamps or branches on the FLOAT coordinate before it becomes an index (flows may point far outside the image)
// Tiled kernels use one 256-thread workgroup per 16 x 64 output tile with the halo in LDS; blockIdx.z is the frame.
#include "flow.h"

#include <math.h>
#include <string.h>

namespace smk {

namespace {
constexpr int TH = 16, TW = 64, NT = 256;
constexpr int POLY_N = 5;                      // poly_n 5 -> 11 x 11 neighbourhood
constexpr double POLY_SIGMA = 1.2;             // the reference's call: calcOpticalFlowFarneback(..., 5, 1.2, 0)
constexpr int FB_WIN = 15, FB_R = FB_WIN / 2, FB_ITERS = 3;
constexpr int EIG_BLOCK = 7, EIG_R = EIG_BLOCK / 2;
constexpr int LK_WIN = 15, LK_R = LK_WIN / 2, LK_PIX = LK_WIN * LK_WIN, LK_ITERS = 30;

struct BlurTaps {
    float t[9];
    int r;                                      // radius: 1 (3 taps) or 4 (9 taps)
};
struct PolyConsts {
    float g[POLY_N + 1], xg[POLY_N + 1], xxg[POLY_N + 1];
    float ig11, ig03, ig33, ig55;
};

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
// One reflection is exact while the overshoot is below n - 1, which covers every tap of an in-image output.  The halo of the part of a
// tile that hangs over the image edge can lie further out (its results are never stored): the final clamp keeps those reads in bounds.
__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return clampi(i, n);
}

// ------------------------------------------------------------------ Farneback: level image
// separable Gaussian of the uint8 frame, border reflect-101, horizontal pass then vertical pass, taps summed left to right
__global__ __launch_bounds__(NT) void k_gauss_blur(const uint8_t *__restrict__ frames, int H, int W, BlurTaps tp, float *__restrict__ out) {
    __shared__ float s_in[(TH + 8) * (TW + 8)];
    __shared__ float s_h[(TH + 8) * TW];
    const int r = tp.r, R = TH + 2 * r, C = TW + 2 * r;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const uint8_t *src = frames + plane;
    const int row0 = blockIdx.y * TH - r, col0 = blockIdx.x * TW - r;
    for (int i = threadIdx.x; i < R * C; i += NT) {
        const int rr = i / C, cc = i - rr * C;
        s_in[i] = (float)src[(size_t)reflect101(row0 + rr, H) * W + reflect101(col0 + cc, W)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * TW; i += NT) {
        const int rr = i / TW, cc = i - rr * TW;
        const float *p = s_in + rr * C + cc;
        float acc = tp.t[0] * p[0];
        for (int t = 1; t <= 2 * r; ++t) acc = acc + tp.t[t] * p[t];
        s_h[i] = acc;
    }
    __syncthreads();
    const int c = threadIdx.x & (TW - 1);
    for (int rr = threadIdx.x / TW; rr < TH; rr += NT / TW) {
        const int gy = blockIdx.y * TH + rr, gx = blockIdx.x * TW + c;
        if (gy >= H || gx >= W) continue;
        float acc = tp.t[0] * s_h[rr * TW + c];
        for (int t = 1; t <= 2 * r; ++t) acc = acc + tp.t[t] * s_h[(rr + t) * TW + c];
        out[plane + (size_t)gy * W + gx] = acc;
    }
}

// bilinear resize of planes with `ch` interleaved channels: src = (dst + 0.5) * inv - 0.5, clamped to the source; result * mul
__global__ __launch_bounds__(NT) void k_resize(const float *__restrict__ src, int hs, int ws, float *__restrict__ dst, int hd, int wd,
                                               int ch, float inv, float mul) {
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    if (x >= wd) return;
    const float *s = src + (size_t)blockIdx.z * hs * ws * ch;
    float *d = dst + (size_t)blockIdx.z * hd * wd * ch;
    float sx = ((float)x + 0.5f) * inv - 0.5f, sy = ((float)y + 0.5f) * inv - 0.5f;
    sx = fminf(fmaxf(sx, 0.f), (float)(ws - 1));
    sy = fminf(fmaxf(sy, 0.f), (float)(hs - 1));
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int x1 = min(x0 + 1, ws - 1), y1 = min(y0 + 1, hs - 1);
    for (int c = 0; c < ch; ++c) {
        const float a = s[((size_t)y0 * ws + x0) * ch + c], b = s[((size_t)y0 * ws + x1) * ch + c];
        const float e = s[((size_t)y1 * ws + x0) * ch + c], f = s[((size_t)y1 * ws + x1) * ch + c];
        const float top = a * (1.f - fx) + b * fx, bot = e * (1.f - fx) + f * fx;
        d[((size_t)y * wd + x) * ch + c] = (top * (1.f - fy) + bot * fy) * mul;
    }
}

// ------------------------------------------------------------------ Farneback: polynomial expansion
// img [n][h][w] -> coef [n][5][h][w] = (bx, by, axx, ayy, axy).  Vertical pass over the 26 x 74 halo tile (border replicate) into
// three LDS row sets (sum g I, sum g y I, sum g y^2 I), then the horizontal pass; the +k / -k taps are paired before the multiply.
__global__ __launch_bounds__(NT) void k_poly_exp(const float *__restrict__ img, int h, int w, PolyConsts pc, float *__restrict__ coef) {
    constexpr int R = TH + 2 * POLY_N, C = TW + 2 * POLY_N;
    __shared__ float s_in[R * C];
    __shared__ float s_v[3][TH * C];
    const size_t plane = (size_t)h * w;
    const float *src = img + (size_t)blockIdx.z * plane;
    const int row0 = blockIdx.y * TH - POLY_N, col0 = blockIdx.x * TW - POLY_N;
    for (int i = threadIdx.x; i < R * C; i += NT) {
        const int rr = i / C, cc = i - rr * C;
        s_in[i] = src[(size_t)clampi(row0 + rr, h) * w + clampi(col0 + cc, w)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * C; i += NT) {
        const int rr = i / C, cc = i - rr * C;
        const float *p = s_in + (rr + POLY_N) * C + cc;
        float r0 = pc.g[0] * p[0], r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int k = 1; k <= POLY_N; ++k) {
            const float a = p[k * C], b = p[-k * C];
            const float s = a + b, d = a - b;
            r0 = r0 + pc.g[k] * s;
            r1 = r1 + pc.xg[k] * d;
            r2 = r2 + pc.xxg[k] * s;
        }
        s_v[0][i] = r0; s_v[1][i] = r1; s_v[2][i] = r2;
    }
    __syncthreads();
    const int c = threadIdx.x & (TW - 1);
    for (int rr = threadIdx.x / TW; rr < TH; rr += NT / TW) {
        const int gy = blockIdx.y * TH + rr, gx = blockIdx.x * TW + c;
        if (gy >= h || gx >= w) continue;
        const float *q0 = s_v[0] + rr * C + c + POLY_N, *q1 = s_v[1] + rr * C + c + POLY_N, *q2 = s_v[2] + rr * C + c + POLY_N;
        float b1 = pc.g[0] * q0[0], b3 = pc.g[0] * q1[0], b6 = pc.g[0] * q2[0], b2 = 0.f, b4 = 0.f, b5 = 0.f;
#pragma unroll
        for (int k = 1; k <= POLY_N; ++k) {
            const float s0 = q0[k] + q0[-k], d0 = q0[k] - q0[-k];
            const float s1 = q1[k] + q1[-k], d1 = q1[k] - q1[-k];
            const float s2 = q2[k] + q2[-k];
            b1 = b1 + pc.g[k] * s0;
            b2 = b2 + pc.xg[k] * d0;
            b4 = b4 + pc.xxg[k] * s0;
            b3 = b3 + pc.g[k] * s1;
            b5 = b5 + pc.xg[k] * d1;
            b6 = b6 + pc.g[k] * s2;
        }
        float *o = coef + (size_t)blockIdx.z * 5 * plane + (size_t)gy * w + gx;
        o[0] = b2 * pc.ig11;
        o[plane] = b3 * pc.ig11;
        o[2 * plane] = b1 * pc.ig03 + b4 * pc.ig33;
        o[3 * plane] = b1 * pc.ig03 + b6 * pc.ig33;
        o[4 * plane] = b5 * pc.ig55;
    }
}

// ------------------------------------------------------------------ Farneback: matrix update
// coef0, coef1 [n][5][h][w], flow [n][h][w][2] -> M [n][5][h][w] = (g11, g12, g22, h1, h2)
__device__ __forceinline__ float border_scale(int i, int n) {
    const float tab[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    float s = 1.f;
    if (i < 5) s = tab[i];
    if (i >= n - 5) s = s * tab[n - 1 - i];
    return s;
}

__global__ __launch_bounds__(NT) void k_update_matrices(const float *__restrict__ coef0, const float *__restrict__ coef1,
                                                        const float *__restrict__ flow, int h, int w, float *__restrict__ M) {
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const size_t plane = (size_t)h * w, base = (size_t)blockIdx.z * 5 * plane, pix = (size_t)y * w + x;
    const float *c0 = coef0 + base + pix, *c1 = coef1 + base;
    const float2 d = ((const float2 *)flow)[(size_t)blockIdx.z * plane + pix];
    const float dx = d.x, dy = d.y;
    const float fxp = (float)x + dx, fyp = (float)y + dy;
    float axx = c0[2 * plane], ayy = c0[3 * plane], axyh, dbx = 0.f, dby = 0.f;
    // the comparison is on the float position: NaN and far-away flows take the outside branch and no index is formed from them
    if (fxp >= 0.f && fxp < (float)(w - 1) && fyp >= 0.f && fyp < (float)(h - 1)) {
        const float x0f = floorf(fxp), y0f = floorf(fyp);
        const float fx = fxp - x0f, fy = fyp - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        const float *q = c1 + (size_t)y0 * w + x0;
        float s[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float *qk = q + k * plane;
            s[k] = ((a00 * qk[0] + a01 * qk[1]) + a10 * qk[w]) + a11 * qk[w + 1];
        }
        dbx = (c0[0] - s[0]) * 0.5f;
        dby = (c0[plane] - s[1]) * 0.5f;
        axx = (axx + s[2]) * 0.5f;
        ayy = (ayy + s[3]) * 0.5f;
        axyh = (c0[4 * plane] + s[4]) * 0.25f;
    } else {
        axyh = c0[4 * plane] * 0.5f;
    }
    dbx = (dbx + axx * dx) + axyh * dy;
    dby = (dby + axyh * dx) + ayy * dy;
    const float sc = border_scale(x, w) * border_scale(y, h);
    axx = axx * sc; ayy = ayy * sc; axyh = axyh * sc; dbx = dbx * sc; dby = dby * sc;
    float *o = M + base + pix;
    o[0] = axx * axx + axyh * axyh;
    o[plane] = axyh * (axx + ayy);
    o[2 * plane] = ayy * ayy + axyh * axyh;
    o[3 * plane] = axx * dbx + axyh * dby;
    o[4 * plane] = axyh * dbx + ayy * dby;
}

// ------------------------------------------------------------------ Farneback: 15 x 15 box mean (border replicate) + 2 x 2 solve
// One channel at a time through LDS (30 x 78 halo, then 30 x 64 horizontal sums); each thread keeps the five means of its four pixels.
__global__ __launch_bounds__(NT) void k_blur_solve(const float *__restrict__ M, int h, int w, float inv_area, float *__restrict__ flow) {
    constexpr int R = TH + 2 * FB_R, C = TW + 2 * FB_R;
    __shared__ float s_in[R * C];
    __shared__ float s_h[R * TW];
    const size_t plane = (size_t)h * w;
    const int row0 = blockIdx.y * TH - FB_R, col0 = blockIdx.x * TW - FB_R;
    const int c = threadIdx.x & (TW - 1), rbase = threadIdx.x / TW;
    float m[4][5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float *src = M + ((size_t)blockIdx.z * 5 + k) * plane;
        for (int i = threadIdx.x; i < R * C; i += NT) {
            const int rr = i / C, cc = i - rr * C;
            s_in[i] = src[(size_t)clampi(row0 + rr, h) * w + clampi(col0 + cc, w)];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < R * TW; i += NT) {
            const int rr = i / TW, cc = i - rr * TW;
            const float *p = s_in + rr * C + cc;
            float acc = p[0];
            for (int t = 1; t < FB_WIN; ++t) acc = acc + p[t];
            s_h[i] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rr = rbase + 4 * j;
            float acc = s_h[rr * TW + c];
            for (int t = 1; t < FB_WIN; ++t) acc = acc + s_h[(rr + t) * TW + c];
            m[j][k] = acc * inv_area;
        }
        // the next channel's tile load waits for every read of s_in / s_h above
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gy = blockIdx.y * TH + rbase + 4 * j, gx = blockIdx.x * TW + c;
        if (gy >= h || gx >= w) continue;
        const float g11 = m[j][0], g12 = m[j][1], g22 = m[j][2], h1 = m[j][3], h2 = m[j][4];
        const float idet = 1.f / ((g11 * g22 - g12 * g12) + 1e-3f);
        float2 d;
        d.x = (g22 * h1 - g12 * h2) * idet;
        d.y = (g11 * h2 - g12 * h1) * idet;
        ((float2 *)flow)[(size_t)blockIdx.z * plane + (size_t)gy * w + gx] = d;
    }
}

// ------------------------------------------------------------------ warp + squared error
// pred = bilinear sample of prev at (x + dx, y + dy), taps outside the image read 0, round half to even, saturate.  With `next`, each
// workgroup also writes the uint32 sum of (next - pred)^2 over its 256 pixels (exact integers: the summation order cannot matter).
__global__ __launch_bounds__(NT) void k_warp(const uint8_t *__restrict__ prev, const float *__restrict__ flow, const uint8_t *__restrict__ next,
                                             int H, int W, uint8_t *__restrict__ pred, uint32_t *__restrict__ partial) {
    __shared__ uint32_t red[NT / 64];
    const int npix = H * W;
    const int i = blockIdx.x * NT + threadIdx.x;
    const size_t plane = (size_t)blockIdx.y * npix;
    uint32_t sq = 0;
    if (i < npix) {
        const int y = i / W, x = i - y * W;
        const float2 d = ((const float2 *)flow)[plane + i];
        const float sx = (float)x + d.x, sy = (float)y + d.y;
        float v = 0.f;
        if (sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H) {            // false for NaN: the sample is 0
            const float x0f = floorf(sx), y0f = floorf(sy);
            const float fx = sx - x0f, fy = sy - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;                               // in [-1, W-1] x [-1, H-1]
            const uint8_t *p = prev + plane;
            const bool xl = x0 >= 0, xr = x0 + 1 < W, yt = y0 >= 0, yb = y0 + 1 < H;
            const float p00 = (xl && yt) ? (float)p[(size_t)y0 * W + x0] : 0.f;
            const float p01 = (xr && yt) ? (float)p[(size_t)y0 * W + x0 + 1] : 0.f;
            const float p10 = (xl && yb) ? (float)p[(size_t)(y0 + 1) * W + x0] : 0.f;
            const float p11 = (xr && yb) ? (float)p[(size_t)(y0 + 1) * W + x0 + 1] : 0.f;
            const float top = p00 * (1.f - fx) + p01 * fx, bot = p10 * (1.f - fx) + p11 * fx;
            v = top * (1.f - fy) + bot * fy;
        }
        v = fminf(fmaxf(rintf(v), 0.f), 255.f);
        const int q = (int)v;
        pred[plane + i] = (uint8_t)q;
        if (next) {
            const int e = (int)next[plane + i] - q;
            sq = (uint32_t)(e * e);
        }
    }
    if (partial) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
        __syncthreads();
        if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

__global__ __launch_bounds__(NT) void k_mse_sum(const uint32_t *__restrict__ partial, int blocks, double inv_pixels, double *__restrict__ mse) {
    __shared__ unsigned long long red[NT];
    const uint32_t *p = partial + (size_t)blockIdx.x * blocks;
    unsigned long long s = 0;
    for (int i = threadIdx.x; i < blocks; i += NT) s += p[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) mse[blockIdx.x] = (double)red[0] * inv_pixels;
}

// ------------------------------------------------------------------ Shi-Tomasi: smaller eigenvalue of the 7 x 7 structure tensor
// Sobel 3 x 3 on the uint8 frame (reflect-101), products and box sums in exact integers (the box reflects the derivative maps, 101),
// then lambda_min = (a + c) - sqrt((a - c)^2 + b^2) with a = Sxx / 2, b = Sxy, c = Syy / 2 in fp32.
__global__ __launch_bounds__(NT) void k_min_eigen(const uint8_t *__restrict__ frames, int H, int W, float *__restrict__ eig) {
    constexpr int R = TH + 2 * EIG_R, C = TW + 2 * EIG_R;
    __shared__ int s_d[3][R * C];
    __shared__ int s_h[3][R * TW];
    const size_t plane = (size_t)blockIdx.z * H * W;
    const uint8_t *I = frames + plane;
    const int row0 = blockIdx.y * TH - EIG_R, col0 = blockIdx.x * TW - EIG_R;
    for (int i = threadIdx.x; i < R * C; i += NT) {
        const int rr = i / C, cc = i - rr * C;
        const int y = reflect101(row0 + rr, H), x = reflect101(col0 + cc, W);
        const int ym = reflect101(y - 1, H), yp = reflect101(y + 1, H), xm = reflect101(x - 1, W), xp = reflect101(x + 1, W);
        const int a = I[(size_t)ym * W + xm], b = I[(size_t)ym * W + x], c = I[(size_t)ym * W + xp];
        const int d = I[(size_t)y * W + xm], f = I[(size_t)y * W + xp];
        const int g = I[(size_t)yp * W + xm], hh = I[(size_t)yp * W + x], k = I[(size_t)yp * W + xp];
        const int ix = (c + 2 * f + k) - (a + 2 * d + g), iy = (g + 2 * hh + k) - (a + 2 * b + c);
        s_d[0][i] = ix * ix; s_d[1][i] = ix * iy; s_d[2][i] = iy * iy;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * TW; i += NT) {
        const int rr = i / TW, cc = i - rr * TW;
        for (int k = 0; k < 3; ++k) {
            const int *p = s_d[k] + rr * C + cc;
            int acc = 0;
            for (int t = 0; t < EIG_BLOCK; ++t) acc += p[t];
            s_h[k][i] = acc;
        }
    }
    __syncthreads();
    const int c = threadIdx.x & (TW - 1);
    for (int rr = threadIdx.x / TW; rr < TH; rr += NT / TW) {
        const int gy = blockIdx.y * TH + rr, gx = blockIdx.x * TW + c;
        if (gy >= H || gx >= W) continue;
        int sxx = 0, sxy = 0, syy = 0;
        for (int t = 0; t < EIG_BLOCK; ++t) {
            sxx += s_h[0][(rr + t) * TW + c];
            sxy += s_h[1][(rr + t) * TW + c];
            syy += s_h[2][(rr + t) * TW + c];
        }
        const float a = (float)sxx * 0.5f, b = (float)sxy, cc2 = (float)syy * 0.5f;
        const float dd = a - cc2;
        eig[plane + (size_t)gy * W + gx] = (a + cc2) - sqrtf(dd * dd + b * b);
    }
}

__global__ __launch_bounds__(NT) void k_frame_max(const float *__restrict__ eig, int npix, float *__restrict__ fmax) {
    __shared__ float red[NT / 64];
    const float *p = eig + (size_t)blockIdx.x * npix;
    float m = 0.f;                                              // eigenvalues of a positive semi-definite tensor: the maximum is >= 0
    for (int i = threadIdx.x; i < npix; i += NT) m = fmaxf(m, p[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) fmax[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// One workgroup per frame.  Pass 1 lists the candidates (value > 0.3 max, equal to the 3 x 3 maximum, off the 1-pixel border) in the
// workspace; pass 2 repeats: argmax over the live entries (ties: the smaller y * W + x), emit it, kill every entry nearer than 7.
// Thread t owns list entries t, t + 256, ... in both the argmax and the kill, so a kill is seen by the only thread that reads it.
__global__ __launch_bounds__(NT) void k_select_corners(const float *__restrict__ eig, const float *__restrict__ fmax, int H, int W,
                                                       float *__restrict__ cand_val, int *__restrict__ cand_idx, float *__restrict__ pts,
                                                       int32_t *__restrict__ counts) {
    __shared__ int s_count;
    __shared__ float s_v[NT / 64];
    __shared__ int s_i[NT / 64];
    __shared__ int s_best;
    const int npix = H * W, f = blockIdx.x;
    const float *e = eig + (size_t)f * npix;
    float *cv = cand_val + (size_t)f * npix;
    int *ci = cand_idx + (size_t)f * npix;
    const float thr = fmax[f] * 0.3f;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < npix; i += NT) {
        const int y = i / W, x = i - y * W;
        if (y < 1 || y >= H - 1 || x < 1 || x >= W - 1) continue;
        const float v = e[i];
        if (!(v > thr)) continue;
        float m = v;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) m = fmaxf(m, e[i + dy * W + dx]);
        if (v == m) {
            const int slot = atomicAdd(&s_count, 1);            // slot < npix: at most one per pixel
            cv[slot] = v;
            ci[slot] = i;
        }
    }
    __syncthreads();
    const int ncand = s_count;
    int found = 0;
    for (; found < LK_MAX_CORNERS; ++found) {
        float bv = -1.f;
        int bi = 0x7fffffff;
        for (int j = threadIdx.x; j < ncand; j += NT) {
            const float v = cv[j];
            const int idx = ci[j];
            if (v > bv || (v == bv && idx < bi)) { bv = v; bi = idx; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_down(bv, off);
            const int oi = __shfl_down(bi, off);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < NT / 64; ++k)
                if (s_v[k] > bv || (s_v[k] == bv && s_i[k] < bi)) { bv = s_v[k]; bi = s_i[k]; }
            s_best = bv > 0.f ? bi : -1;
        }
        __syncthreads();
        const int best = s_best;
        if (best < 0) break;                                     // uniform: every thread reads the same s_best
        const int by = best / W, bx = best - by * W;
        if (threadIdx.x == 0) {
            pts[((size_t)f * LK_MAX_CORNERS + found) * 2] = (float)bx;
            pts[((size_t)f * LK_MAX_CORNERS + found) * 2 + 1] = (float)by;
        }
        for (int j = threadIdx.x; j < ncand; j += NT) {
            const int idx = ci[j];
            const int y = idx / W, x = idx - y * W;
            const int dx = x - bx, dy = y - by;
            if (dx * dx + dy * dy < 49) cv[j] = -1.f;
        }
        __syncthreads();                                         // s_best is rewritten in the next round
    }
    for (int k = found + threadIdx.x; k < LK_MAX_CORNERS; k += NT) {
        pts[((size_t)f * LK_MAX_CORNERS + k) * 2] = 0.f;
        pts[((size_t)f * LK_MAX_CORNERS + k) * 2 + 1] = 0.f;
    }
    if (threadIdx.x == 0) counts[f] = found;
}

// ------------------------------------------------------------------ Lucas-Kanade: pyramids
__global__ __launch_bounds__(NT) void k_u8_to_f32(const uint8_t *__restrict__ src, size_t count, float *__restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < count) dst[i] = (float)src[i];
}

// (1, 4, 6, 4, 1) / 16 in both directions, reflect-101, even samples: rows first (left to right), then the five row results top down
__global__ __launch_bounds__(NT) void k_pyr_down(const float *__restrict__ src, int hs, int ws, float *__restrict__ dst, int hd, int wd) {
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    if (x >= wd) return;
    const float wt[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float *s = src + (size_t)blockIdx.z * hs * ws;
    int xs[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) xs[j] = reflect101(2 * x + j - 2, ws);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float *row = s + (size_t)reflect101(2 * y + i - 2, hs) * ws;
        float r = wt[0] * row[xs[0]];
#pragma unroll
        for (int j = 1; j < 5; ++j) r = r + wt[j] * row[xs[j]];
        acc = i == 0 ? wt[0] * r : acc + wt[i] * r;
    }
    dst[(size_t)blockIdx.z * hd * wd + (size_t)y * wd + x] = acc;
}

// ------------------------------------------------------------------ Lucas-Kanade: tracking, one wave per point
struct LkPyr {
    const float *I[LK_MAX_LEVEL + 1], *J[LK_MAX_LEVEL + 1];
    int h[LK_MAX_LEVEL + 1], w[LK_MAX_LEVEL + 1];
};

// bilinear sample with the coordinate clamped to the image (fmaxf / fminf also turn NaN into a valid coordinate)
__device__ __forceinline__ void bil_setup(float x, float y, int w, int h, int &x0, int &y0, int &x1, int &y1, float &fx, float &fy) {
    x = fminf(fmaxf(x, 0.f), (float)(w - 1));
    y = fminf(fmaxf(y, 0.f), (float)(h - 1));
    const float x0f = floorf(x), y0f = floorf(y);
    fx = x - x0f; fy = y - y0f;
    x0 = (int)x0f; y0 = (int)y0f;
    x1 = min(x0 + 1, w - 1); y1 = min(y0 + 1, h - 1);
}
__device__ __forceinline__ float bil_mix(float a, float b, float c, float d, float fx, float fy) {
    const float top = a * (1.f - fx) + b * fx, bot = c * (1.f - fx) + d * fx;
    return top * (1.f - fy) + bot * fy;
}
// Scharr / 32 at an integer pixel, border replicate
__device__ __forceinline__ void scharr_at(const float *img, int w, int h, int x, int y, float &gx, float &gy) {
    const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
    const float a = img[(size_t)ym * w + xm], b = img[(size_t)ym * w + x], c = img[(size_t)ym * w + xp];
    const float d = img[(size_t)y * w + xm], f = img[(size_t)y * w + xp];
    const float g = img[(size_t)yp * w + xm], hh = img[(size_t)yp * w + x], k = img[(size_t)yp * w + xp];
    gx = ((3.f * (c - a) + 10.f * (f - d)) + 3.f * (k - g)) * 0.03125f;
    gy = ((3.f * (g - a) + 10.f * (hh - b)) + 3.f * (k - c)) * 0.03125f;
}
__device__ __forceinline__ float wave_sum_all(float v) {       // butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ bool inside(float x, float y, int w, int h) {
    return x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1);
}

__global__ __launch_bounds__(64) void k_lk_track(LkPyr P, const float *__restrict__ pts, const int32_t *__restrict__ counts,
                                                 float *__restrict__ out_pts, uint8_t *__restrict__ status) {
    __shared__ float s_I[LK_PIX], s_gx[LK_PIX], s_gy[LK_PIX];
    const int pt = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    const size_t o = (size_t)f * LK_MAX_CORNERS + pt;
    if (pt >= counts[f]) {                                      // uniform over the workgroup
        if (lane == 0) { out_pts[o * 2] = 0.f; out_pts[o * 2 + 1] = 0.f; status[o] = 0; }
        return;
    }
    const float px0 = pts[o * 2], py0 = pts[o * 2 + 1];
    float vx = 0.f, vy = 0.f;
    bool ok = true;
    for (int L = LK_MAX_LEVEL; L >= 0; --L) {
        const int w = P.w[L], h = P.h[L];
        const float *I = P.I[L] + (size_t)f * w * h, *J = P.J[L] + (size_t)f * w * h;
        const float sc = L == 2 ? 0.25f : (L == 1 ? 0.5f : 1.f);
        const float px = px0 * sc, py = py0 * sc;
        bool level_ok = inside(px, py, w, h) && inside(px + vx, py + vy, w, h);
        if (level_ok) {
            float gxx = 0.f, gxy = 0.f, gyy = 0.f;
            for (int e = lane; e < LK_PIX; e += 64) {
                const int wy = e / LK_WIN, wx = e - wy * LK_WIN;
                int x0, y0, x1, y1;
                float fx, fy;
                bil_setup(px + (float)(wx - LK_R), py + (float)(wy - LK_R), w, h, x0, y0, x1, y1, fx, fy);
                const float iv = bil_mix(I[(size_t)y0 * w + x0], I[(size_t)y0 * w + x1], I[(size_t)y1 * w + x0], I[(size_t)y1 * w + x1], fx, fy);
                float ax, ay, bx, by, cx, cy, dx, dy;
                scharr_at(I, w, h, x0, y0, ax, ay);
                scharr_at(I, w, h, x1, y0, bx, by);
                scharr_at(I, w, h, x0, y1, cx, cy);
                scharr_at(I, w, h, x1, y1, dx, dy);
                const float gx = bil_mix(ax, bx, cx, dx, fx, fy), gy = bil_mix(ay, by, cy, dy, fx, fy);
                s_I[e] = iv; s_gx[e] = gx; s_gy[e] = gy;
                gxx = gxx + gx * gx; gxy = gxy + gx * gy; gyy = gyy + gy * gy;
            }
            gxx = wave_sum_all(gxx); gxy = wave_sum_all(gxy); gyy = wave_sum_all(gyy);
            const float det = gxx * gyy - gxy * gxy;
            const float dd = gxx - gyy;
            const float min_eig = ((gyy + gxx) - sqrtf(dd * dd + 4.f * gxy * gxy)) / (2.f * (float)LK_PIX);
            level_ok = min_eig >= 1e-4f && det > 0.f;
            if (level_ok) {
                __syncthreads();                                 // one wave: orders the LDS writes above before the reads below
                for (int it = 0; it < LK_ITERS; ++it) {
                    float b1 = 0.f, b2 = 0.f;
                    for (int e = lane; e < LK_PIX; e += 64) {
                        const int wy = e / LK_WIN, wx = e - wy * LK_WIN;
                        int x0, y0, x1, y1;
                        float fx, fy;
                        bil_setup((px + vx) + (float)(wx - LK_R), (py + vy) + (float)(wy - LK_R), w, h, x0, y0, x1, y1, fx, fy);
                        const float jv = bil_mix(J[(size_t)y0 * w + x0], J[(size_t)y0 * w + x1], J[(size_t)y1 * w + x0], J[(size_t)y1 * w + x1], fx, fy);
                        const float diff = s_I[e] - jv;
                        b1 = b1 + diff * s_gx[e];
                        b2 = b2 + diff * s_gy[e];
                    }
                    b1 = wave_sum_all(b1); b2 = wave_sum_all(b2);
                    const float ddx = (gyy * b1 - gxy * b2) / det, ddy = (gxx * b2 - gxy * b1) / det;
                    vx = vx + ddx; vy = vy + ddy;
                    if (!inside(px + vx, py + vy, w, h)) { level_ok = false; break; }
                    if (ddx * ddx + ddy * ddy < 1e-4f) break;
                }
                __syncthreads();                                 // the next level rewrites s_I / s_gx / s_gy
            }
        }
        if (L == 0) ok = level_ok;
        else { vx = vx * 2.f; vy = vy * 2.f; }
    }
    if (lane == 0) {
        out_pts[o * 2] = px0 + vx;
        out_pts[o * 2 + 1] = py0 + vy;
        status[o] = ok ? 1 : 0;
    }
}

// flow[int(y0), int(x0)] = (x1 - x0, y1 - y0) for tracked points; the field was zeroed before
__global__ __launch_bounds__(128) void k_lk_scatter(const float *__restrict__ pts, const float *__restrict__ out_pts,
                                                    const uint8_t *__restrict__ status, const int32_t *__restrict__ counts, int H, int W,
                                                    float *__restrict__ flow) {
    const int f = blockIdx.x, i = threadIdx.x;
    if (i >= LK_MAX_CORNERS || i >= counts[f]) return;
    const size_t o = (size_t)f * LK_MAX_CORNERS + i;
    if (!status[o]) return;
    const float x0 = pts[o * 2], y0 = pts[o * 2 + 1];
    if (!(x0 >= 0.f && x0 < (float)W && y0 >= 0.f && y0 < (float)H)) return;
    float2 d;
    d.x = out_pts[o * 2] - x0;
    d.y = out_pts[o * 2 + 1] - y0;
    ((float2 *)flow)[(size_t)f * H * W + (size_t)(int)y0 * W + (int)x0] = d;
}

// ------------------------------------------------------------------ host side
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

BlurTaps blur_taps(int level) {
    BlurTaps tp;
    memset(&tp, 0, sizeof(tp));
    if (level == 0) {
        tp.r = 1;
        tp.t[0] = 0.25f; tp.t[1] = 0.5f; tp.t[2] = 0.25f;
        return tp;
    }
    const double sigma = level == 1 ? 0.5 : 1.5;
    tp.r = level == 1 ? 1 : 4;
    double g[9], sum = 0.0;
    for (int i = 0; i <= 2 * tp.r; ++i) {
        const double x = i - tp.r;
        g[i] = exp(-(x * x) / (2.0 * sigma * sigma));
        sum += g[i];
    }
    for (int i = 0; i <= 2 * tp.r; ++i) tp.t[i] = (float)(g[i] / sum);
    return tp;
}

// Normalised Gaussian weights and the four entries of the inverse 6 x 6 moment matrix that the closed form needs.  With second and
// fourth moments m2, m4 of the 1-D weight: inv(x,x) = inv(y,y) = 1/m2, inv(1,x^2) = -m2/(m4 - m2^2), inv(x^2,x^2) = 1/(m4 - m2^2),
// inv(xy,xy) = 1/m2^2.
PolyConsts poly_consts() {
    PolyConsts pc;
    double g[2 * POLY_N + 1], sum = 0.0;
    for (int i = -POLY_N; i <= POLY_N; ++i) {
        g[i + POLY_N] = exp(-(double)(i * i) / (2.0 * POLY_SIGMA * POLY_SIGMA));
        sum += g[i + POLY_N];
    }
    double m2 = 0.0, m4 = 0.0;
    for (int i = -POLY_N; i <= POLY_N; ++i) {
        g[i + POLY_N] /= sum;
        m2 += g[i + POLY_N] * i * i;
        m4 += g[i + POLY_N] * i * i * i * i;
    }
    for (int k = 0; k <= POLY_N; ++k) {
        pc.g[k] = (float)g[k + POLY_N];
        pc.xg[k] = (float)(g[k + POLY_N] * k);
        pc.xxg[k] = (float)(g[k + POLY_N] * k * k);
    }
    pc.ig11 = (float)(1.0 / m2);
    pc.ig03 = (float)(-m2 / (m4 - m2 * m2));
    pc.ig33 = (float)(1.0 / (m4 - m2 * m2));
    pc.ig55 = (float)(1.0 / (m2 * m2));
    return pc;
}

inline dim3 tile_grid(int n, int h, int w) { return dim3(cdiv(w, TW), cdiv(h, TH), n); }
inline dim3 row_grid(int n, int h, int w) { return dim3(cdiv(w, NT), h, n); }

struct FbWorkspace {
    float *blur, *img[2], *coef[2], *M, *fa, *fb;
};
FbWorkspace fb_carve(void *ws, int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    char *p = (char *)ws;
    FbWorkspace f;
    f.blur = (float *)p; p += align256(px * 4);
    f.img[0] = (float *)p; p += align256(px * 4);
    f.img[1] = (float *)p; p += align256(px * 4);
    f.coef[0] = (float *)p; p += align256(px * 20);
    f.coef[1] = (float *)p; p += align256(px * 20);
    f.M = (float *)p; p += align256(px * 20);
    f.fa = (float *)p; p += align256(px * 4);          // level-1 flow: ((H+1)/2) * ((W+1)/2) pixels at most, two floats each
    f.fb = (float *)p;                                 // level-2 flow (same bound)
    return f;
}
}  // namespace

int flow_levels(int H, int W) {
    if (H < FLOW_MIN_DIM || W < FLOW_MIN_DIM || H > FLOW_MAX_DIM || W > FLOW_MAX_DIM) return 0;
    const int m = H < W ? H : W;
    int K = 1;
    while (K < FLOW_MAX_LEVELS && m >= (FLOW_MIN_DIM << K)) ++K;         // m * 0.5^K >= 32
    return K;
}

void flow_level_size(int H, int W, int level, int *h, int *w) {
    const double s = 1.0 / (double)(1 << level);
    *h = (int)nearbyint(H * s);                                          // round half to even
    *w = (int)nearbyint(W * s);
}

size_t farneback_workspace_bytes(int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    return 5 * align256(px * 4) + 3 * align256(px * 20);
}

size_t warp_workspace_bytes(int n, int H, int W) { return (size_t)n * cdiv(H * W, NT) * sizeof(uint32_t); }

hipError_t launch_flow_level_image(const uint8_t *frames, int n, int H, int W, int level, float *out, void *ws, hipStream_t st) {
    const BlurTaps tp = blur_taps(level);
    float *blur = level == 0 ? out : (float *)ws;
    hipLaunchKernelGGL(k_gauss_blur, tile_grid(n, H, W), dim3(NT), 0, st, frames, H, W, tp, blur);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || level == 0) return e;
    int h, w;
    flow_level_size(H, W, level, &h, &w);
    hipLaunchKernelGGL(k_resize, row_grid(n, h, w), dim3(NT), 0, st, (const float *)blur, H, W, out, h, w, 1, (float)(1 << level), 1.f);
    return hipGetLastError();
}

hipError_t launch_flow_poly_exp(const float *img, int n, int h, int w, float *coef, hipStream_t st) {
    static const PolyConsts pc = poly_consts();
    hipLaunchKernelGGL(k_poly_exp, tile_grid(n, h, w), dim3(NT), 0, st, img, h, w, pc, coef);
    return hipGetLastError();
}

hipError_t launch_flow_iteration(const float *coef0, const float *coef1, float *flow, int n, int h, int w, void *ws, hipStream_t st) {
    float *M = (float *)ws;
    hipLaunchKernelGGL(k_update_matrices, row_grid(n, h, w), dim3(NT), 0, st, coef0, coef1, (const float *)flow, h, w, M);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_blur_solve, tile_grid(n, h, w), dim3(NT), 0, st, (const float *)M, h, w, (float)(1.0 / (FB_WIN * FB_WIN)), flow);
    return hipGetLastError();
}

hipError_t launch_flow_farneback(const uint8_t *prev, const uint8_t *next, int n, int H, int W, float *flow, void *ws, hipStream_t st) {
    const FbWorkspace f = fb_carve(ws, n, H, W);
    const int K = flow_levels(H, W);
    float *level_flow[FLOW_MAX_LEVELS] = {flow, f.fa, f.fb};
    hipError_t e;
    int hp = 0, wp = 0;
    for (int k = K - 1; k >= 0; --k) {
        int h, w;
        flow_level_size(H, W, k, &h, &w);
        float *fl = level_flow[k];
        if (k == K - 1) {
            e = hipMemsetAsync(fl, 0, (size_t)n * h * w * 2 * sizeof(float), st);
            if (e != hipSuccess) return e;
        } else {
            hipLaunchKernelGGL(k_resize, row_grid(n, h, w), dim3(NT), 0, st, (const float *)level_flow[k + 1], hp, wp, fl, h, w, 2, 0.5f, 2.f);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        const uint8_t *frames[2] = {prev, next};
        for (int s = 0; s < 2; ++s) {
            if ((e = launch_flow_level_image(frames[s], n, H, W, k, f.img[s], f.blur, st)) != hipSuccess) return e;
            if ((e = launch_flow_poly_exp(f.img[s], n, h, w, f.coef[s], st)) != hipSuccess) return e;
        }
        for (int it = 0; it < FB_ITERS; ++it)
            if ((e = launch_flow_iteration(f.coef[0], f.coef[1], fl, n, h, w, f.M, st)) != hipSuccess) return e;
        hp = h; wp = w;
    }
    return hipSuccess;
}

hipError_t launch_warp_frames(const uint8_t *prev, const float *flow, const uint8_t *next, int n, int H, int W, uint8_t *pred,
                              double *mse, void *ws, hipStream_t st) {
    const int blocks = cdiv(H * W, NT);
    const bool err = next && mse;
    hipLaunchKernelGGL(k_warp, dim3(blocks, n), dim3(NT), 0, st, prev, flow, err ? next : (const uint8_t *)nullptr, H, W, pred,
                       err ? (uint32_t *)ws : (uint32_t *)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !err) return e;
    hipLaunchKernelGGL(k_mse_sum, dim3(n), dim3(NT), 0, st, (const uint32_t *)ws, blocks, 1.0 / ((double)H * (double)W), mse);
    return hipGetLastError();
}

// ------------------------------------------------------------------ Lucas-Kanade host side
namespace {
struct LkWorkspace {
    float *pyr[2][LK_MAX_LEVEL + 1];      // [frame set][level]
    float *eig, *fmax, *cand_val, *pts, *out_pts;
    int *cand_idx;
    int32_t *counts;
    uint8_t *status;
    int h[LK_MAX_LEVEL + 1], w[LK_MAX_LEVEL + 1];
};
LkWorkspace lk_carve(void *ws, int n, int H, int W) {
    LkWorkspace k;
    char *p = (char *)ws;
    k.h[0] = H; k.w[0] = W;
    for (int L = 1; L <= LK_MAX_LEVEL; ++L) { k.h[L] = (k.h[L - 1] + 1) / 2; k.w[L] = (k.w[L - 1] + 1) / 2; }
    for (int s = 0; s < 2; ++s)
        for (int L = 0; L <= LK_MAX_LEVEL; ++L) { k.pyr[s][L] = (float *)p; p += align256((size_t)n * k.h[L] * k.w[L] * 4); }
    const size_t px = (size_t)n * H * W;
    k.eig = (float *)p; p += align256(px * 4);
    k.cand_val = (float *)p; p += align256(px * 4);
    k.cand_idx = (int *)p; p += align256(px * 4);
    k.fmax = (float *)p; p += align256((size_t)n * 4);
    k.pts = (float *)p; p += align256((size_t)n * LK_MAX_CORNERS * 8);
    k.out_pts = (float *)p; p += align256((size_t)n * LK_MAX_CORNERS * 8);
    k.counts = (int32_t *)p; p += align256((size_t)n * 4);
    k.status = (uint8_t *)p;
    return k;
}
}  // namespace

size_t lk_workspace_bytes(int n, int H, int W) {
    size_t b = 0;
    int h = H, w = W;
    for (int L = 0; L <= LK_MAX_LEVEL; ++L) { b += 2 * align256((size_t)n * h * w * 4); h = (h + 1) / 2; w = (w + 1) / 2; }
    const size_t px = (size_t)n * H * W;
    b += 3 * align256(px * 4) + 2 * align256((size_t)n * 4) + 2 * align256((size_t)n * LK_MAX_CORNERS * 8) + align256((size_t)n * LK_MAX_CORNERS);
    return b;
}

hipError_t launch_flow_min_eigen(const uint8_t *frames, int n, int H, int W, float *eig, hipStream_t st) {
    hipLaunchKernelGGL(k_min_eigen, tile_grid(n, H, W), dim3(NT), 0, st, frames, H, W, eig);
    return hipGetLastError();
}

// ws: the cand_val / cand_idx / fmax part of the Lucas-Kanade workspace (lk_carve)
hipError_t launch_good_features(const float *eig, int n, int H, int W, float *pts, int32_t *counts, void *ws, hipStream_t st) {
    const LkWorkspace k = lk_carve(ws, n, H, W);
    hipLaunchKernelGGL(k_frame_max, dim3(n), dim3(NT), 0, st, eig, H * W, k.fmax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_select_corners, dim3(n), dim3(NT), 0, st, eig, (const float *)k.fmax, H, W, k.cand_val, k.cand_idx, pts, counts);
    return hipGetLastError();
}

hipError_t launch_lk_track(const uint8_t *prev, const uint8_t *next, int n, int H, int W, const float *pts, const int32_t *counts,
                           float *out_pts, uint8_t *status, void *ws, hipStream_t st) {
    const LkWorkspace k = lk_carve(ws, n, H, W);
    const uint8_t *frames[2] = {prev, next};
    hipError_t e;
    LkPyr P;
    for (int s = 0; s < 2; ++s) {
        const size_t count = (size_t)n * H * W;
        hipLaunchKernelGGL(k_u8_to_f32, dim3((unsigned)((count + NT - 1) / NT)), dim3(NT), 0, st, frames[s], count, k.pyr[s][0]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        for (int L = 1; L <= LK_MAX_LEVEL; ++L) {
            hipLaunchKernelGGL(k_pyr_down, row_grid(n, k.h[L], k.w[L]), dim3(NT), 0, st, (const float *)k.pyr[s][L - 1], k.h[L - 1], k.w[L - 1],
                               k.pyr[s][L], k.h[L], k.w[L]);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    for (int L = 0; L <= LK_MAX_LEVEL; ++L) { P.I[L] = k.pyr[0][L]; P.J[L] = k.pyr[1][L]; P.h[L] = k.h[L]; P.w[L] = k.w[L]; }
    hipLaunchKernelGGL(k_lk_track, dim3(LK_MAX_CORNERS, n), dim3(64), 0, st, P, pts, counts, out_pts, status);
    return hipGetLastError();
}

hipError_t launch_lk_scatter(const float *pts, const float *out_pts, const uint8_t *status, const int32_t *counts, int n, int H, int W,
                             float *flow, hipStream_t st) {
    hipError_t e = hipMemsetAsync(flow, 0, (size_t)n * H * W * 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lk_scatter, dim3(n), dim3(128), 0, st, pts, out_pts, status, counts, H, W, flow);
    return hipGetLastError();
}

hipError_t launch_flow_lucas_kanade(const uint8_t *prev, const uint8_t *next, int n, int H, int W, float *flow, void *ws, hipStream_t st) {
    const LkWorkspace k = lk_carve(ws, n, H, W);
    hipError_t e;
    if ((e = launch_flow_min_eigen(prev, n, H, W, k.eig, st)) != hipSuccess) return e;
    if ((e = launch_good_features(k.eig, n, H, W, k.pts, k.counts, ws, st)) != hipSuccess) return e;
    if ((e = launch_lk_track(prev, next, n, H, W, k.pts, k.counts, k.out_pts, k.status, ws, st)) != hipSuccess) return e;
    return launch_lk_scatter(k.pts, k.out_pts, k.status, k.counts, n, H, W, flow, st);
}

}  // namespace smk
