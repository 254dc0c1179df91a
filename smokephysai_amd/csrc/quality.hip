// Image-quality metrics of RobustnessEvaluator (src/evaluation/robustness_metrics.py:76-103) over n fp32 planes [H][W]:
// the SSIM map of compute_ssim and the squared error of F.mse_loss, reduced to per-plane fp64 sums.
//   avg_pool2d(., k, stride=1, padding=k/2): count_include_pad -> zeros outside the plane, divisor always k*k
//   sigma^2 = E[x^2] - mu^2, sigma_xy = E[xy] - mu_x mu_y (the reference's cancellation kept), per-pixel arithmetic fp32
// One workgroup per 16 x 64 output tile: the (16+k-1) x (64+k-1) halo of both planes goes to LDS, the five moments
// (x, y, x^2, y^2, xy) are summed horizontally into LDS and then vertically per output pixel (direct k-term sums,
// no running add/subtract).  Each workgroup writes one (ssim, sqerr) fp64 pair; a second launch sums a plane's
// pairs in a fixed order, so repeated calls are bit-identical (no float atomics).
// The gradient of a plane's mean SSIM with respect to pred (for a training loss) is two more launches on the same tiling, below.
#include "quality.h"

namespace smk {

namespace {
constexpr int QT_H = 16, QT_W = 64, QT_THREADS = 256;

__device__ __forceinline__ double q_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// sum of one double per thread over a 256-thread workgroup, fixed order; valid in thread 0
__device__ __forceinline__ double q_block_sum(double v, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = q_wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) t = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return t;
}
}  // namespace

size_t quality_lds_bytes(int k) {
    const int R = QT_H + k - 1, C = QT_W + k - 1;
    return (size_t)(2 * R * C + 5 * R * QT_W) * sizeof(float);
}

int64_t quality_tiles(int H, int W) { return (int64_t)((H + QT_H - 1) / QT_H) * ((W + QT_W - 1) / QT_W); }

namespace {
// One tile's LDS: the halo [R][C] of both planes and the horizontal k-sums [R][QT_W] of the five moments.
struct QTile {
    const float *sx, *sy, *hx, *hy, *hxx, *hyy, *hxy;
    int C;
};
struct QMoments {
    float s1, s2, s11, s22, s12;
};

// Fills the tile whose halo starts at (row0, col0) of planes a, b (zeros outside the plane); ends with a barrier.
__device__ __forceinline__ QTile q_fill_tile(float *lds, const float *__restrict__ a, const float *__restrict__ b, int H, int W, int k,
                                             int row0, int col0) {
    const int R = QT_H + k - 1, C = QT_W + k - 1;
    float *sx = lds, *sy = sx + R * C;                                    // halo [R][C] of pred / target
    float *hx = sy + R * C, *hy = hx + R * QT_W, *hxx = hy + R * QT_W, *hyy = hxx + R * QT_W, *hxy = hyy + R * QT_W;
    const int tid = threadIdx.x;
    for (int i = tid; i < R * C; i += QT_THREADS) {
        const int r = i / C, c = i - r * C;
        const int gr = row0 + r, gc = col0 + c;
        const bool in = gr >= 0 && gr < H && gc >= 0 && gc < W;
        const size_t off = in ? (size_t)gr * W + gc : 0;
        sx[i] = in ? a[off] : 0.f;
        sy[i] = in ? b[off] : 0.f;
    }
    __syncthreads();
    // horizontal k-sums of the five moments for every halo row and output column
    for (int i = tid; i < R * QT_W; i += QT_THREADS) {
        const int r = i / QT_W, c = i - r * QT_W;
        const float *px = sx + r * C + c, *py = sy + r * C + c;
        float s1 = 0.f, s2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
        for (int j = 0; j < k; ++j) {
            const float x = px[j], y = py[j];
            s1 += x;
            s2 += y;
            s11 += x * x;
            s22 += y * y;
            s12 += x * y;
        }
        hx[i] = s1; hy[i] = s2; hxx[i] = s11; hyy[i] = s22; hxy[i] = s12;
    }
    __syncthreads();
    return QTile{sx, sy, hx, hy, hxx, hyy, hxy, C};
}

// vertical k-sums of the five moments at output pixel (r, c) of the tile
__device__ __forceinline__ QMoments q_pixel_sums(const QTile &t, int r, int c, int k) {
    QMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
        const int o = (r + j) * QT_W + c;
        m.s1 += t.hx[o];
        m.s2 += t.hy[o];
        m.s11 += t.hxx[o];
        m.s22 += t.hyy[o];
        m.s12 += t.hxy[o];
    }
    return m;
}
}  // namespace

__global__ __launch_bounds__(QT_THREADS) void k_image_quality(const float *__restrict__ pred, int64_t pred_stride,
                                                              const float *__restrict__ target, int64_t target_stride, int H,
                                                              int W, int k, float c1, float c2, int tiles_x,
                                                              double2 *__restrict__ partial) {
    extern __shared__ float lds[];
    __shared__ double red[4];
    const int half = k / 2;
    const int tile = blockIdx.x, plane = blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int tid = threadIdx.x;
    const QTile t = q_fill_tile(lds, pred + (size_t)plane * pred_stride, target + (size_t)plane * target_stride, H, W, k,
                                ty * QT_H - half, tx * QT_W - half);
    const float area = (float)(k * k);           // count_include_pad: the divisor is always k^2
    double ssim_acc = 0.0, sq_acc = 0.0;
    const int c = tid & (QT_W - 1);
    for (int r = tid / QT_W; r < QT_H; r += QT_THREADS / QT_W) {
        const int gr = ty * QT_H + r, gc = tx * QT_W + c;
        if (gr >= H || gc >= W) continue;
        const QMoments m = q_pixel_sums(t, r, c, k);
        const float mu1 = m.s1 / area, mu2 = m.s2 / area;
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float sigma1_sq = m.s11 / area - mu1_sq, sigma2_sq = m.s22 / area - mu2_sq, sigma12 = m.s12 / area - mu1_mu2;
        const float num = (2.f * mu1_mu2 + c1) * (2.f * sigma12 + c2);
        const float den = (mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2);
        ssim_acc += (double)(num / den);
        const int o = (r + half) * t.C + c + half;
        const float d = t.sx[o] - t.sy[o];
        sq_acc += (double)(d * d);
    }
    const double ts = q_block_sum(ssim_acc, red);
    const double te = q_block_sum(sq_acc, red);
    if (tid == 0) partial[(size_t)plane * gridDim.x + tile] = make_double2(ts, te);
}

// one workgroup per plane: its tiles' pairs in a fixed order
__global__ __launch_bounds__(QT_THREADS) void k_image_quality_sum(const double2 *__restrict__ partial, int tiles,
                                                                  double *__restrict__ ssim_sum, double *__restrict__ sqerr_sum) {
    __shared__ double red[4];
    const double2 *p = partial + (size_t)blockIdx.x * tiles;
    double s = 0.0, e = 0.0;
    for (int i = threadIdx.x; i < tiles; i += QT_THREADS) {
        s += p[i].x;
        e += p[i].y;
    }
    const double ts = q_block_sum(s, red);
    const double te = q_block_sum(e, red);
    if (threadIdx.x == 0) {
        ssim_sum[blockIdx.x] = ts;
        sqerr_sum[blockIdx.x] = te;
    }
}

hipError_t launch_image_quality(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int n, int H,
                                int W, int k, float c1, float c2, void *workspace, double *ssim_sum, double *sqerr_sum,
                                hipStream_t st) {
    const size_t lds = quality_lds_bytes(k);
    once_per_device((const void *)k_image_quality, [] {                  // k = 31 needs 92 KiB of the CU's 160 KiB
        (void)hipFuncSetAttribute((const void *)k_image_quality, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)quality_lds_bytes(QUALITY_MAX_WINDOW));
    });
    const int tiles_x = (W + QT_W - 1) / QT_W;
    const int tiles = (int)quality_tiles(H, W);
    double2 *partial = (double2 *)workspace;
    hipLaunchKernelGGL(k_image_quality, dim3(tiles, n), dim3(QT_THREADS), lds, st, pred, pred_stride, target, target_stride, H, W, k,
                       c1, c2, tiles_x, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_image_quality_sum, dim3(n), dim3(QT_THREADS), 0, st, partial, tiles, ssim_sum, sqerr_sum);
    return hipGetLastError();
}

// ---- gradient of each plane's mean SSIM with respect to pred (DESIGN.md 8.1 "Gradient") ---------------------------------
// With g = plane_grad / (H W) and the forward's per-pixel quantities (A1, A2 the numerator's factors, B1, B2 the denominator's):
//   b = g (-S / B2)                                              dS/dE[xx]
//   c = g (2 A1 / (B1 B2))                                       dS/dE[xy]
//   a = g (2 mu_y A2 / (B1 B2) - 2 mu_x S / B1) - (mu_y c + 2 mu_x b)   total dS/dmu_x
//   dpred = box(a) + (2 x box(b) + y box(c))
// Where the window is flat, b and c grow like 1 / C2 while the gradient stays small: the bracketed pairs have opposite signs and are
// summed first, so that cancellation happens between them and not against the small terms (a single pixel with pred ~ target at
// k = 1: 2e-5 .. 8e-5 of the float64 gradient, against 3e-3 .. 2e-2 in the order written without brackets).
// The zero-padded box with a constant divisor is its own transpose, so the outer boxes are the forward's filter again.  Launch 1
// is the forward's tile up to the moments and writes a, b, c [n][3][H][W] to the workspace; launch 2 box-sums them over the same
// tiling and writes every element of dpred once.  Direct k-term sums in a fixed order, no atomics.
size_t quality_backward_lds_bytes(int k) {
    const int R = QT_H + k - 1, C = QT_W + k - 1;
    return (size_t)(3 * R * C + 3 * R * QT_W) * sizeof(float);
}

__global__ __launch_bounds__(QT_THREADS) void k_image_quality_coeff(const float *__restrict__ pred, int64_t pred_stride,
                                                                    const float *__restrict__ target, int64_t target_stride, int H,
                                                                    int W, int k, float c1, float c2, int tiles_x,
                                                                    const float *__restrict__ plane_grad, float *__restrict__ coeff) {
    extern __shared__ float lds[];
    const int half = k / 2;
    const int tile = blockIdx.x, plane = blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int tid = threadIdx.x;
    const QTile t = q_fill_tile(lds, pred + (size_t)plane * pred_stride, target + (size_t)plane * target_stride, H, W, k,
                                ty * QT_H - half, tx * QT_W - half);
    const float area = (float)(k * k);
    const size_t hw = (size_t)H * W;
    const float g = plane_grad[plane] / (float)hw;
    float *ca = coeff + (size_t)plane * 3 * hw, *cb = ca + hw, *cc = cb + hw;
    const int c = tid & (QT_W - 1);
    for (int r = tid / QT_W; r < QT_H; r += QT_THREADS / QT_W) {
        const int gr = ty * QT_H + r, gc = tx * QT_W + c;
        if (gr >= H || gc >= W) continue;
        const QMoments m = q_pixel_sums(t, r, c, k);
        const float mu1 = m.s1 / area, mu2 = m.s2 / area;
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float sigma1_sq = m.s11 / area - mu1_sq, sigma2_sq = m.s22 / area - mu2_sq, sigma12 = m.s12 / area - mu1_mu2;
        const float a1 = 2.f * mu1_mu2 + c1, a2 = 2.f * sigma12 + c2;
        const float b1 = mu1_sq + mu2_sq + c1, b2 = sigma1_sq + sigma2_sq + c2;
        const float den = b1 * b2;
        const float s = (a1 * a2) / den;
        const float vb = g * (-s / b2);
        const float vc = g * (2.f * a1 / den);
        // mu2 * vc and 2 mu1 * vb are of size 1 / B2 with opposite signs: summed first, they cancel before they meet the small term
        const float va = g * (2.f * mu2 * a2 / den - 2.f * mu1 * s / b1) - (mu2 * vc + 2.f * mu1 * vb);
        const size_t o = (size_t)gr * W + gc;
        ca[o] = va;
        cb[o] = vb;
        cc[o] = vc;
    }
}

__global__ __launch_bounds__(QT_THREADS) void k_image_quality_dpred(const float *__restrict__ pred, int64_t pred_stride,
                                                                    const float *__restrict__ target, int64_t target_stride, int H,
                                                                    int W, int k, int tiles_x, const float *__restrict__ coeff,
                                                                    float *__restrict__ dpred, int64_t dpred_stride) {
    extern __shared__ float lds[];
    const int R = QT_H + k - 1, C = QT_W + k - 1, half = k / 2;
    float *sc = lds;                                                      // halo [3][R][C] of a, b, c
    float *hc = sc + 3 * R * C;                                           // their horizontal k-sums [3][R][QT_W]
    const int tile = blockIdx.x, plane = blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int row0 = ty * QT_H - half, col0 = tx * QT_W - half;
    const size_t hw = (size_t)H * W;
    const float *co = coeff + (size_t)plane * 3 * hw;
    const int tid = threadIdx.x;
    for (int i = tid; i < R * C; i += QT_THREADS) {
        const int r = i / C, c = i - r * C;
        const int gr = row0 + r, gc = col0 + c;
        const bool in = gr >= 0 && gr < H && gc >= 0 && gc < W;
        const size_t off = in ? (size_t)gr * W + gc : 0;
        sc[i] = in ? co[off] : 0.f;
        sc[R * C + i] = in ? co[hw + off] : 0.f;
        sc[2 * R * C + i] = in ? co[2 * hw + off] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < R * QT_W; i += QT_THREADS) {
        const int r = i / QT_W, c = i - r * QT_W;
        const float *p = sc + r * C + c;
        float sa = 0.f, sb = 0.f, sv = 0.f;
        for (int j = 0; j < k; ++j) {
            sa += p[j];
            sb += p[R * C + j];
            sv += p[2 * R * C + j];
        }
        hc[i] = sa; hc[R * QT_W + i] = sb; hc[2 * R * QT_W + i] = sv;
    }
    __syncthreads();
    const float area = (float)(k * k);
    const float *x = pred + (size_t)plane * pred_stride, *y = target + (size_t)plane * target_stride;
    float *d = dpred + (size_t)plane * dpred_stride;
    const int c = tid & (QT_W - 1);
    for (int r = tid / QT_W; r < QT_H; r += QT_THREADS / QT_W) {
        const int gr = ty * QT_H + r, gc = tx * QT_W + c;
        if (gr >= H || gc >= W) continue;
        float sa = 0.f, sb = 0.f, sv = 0.f;
        for (int j = 0; j < k; ++j) {
            const int o = (r + j) * QT_W + c;
            sa += hc[o];
            sb += hc[R * QT_W + o];
            sv += hc[2 * R * QT_W + o];
        }
        const size_t o = (size_t)gr * W + gc;
        d[o] = sa / area + (2.f * x[o] * (sb / area) + y[o] * (sv / area));          // the two large terms first, as in a
    }
}

hipError_t launch_image_quality_backward(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int n,
                                         int H, int W, int k, float c1, float c2, const float *plane_grad, void *workspace,
                                         float *dpred, int64_t dpred_stride, hipStream_t st) {
    once_per_device((const void *)k_image_quality_coeff, [] {
        (void)hipFuncSetAttribute((const void *)k_image_quality_coeff, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)quality_lds_bytes(QUALITY_MAX_WINDOW));
        (void)hipFuncSetAttribute((const void *)k_image_quality_dpred, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)quality_backward_lds_bytes(QUALITY_MAX_WINDOW));
    });
    const int tiles_x = (W + QT_W - 1) / QT_W;
    const int tiles = (int)quality_tiles(H, W);
    float *coeff = (float *)workspace;
    hipLaunchKernelGGL(k_image_quality_coeff, dim3(tiles, n), dim3(QT_THREADS), quality_lds_bytes(k), st, pred, pred_stride, target,
                       target_stride, H, W, k, c1, c2, tiles_x, plane_grad, coeff);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_image_quality_dpred, dim3(tiles, n), dim3(QT_THREADS), quality_backward_lds_bytes(k), st, pred, pred_stride,
                       target, target_stride, H, W, k, tiles_x, coeff, dpred, dpred_stride);
    return hipGetLastError();
}

}  // namespace smk
