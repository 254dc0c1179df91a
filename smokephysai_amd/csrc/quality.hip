// Image-quality metrics of RobustnessEvaluator (src/evaluation/robustness_metrics.py:76-103) over n fp32 planes [H][W]:
// the SSIM map of compute_ssim and the squared error of F.mse_loss, reduced to per-plane fp64 sums.
//   avg_pool2d(., k, stride=1, padding=k/2): count_include_pad -> zeros outside the plane, divisor always k*k
//   sigma^2 = E[x^2] - mu^2, sigma_xy = E[xy] - mu_x mu_y (the reference's cancellation kept), per-pixel arithmetic fp32
// One workgroup per 16 x 64 output tile: the (16+k-1) x (64+k-1) halo of both planes goes to LDS, the five moments
// (x, y, x^2, y^2, xy) are summed horizontally into LDS and then vertically per output pixel (direct k-term sums,
// no running add/subtract).  Each workgroup writes one (ssim, sqerr) fp64 pair; a second launch sums a plane's
// pairs in a fixed order, so repeated calls are bit-identical (no float atomics).
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

__global__ __launch_bounds__(QT_THREADS) void k_image_quality(const float *__restrict__ pred, int64_t pred_stride,
                                                              const float *__restrict__ target, int64_t target_stride, int H,
                                                              int W, int k, float c1, float c2, int tiles_x,
                                                              double2 *__restrict__ partial) {
    extern __shared__ float lds[];
    __shared__ double red[4];
    const int R = QT_H + k - 1, C = QT_W + k - 1, half = k / 2;
    float *sx = lds, *sy = sx + R * C;                                    // halo [R][C] of pred / target
    float *hx = sy + R * C, *hy = hx + R * QT_W, *hxx = hy + R * QT_W, *hyy = hxx + R * QT_W, *hxy = hyy + R * QT_W;
    const int tile = blockIdx.x, plane = blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int row0 = ty * QT_H - half, col0 = tx * QT_W - half;
    const float *a = pred + (size_t)plane * pred_stride, *b = target + (size_t)plane * target_stride;
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
    const float area = (float)(k * k);           // count_include_pad: the divisor is always k^2
    double ssim_acc = 0.0, sq_acc = 0.0;
    const int c = tid & (QT_W - 1);
    for (int r = tid / QT_W; r < QT_H; r += QT_THREADS / QT_W) {
        const int gr = ty * QT_H + r, gc = tx * QT_W + c;
        if (gr >= H || gc >= W) continue;
        float s1 = 0.f, s2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
        for (int j = 0; j < k; ++j) {
            const int o = (r + j) * QT_W + c;
            s1 += hx[o];
            s2 += hy[o];
            s11 += hxx[o];
            s22 += hyy[o];
            s12 += hxy[o];
        }
        const float mu1 = s1 / area, mu2 = s2 / area;
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float sigma1_sq = s11 / area - mu1_sq, sigma2_sq = s22 / area - mu2_sq, sigma12 = s12 / area - mu1_mu2;
        const float num = (2.f * mu1_mu2 + c1) * (2.f * sigma12 + c2);
        const float den = (mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2);
        ssim_acc += (double)(num / den);
        const int o = (r + half) * C + c + half;
        const float d = sx[o] - sy[o];
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

}  // namespace smk
