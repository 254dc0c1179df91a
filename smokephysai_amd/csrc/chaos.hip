// Chaos-statistics kernels: the integer/reduction parts of SmokeSimulator.get_chaos_features
// (/root/reference/src/physics/smoke_simulator.py:47-140), batched over n frames.
//   mean            : frame.mean() (fp64 accumulation, rounded once to fp32)
//   box counts      : scales 2,4,8,16,32 of (frame > mean)  (:89-124, the reference's Python double loop)
//   histogram       : torch.histogram(bins=256, range=(0,1)) counts (:134-135): values outside [0,1] dropped, 1.0 -> last bin
//   difference norms: ||frame[i+1] - frame[i]||_2 (:73-79), fp64 accumulation
// One 1024-thread workgroup per frame; wavefront shuffles + LDS for the reductions.
//   label scalars   : the formulas on those results (:67-87 Lyapunov, :116-122 slope, :136-140 entropy) in fp64, one wave per
//                     feature row, and the per-sample means of data_loader.py:71-88 (k_chaos_features)
#include "chaos.h"

namespace smk {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// block-wide sum of one double per thread (1024 threads = 16 waves); result valid in every thread
__device__ __forceinline__ double block_sum(double v, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];      // fixed order: deterministic
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(1024) void k_chaos_stats(const float *__restrict__ frames, int64_t stride, int H, int W,
                                                      float *__restrict__ means, int32_t *__restrict__ box_counts,
                                                      int32_t *__restrict__ hist) {
    extern __shared__ unsigned char flags[];        // level-2 box flags [bh2][bw2], reduced in place level by level
    __shared__ double red[16];
    __shared__ int lhist[256];
    __shared__ int lcount[5];
    const float *f = frames + (size_t)blockIdx.x * stride;
    const int tid = threadIdx.x, n = H * W;
    if (tid < 256) lhist[tid] = 0;
    if (tid < 5) lcount[tid] = 0;
    double s = 0.0;
    for (int k = tid; k < n; k += 1024) s += (double)f[k];
    const float mean = (float)(block_sum(s, red) / (double)n);
    if (tid == 0) means[blockIdx.x] = mean;

    // histogram + level-2 boxes
    for (int k = tid; k < n; k += 1024) {
        const float x = f[k];
        if (x >= 0.f && x <= 1.f) {
            int bin = (int)(x * 256.0f);            // exact: power-of-two scale
            bin = bin > 255 ? 255 : bin;
            atomicAdd(&lhist[bin], 1);
        }
    }
    int bh = H / 2, bw = W / 2;
    for (int k = tid; k < bh * bw; k += 1024) {
        const int bi = k / bw, bj = k - bi * bw;
        const float *p = f + (size_t)(2 * bi) * W + 2 * bj;
        const bool any = p[0] > mean || p[1] > mean || p[W] > mean || p[W + 1] > mean;
        flags[k] = any;
        if (any) atomicAdd(&lcount[0], 1);
    }
    __syncthreads();
    // levels 4, 8, 16, 32: a box has a set cell iff one of its four half-size boxes has
    int pw = bw;                                    // row pitch of the current flag level
    for (int lvl = 1; lvl < 5; ++lvl) {
        const int nh = H >> (lvl + 1), nw = W >> (lvl + 1);
        unsigned char vals[16];                     // <= 16 boxes per thread for 512^2 at level 4
        int cnt = 0;
        for (int k = tid, q = 0; k < nh * nw; k += 1024, ++q) {
            const int bi = k / nw, bj = k - bi * nw;
            const unsigned char *p = flags + (size_t)(2 * bi) * pw + 2 * bj;
            const unsigned char any = p[0] | p[1] | p[pw] | p[pw + 1];
            vals[q] = any;
            cnt += any;
        }
        __syncthreads();                            // everyone has read the previous level
        for (int k = tid, q = 0; k < nh * nw; k += 1024, ++q) flags[k] = vals[q];
        if (cnt) atomicAdd(&lcount[lvl], cnt);
        pw = nw;
        __syncthreads();
    }
    if (tid < 256) hist[(size_t)blockIdx.x * 256 + tid] = lhist[tid];
    if (tid < 5) box_counts[(size_t)blockIdx.x * 5 + tid] = lcount[tid];
}

__global__ __launch_bounds__(1024) void k_diff_norms(const float *__restrict__ frames, int64_t stride, int n_cells,
                                                     float *__restrict__ norms) {
    __shared__ double red[16];
    const float *a = frames + (size_t)blockIdx.x * stride, *b = a + stride;
    double s = 0.0;
    for (int k = threadIdx.x; k < n_cells; k += 1024) {
        const double d = (double)b[k] - (double)a[k];
        s += d * d;
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) norms[blockIdx.x] = (float)sqrt(t);
}

// ---- label scalars from the reduction results (no host round trip) ------------------------------------------------------
// One wave per feature row.  A block owns `rows_per_block` consecutive rows (its waves stride over them); with group means that
// is one group, and after a barrier threads 0..2 add the group's rows in ascending order.  No float atomics anywhere: every sum
// has one fixed order, so a call repeats bit for bit.
__device__ __forceinline__ void chaos_feature_row(const float *__restrict__ norms, const int32_t *__restrict__ box_counts,
                                                  const int32_t *__restrict__ hist, int S, int pos, int hist_len, int lane,
                                                  double *__restrict__ out) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (pos < 0 || pos >= S) {                      // wave-uniform: the row names no frame of the stream
        if (lane < 3) out[lane] = nan;
        return;
    }
    // entropy: p = count / total, -sum p log2(p + 1e-8); four consecutive bins per lane, then the shuffle tree
    const int4 c = *reinterpret_cast<const int4 *>(hist + (size_t)pos * 256 + 4 * lane);
    long long tot = (long long)c.x + c.y + c.z + c.w;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);      // integers: exact, the same in every lane
    const double total = (double)tot;                                        // 0 -> 0/0 = NaN, as the host formula
    const double p0 = (double)c.x / total, p1 = (double)c.y / total, p2 = (double)c.z / total, p3 = (double)c.w / total;
    double e = p0 * log2(p0 + 1e-8);
    e += p1 * log2(p1 + 1e-8);
    e += p2 * log2(p2 + 1e-8);
    e += p3 * log2(p3 + 1e-8);
    e = -wave_sum(e);                                                        // valid in lane 0

    // fractal dimension: |slope| of the least-squares line through (log s, log(count_s + 1)), s = 2..32, centred closed form
    double x = 0.0, y = 0.0;
    if (lane < 5) {
        x = log((double)(2 << lane));
        y = log((double)box_counts[(size_t)pos * 5 + lane] + 1.0);
    }
    double xs[5], ys[5], xm = 0.0, ym = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        xs[i] = __shfl(x, i);
        ys[i] = __shfl(y, i);
        xm += xs[i];
        ym += ys[i];
    }
    xm /= 5.0;
    ym /= 5.0;
    double sxy = 0.0, sxx = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sxy += (xs[i] - xm) * (ys[i] - ym);
        sxx += (xs[i] - xm) * (xs[i] - xm);
    }
    const double slope = fabs(sxy / sxx);

    // Lyapunov: 0 below 20 frames of history, else max(0, mean of the 18 log-ratios of the last 19 distances), summed in
    // ascending order and NOT telescoped (the host formula rounds every difference)
    double lyap = 0.0;
    if (hist_len >= 20) {                           // wave-uniform
        if (pos < 19) {
            lyap = nan;                             // the caller's error: the window would start before the stream
        } else {
            double l = 0.0;
            if (lane < 19) l = log((double)norms[pos - 19 + lane] + 1e-8);   // norms[pos-19 .. pos-1], pos - 1 <= S - 2
            const double d = __shfl_down(l, 1) - l;                          // lanes 0..17
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 18; ++i) s += __shfl(d, i);
            s /= 18.0;
            lyap = s > 0.0 ? s : 0.0;
        }
    }
    if (lane == 0) {
        out[0] = lyap;
        out[1] = slope;
        out[2] = e;
    }
}

__global__ __launch_bounds__(256) void k_chaos_features(const float *__restrict__ norms, const int32_t *__restrict__ box_counts,
                                                        const int32_t *__restrict__ hist, int S, const int32_t *__restrict__ pos,
                                                        const int32_t *__restrict__ hist_len, int F, int rows_per_block,
                                                        double *features, double *__restrict__ means) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = r0 + rows_per_block < F ? r0 + rows_per_block : F;
    for (int k = r0 + wave; k < r1; k += 4)
        chaos_feature_row(norms, box_counts, hist, S, pos[k], hist_len[k], lane, features + (size_t)k * 3);
    if (means == nullptr) return;                   // kernel argument: uniform over the grid
    __syncthreads();                                // the block's own global writes are visible to it past the barrier
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int k = r0; k < r1; ++k) s += features[(size_t)k * 3 + threadIdx.x];
        means[(size_t)blockIdx.x * 3 + threadIdx.x] = s / (double)(r1 - r0);
    }
}

hipError_t launch_chaos_stats(const float *frames, int64_t stride, int n, int H, int W, float *means, int32_t *box_counts,
                              int32_t *hist, hipStream_t st) {
    const size_t lds = (size_t)(H / 2) * (W / 2);
    hipLaunchKernelGGL(k_chaos_stats, dim3(n), dim3(1024), lds, st, frames, stride, H, W, means, box_counts, hist);
    return hipGetLastError();
}

hipError_t launch_diff_norms(const float *frames, int64_t stride, int n_pairs, int n_cells, float *norms, hipStream_t st) {
    hipLaunchKernelGGL(k_diff_norms, dim3(n_pairs), dim3(1024), 0, st, frames, stride, n_cells, norms);
    return hipGetLastError();
}

hipError_t launch_chaos_features(const float *norms, const int32_t *box_counts, const int32_t *hist, int S, const int32_t *pos,
                                 const int32_t *hist_len, int F, int n_groups, double *features, double *means, hipStream_t st) {
    const int rows = n_groups > 0 ? F / n_groups : 4;                       // one group per block, else one row per wave
    const int blocks = n_groups > 0 ? n_groups : (F + 3) / 4;
    hipLaunchKernelGGL(k_chaos_features, dim3(blocks), dim3(256), 0, st, norms, box_counts, hist, S, pos, hist_len, F, rows, features,
                       n_groups > 0 ? means : nullptr);
    return hipGetLastError();
}

}  // namespace smk
