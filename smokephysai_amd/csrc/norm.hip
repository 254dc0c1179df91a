// Training-mode BatchNorm2d + ReLU + mean pooling of the CNN encoder as HBM-rate kernels (smokephys_net.py:24-32: Conv -> BatchNorm2d
// -> ReLU twice, :87-91: two adaptive average pools = one P x P block mean; under autograd in train.py:88-89).  PyTorch-ROCm runs
// this as MIOpen BatchNorm + ReLU + two pooling kernels, each a full pass over the 2.1 GB of 256 x 256 maps of a batch of 64 (and
// the pooling backward as an atomic scatter); here the forward is two passes over z (statistics; normalise + ReLU + pool, writing
// only the pooled map) and the backward two passes over z plus the write of dz, the ReLU mask being recomputed from z.
//
// Layout: NCHW fp32, planes contiguous.  A workgroup owns one chunk of one (b, c) plane (bn_chunk_floats in norm.h) -- 4,096 floats, or
// 64 rows x 256 columns when pooling 8 x 8 -- as float4 per lane: consecutive lanes read consecutive 16- or 32-byte pieces of a row
// (coalesced).  Pool 4 and 8: each thread holds exactly one output cell's P x P block (256 cells per chunk: no cross-lane traffic for the
// pool).  Pool 2 (W = 64): a thread takes the float4s of a row pair, i.e. two cells side by side, again without cross-lane traffic.
// Pool 16 and 32 (W = 512 / 1,024): the chunk is one row of 32 cells, and a cell spans several lanes.  Lanes stay consecutive along a row
// -- pool 32: thread t reads the t-th float4 of each of the 32 rows (1 KiB per wave instruction); pool 16: a wave owns 128 columns, its
// lanes 0-31 read them in row 2k and lanes 32-63 in row 2k + 1 (two 512-byte runs, adjacent rows of the same chunk) -- each lane adds its
// rows in ascending order in a register, and the lanes of a cell are combined by a fixed butterfly inside the wave (__shfl_xor 1, 2, then
// 4 at pool 32 or 32 at pool 16).  In the backward passes every lane of a cell fetches the cell's dout itself.
// Reductions over (B, H, W) are two-stage and deterministic: per-chunk partial sums in a fixed lane/wave order, then one workgroup
// per channel adds the partials in a fixed order.  Variance uses sums shifted by the channel's first element (no cancellation).
#include "norm.h"
#include <type_traits>

namespace smk {

// float offset (inside the chunk) of this thread's k-th float4, and for P == 4 / 8 the chunk-local output cell = threadIdx.x
template <int P>
__device__ __forceinline__ int bn_off(int tid, int k, int W) {
    if (P == 1) return (tid + 256 * k) * 4;
    if (P == 2) return (2 * ((tid >> 4) + 16 * (k >> 1)) + (k & 1)) * W + 4 * (tid & 15);      // row pair (tid >> 4) + 16 (k >> 1), cells 2 (tid & 15), + 1
    if (P == 16) return (2 * k + ((tid >> 5) & 1)) * W + 4 * (32 * (tid >> 6) + (tid & 31));
    if (P == 32) return k * W + 4 * tid;
    const int oi = tid >> 5, oj = tid & 31;
    if (P == 8) return (8 * oi + (k >> 1)) * W + 8 * oj + 4 * (k & 1);
    return (4 * oi + k) * W + 4 * oj;                        // P == 4
}

// this thread's k-th float4 of z.  Pool 16 / 32: the loads issue G rows at a time into `rows` ahead of their use (left alone the compiler
// waits for each load before it issues the next: one KiB in flight per wave); k is a constant of the unrolled loop
template <int P>
__device__ __forceinline__ float4 bn_load(const float *zp, int tid, int k, int W, float4 (&rows)[BnShape<P>::G]) {
    constexpr int G = BnShape<P>::G;
    if (G == 1) return *reinterpret_cast<const float4 *>(zp + bn_off<P>(tid, k, W));
    if (k % G == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) rows[g] = *reinterpret_cast<const float4 *>(zp + bn_off<P>(tid, k + g, W));
    }
    return rows[k % G];
}

// P >= 4: the output cell (row, column of the pooled plane) that this thread's elements belong to, in chunk ch of the plane
template <int P>
__device__ __forceinline__ int bn_cell_row(int tid, int ch) {
    return P >= 16 ? ch : ch * (BnShape<P>::CHUNK / (32 * P) / P) + (tid >> 5);
}
template <int P>
__device__ __forceinline__ int bn_cell_col(int tid) {
    return P == 16 ? 8 * (tid >> 6) + ((tid & 31) >> 2) : P == 32 ? tid >> 3 : tid & 31;
}

// P == 16 / 32: sum over the lanes of a cell (a fixed butterfly, every lane ends with the cell's sum); true in the one lane that stores it
template <int P>
__device__ __forceinline__ bool bn_cell_sum(int tid, float &acc) {
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, P == 32 ? 4 : 32);
    return (tid & (P == 32 ? 7 : 35)) == 0;
}

__device__ __forceinline__ float2 wg_sum2(float a, float b) {   // sum over the 256 threads in a fixed order; valid in thread 0
    __shared__ float2 red[4];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m);
        b += __shfl_xor(b, m);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = make_float2(a, b);
    __syncthreads();
    return make_float2((red[0].x + red[1].x) + (red[2].x + red[3].x), (red[0].y + red[1].y) + (red[2].y + red[3].y));
}

// chunk id within a channel: b * chunks_per_plane + chunk_in_plane = blockIdx.x; channel = blockIdx.y
template <int P>
__global__ __launch_bounds__(256) void k_bn_stats(const BnTrainArgs a) {
    constexpr int CHUNK = BnShape<P>::CHUNK, NK = BnShape<P>::NK;
    const int c = blockIdx.y, cpp = a.H * a.W / CHUNK;
    const int b = blockIdx.x / cpp, ch = blockIdx.x - b * cpp;
    const float *zp = a.z + ((size_t)b * a.C + c) * a.H * a.W + (size_t)ch * CHUNK;
    const float shift = a.z[(size_t)c * a.H * a.W];                      // the channel's first element (batch 0)
    float s1 = 0.f, s2 = 0.f;
    float4 rows[BnShape<P>::G];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const float4 v = bn_load<P>(zp, threadIdx.x, k, a.W, rows);
        const float d0 = v.x - shift, d1 = v.y - shift, d2 = v.z - shift, d3 = v.w - shift;
        s1 += (d0 + d1) + (d2 + d3);
        s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    const float2 t = wg_sum2(s1, s2);
    if (threadIdx.x == 0) reinterpret_cast<float2 *>(a.part)[(size_t)c * gridDim.x + blockIdx.x] = t;
}

// one workgroup per channel: partials -> (mean, var, rstd) or (dgamma, dbeta)
__global__ __launch_bounds__(256) void k_bn_finish(const BnTrainArgs a, int nchunks, int backward) {
    const int c = blockIdx.x;
    const float2 *pp = reinterpret_cast<const float2 *>(a.part) + (size_t)c * nchunks;
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < nchunks; i += 256) { s1 += pp[i].x; s2 += pp[i].y; }
    const float2 t = wg_sum2(s1, s2);
    if (threadIdx.x != 0) return;
    if (backward) {
        a.dbeta[c] = t.x;
        a.dgamma[c] = t.y;
    } else {
        const float n = (float)a.B * (float)a.H * (float)a.W;
        const float shift = a.z[(size_t)c * a.H * a.W];
        const float m1 = t.x / n;
        float var = t.y / n - m1 * m1;
        var = var > 0.f ? var : 0.f;
        a.mean[c] = shift + m1;
        a.var[c] = var;
        a.rstd[c] = 1.0f / sqrtf(var + a.eps);
    }
}

template <int P>
__global__ __launch_bounds__(256) void k_bn_relu_pool_fwd(const BnTrainArgs a) {
    constexpr int CHUNK = BnShape<P>::CHUNK, NK = BnShape<P>::NK;
    const int c = blockIdx.y, cpp = (a.H * a.W + CHUNK - 1) / CHUNK;       // (P == 1 from given statistics: the plane's last chunk may be partial)
    const int b = blockIdx.x / cpp, ch = blockIdx.x - b * cpp;
    const size_t plane = ((size_t)b * a.C + c) * a.H * a.W;
    const float *zp = a.z + plane + (size_t)ch * CHUNK;
    const float sc = a.gamma[c] * a.rstd[c], sh = a.beta[c] - a.mean[c] * sc;      // y = z * sc + sh
    float acc = 0.f, accr = 0.f;                       // (P == 2: the left and the right cell of the float4)
    float4 rows[BnShape<P>::G];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int off = bn_off<P>(threadIdx.x, k, a.W);
        if (P == 1 && ch * CHUNK + off >= a.H * a.W) break;
        const float4 v = bn_load<P>(zp, threadIdx.x, k, a.W, rows);
        float4 y = make_float4(fmaxf(v.x * sc + sh, 0.f), fmaxf(v.y * sc + sh, 0.f), fmaxf(v.z * sc + sh, 0.f), fmaxf(v.w * sc + sh, 0.f));
        if (P == 1) *reinterpret_cast<float4 *>(a.out + plane + (size_t)ch * CHUNK + off) = y;
        else if (P == 2) {                             // rows 2 r (k even) and 2 r + 1 (k odd) of cell row r = chunk-local (tid >> 4) + 16 (k >> 1)
            acc += y.x + y.y;
            accr += y.z + y.w;
            if (k & 1) {
                const size_t oi = (size_t)ch * 32 + (threadIdx.x >> 4) + 16 * (k >> 1);
                *reinterpret_cast<float2 *>(a.out + (((size_t)b * a.C + c) * (a.H / 2) + oi) * 32 + 2 * (threadIdx.x & 15)) = make_float2(acc * 0.25f, accr * 0.25f);
                acc = accr = 0.f;
            }
        }
        else acc += (y.x + y.y) + (y.z + y.w);
    }
    if (P > 2) {     // this thread's cell; P == 4 / 8: chunk-local (tid >> 5, tid & 31) -> plane row ch * (CHUNK / W / P) + (tid >> 5)
        const int ow = a.W / P, oh = a.H / P;
        const int oi = bn_cell_row<P>(threadIdx.x, ch), oj = bn_cell_col<P>(threadIdx.x);
        if (P >= 16 && !bn_cell_sum<P>(threadIdx.x, acc)) return;
        a.out[(((size_t)b * a.C + c) * oh + oi) * ow + oj] = acc * (1.0f / (P * P));
    }
}

// dy = dout (spread over the P x P block) where y > 0; MODE 0: partial sums of (dy, dy * zhat); MODE 1: dz
template <int P, int MODE>
__global__ __launch_bounds__(256) void k_bn_relu_pool_bwd(const BnTrainArgs a) {
    constexpr int CHUNK = BnShape<P>::CHUNK, NK = BnShape<P>::NK;
    const int c = blockIdx.y, cpp = (a.H * a.W + CHUNK - 1) / CHUNK;
    const int b = blockIdx.x / cpp, ch = blockIdx.x - b * cpp;
    const size_t plane = ((size_t)b * a.C + c) * a.H * a.W;
    const float *zp = a.z + plane + (size_t)ch * CHUNK;
    const float mean = a.mean[c], rstd = a.rstd[c], g = a.gamma[c], be = a.beta[c];
    float gcell = 0.f;
    if (P > 2) {
        const int ow = a.W / P, oh = a.H / P;
        const int oi = bn_cell_row<P>(threadIdx.x, ch), oj = bn_cell_col<P>(threadIdx.x);
        gcell = a.dout[(((size_t)b * a.C + c) * oh + oi) * ow + oj] * (1.0f / (P * P));
    }
    float k1 = 0.f, k2 = 0.f;
    if (MODE == 1) {
        const float n = a.count > 0.f ? a.count : (float)a.B * (float)a.H * (float)a.W;
        k1 = a.dbeta[c] / n;
        k2 = a.dgamma[c] / n;
    }
    float s1 = 0.f, s2 = 0.f;
    float4 rows[BnShape<P>::G];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int off = bn_off<P>(threadIdx.x, k, a.W);
        if (P == 1 && ch * CHUNK + off >= a.H * a.W) break;
        const float4 v = bn_load<P>(zp, threadIdx.x, k, a.W, rows);
        float4 go = make_float4(gcell, gcell, gcell, gcell);
        if (P == 1) go = *reinterpret_cast<const float4 *>(a.dout + plane + (size_t)ch * CHUNK + off);
        if (P == 2) {                                  // the two cells of this float4, cell row chunk-local (tid >> 4) + 16 (k >> 1)
            const size_t oi = (size_t)ch * 32 + (threadIdx.x >> 4) + 16 * (k >> 1);
            const float2 g2 = *reinterpret_cast<const float2 *>(a.dout + (((size_t)b * a.C + c) * (a.H / 2) + oi) * 32 + 2 * (threadIdx.x & 15));
            go = make_float4(g2.x * 0.25f, g2.x * 0.25f, g2.y * 0.25f, g2.y * 0.25f);
        }
        const float zv[4] = {v.x, v.y, v.z, v.w}, gv[4] = {go.x, go.y, go.z, go.w};
        float r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float zh = (zv[i] - mean) * rstd;
            const float dy = (zh * g + be) > 0.f ? gv[i] : 0.f;
            if (MODE == 0) { s1 += dy; s2 += dy * zh; }
            else r[i] = g * rstd * (dy - k1 - zh * k2);
        }
        if (MODE == 1) *reinterpret_cast<float4 *>(a.dz + plane + (size_t)ch * CHUNK + off) = make_float4(r[0], r[1], r[2], r[3]);
    }
    if (MODE == 0) {
        const float2 t = wg_sum2(s1, s2);
        if (threadIdx.x == 0) reinterpret_cast<float2 *>(a.part)[(size_t)c * gridDim.x + blockIdx.x] = t;
    }
}

static int bn_chunks(const BnTrainArgs &a) { return a.B * (int)bn_chunks_per_plane(a.H, a.W, a.pool); }      // bn_check: < 2^31

long long bn_train_workspace_floats(int B, int C, int H, int W, int pool) {       // k_bn_stats / k_bn_relu_pool_bwd<., 0>: one float2 per chunk
    return 2LL * C * B * bn_chunks_per_plane(H, W, pool);
}

// f(integral_constant<int, P>) for the built pool; false for any other
template <typename F>
static bool bn_for_pool(int pool, F &&f) {
    switch (pool) {
        case 1: f(std::integral_constant<int, 1>()); return true;
        case 2: f(std::integral_constant<int, 2>()); return true;
        case 4: f(std::integral_constant<int, 4>()); return true;
        case 8: f(std::integral_constant<int, 8>()); return true;
        case 16: f(std::integral_constant<int, 16>()); return true;
        case 32: f(std::integral_constant<int, 32>()); return true;
    }
    static_assert(bn_pool_built(1) && bn_pool_built(2) && bn_pool_built(4) && bn_pool_built(8) && bn_pool_built(16) && bn_pool_built(32),
                  "bn_pool_built (norm.h) names the pools instantiated here");
    return false;
}

static bool bn_launch_stats(const BnTrainArgs &a, dim3 grid, hipStream_t st) {
    return bn_for_pool(a.pool, [&](auto p) { hipLaunchKernelGGL(k_bn_stats<decltype(p)::value>, grid, dim3(256), 0, st, a); });
}
static bool bn_launch_fwd(const BnTrainArgs &a, dim3 grid, hipStream_t st) {
    return bn_for_pool(a.pool, [&](auto p) { hipLaunchKernelGGL(k_bn_relu_pool_fwd<decltype(p)::value>, grid, dim3(256), 0, st, a); });
}
template <int MODE>
static bool bn_launch_bwd(const BnTrainArgs &a, dim3 grid, hipStream_t st) {
    return bn_for_pool(a.pool, [&](auto p) { hipLaunchKernelGGL((k_bn_relu_pool_bwd<decltype(p)::value, MODE>), grid, dim3(256), 0, st, a); });
}

hipError_t launch_bn_relu_pool_forward(const BnTrainArgs &a, hipStream_t st) {
    const int nch = bn_chunks(a);
    dim3 grid(nch, a.C);
    if (!bn_launch_stats(a, grid, st)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bn_finish, dim3(a.C), dim3(256), 0, st, a, nch, 0);
    bn_launch_fwd(a, grid, st);
    return hipGetLastError();
}

hipError_t launch_bn_stats(const BnTrainArgs &a, hipStream_t st) {
    const int nch = bn_chunks(a);
    if (!bn_launch_stats(a, dim3(nch, a.C), st)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bn_finish, dim3(a.C), dim3(256), 0, st, a, nch, 0);
    return hipGetLastError();
}

hipError_t launch_bn_relu_pool_apply(const BnTrainArgs &a, hipStream_t st) {
    if (!bn_launch_fwd(a, dim3(bn_chunks(a), a.C), st)) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_bn_relu_pool_backward_sums(const BnTrainArgs &a, hipStream_t st) {
    const int nch = bn_chunks(a);
    if (!bn_launch_bwd<0>(a, dim3(nch, a.C), st)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bn_finish, dim3(a.C), dim3(256), 0, st, a, nch, 1);
    return hipGetLastError();
}

hipError_t launch_bn_relu_pool_backward_dz(const BnTrainArgs &a, hipStream_t st) {
    if (!bn_launch_bwd<1>(a, dim3(bn_chunks(a), a.C), st)) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_bn_relu_pool_backward(const BnTrainArgs &a, hipStream_t st) {
    const int nch = bn_chunks(a);
    dim3 grid(nch, a.C);
    if (!bn_launch_bwd<0>(a, grid, st)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bn_finish, dim3(a.C), dim3(256), 0, st, a, nch, 1);
    bn_launch_bwd<1>(a, grid, st);
    return hipGetLastError();
}

}  // namespace smk
