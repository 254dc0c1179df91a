// The optimizer tail of the training step: the gradients' total 2-norm with torch's clip coefficient (clip_grads_with_norm_), and
// torch.optim.AdamW's update (decoupled weight decay, single-tensor order) with the clip folded in as a device-side scale of g.
// Both are multi-tensor launches over a host table (optim.h).  A chunk is OPT_CHUNK elements counted from element 0 of its tensor; thread
// `tid` of its workgroup owns the float4 groups (j * 256 + tid), j = 0..7, of the chunk.  That mapping, and the order in which a thread
// adds its 32 squares, is the same whether the tensor is read with 16-byte loads (pointers 16-byte aligned: every chunk then starts
// aligned too) or element by element (not aligned, or the chunk's tail), so a chunk's partial is a function of its values alone.
// Squares and sums are fp64 (the product of two floats is exact there); the partials are added in one fixed order: no atomics.
#include "optim.h"

namespace smk {

namespace {
constexpr int GROUPS = OPT_CHUNK / (OPT_THREADS * 4);       // float4 groups per thread and chunk: 8

struct NormArgs {
    const float *g[OPT_BATCH];
    long long n[OPT_BATCH];
    int start[OPT_BATCH + 1];        // first workgroup of each tensor in this launch; start[count] = the grid size
    int count;
    int partial_base;                // this launch's first slot in the partial array
};

struct AdamArgs {
    float *p[OPT_BATCH], *g[OPT_BATCH], *m[OPT_BATCH], *v[OPT_BATCH];
    long long n[OPT_BATCH];
    int start[OPT_BATCH + 1];
    int count;
};

// the tensor whose chunk range holds workgroup b (tensors without chunks are not in the table, so `start` increases strictly)
template <class A>
__device__ __forceinline__ int find_tensor(const A &a, int b) {
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.start[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// one double per thread over the 256-thread workgroup, fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return threadIdx.x == 0 ? ((red[0] + red[1]) + red[2]) + red[3] : 0.0;
}
}  // namespace

__global__ __launch_bounds__(OPT_THREADS) void k_grad_sq(const NormArgs a, double *__restrict__ partial) {
    __shared__ double red[4];
    const int b = blockIdx.x, i = find_tensor(a, b), tid = threadIdx.x;
    const long long e0 = (long long)(b - a.start[i]) * OPT_CHUNK, left = a.n[i] - e0;
    const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const float *g = a.g[i] + e0;
    float x[GROUPS][4];
    if (len == OPT_CHUNK && ((uintptr_t)a.g[i] & 15) == 0) {
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) {
            const float4 q = *(const float4 *)(g + (j * OPT_THREADS + tid) * 4);
            x[j][0] = q.x; x[j][1] = q.y; x[j][2] = q.z; x[j][3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) {
            const int o = (j * OPT_THREADS + tid) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) x[j][k] = o + k < len ? g[o + k] : 0.f;
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < GROUPS; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)x[j][k] * (double)x[j][k];
    const double t = block_sum(acc, red);
    if (tid == 0) partial[a.partial_base + b] = t;
}

// one workgroup: the partials in a fixed order (thread t takes t, t + 256, ...; then the workgroup's tree), the norm and torch's
// clip_coef = clamp(max_norm / (norm + 1e-6), max = 1) in fp32.  A NaN norm stays a NaN coefficient (the compare is false for it).
__global__ __launch_bounds__(OPT_THREADS) void k_grad_norm_finish(const double *__restrict__ partial, int count, float max_norm,
                                                                  float *__restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += OPT_THREADS) acc += partial[i];
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(t);
        const float coef = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = coef > 1.f ? 1.f : coef;
    }
}

// torch's update with ONE rounding of p: the decay p (1 - lr wd) and the step are algebraically p - (lr wd p + step m / denom); the small
// term is formed first and subtracted once, so p carries half an ulp of error per step instead of the two roundings (and the rounding of
// the coefficient 1 - lr wd to fp32) of the literal order.
__device__ __forceinline__ void adamw_update(float &p, float &g, float &m, float &v, const AdamCoef &c, float scale) {
    g = g * scale;
    m = fmaf(c.w1, g - m, m);
    v = fmaf(c.w2 * g, g, c.beta2 * v);
    const float denom = sqrtf(v) / c.rsq_bc2 + c.eps;
    p = p - fmaf(c.step, m / denom, c.lr_wd * p);
}

__device__ __forceinline__ void adamw_update4(float4 &p, float4 &g, float4 &m, float4 &v, const AdamCoef &c, float scale) {
    adamw_update(p.x, g.x, m.x, v.x, c, scale);
    adamw_update(p.y, g.y, m.y, v.y, c, scale);
    adamw_update(p.z, g.z, m.z, v.z, c, scale);
    adamw_update(p.w, g.w, m.w, v.w, c, scale);
}

// p, m, v read once and written once; g read once (and written when WRITE_G).  Four float4 groups of all four tensors are loaded
// before the first is stored (16 x 16-byte loads in flight per thread: the tensors may alias as far as the compiler knows).
template <bool WRITE_G>
__global__ __launch_bounds__(OPT_THREADS) void k_adamw(const AdamArgs a, const AdamCoef c, const float *__restrict__ grad_scale) {
    const int b = blockIdx.x, i = find_tensor(a, b), tid = threadIdx.x;
    const long long e0 = (long long)(b - a.start[i]) * OPT_CHUNK, left = a.n[i] - e0;
    const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    float *p = a.p[i] + e0, *g = a.g[i] + e0, *m = a.m[i] + e0, *v = a.v[i] + e0;
    const float scale = grad_scale ? *grad_scale : 1.f;
    const uintptr_t align = (uintptr_t)a.p[i] | (uintptr_t)a.g[i] | (uintptr_t)a.m[i] | (uintptr_t)a.v[i];
    if (len == OPT_CHUNK && (align & 15) == 0) {
        constexpr int U = 4;
#pragma unroll
        for (int j0 = 0; j0 < GROUPS; j0 += U) {
            float4 qp[U], qg[U], qm[U], qv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int o = ((j0 + u) * OPT_THREADS + tid) * 4;
                qp[u] = *(const float4 *)(p + o);
                qg[u] = *(const float4 *)(g + o);
                qm[u] = *(const float4 *)(m + o);
                qv[u] = *(const float4 *)(v + o);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int o = ((j0 + u) * OPT_THREADS + tid) * 4;
                adamw_update4(qp[u], qg[u], qm[u], qv[u], c, scale);
                *(float4 *)(p + o) = qp[u];
                *(float4 *)(m + o) = qm[u];
                *(float4 *)(v + o) = qv[u];
                if (WRITE_G) *(float4 *)(g + o) = qg[u];
            }
        }
    } else {
        for (int j = 0; j < GROUPS; ++j) {
            const int o = (j * OPT_THREADS + tid) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (o + k < len) {
                    float xp = p[o + k], xg = g[o + k], xm = m[o + k], xv = v[o + k];
                    adamw_update(xp, xg, xm, xv, c, scale);
                    p[o + k] = xp;
                    m[o + k] = xm;
                    v[o + k] = xv;
                    if (WRITE_G) g[o + k] = xg;
                }
            }
        }
    }
}

int64_t opt_chunks(const smk_opt_tensor *t, int n_tensors) {
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (t[i].n < 0) return -1;
        chunks += (t[i].n + OPT_CHUNK - 1) / OPT_CHUNK;
    }
    return chunks;
}

// Fills one launch's descriptor block from table entries [*next, ...): up to OPT_BATCH tensors that have elements, and at most `max_grid`
// workgroups unless a single tensor needs more.  Returns the grid size (0: the table is exhausted).
template <class A, class F>
static int fill_batch(const smk_opt_tensor *t, int n_tensors, int *next, A &a, F &&set) {
    constexpr int64_t max_grid = 1 << 30;
    int count = 0;
    int64_t grid = 0;
    while (*next < n_tensors && count < OPT_BATCH) {
        const smk_opt_tensor &e = t[*next];
        if (e.n > 0) {
            const int64_t c = (e.n + OPT_CHUNK - 1) / OPT_CHUNK;
            if (count > 0 && grid + c > max_grid) break;
            a.start[count] = (int)grid;
            a.n[count] = e.n;
            set(count, e);
            grid += c;
            ++count;
        }
        ++*next;
    }
    a.start[count] = (int)grid;
    a.count = count;
    return (int)grid;
}

hipError_t launch_grad_norm(const smk_opt_tensor *t, int n_tensors, float max_norm, float *out, double *partial, hipStream_t st) {
    NormArgs a;
    int next = 0, base = 0;
    for (;;) {
        const int grid = fill_batch(t, n_tensors, &next, a, [&](int k, const smk_opt_tensor &e) { a.g[k] = e.grad; });
        if (grid == 0) break;
        a.partial_base = base;
        hipLaunchKernelGGL(k_grad_sq, dim3(grid), dim3(OPT_THREADS), 0, st, a, partial);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        base += grid;
    }
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(OPT_THREADS), 0, st, partial, base, max_norm, out);
    return hipGetLastError();
}

hipError_t launch_adamw(const smk_opt_tensor *t, int n_tensors, const AdamCoef &c, const float *grad_scale, int write_grad,
                        hipStream_t st) {
    AdamArgs a;
    int next = 0;
    for (;;) {
        const int grid = fill_batch(t, n_tensors, &next, a, [&](int k, const smk_opt_tensor &e) {
            a.p[k] = e.param; a.g[k] = e.grad; a.m[k] = e.exp_avg; a.v[k] = e.exp_avg_sq;
        });
        if (grid == 0) break;
        if (write_grad) hipLaunchKernelGGL(k_adamw<true>, dim3(grid), dim3(OPT_THREADS), 0, st, a, c, grad_scale);
        else hipLaunchKernelGGL(k_adamw<false>, dim3(grid), dim3(OPT_THREADS), 0, st, a, c, grad_scale);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace smk
