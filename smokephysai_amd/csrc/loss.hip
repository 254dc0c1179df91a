// The training loss of train.py's batch_losses on the device:
//   recon = mean((pred - target)^2)                                  F.mse_loss
//   chaos = mean((chaos_pred - chaos_target)^2)                      F.mse_loss
//   mass  = mean over planes of (sum pred - sum target)^2            PhysicsRegularizer.mass_conservation_loss
//   continuity = mean |seq[:, t+1] - seq[:, t]|                      PhysicsRegularizer.continuity_loss (0 for T < 2)
//   physics = w_mass mass + w_continuity continuity,  total = recon + w_chaos chaos + w_physics physics
// Forward: workgroups write fp64 partial sums (differences taken in fp64, where the difference of two floats is exact), a one-workgroup
// finish adds them in a fixed order: no float atomics, repeated calls are bit-identical.  The sequence is read once: a thread walks four
// neighbouring pixels through t with the previous frame's values in registers.  Backward: one launch, the six upstream gradients read on
// the device.  16-byte accesses where the pointers and the plane sizes allow, element-wise otherwise.
#include "loss.h"

namespace smk {

namespace {
__device__ __forceinline__ double l_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// one double per thread over the 256-thread workgroup, fixed order; valid in thread 0
__device__ __forceinline__ double l_block_sum(double v, double *red) {
    v = l_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = threadIdx.x == 0 ? ((red[0] + red[1]) + red[2]) + red[3] : 0.0;
    __syncthreads();
    return t;
}
}  // namespace

int64_t loss_plane_chunks(int plane_elems) { return ((int64_t)plane_elems + LOSS_PLANE_CHUNK - 1) / LOSS_PLANE_CHUNK; }
int64_t loss_seq_chunks(long long seq_plane) { return (seq_plane + LOSS_SEQ_CHUNK - 1) / LOSS_SEQ_CHUNK; }
static bool has_sequence(const LossShape &s) { return s.seq_batch > 0 && s.seq_T >= 2 && s.seq_plane > 0; }
int64_t loss_workspace_doubles(const LossShape &s) {
    return 2 * (int64_t)s.planes * loss_plane_chunks(s.plane_elems) + (has_sequence(s) ? (int64_t)s.seq_batch * loss_seq_chunks(s.seq_plane) : 0);
}

// workgroup b = (plane, chunk): (sum d^2, sum d) of d = pred - target over the chunk
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_planes(const float *__restrict__ pred, const float *__restrict__ target,
                                                              int plane_elems, int chunks, int vec, double2 *__restrict__ partial) {
    __shared__ double red[4];
    const int b = blockIdx.x, plane = b / chunks, chunk = b - plane * chunks;
    const int c0 = chunk * LOSS_PLANE_CHUNK, len = min(plane_elems - c0, LOSS_PLANE_CHUNK);
    const size_t base = (size_t)plane * plane_elems + c0;
    const float *p = pred + base, *t = target + base;
    double sq = 0.0, sd = 0.0;
#pragma unroll
    for (int j = 0; j < LOSS_PLANE_CHUNK / (LOSS_THREADS * 4); ++j) {
        const int o = (j * LOSS_THREADS + threadIdx.x) * 4;
        float a[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && o + 4 <= len) {
            const float4 qa = *(const float4 *)(p + o), qc = *(const float4 *)(t + o);
            a[0] = qa.x; a[1] = qa.y; a[2] = qa.z; a[3] = qa.w;
            c[0] = qc.x; c[1] = qc.y; c[2] = qc.z; c[3] = qc.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (o + k < len) {
                    a[k] = p[o + k];
                    c[k] = t[o + k];
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = (double)a[k] - (double)c[k];
            sq += d * d;
            sd += d;
        }
    }
    const double tsq = l_block_sum(sq, red), tsd = l_block_sum(sd, red);
    if (threadIdx.x == 0) partial[b] = make_double2(tsq, tsd);
}

// workgroup b = (sequence, chunk of LOSS_SEQ_CHUNK pixels): sum over t of |seq[t+1] - seq[t]| for its pixels
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_continuity(const float *__restrict__ seq, int T, long long seq_plane, int chunks,
                                                                  int vec, double *__restrict__ partial) {
    __shared__ double red[4];
    const int b = blockIdx.x, s = b / chunks, chunk = b - s * chunks;
    const long long pix = (long long)chunk * LOSS_SEQ_CHUNK + threadIdx.x * 4;
    const float *f = seq + (size_t)s * T * seq_plane + pix;
    double acc = 0.0;
    if (vec && pix + 4 <= seq_plane) {
        float4 prev = *(const float4 *)f;
#pragma unroll 4
        for (int t = 1; t < T; ++t) {
            const float4 cur = *(const float4 *)(f + (size_t)t * seq_plane);
            acc += fabs((double)cur.x - (double)prev.x);
            acc += fabs((double)cur.y - (double)prev.y);
            acc += fabs((double)cur.z - (double)prev.z);
            acc += fabs((double)cur.w - (double)prev.w);
            prev = cur;
        }
    } else {
        for (int k = 0; k < 4; ++k) {
            if (pix + k >= seq_plane) break;
            float prev = f[k];
            for (int t = 1; t < T; ++t) {
                const float cur = f[(size_t)t * seq_plane + k];
                acc += fabs((double)cur - (double)prev);
                prev = cur;
            }
        }
    }
    const double total = l_block_sum(acc, red);
    if (threadIdx.x == 0) partial[b] = total;
}

struct LossFinish {
    const double2 *plane_partial;      // [planes][chunks]
    const double *seq_partial;         // [n_seq_partial]
    const float *chaos_pred, *chaos_target;
    int planes, chunks, n_chaos, n_seq_partial;
    double n_pred, n_seq;              // element counts of the two means
    double w_chaos, w_physics, w_mass, w_continuity;
    float *out, *mass_diff;
};

// one workgroup; every sum in an order that depends on the shapes only
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_finish(const LossFinish a) {
    __shared__ double red[4];
    double sq = 0.0, mass = 0.0, chaos = 0.0, cont = 0.0;
    for (int plane = threadIdx.x; plane < a.planes; plane += LOSS_THREADS) {
        const double2 *p = a.plane_partial + (size_t)plane * a.chunks;
        double psq = 0.0, pd = 0.0;
        for (int i = 0; i < a.chunks; ++i) {
            psq += p[i].x;
            pd += p[i].y;
        }
        a.mass_diff[plane] = (float)pd;
        sq += psq;
        mass += pd * pd;
    }
    for (int i = threadIdx.x; i < a.n_chaos; i += LOSS_THREADS) {
        const double d = (double)a.chaos_pred[i] - (double)a.chaos_target[i];
        chaos += d * d;
    }
    for (int i = threadIdx.x; i < a.n_seq_partial; i += LOSS_THREADS) cont += a.seq_partial[i];
    sq = l_block_sum(sq, red);
    mass = l_block_sum(mass, red);
    chaos = l_block_sum(chaos, red);
    cont = l_block_sum(cont, red);
    if (threadIdx.x == 0) {
        const double recon = sq / a.n_pred, m = mass / a.planes, c = chaos / a.n_chaos;
        const double ct = a.n_seq_partial > 0 ? cont / a.n_seq : 0.0;
        const double physics = a.w_mass * m + a.w_continuity * ct;
        a.out[0] = (float)(recon + a.w_chaos * c + a.w_physics * physics);
        a.out[1] = (float)recon;
        a.out[2] = (float)physics;
        a.out[3] = (float)c;
        a.out[4] = (float)m;
        a.out[5] = (float)ct;
    }
}

struct LossBackward {
    const float *pred, *target, *mass_diff, *chaos_pred, *chaos_target, *grad_out;
    float *d_pred, *d_chaos;
    int plane_elems, chunks, pred_blocks, n_chaos, vec;
    double two_over_n, two_over_planes, two_over_chaos, w_chaos, w_physics, w_mass;
};

// workgroups [0, pred_blocks): 1024 elements of one plane of d_pred each; the rest: 1024 elements of d_chaos each
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_backward(const LossBackward a) {
    const float g_total = a.grad_out[0], g_recon = a.grad_out[1], g_physics = a.grad_out[2], g_chaos = a.grad_out[3],
                g_mass = a.grad_out[4];
    const int b = blockIdx.x;
    if (b < a.pred_blocks) {
        const int plane = b / a.chunks, chunk = b - plane * a.chunks;
        const int o = chunk * 1024 + threadIdx.x * 4;
        const float ca = (float)(((double)g_total + (double)g_recon) * a.two_over_n);
        const float cb = (float)(((double)g_total * a.w_physics * a.w_mass + (double)g_physics * a.w_mass + (double)g_mass) * a.two_over_planes);
        const float add = cb * a.mass_diff[plane];
        const size_t base = (size_t)plane * a.plane_elems + o;
        if (a.vec && o + 4 <= a.plane_elems) {
            const float4 p = *(const float4 *)(a.pred + base), t = *(const float4 *)(a.target + base);
            float4 d;
            d.x = fmaf(ca, p.x - t.x, add);
            d.y = fmaf(ca, p.y - t.y, add);
            d.z = fmaf(ca, p.z - t.z, add);
            d.w = fmaf(ca, p.w - t.w, add);
            *(float4 *)(a.d_pred + base) = d;
        } else {
            for (int k = 0; k < 4 && o + k < a.plane_elems; ++k) a.d_pred[base + k] = fmaf(ca, a.pred[base + k] - a.target[base + k], add);
        }
    } else {
        const int i0 = (b - a.pred_blocks) * 1024 + threadIdx.x * 4;
        const float cc = (float)(((double)g_total * a.w_chaos + (double)g_chaos) * a.two_over_chaos);
        for (int k = 0; k < 4 && i0 + k < a.n_chaos; ++k) a.d_chaos[i0 + k] = cc * (a.chaos_pred[i0 + k] - a.chaos_target[i0 + k]);
    }
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

hipError_t launch_train_loss_forward(const float *pred, const float *target, const float *chaos_pred, const float *chaos_target,
                                     const float *sequence, const LossShape &s, double w_chaos, double w_physics, double w_mass,
                                     double w_continuity, float *out, float *mass_diff, double *workspace, hipStream_t st) {
    const int chunks = (int)loss_plane_chunks(s.plane_elems);
    const int vec = aligned16(pred) && aligned16(target) && s.plane_elems % 4 == 0;
    double2 *plane_partial = (double2 *)workspace;
    double *seq_partial = workspace + 2 * (size_t)s.planes * chunks;
    hipLaunchKernelGGL(k_loss_planes, dim3(s.planes * chunks), dim3(LOSS_THREADS), 0, st, pred, target, s.plane_elems, chunks, vec,
                       plane_partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int n_seq_partial = 0;
    if (sequence && has_sequence(s)) {
        const int sc = (int)loss_seq_chunks(s.seq_plane);
        n_seq_partial = s.seq_batch * sc;
        hipLaunchKernelGGL(k_loss_continuity, dim3(n_seq_partial), dim3(LOSS_THREADS), 0, st, sequence, s.seq_T, s.seq_plane, sc,
                           (int)(aligned16(sequence) && s.seq_plane % 4 == 0), seq_partial);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    LossFinish f;
    f.plane_partial = plane_partial;
    f.seq_partial = seq_partial;
    f.chaos_pred = chaos_pred;
    f.chaos_target = chaos_target;
    f.planes = s.planes;
    f.chunks = chunks;
    f.n_chaos = s.n_chaos;
    f.n_seq_partial = n_seq_partial;
    f.n_pred = (double)s.planes * s.plane_elems;
    f.n_seq = n_seq_partial ? (double)s.seq_batch * (s.seq_T - 1) * (double)s.seq_plane : 1.0;
    f.w_chaos = w_chaos;
    f.w_physics = w_physics;
    f.w_mass = w_mass;
    f.w_continuity = w_continuity;
    f.out = out;
    f.mass_diff = mass_diff;
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(LOSS_THREADS), 0, st, f);
    return hipGetLastError();
}

hipError_t launch_train_loss_backward(const float *pred, const float *target, const float *mass_diff, const float *chaos_pred,
                                      const float *chaos_target, const LossShape &s, const float *grad_out, double w_chaos,
                                      double w_physics, double w_mass, float *d_pred, float *d_chaos, hipStream_t st) {
    LossBackward a;
    a.pred = pred; a.target = target; a.mass_diff = mass_diff; a.chaos_pred = chaos_pred; a.chaos_target = chaos_target;
    a.grad_out = grad_out; a.d_pred = d_pred; a.d_chaos = d_chaos;
    a.plane_elems = s.plane_elems;
    a.chunks = (s.plane_elems + 1023) / 1024;
    a.pred_blocks = d_pred ? s.planes * a.chunks : 0;
    a.n_chaos = s.n_chaos;
    a.vec = aligned16(pred) && aligned16(target) && aligned16(d_pred) && s.plane_elems % 4 == 0;
    a.two_over_n = 2.0 / ((double)s.planes * s.plane_elems);
    a.two_over_planes = 2.0 / s.planes;
    a.two_over_chaos = 2.0 / s.n_chaos;
    a.w_chaos = w_chaos; a.w_physics = w_physics; a.w_mass = w_mass;
    const int grid = a.pred_blocks + (d_chaos ? (s.n_chaos + 1023) / 1024 : 0);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_loss_backward, dim3(grid), dim3(LOSS_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace smk
