// Stencil kernels of the batched stable-fluids step (gfx950).
//
// Arithmetic contract: every kernel evaluates the reference's fp32 expression tree with ONE rounding per
// reference elementwise op (file is compiled with -ffp-contract=off; divides/sqrt are the correctly rounded
// forms), so velocity/pressure/density grids are bit-identical to the torch-CPU reference for identical inputs.
// Reference: /root/reference/src/physics/navier_stokes.py (lines cited per kernel).
#include <map>
#include <mutex>

#include "stencil.h"
#include "jacobi_plan.h"

#include <math.h>
#include <stdlib.h>
#include <type_traits>

namespace smk {

#define TX 64
#define TY 4

__device__ __forceinline__ float clampf(float x, float lo, float hi) {
    float t = x < lo ? lo : x;   // torch.clamp = min(max(x, lo), hi)
    return t > hi ? hi : t;
}
__device__ __forceinline__ int clampi(int x, int lo, int hi) {
    int t = x < lo ? lo : x;
    return t > hi ? hi : t;
}

// The plan's view of a call: the geometry (plan_geom), and the layout it runs on (plan_layout): the strides and the alignment of the state
// the step reads (`in`, may be null: no such stage in this call) and of the u, v the projection rewrites.
static unsigned long long addr_bits(const float *a, const float *b, const float *c = nullptr) {
    return (unsigned long long)(uintptr_t)a | (unsigned long long)(uintptr_t)b | (unsigned long long)(uintptr_t)c;
}
static PlanGeom plan_geom(const Geom &g) { return PlanGeom{g.H, g.W, g.B, g.pc, g.pv, g.sc}; }
static PlanLayout plan_layout(const Geom &g, const StateView *in, const float *u, const float *v) {
    return PlanLayout{g.su, g.sv, in ? ptr_align(addr_bits(in->u, in->v, in->d)) : 16, ptr_align(addr_bits(u, v))};
}
// The buoyancy + diffusion stage as a launch of its own has one gate for the loads of `in` and the stores of `out`: both sides' pointers count.
static PlanLayout buoy_diffuse_layout(const Geom &g, const StateView &in, const StateView &out) {
    PlanLayout l = plan_layout(g, &in, out.u, out.v);
    l.in_align = ptr_align(addr_bits(in.u, in.v, in.d) | addr_bits(out.u, out.v, out.d));
    return l;
}

// ---------------------------------------------------------------- reset (navier_stokes.py:24-35)
__global__ void k_zero_state(Geom g, StateView s, const uint8_t *mask) {
    int b = blockIdx.z;
    if (mask && !mask[b]) return;
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i <= g.H && j < g.pc) s.u[b * g.su + (size_t)i * g.pc + j] = 0.f;
    if (i < g.H && j < g.pv) s.v[b * g.sv + (size_t)i * g.pv + j] = 0.f;
    if (i < g.H && j < g.pc) {
        s.p[b * g.sc + (size_t)i * g.pc + j] = 0.f;
        s.d[b * g.sc + (size_t)i * g.pc + j] = 0.f;
    }
}

hipError_t launch_zero_state(const Geom &g, StateView s, const uint8_t *dev_mask, hipStream_t st) {
    int maxp = g.pc > g.pv ? g.pc : g.pv;
    dim3 grid(cdiv(maxp, TX), cdiv(g.H + 1, TY), g.B), block(TX, TY);
    hipLaunchKernelGGL(k_zero_state, grid, block, 0, st, g, s, dev_mask);
    return hipGetLastError();
}

// ---------------------------------------------------------------- sources (navier_stokes.py:37-48)
// dist = sqrt(float(dx^2+dy^2)); mask dist<=radius; density += fint * exp(-(dist*dist)/denom)
__global__ void k_add_sources(Geom g, float *density, const SrcDev *src, const int *first) {
    int b = blockIdx.z;
    int s0 = first[b], s1 = first[b + 1];
    if (s0 == s1) return;
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= g.H || j >= g.W) return;
    float *cell = density + b * g.sc + (size_t)i * g.pc + j;
    float d = *cell;
    for (int s = s0; s < s1; ++s) {
        SrcDev q = src[s];
        int dx = j - q.x, dy = i - q.y;
        float dist = __fsqrt_rn((float)(dx * dx + dy * dy));
        if (dist <= (float)q.radius) {
            float e = expf(-__fdiv_rn(dist * dist, q.denom));
            d = d + q.fint * e;
        }
    }
    *cell = d;
}

hipError_t launch_add_sources(const Geom &g, float *density, const SrcDev *dev_src, const int *dev_first, hipStream_t st) {
    dim3 grid(cdiv(g.W, TX), cdiv(g.H, TY), g.B), block(TX, TY);
    hipLaunchKernelGGL(k_add_sources, grid, block, 0, st, g, density, dev_src, dev_first);
    return hipGetLastError();
}

// ---------------------------------------------------------------- diffusion (navier_stokes.py:50-72)
// out = c + coef*((((up+down)+left)+right) - 4*c), replicate padding.
__device__ __forceinline__ float diffuse_at(const float *f, int R, int C, int pitch, int i, int j, float coef) {
    int iu = i > 0 ? i - 1 : 0, id = i < R - 1 ? i + 1 : R - 1;
    int jl = j > 0 ? j - 1 : 0, jr = j < C - 1 ? j + 1 : C - 1;
    float c = f[(size_t)i * pitch + j];
    float lap = f[(size_t)iu * pitch + j] + f[(size_t)id * pitch + j];
    lap = lap + f[(size_t)i * pitch + jl];
    lap = lap + f[(size_t)i * pitch + jr];
    lap = lap - 4.0f * c;
    return c + coef * lap;
}

__global__ void k_diffuse(const float *in, float *out, int R, int C, int pitch, size_t stride, float coef) {
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= R || j >= C) return;
    const float *f = in + blockIdx.z * stride;
    out[blockIdx.z * stride + (size_t)i * pitch + j] = diffuse_at(f, R, C, pitch, i, j, coef);
}

hipError_t launch_diffuse(const float *in, float *out, int B, int R, int C, int pitch, float coef, hipStream_t st) {
    dim3 grid(cdiv(C, TX), cdiv(R, TY), B), block(TX, TY);
    hipLaunchKernelGGL(k_diffuse, grid, block, 0, st, in, out, R, C, pitch, (size_t)R * pitch, coef);
    return hipGetLastError();
}

// buoyancy (navier_stokes.py:154-155) fused into the three diffusions (:158-160).
// v_b(i,j) = j < W ? v + dt*(density*0.1) : v    -- the buoyancy-updated v that diffusion_step(v) sees.
__device__ __forceinline__ float vbuoy(const float *v, const float *d, const Geom &g, int i, int j) {
    float x = v[(size_t)i * g.pv + j];
    if (j < g.W) {
        float b = d[(size_t)i * g.pc + j] * 0.1f;
        x = x + g.dt * b;
    }
    return x;
}

__global__ void k_buoy_diffuse(Geom g, StateView in, StateView out) {
    int b = blockIdx.z;
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    const float *u = in.u + b * g.su, *v = in.v + b * g.sv, *d = in.d + b * g.sc;
    if (i <= g.H && j < g.W)
        out.u[b * g.su + (size_t)i * g.pc + j] = diffuse_at(u, g.H + 1, g.W, g.pc, i, j, g.coef_uv);
    if (i < g.H && j < g.W)
        out.d[b * g.sc + (size_t)i * g.pc + j] = diffuse_at(d, g.H, g.W, g.pc, i, j, g.coef_d);
    if (i < g.H && j <= g.W) {
        int iu = i > 0 ? i - 1 : 0, id = i < g.H - 1 ? i + 1 : g.H - 1;
        int jl = j > 0 ? j - 1 : 0, jr = j < g.W ? j + 1 : g.W;
        float c = vbuoy(v, d, g, i, j);
        float lap = vbuoy(v, d, g, iu, j) + vbuoy(v, d, g, id, j);
        lap = lap + vbuoy(v, d, g, i, jl);
        lap = lap + vbuoy(v, d, g, i, jr);
        lap = lap - 4.0f * c;
        out.v[b * g.sv + (size_t)i * g.pv + j] = c + g.coef_uv * lap;
    }
}

// The same stage with four consecutive columns per thread (W % 4 == 0): the centre / up / down rows of u, v, density arrive as nine
// 16-byte loads plus the row's two outer neighbours instead of ~20 dword loads per cell (k_buoy_diffuse moved 173 MB for 117 MB of
// fields and spent 78 % of its wave cycles waiting on them).  Per cell the expression tree is diffuse_at's / vbuoy's.
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void diffuse4(const float4 &cc, const float4 &uu, const float4 &dd, float left, float right, float coef,
                                         float (&out)[4]) {
    const float c[4] = {cc.x, cc.y, cc.z, cc.w}, up[4] = {uu.x, uu.y, uu.z, uu.w}, dn[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float lap = up[k] + dn[k];
        lap = lap + (k > 0 ? c[k - 1] : left);
        lap = lap + (k < 3 ? c[k + 1] : right);
        lap = lap - 4.0f * c[k];
        out[k] = c[k] + coef * lap;
    }
}
__device__ __forceinline__ float4 buoy4(const float4 &v, const float4 &d, float dt) {   // v + dt * (d * 0.1): two roundings per product chain
    float4 r;
    float b;
    b = d.x * 0.1f; r.x = v.x + dt * b;
    b = d.y * 0.1f; r.y = v.y + dt * b;
    b = d.z * 0.1f; r.z = v.z + dt * b;
    b = d.w * 0.1f; r.w = v.w + dt * b;
    return r;
}

__global__ __launch_bounds__(256) void k_buoy_diffuse4(Geom g, StateView in, StateView out) {
    const int b = blockIdx.z, jq = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y, j0 = 4 * jq;
    if (j0 >= g.W || i > g.H) return;
    const float *u = in.u + b * g.su, *v = in.v + b * g.sv, *d = in.d + b * g.sc;
    const int jl = j0 > 0 ? j0 - 1 : 0, jr = j0 + 4 < g.W ? j0 + 4 : g.W - 1;
    {   // u: H+1 rows
        const int iu = i > 0 ? i - 1 : 0, id = i < g.H ? i + 1 : g.H;
        const float *row = u + (size_t)i * g.pc;
        float o[4];
        diffuse4(ld4(row + j0), ld4(u + (size_t)iu * g.pc + j0), ld4(u + (size_t)id * g.pc + j0), row[jl], row[jr], g.coef_uv, o);
        st4(out.u + b * g.su + (size_t)i * g.pc + j0, o);
    }
    if (i >= g.H) return;
    const int iu = i > 0 ? i - 1 : 0, id = i < g.H - 1 ? i + 1 : g.H - 1;
    const float *drow = d + (size_t)i * g.pc, *vrow = v + (size_t)i * g.pv;
    const float4 dc = ld4(drow + j0), du = ld4(d + (size_t)iu * g.pc + j0), dd = ld4(d + (size_t)id * g.pc + j0);
    const float dl = drow[jl], dr = drow[jr];
    {   // density
        float o[4];
        diffuse4(dc, du, dd, dl, dr, g.coef_d, o);
        st4(out.d + b * g.sc + (size_t)i * g.pc + j0, o);
    }
    {   // v with the buoyancy of this step folded in (columns < W receive it; column W does not)
        const float4 vc = buoy4(ld4(vrow + j0), dc, g.dt), vu = buoy4(ld4(v + (size_t)iu * g.pv + j0), du, g.dt),
                     vd = buoy4(ld4(v + (size_t)id * g.pv + j0), dd, g.dt);
        float left = vc.x, right;
        if (j0 > 0) {
            const float bb = dl * 0.1f;
            left = vrow[j0 - 1] + g.dt * bb;
        }
        if (j0 + 4 < g.W) {
            const float bb = drow[j0 + 4] * 0.1f;
            right = vrow[j0 + 4] + g.dt * bb;
        } else {
            right = vrow[g.W];                                // v_b(i, W) = v(i, W)
        }
        float o[4];
        diffuse4(vc, vu, vd, left, right, g.coef_uv, o);
        st4(out.v + b * g.sv + (size_t)i * g.pv + j0, o);
        if (j0 + 4 == g.W) {                                  // the field's last column j = W: right neighbour = itself
            const float c = vrow[g.W];
            float lap = v[(size_t)iu * g.pv + g.W] + v[(size_t)id * g.pv + g.W];
            lap = lap + vc.w;
            lap = lap + c;
            lap = lap - 4.0f * c;
            out.v[b * g.sv + (size_t)i * g.pv + g.W] = c + g.coef_uv * lap;
        }
    }
}

hipError_t launch_buoy_diffuse(const Geom &g, StateView in, StateView out, hipStream_t st) {
    if (buoy_diffuse_vec4(plan_geom(g), buoy_diffuse_layout(g, in, out))) {
        dim3 grid(cdiv(g.W / 4, TX), cdiv(g.H + 1, TY), g.B), block(TX, TY);
        hipLaunchKernelGGL(k_buoy_diffuse4, grid, block, 0, st, g, in, out);
        return hipGetLastError();
    }
    dim3 grid(cdiv(g.W + 1, TX), cdiv(g.H + 1, TY), g.B), block(TX, TY);
    hipLaunchKernelGGL(k_buoy_diffuse, grid, block, 0, st, g, in, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- projection (navier_stokes.py:133-149)
// div = (((u[i+1,j]-u[i,j]) + v[i,j+1]) - v[i,j]) / dt       (true fp32 divide, as torch CPU)
__global__ void k_divergence(Geom g, const float *u, const float *v, float *div, int dp, size_t ds) {
    int b = blockIdx.z;
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= g.H || j >= g.W) return;
    const float *ub = u + b * g.su, *vb = v + b * g.sv;
    float a = ub[(size_t)(i + 1) * g.pc + j] - ub[(size_t)i * g.pc + j];
    a = a + vb[(size_t)i * g.pv + j + 1];
    a = a - vb[(size_t)i * g.pv + j];
    div[b * ds + (size_t)i * dp + j] = __fdiv_rn(a, g.dt);
}

hipError_t launch_divergence(const Geom &g, const float *u, const float *v, float *div, int dp, size_t ds,
                             hipStream_t st) {
    dim3 grid(cdiv(g.W, TX), cdiv(g.H, TY), g.B), block(TX, TY);
    hipLaunchKernelGGL(k_divergence, grid, block, 0, st, g, u, v, div, dp, ds);
    return hipGetLastError();
}

// One Jacobi sweep: ring = 0, interior 0.25*((((up+down)+left)+right) - div)   (:140-145)
__global__ void k_jacobi_sweep(Geom g, const float *p, float *pn, const float *div) {
    int b = blockIdx.z;
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= g.H || j >= g.W) return;
    const float *pb = p + b * g.sc;
    size_t o = (size_t)i * g.pc + j;
    float r = 0.f;
    if (i > 0 && i < g.H - 1 && j > 0 && j < g.W - 1) {
        float s = pb[o - g.pc] + pb[o + g.pc];
        s = s + pb[o - 1];
        s = s + pb[o + 1];
        s = s - div[b * g.sc + o];
        r = 0.25f * s;
    }
    pn[b * g.sc + o] = r;
}

__global__ void k_copy_cells(Geom g, const float *src, float *dst) {
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= g.H || j >= g.W) return;
    size_t o = blockIdx.z * g.sc + (size_t)i * g.pc + j;
    dst[o] = src[o];
}

// ---- register-resident, temporally blocked Jacobi (one wave = one grid row, VEC = W/64 cells per lane) -------------
// A workgroup of 16 waves holds a band of TR = 16*RPW full rows of p and div in registers and runs `iters` sweeps
// without touching HBM: horizontal neighbours come from the adjacent lanes (DPP wave shifts), vertical neighbours
// across waves through a double-buffered LDS edge exchange (one barrier per sweep).  Each band carries `halo`
// redundant rows on every non-physical side, so `iters` <= that many sweeps are exact on the rows it owns
// (the garbage front moves one row per sweep).  Per cell the arithmetic is exactly k_jacobi_sweep's.
// bound_ctrl zero-fills the lane without a source (lane 0 / lane 63: grid-edge cells, whose neighbour value is never used), so no
// copy of `x` into the destination is needed before the DPP move: one instruction per shift instead of two.
__device__ __forceinline__ float wave_shr1(float x) {   // lane i <- lane i-1 (lane 0: 0, unused)
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_shl1(float x) {   // lane i <- lane i+1 (lane 63: 0, unused)
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x130, 0xf, 0xf, true));
}
// One step of the sweep's priority staircase (jb_prio_stairs, jacobi_plan.h): nothing at all in an instantiation without it.  The
// scheduling barriers keep the compiler from moving the change off the stage boundary it marks.
template <bool ON, int LEVEL>
__device__ __forceinline__ void wave_prio() {
    if constexpr (ON) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(LEVEL);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int VEC> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<2> { using type = float2; };
template <> struct VecT<4> { using type = float4; };
template <> struct VecT<8> { using type = float4; };
// VEC consecutive floats of a lane as vector loads / stores of jb_access_bytes(VEC) bytes.  A lane's cells start at a multiple of VEC; that the
// rows do at a multiple of those bytes is what jb_tail_aligned / jb_fold_aligned (jacobi_plan.h) hold a band plan to before it is launched
template <int VEC>
__device__ __forceinline__ void ldv(float (&dst)[VEC], const float *src) {
    using V = typename VecT<VEC>::type;
    constexpr int N = sizeof(V) / 4;
#pragma unroll
    for (int q = 0; q < VEC / N; ++q) {
        const V t = reinterpret_cast<const V *>(src)[q];
        const float *f = reinterpret_cast<const float *>(&t);
#pragma unroll
        for (int c = 0; c < N; ++c) dst[q * N + c] = f[c];
    }
}
template <int VEC>
__device__ __forceinline__ void stv(float *dst, const float (&src)[VEC]) {
    using V = typename VecT<VEC>::type;
    constexpr int N = sizeof(V) / 4;
#pragma unroll
    for (int q = 0; q < VEC / N; ++q) {
        V t;
        float *f = reinterpret_cast<float *>(&t);
#pragma unroll
        for (int c = 0; c < N; ++c) f[c] = src[q * N + c];
        reinterpret_cast<V *>(dst)[q] = t;
    }
}

// MODE bit 0 (FIRST launch of a projection): the divergence of (u, v) is computed here for all tile rows (navier_stokes.py:136,
//   same expression tree as k_divergence) and stored for the owned rows so that later launches can read it;
// MODE bit 1 (LAST launch): after the final sweep the gradient subtraction (navier_stokes.py:148-149, as k_grad_subtract)
//   is applied to the owned rows of u and v from the p held in registers (needs iters <= halo - 1: the row above the
//   owned range must still be exact).
// PERSIST (with MODE 3): the whole projection in ONE launch.  p and div stay in registers for all `iters` sweeps; after each chunk of
//   at most `halo` sweeps a band hands the `halo` owned rows next to each inner boundary to its neighbour band through HBM (exchange
//   buffers x0 / x1 alternate, so a band never overwrites rows its neighbour may still be reading) and refreshes its own halo rows
//   from the neighbours'.  Hand-off as MI355X_MICROARCH.md "inter-workgroup visibility" prescribes for one workgroup per CU: every
//   payload store and load is a 16-byte `sc1` access, every storing wave drains its stores (s_waitcnt vmcnt(0)) before the workgroup
//   barrier, one lane then stores the band's flag `sc1`, the consumer's lane 0 polls the two neighbour flags with `sc1` loads and joins
//   a workgroup barrier before any wave loads.  Every spin is bounded (JacobiSync::timeout_ticks of the 100 MHz wall clock): a band
//   whose neighbour never arrives sets *status and the abort word and runs on, so the grid always drains; the host reports it on the
//   next call.  All bands x grids of one launch must be co-resident (the launcher sizes the grid to the CU count).
struct JacobiSync {
    unsigned *flags;          // [B * nb + 1]: per band the number of hand-offs it has published (monotonic over the handle's life); last = abort;
                              // behind the abort word, per (grid, band): 1 when the launch's sweeps took the fused cell (stencil.h), 0 the exact one
    unsigned *status;         // host-visible word, set non-zero when a wait timed out
    float *x0, *x1;           // exchange buffers, laid out like p (div and p2 of the handle)
    unsigned base;            // flag value before this projection's first hand-off
    int chunks, nb, grid0, ngrids, abort_slot, fault;
    long long timeout_ticks;
    // FOLD: this step's buoyancy + diffusion stage runs as the launch's prologue: (u_in, v_in, d_in) -> the kernel's u, v (= u2, v2) and d_out
    const float *u_in, *v_in, *d_in;
    float *d_out;
};

template <int VEC>
__device__ __forceinline__ void ldv_sc1(float (&dst)[VEC], __amdgpu_buffer_rsrc_t rs, unsigned byte_off) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    if constexpr (VEC >= 4) {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
            const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off + 16 * q, 0, 16);
#pragma unroll
            for (int c = 0; c < 4; ++c) dst[4 * q + c] = __uint_as_float(t[c]);
        }
    } else if constexpr (VEC == 2) {
        const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rs, byte_off, 0, 16);
        dst[0] = __uint_as_float(t[0]);
        dst[1] = __uint_as_float(t[1]);
    } else {
        dst[0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, byte_off, 0, 16));
    }
}
template <int VEC>
__device__ __forceinline__ void stv_sc1(__amdgpu_buffer_rsrc_t rs, unsigned byte_off, const float (&src)[VEC]) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    if constexpr (VEC >= 4) {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
            u32x4 t;
#pragma unroll
            for (int c = 0; c < 4; ++c) t[c] = __float_as_uint(src[4 * q + c]);
            __builtin_amdgcn_raw_buffer_store_b128(t, rs, byte_off + 16 * q, 0, 16);
        }
    } else if constexpr (VEC == 2) {
        u32x2 t;
        t[0] = __float_as_uint(src[0]);
        t[1] = __float_as_uint(src[1]);
        __builtin_amdgcn_raw_buffer_store_b64(t, rs, byte_off, 0, 16);
    } else {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(src[0]), rs, byte_off, 0, 16);
    }
}

template <int VEC, int RPW, int MODE, bool PERSIST = false, bool FOLD = false>
__global__ __launch_bounds__(JB_NW * 64) void k_jacobi_band(Geom g, const float *__restrict__ p_in,
                                                            float *__restrict__ p_out, float *__restrict__ div,
                                                            float *__restrict__ u, float *__restrict__ v,
                                                            int iters, int BR, JacobiSync sy) {
    constexpr int TR = JB_NW * RPW, ROWF = 64 * VEC;
    __shared__ float edge[2][JB_NW][2][ROWF];
    __shared__ int handoff_failed;                            // PERSIST: lane 0 saw a timed-out / aborted hand-off wait -> poison the band's results
    __shared__ int guard_failed[JB_NW];                       // per wave: some divergence value of it fails jacobi_cell_guard
    constexpr bool KEEP = PERSIST && FOLD && jb_keep_rows(VEC, RPW) > 0;
    constexpr int KROWS = KEEP ? jb_keep_rows(VEC, RPW) : 1;
    __shared__ __attribute__((aligned(16))) float keep[KROWS][ROWF];      // KEEP: u2 / v2 rows between prologue and epilogue (slot: keep_of)
    static_assert(sizeof(edge) + sizeof(keep) + sizeof(guard_failed) + 16 <= JB_LDS_BYTES, "edge + keep + the flag word exceed the CU's LDS");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int band_, grid_, nb_;
    if constexpr (PERSIST) {
        // 1-D launch.  Blocks i and i + 8 share an XCD (round-robin dispatch: observed, not promised -- only the hand-off's speed depends
        // on it): when the grids divide by 8, the bands of one grid take consecutive slots of one XCD.
        nb_ = sy.nb;
        const int id = blockIdx.x;
        if ((sy.ngrids & 7) == 0) {
            const int xcd = id & 7, slot = id >> 3;
            grid_ = (slot / nb_) * 8 + xcd;
            band_ = slot % nb_;
        } else {
            grid_ = id / nb_;
            band_ = id % nb_;
        }
        grid_ += sy.grid0;
    } else {
        band_ = blockIdx.x; grid_ = blockIdx.y; nb_ = gridDim.x;
    }
    const int band = band_, b = grid_, nb = nb_, halo = BR;
    // The rows this band owns and its tile's first row: the lines of jb_band_rows (jacobi_plan.h), which the host side calls.  Here they
    // stay as text: behind the call the same arithmetic is scheduled differently in every instantiation.
    const int e_rows = TR - halo, m_rows = TR - 2 * halo;
    const int own0 = band == 0 ? 0 : e_rows + (band - 1) * m_rows;
    int own1 = band == nb - 1 ? g.H : e_rows + band * m_rows;
    own1 = own1 < g.H ? own1 : g.H;
    int r0 = band == 0 ? 0 : (band == nb - 1 ? g.H - TR : own0 - halo);
    if (r0 > g.H - TR) r0 = g.H - TR;
    if (r0 < 0) r0 = 0;
    const int row0 = r0 + wave * RPW, j0 = lane * VEC;
    const size_t base = b * g.sc + (size_t)row0 * g.pc + j0;
    float pv[RPW][VEC], dv[RPW][VEC];
    const bool first_col = lane == 0, last_col = lane == 63;
    // KEEP: slot of the owned u (field 1) / v (field 0) row gi, -1 when the row takes the HBM path.  Wave-uniform; only the wave that
    // wrote a slot reads it, so no barrier orders the two.
    const int u_first = own0 > 1 ? own0 : 1;
    const int keep_scale = jb_keep_scale((own1 - u_first) + (own1 - own0), KROWS);      // (jb_keep_rows_numbered)
    auto keep_of = [&](int gi, int field) {
        const int first = field ? u_first : own0;
        const int s = (gi >= first && gi < own1) ? jb_keep_slot(2 * (gi - first) + field, keep_scale) : -1;
        return __builtin_amdgcn_readfirstlane(s);
    };
    if constexpr (FOLD) {
        // ---- buoyancy + the three diffusions (navier_stokes.py:154-160; per cell the expression trees of k_buoy_diffuse4) for the
        // tile's rows, each wave for itself from the step's input state: u2 rows row0 .. row0+RPW, v2 / d2 rows row0 .. row0+RPW-1.
        // Halo rows are computed redundantly by the neighbour bands (no band reads another band's u2 / v2); owned rows are stored
        // (the advection reads them) and the divergence is formed from the registers.  Rows roll through a 3-row window.
        const float *ui = sy.u_in + b * g.su, *vi = sy.v_in + b * g.sv, *di = sy.d_in + b * g.sc;
        float *uo = u + b * g.su, *vo = v + b * g.sv, *dout = sy.d_out + b * g.sc;
        const int H = g.H, W = g.W;
        auto rowu = [&](int i, float (&x)[VEC]) {
            i = i < 0 ? 0 : (i > H ? H : i);
            ldv<VEC>(x, ui + (size_t)i * g.pc + j0);
        };
        auto rowdv = [&](int i, float (&dx)[VEC], float (&vx)[VEC], float &vW) {       // d row; v row with this step's buoyancy; raw v(i, W)
            i = i < 0 ? 0 : (i > H - 1 ? H - 1 : i);
            ldv<VEC>(dx, di + (size_t)i * g.pc + j0);
            ldv<VEC>(vx, vi + (size_t)i * g.pv + j0);
            vW = vi[(size_t)i * g.pv + W];
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                const float bb = dx[c] * 0.1f;
                vx[c] = vx[c] + g.dt * bb;
            }
        };
        auto lap = [&](const float (&cc)[VEC], const float (&up)[VEC], const float (&dn)[VEC], float left, float right, float coef,
                       float (&o)[VEC]) {
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                float l = up[c] + dn[c];
                l = l + (c > 0 ? cc[c - 1] : left);
                l = l + (c < VEC - 1 ? cc[c + 1] : right);
                l = l - 4.0f * cc[c];
                o[c] = cc[c] + coef * l;
            }
        };
        float um[VEC], uc[VEC], un[VEC], dm[VEC], dc[VEC], dn[VEC], vm[VEC], vc[VEC], vn[VEC], vWm, vWc, vWn;
        rowu(row0 - 1, um);
        rowu(row0, uc);
        rowdv(row0 - 1, dm, vm, vWm);
        rowdv(row0, dc, vc, vWc);
        float u2prev[VEC], v2keep[VEC + 1];
#pragma unroll
        for (int k = 0; k <= RPW; ++k) {
            const int gi = row0 + k;
            rowu(gi + 1, un);
            float u2[VEC];
            {
                const float sl = wave_shr1(uc[VEC - 1]), sr = wave_shl1(uc[0]);
                lap(uc, um, un, first_col ? uc[0] : sl, last_col ? uc[VEC - 1] : sr, g.coef_uv, u2);
            }
            // (rows 0 and H of u are final as they are: always to HBM.  The row after the wave's last, k = RPW, is the next wave's first:
            // with KEEP that wave alone puts it away, so a slot has one writer, which is also its reader)
            const bool mine = !KEEP || k < RPW;
            const int ku = KEEP && k < RPW ? keep_of(gi, 1) : -1;
            if (ku >= 0) stv<VEC>(&keep[ku][j0], u2);
            else if ((mine && gi >= own0 && gi < own1) || (gi == H && band == nb - 1)) stv<VEC>(uo + (size_t)gi * g.pc + j0, u2);
            if (k > 0) {
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    float a = u2[c] - u2prev[c];
                    a = a + v2keep[c + 1];
                    a = a - v2keep[c];
                    dv[k - 1][c] = __fdiv_rn(a, g.dt);
                }
            }
#pragma unroll
            for (int c = 0; c < VEC; ++c) { u2prev[c] = u2[c]; um[c] = uc[c]; uc[c] = un[c]; }
            if (k < RPW) {
                rowdv(gi + 1, dn, vn, vWn);
                float d2[VEC], v2[VEC];
                {
                    const float sl = wave_shr1(dc[VEC - 1]), sr = wave_shl1(dc[0]);
                    lap(dc, dm, dn, first_col ? dc[0] : sl, last_col ? dc[VEC - 1] : sr, g.coef_d, d2);
                }
                {
                    const float sl = wave_shr1(vc[VEC - 1]), sr = wave_shl1(vc[0]);
                    lap(vc, vm, vn, first_col ? vc[0] : sl, last_col ? vWc : sr, g.coef_uv, v2);
                }
                // the field's last column j = W (no buoyancy; right neighbour = itself): meaningful in the last lane only
                float lw = vWm + vWn;
                lw = lw + vc[VEC - 1];
                lw = lw + vWc;
                lw = lw - 4.0f * vWc;
                const float v2W = vWc + g.coef_uv * lw;
                if (gi >= own0 && gi < own1) {
                    stv<VEC>(dout + (size_t)gi * g.pc + j0, d2);
                    const int kv = KEEP ? keep_of(gi, 0) : -1;
                    if (kv >= 0) stv<VEC>(&keep[kv][j0], v2);
                    else stv<VEC>(vo + (size_t)gi * g.pv + j0, v2);
                    if (last_col) vo[(size_t)gi * g.pv + W] = v2W;     // (column W is final as it is)
                }
                const float nx = wave_shl1(v2[0]);
#pragma unroll
                for (int c = 0; c < VEC; ++c) v2keep[c] = v2[c];
                v2keep[VEC] = last_col ? v2W : nx;
#pragma unroll
                for (int c = 0; c < VEC; ++c) { dm[c] = dc[c]; dc[c] = dn[c]; vm[c] = vc[c]; vc[c] = vn[c]; }
                vWm = vWc; vWc = vWn;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) pv[k][c] = p_in[base + (size_t)k * g.pc + c];
    if constexpr (FOLD) {
        // (divergence already in dv)
    } else if (MODE & 1) {
        const float *ub = u + b * g.su + (size_t)row0 * g.pc + j0, *vb = v + b * g.sv + (size_t)row0 * g.pv + j0;
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            float vr[VEC + 1];
#pragma unroll
            for (int c = 0; c <= VEC; ++c) vr[c] = vb[(size_t)k * g.pv + c];
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                float a = ub[(size_t)(k + 1) * g.pc + c] - ub[(size_t)k * g.pc + c];
                a = a + vr[c + 1];
                a = a - vr[c];
                dv[k][c] = __fdiv_rn(a, g.dt);
            }
            const int gi = row0 + k;
            if (!PERSIST && gi >= own0 && gi < own1) {        // (a persistent launch keeps div in registers to the end)
#pragma unroll
                for (int c = 0; c < VEC; ++c) div[base + (size_t)k * g.pc + c] = dv[k][c];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < RPW; ++k)
#pragma unroll
            for (int c = 0; c < VEC; ++c) dv[k][c] = div[base + (size_t)k * g.pc + c];
    }
    // ring rows (grid row 0 / H-1) exist only in the first wave of the first band and the last wave of the last band
    const int ring_k = __builtin_amdgcn_readfirstlane(row0 == 0 ? 0 : (row0 + RPW == g.H ? RPW - 1 : -1));   // wave-uniform
    static_assert(RPW >= 2, "the sweep keeps a wave's first and last row apart");
    // Which cell the sweeps of this launch take (stencil.h): the divergence is the same in all of them, so where every value of the
    // workgroup passes jacobi_cell_guard, dv becomes -0.25 * div once and a cell is three adds and one fma -- the same words as the exact
    // cell's five operations.  One verdict per workgroup (the waves meet at the sweeps' barriers and must run the same code); the bands
    // of a grid may differ.  Nothing reads dv after the sweeps.
    constexpr bool CAN_FUSE = jb_two_forms(VEC, RPW, PERSIST, FOLD);
    bool fused = false;
    if constexpr (CAN_FUSE) {
        bool lane_bad = false;
#pragma unroll
        for (int k = 0; k < RPW; ++k)
#pragma unroll
            for (int c = 0; c < VEC; ++c) lane_bad |= !jacobi_cell_guard(dv[k][c]);
        const bool wave_bad = __builtin_amdgcn_ballot_w64(lane_bad) != 0ull;       // (all lanes active here: the vote covers the wave)
        if (lane == 0) guard_failed[wave] = wave_bad;
        __syncthreads();
        static_assert(JB_NW <= 64, "one lane per wave's word");
        fused = __builtin_amdgcn_ballot_w64(guard_failed[lane < JB_NW ? lane : 0] != 0) == 0ull;    // the same words in every wave
        if (threadIdx.x == 0) sy.flags[sy.abort_slot + 1 + b * nb + band] = fused ? 1u : 0u;      // (a plain store: tests and tools read it)
        auto rest = [&](auto form) {                          // once per cell form, behind one scalar branch
            constexpr bool FUSED = decltype(form)::value;
#include "jacobi_band_tail.h"
        };
        if (fused) rest(std::true_type{});
        else rest(std::false_type{});
    } else {
        constexpr bool FUSED = false;
#include "jacobi_band_tail.h"
    }
}

// Switches of the projection, read ONCE per process (never on the per-step path):
//   SMK_JACOBI_PERSIST=0   one launch per chunk of sweeps instead of the single persistent launch
//   SMK_JACOBI_FAULT=1     (test only) one band never publishes its hand-off: exercises the bounded wait and the error report
struct StencilKnobs {
    bool persist, fault;
    StencilKnobs() {
        auto flag = [](const char *n, bool dflt) { const char *v = getenv(n); return v ? v[0] == '1' : dflt; };
        persist = flag("SMK_JACOBI_PERSIST", true);
        fault = flag("SMK_JACOBI_FAULT", false);
    }
};
static const StencilKnobs &knobs() {
    static const StencilKnobs k;
    return k;
}

// A plan's (vec, rpw) as compile-time constants: f(VEC, RPW), two std::integral_constant, for every pair that has a kernel -- 6 and 8
// rows per wave only up to 4 cells per lane (the register budget of jb_search_bands).
template <class F>
static void with_band_shape(const ProjectionPlan &pp, F &&f) {
    auto call = [&](auto vec, auto rpw) {
        if constexpr (decltype(rpw)::value <= 4 || decltype(vec)::value <= 4) f(vec, rpw);
    };
    auto with_rpw = [&](auto vec) {
        switch (pp.rpw) {
            case 2: call(vec, std::integral_constant<int, 2>{}); break;
            case 3: call(vec, std::integral_constant<int, 3>{}); break;
            case 4: call(vec, std::integral_constant<int, 4>{}); break;
            case 6: call(vec, std::integral_constant<int, 6>{}); break;
            case 8: call(vec, std::integral_constant<int, 8>{}); break;
        }
    };
    switch (pp.vec) {
        case 1: with_rpw(std::integral_constant<int, 1>{}); break;
        case 2: with_rpw(std::integral_constant<int, 2>{}); break;
        case 4: with_rpw(std::integral_constant<int, 4>{}); break;
        case 8: with_rpw(std::integral_constant<int, 8>{}); break;
    }
}

// The multi-launch form: pp.parts launches of k_jacobi_band, each a run of sweeps, ping-pong between p and p2; returns the one that holds
// the result (p after an even number).  With u and v the divergence is computed inside the first launch and the gradient subtraction
// inside the last (MODE 1, 2).
static float *launch_band_runs(const Geom &g, const ProjectionPlan &pp, float *p, float *p2, float *div, float *u, float *v, int iters,
                             hipStream_t st) {
    dim3 grid(pp.nb, g.B), block(JB_NW * 64);
    const JacobiSync none{};
    float *cur = p, *nxt = p2;
    int done = 0;
    for (int c = 0; c < pp.parts; ++c) {
        const int n = jb_run_sweeps(iters, done, pp.parts, c), mode = !u ? 0 : (c == 0 ? 1 : (c == pp.parts - 1 ? 2 : 0));
        with_band_shape(pp, [&](auto vec, auto rpw) {
            constexpr int VEC = decltype(vec)::value, RPW = decltype(rpw)::value;
            auto go = [&](auto m) {
                hipLaunchKernelGGL((k_jacobi_band<VEC, RPW, decltype(m)::value>), grid, block, 0, st, g, cur, nxt, div, u, v, n, pp.halo, none);
            };
            if (mode == 0) go(std::integral_constant<int, 0>{});
            else if (mode == 1) go(std::integral_constant<int, 1>{});
            else go(std::integral_constant<int, 2>{});
        });
        done += n;
        float *t = cur; cur = nxt; nxt = t;
    }
    return cur;
}

// the whole projection (fold: with the step's buoyancy + diffusion stage as its prologue) as one persistent launch per group of
// co-resident grids
static void launch_persist(const Geom &g, const ProjectionPlan &pp, bool fold, float *p, float *u, float *v, int iters, const JacobiSync &sy,
                           hipStream_t st) {
    dim3 grid(pp.nb * sy.ngrids), block(JB_NW * 64);
    with_band_shape(pp, [&](auto vec, auto rpw) {
        constexpr int VEC = decltype(vec)::value, RPW = decltype(rpw)::value;
        auto go = [&](auto f) {
            constexpr bool FOLD = decltype(f)::value && VEC <= 4;     // (8 cells per lane: the prologue's row windows do not fit, no plan folds)
            hipLaunchKernelGGL((k_jacobi_band<VEC, RPW, 3, true, FOLD>), grid, block, 0, st, g, p, p, nullptr, u, v, iters, pp.halo, sy);
        };
        if (fold) go(std::true_type{});
        else go(std::false_type{});
    });
}

// `iters` Jacobi sweeps on a given divergence field (result in p; p2 scratch).
hipError_t launch_jacobi(const Geom &g, float *p, float *p2, const float *div, int iters, hipStream_t st) {
    if (iters <= 0) return hipSuccess;
    dim3 grid(cdiv(g.W, TX), cdiv(g.H, TY), g.B), block(TX, TY);
    const ProjectionPlan pp = plan_projection_on(plan_geom(g), plan_layout(g, nullptr, nullptr, nullptr), iters, 0, false, false);    // (never persistent: the CU count is not read)
    float *cur = p, *nxt = p2;
    if (pp.form == ProjectionForm::bands) {
        cur = launch_band_runs(g, pp, p, p2, const_cast<float *>(div), nullptr, nullptr, iters, st);
    } else {
        for (int it = 0; it < iters; ++it) {
            hipLaunchKernelGGL(k_jacobi_sweep, grid, block, 0, st, g, cur, nxt, div);
            float *t = cur; cur = nxt; nxt = t;
        }
    }
    if (cur != p) hipLaunchKernelGGL(k_copy_cells, grid, block, 0, st, g, cur, p);
    return hipGetLastError();
}

hipError_t project_sync_create(ProjectSync &ps, int B) {
    ps.flags_len = B * 64 + 1;
    // (behind the flags: one cell-form word per (grid, band) of a persistent plan, which has at most 64 bands)
    hipError_t e = hipMalloc((void **)&ps.flags, (ps.flags_len + B * 64) * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(ps.flags, 0, (ps.flags_len + B * 64) * sizeof(unsigned));
    ps.forms = ps.flags ? ps.flags + ps.flags_len : nullptr;
    if (e == hipSuccess) e = hipHostMalloc((void **)&ps.status, sizeof(unsigned), hipHostMallocMapped);
    if (e == hipSuccess) *ps.status = 0u;
    return e;
}
void project_sync_destroy(ProjectSync &ps) {
    if (ps.flags) (void)hipFree(ps.flags);
    if (ps.status) (void)hipHostFree((void *)ps.status);
    ps.forms = nullptr;
    ps.flags = nullptr;
    ps.status = nullptr;
}

// What of the run-time state the persistent form needs: a handle with hand-off flags that has seen no time-out, and the switch.
static bool handle_allows_persist(const ProjectSync *ps) { return ps && ps->flags && !ps->disabled && knobs().persist; }

// The plan of a projection enqueued on `st` now.  A captured launch would replay with the hand-off count of capture time: under stream
// capture the multi-launch form is recorded.  So it is while a time-out of an earlier launch waits to be reported.
static ProjectionPlan plan_call(const Geom &g, const PlanLayout &lay, int iters, hipStream_t st, const ProjectSync *ps) {
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cap_status) == hipSuccess && cap_status != hipStreamCaptureStatusNone;
    const bool pending_error = ps && ps->status && *ps->status != 0u;
    return plan_projection_on(plan_geom(g), lay, iters, device_num_cu(), handle_allows_persist(ps) && !capturing && !pending_error, true);
}

// Two persistent projections cannot share the device: each needs all of its workgroups resident at once, and two half-resident grids
// would wait for each other until their spins run out.  Launches from ONE stream are ordered anyway; when a launch comes on a different
// stream than the previous one (of this process, on this device), the new stream is made to wait for everything submitted to the previous
// one (an event recorded there now) -- no host stall, and nothing at all in the single-stream case.  Other PROCESSES on the device are
// beyond this: see the bounded waits.
static std::unique_lock<std::mutex> order_persistent_launch(hipStream_t st) {
    struct Last { hipStream_t stream = nullptr; hipEvent_t ev = nullptr; bool any = false; };
    static std::mutex mu;
    static std::map<int, Last> last;
    int dev = 0;
    (void)hipGetDevice(&dev);
    // The caller keeps the lock until its persistent kernels are enqueued: a second host thread must not record its event on this
    // stream before the launch it is meant to wait for has been submitted.
    std::unique_lock<std::mutex> lk(mu);
    Last &l = last[dev];
    if (l.any && l.stream != st) {
        if (!l.ev) (void)hipEventCreateWithFlags(&l.ev, hipEventDisableTiming);
        if (l.ev && hipEventRecord(l.ev, l.stream) == hipSuccess) (void)hipStreamWaitEvent(st, l.ev, 0);
        else (void)hipGetLastError();                         // (the previous stream may have been destroyed: nothing of it is left to wait for)
    }
    l.stream = st;
    l.any = true;
    return lk;
}

// A bounded wait of an earlier persistent launch of this handle ran out (the kernel set the host-visible word and turned the band's results
// into NaN).  Acknowledge it: the word is cleared, the handle uses the multi-launch form from here on, and the caller reports the error
// exactly once.  The word is meaningful after the stream has been synchronised; read earlier it may simply not be set yet.
bool project_sync_take_timeout(ProjectSync &ps) {
    if (!ps.status || *ps.status == 0u) return false;
    *ps.status = 0u;
    ps.disabled = true;
    return true;
}

// The projection as the plan says.  fold_in / fold_d_out (persistent plans that fold only): the step's buoyancy + diffusion stage
// (fold_in -> u, v, fold_d_out) runs as the launch's prologue; otherwise u, v hold the diffused fields.
static hipError_t run_projection(const Geom &g, const ProjectionPlan &pp, float *u, float *v, float *p, float *p2, float *div, int iters,
                                 hipStream_t st, ProjectSync *ps, const StateView *fold_in = nullptr, float *fold_d_out = nullptr) {
    if (pp.form == ProjectionForm::persistent) {
        JacobiSync sy{};
        sy.flags = ps->flags; sy.status = const_cast<unsigned *>(ps->status); sy.x0 = div; sy.x1 = p2;
        sy.base = ps->seq; sy.chunks = pp.parts; sy.nb = pp.nb; sy.abort_slot = ps->flags_len - 1; sy.fault = knobs().fault ? 1 : 0;
        sy.timeout_ticks = knobs().fault ? 200000ll : 50000000ll;      // 100 MHz wall clock: 2 ms under fault injection, 0.5 s otherwise
        ps->forms_nb = pp.nb;
        ps->seq += (unsigned)pp.parts;
        const std::unique_lock<std::mutex> launch_order = order_persistent_launch(st);
        const bool fold = fold_in != nullptr;
        if (fold) { sy.u_in = fold_in->u; sy.v_in = fold_in->v; sy.d_in = fold_in->d; sy.d_out = fold_d_out; }
        ps->forms_two = fold && pp.two_forms;                 // (otherwise no workgroup writes its word: all exact)
        for (int g0 = 0; g0 < g.B; g0 += pp.grids_per_launch) {
            sy.grid0 = g0;
            sy.ngrids = g.B - g0 < pp.grids_per_launch ? g.B - g0 : pp.grids_per_launch;
            launch_persist(g, pp, fold, p, u, v, iters, sy, st);
        }
        return hipGetLastError();
    }
    // (forms_nb 0: no band kernel in this form; the multi-launch forms have the exact cell only: jb_two_forms)
    if (ps) { ps->forms_nb = pp.nb; ps->forms_two = false; }
    if (pp.form == ProjectionForm::sweeps) {
        hipError_t e = launch_divergence(g, u, v, div, g.pc, g.sc, st);
        if (e != hipSuccess) return e;
        e = launch_jacobi(g, p, p2, div, iters, st);
        if (e != hipSuccess) return e;
        return launch_grad_subtract(g, u, v, p, st);
    }
    launch_band_runs(g, pp, p, p2, div, u, v, iters, st);
    return hipGetLastError();                                 // (an even number of launches: the result is back in p)
}

// pressure_projection (navier_stokes.py:133-149) on (u, v, p): divergence, `iters` Jacobi sweeps, gradient subtraction.
// With a band plan the divergence is computed inside the first Jacobi launch and the gradient subtraction inside the last.
hipError_t launch_project(const Geom &g, float *u, float *v, float *p, float *p2, float *div, int iters, hipStream_t st, ProjectSync *ps) {
    // a wait inside an earlier persistent launch timed out (its workgroups were not co-resident within the limit): that projection's
    // result is invalid (NaN).  Say so once, loudly, and use the multi-launch form from here on.
    if (ps && project_sync_take_timeout(*ps)) return hipErrorLaunchTimeOut;
    return run_projection(g, plan_call(g, plan_layout(g, nullptr, u, v), iters, st, ps), u, v, p, p2, div, iters, st, ps);
}

// Stages 1-3 of a time step (navier_stokes.py:154-163): buoyancy + diffusion (in -> out.u, out.v, out.d) and the projection of
// (out.u, out.v) with the pressure p.  One persistent launch where the plan allows, otherwise the two stages as before.
hipError_t launch_buoy_project(const Geom &g, StateView in, StateView out, float *p, float *div, int iters, hipStream_t st, ProjectSync *ps) {
    const ProjectionPlan pp = plan_call(g, plan_layout(g, &in, out.u, out.v), iters, st, ps);
    const bool fold = pp.form == ProjectionForm::persistent && pp.folds;
    if (!fold) {
        const hipError_t e = launch_buoy_diffuse(g, in, out, st);
        if (e != hipSuccess) return e;
    }
    if (ps && project_sync_take_timeout(*ps)) return hipErrorLaunchTimeOut;       // (as launch_project reports it)
    return run_projection(g, pp, out.u, out.v, p, out.p, div, iters, st, ps, fold ? &in : nullptr, out.d);
}

// What one projection launches for this geometry, as a JSON object (describe_plan).
std::string describe_projection(const Geom &g, int iters, const ProjectSync *ps, const StateView *in, const StateView *out) {
    const PlanGeom pg = plan_geom(g);
    const PlanLayout lay = plan_layout(g, in, out ? out->u : nullptr, out ? out->v : nullptr);
    const ProjectionPlan pp = plan_projection_on(pg, lay, iters, device_num_cu(), handle_allows_persist(ps), true);
    std::string d = describe_plan(pp, iters, pg, device_num_cu());
    // (a member of its own, and only where it is true: describe_plan's text is recorded byte for byte, tests/host/projection_plans_parent.txt)
    if (pp.prio_stairs) d.insert(d.size() - 1, ", \"prio_stairs\": true");
    return d;
}

// The form a step's buoyancy + diffusion stage takes (in -> out) and the alignment facts its gate and the projection's were given, as
// members of the JSON object of smk_sim_describe.
std::string describe_step_forms(const Geom &g, int iters, const ProjectSync *ps, const StateView &in, const StateView &out) {
    const PlanLayout lay = plan_layout(g, &in, out.u, out.v);
    const ProjectionPlan pp = plan_projection_on(plan_geom(g), lay, iters, device_num_cu(), handle_allows_persist(ps), true);
    const bool fold = pp.form == ProjectionForm::persistent && pp.folds;
    const int in_align = lay.in_align, uv_align = lay.uv_align;
    const bool vec4 = buoy_diffuse_vec4(plan_geom(g), buoy_diffuse_layout(g, in, out));
    char buf[512];
    snprintf(buf, sizeof buf,
             "\"buoy_diffuse\": \"%s\", \"buoy_diffuse_stage\": \"%s\", \"alignment\": {\"state_in_bytes\": %d, \"projected_uv_bytes\": %d, "
             "\"pitch_c\": %d, \"pitch_v\": %d, \"stride_u\": %zu, \"stride_v\": %zu, \"stride_c\": %zu, \"band_row_access_bytes\": %d}",
             fold ? "folded into the projection" : (vec4 ? "vec4" : "scalar"), vec4 ? "vec4" : "scalar", in_align, uv_align, g.pc, g.pv, g.su,
             g.sv, g.sc, pp.form == ProjectionForm::sweeps ? 4 : jb_access_bytes(pp.vec));
    return buf;
}

__global__ void k_grad_subtract(Geom g, float *u, float *v, const float *p) {
    int b = blockIdx.z;
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    const float *pb = p + b * g.sc;
    if (i >= 1 && i < g.H && j < g.W) {
        float *c = u + b * g.su + (size_t)i * g.pc + j;
        float gr = pb[(size_t)i * g.pc + j] - pb[(size_t)(i - 1) * g.pc + j];
        *c = *c - g.dt * gr;
    }
    if (i < g.H && j >= 1 && j < g.W) {
        float *c = v + b * g.sv + (size_t)i * g.pv + j;
        float gr = pb[(size_t)i * g.pc + j] - pb[(size_t)i * g.pc + j - 1];
        *c = *c - g.dt * gr;
    }
}

hipError_t launch_grad_subtract(const Geom &g, float *u, float *v, const float *p, hipStream_t st) {
    dim3 grid(cdiv(g.W, TX), cdiv(g.H, TY), g.B), block(TX, TY);
    hipLaunchKernelGGL(k_grad_subtract, grid, block, 0, st, g, u, v, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------- advection (navier_stokes.py:74-131)
// bilinear_interpolate (:111-131): indices clamped before the weights are formed.
__device__ __forceinline__ float bilinear(const float *f, int h, int w, int pitch, float y, float x, int *ox0, int *oy0) {
    int x0 = (int)floorf(x), y0 = (int)floorf(y);
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = clampi(x0, 0, w - 1); x1 = clampi(x1, 0, w - 1);
    y0 = clampi(y0, 0, h - 1); y1 = clampi(y1, 0, h - 1);
    float fx0 = (float)x0, fx1 = (float)x1, fy0 = (float)y0, fy1 = (float)y1;
    float wa = (fx1 - x) * (fy1 - y);
    float wb = (x - fx0) * (fy1 - y);
    float wc = (fx1 - x) * (y - fy0);
    float wd = (x - fx0) * (y - fy0);
    float r = wa * f[(size_t)y0 * pitch + x0] + wb * f[(size_t)y0 * pitch + x1];
    r = r + wc * f[(size_t)y1 * pitch + x0];
    r = r + wd * f[(size_t)y1 * pitch + x1];
    if (ox0) { *ox0 = x0; *oy0 = y0; }
    return r;
}

template <int KIND>
__global__ void k_advect(Geom g, const float *field, float *out, const float *u, const float *v, float *frames,
                         int64_t fsb, const float *fractal, float fint, int32_t *x0o, int32_t *y0o) {
    constexpr bool IS_U = KIND == 0, IS_V = KIND == 1;   // KIND 2: density (+decay, frame emit); 3: plain cell field
    const int R = IS_U ? g.H + 1 : g.H, C = IS_V ? g.W + 1 : g.W;
    const int pitch = IS_V ? g.pv : g.pc;
    const size_t fs = IS_U ? g.su : (IS_V ? g.sv : g.sc);
    int b = blockIdx.z;
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= R || j >= C) return;
    const float *ub = u + b * g.su, *vb = v + b * g.sv, *fb = field + b * fs;
    float Y = (float)i, X = (float)j;
    float xu = clampf(X + 0.5f, 0.f, (float)(g.W - 1));           // interpolate_velocity_u (:97-102)
    float ui = bilinear(ub, g.H + 1, g.W, g.pc, Y, xu, nullptr, nullptr);
    float yv = clampf(Y + 0.5f, 0.f, (float)(g.H - 1));           // interpolate_velocity_v (:104-109)
    float vi = bilinear(vb, g.H, g.W + 1, g.pv, yv, X, nullptr, nullptr);
    float px = clampf(X - g.dt * ui, 0.f, (float)(C - 1));        // :87-92
    float py = clampf(Y - g.dt * vi, 0.f, (float)(R - 1));
    int x0, y0;
    float r = bilinear(fb, R, C, pitch, py, px, &x0, &y0);
    if (x0o) {
        size_t o = ((size_t)b * R + i) * C + j;
        x0o[o] = x0; y0o[o] = y0;
    }
    if (KIND == 2) {
        r = r * 0.995f;                                           // :171
        if (frames) {
            float fr = r;
            if (fractal) {                                        // fractal_generator.py:62 (F is [W][H], square)
                float t = fint * fractal[(size_t)i * g.W + j];
                t = t * r;
                fr = r + t;
            }
            frames[(size_t)b * fsb + (size_t)i * g.W + j] = fr;
        }
    }
    if (out) out[b * fs + (size_t)i * pitch + j] = r;
}

hipError_t launch_advect(const Geom &g, int kind, const float *field, float *out, const float *u, const float *v,
                         float *frames, int64_t fsb, const float *fractal, float fint, int32_t *x0, int32_t *y0,
                         hipStream_t st) {
    dim3 block(TX, TY);
    if (kind == 0) {
        dim3 grid(cdiv(g.W, TX), cdiv(g.H + 1, TY), g.B);
        hipLaunchKernelGGL(k_advect<0>, grid, block, 0, st, g, field, out, u, v, frames, fsb, fractal, fint, x0, y0);
    } else if (kind == 1) {
        dim3 grid(cdiv(g.W + 1, TX), cdiv(g.H, TY), g.B);
        hipLaunchKernelGGL(k_advect<1>, grid, block, 0, st, g, field, out, u, v, frames, fsb, fractal, fint, x0, y0);
    } else if (kind == 3) {
        dim3 grid(cdiv(g.W, TX), cdiv(g.H, TY), g.B);
        hipLaunchKernelGGL(k_advect<3>, grid, block, 0, st, g, field, out, u, v, frames, fsb, fractal, fint, x0, y0);
    } else {
        dim3 grid(cdiv(g.W, TX), cdiv(g.H, TY), g.B);
        hipLaunchKernelGGL(k_advect<2>, grid, block, 0, st, g, field, out, u, v, frames, fsb, fractal, fint, x0, y0);
    }
    return hipGetLastError();
}

// ---- the three advections of a step as ONE launch (navier_stokes.py:166-171) --------------------------------------------------------
// u <- adv(u2; u2, v2), v <- adv(v2; u, v2), density <- adv(d2; u, v) * 0.995 are sequentially dependent, but only through the
// velocity SAMPLING, which happens at the integer cell coordinates (advection_step builds Y, X with meshgrid, :79-81), where
// interpolate_velocity_u / _v (:97-109) collapse exactly:
//   u at (Y = i, x + 0.5): y0 = i with weight (y1 - i) in {1, 0}, x-weights 0.5 / 0.5  ->  ui = 0.5*U[i][j] + 0.5*U[i][j+1]   (i <= H-1, j <= W-2)
//   v at (y + 0.5, X = j): x0 = j with weight (x1 - j) in {1, 0}, y-weights 0.5 / 0.5  ->  vi = 0.5*V[i][j] + 0.5*V[i+1][j]   (i <= H-2, j <= W-1)
//   and 0 otherwise (both clamped indices coincide: the zero-at-the-upper-edge quirk).  The dropped terms are products with an exact
//   zero weight: for finite fields they are +-0 and change at most the sign of a zero, which X - dt*ui cannot see (X >= 0).

// One advected value in the general form, every tap from GLOBAL memory: what a wave falls back to when a back-trace of its units leaves the
// 2 x 2 LDS neighbourhood (never in the reference's regime).  A real call, so the hot code carries neither its registers nor its loads.
// Field [Rf][Cf] (pitch `pitch`); (y, x) = the cell; ui, vi = the velocity samples already formed by the caller.
__device__ __attribute__((noinline)) float far_value2(const float *f, int pitch, int Rf, int Cf, float dt, int y, int x, float ui, float vi) {
    const float px = clampf((float)x - dt * ui, 0.f, (float)(Cf - 1));
    const float py = clampf((float)y - dt * vi, 0.f, (float)(Rf - 1));
    const int x0 = (int)px, y0 = (int)py;
    int x1 = x0 + 1, y1 = y0 + 1;
    x1 = x1 > Cf - 1 ? Cf - 1 : x1;
    y1 = y1 > Rf - 1 ? Rf - 1 : y1;
    const float fx0 = (float)x0, fx1 = (float)x1, fy0 = (float)y0, fy1 = (float)y1;
    const float wa = (fx1 - px) * (fy1 - py);
    const float wb = (px - fx0) * (fy1 - py);
    const float wc = (fx1 - px) * (py - fy0);
    const float wd = (px - fx0) * (py - fy0);
    float r = wa * f[(size_t)y0 * pitch + x0] + wb * f[(size_t)y0 * pitch + x1];
    r = r + wc * f[(size_t)y1 * pitch + x0];
    r = r + wd * f[(size_t)y1 * pitch + x1];
    return r;
}


// Wave-autonomous rows (round 4, in place of round 2's LDS-tiled launch; the organisation of csrc/advect3d.hip's k3_advect_march, one plane).
// Workgroup = NW waves = a (NW R) x 64 tile; u2, v2, d2 windows (tile + 1 low, + 2 high; every out-of-grid element holds the CLAMPED in-grid
// value, which is exactly what bilinear()'s clamped indices read) staged once into LDS, ONE barrier.  A wave then owns R consecutive rows:
// thread = column, the advected u and v of its rows (+ the next row) live in REGISTERS -- x + 1 comes from the next lane by DPP, lane 63's
// from the extra-column unit by v_readlane -- so nothing separates the three fields (round 2's LDS-tiled form: two more barriers and two LDS
// round trips).  With |dt * velocity| < 1 cell a back-trace lands on floor(p) in {i-1, i}: four taps at immediate offsets from ONE LDS address;
// the test is one wave-level vote per batch of units, the fall-back the general form per lane (far_value2).  EDGE = false is the same
// arithmetic with the tests that cannot fail inside the grid removed (existence, the sampling rules' extents, the clamps: an unclamped
// back-trace that would have needed its clamp fails the neighbourhood test).  Bit-identical to the staged k_advect launches.
template <int R, int NW, int BU>
__global__ __launch_bounds__(NW * 64) void k_advect_rows(Geom g, StateView in, StateView out, float *frames, int64_t fsb,
                                                         const float *__restrict__ fractal, float fint) {
    constexpr int TYR = R * NW, TXC = 64, NT = NW * 64;
    constexpr int WR = TYR + 3, WC = TXC + 3, WP = 68, WPL = WR * WP;
    constexpr int NST = (WR * WC + NT - 1) / NT;
    __shared__ float U2s[WPL], V2s[WPL], D2s[WPL];
    const int H = g.H, W = g.W, pc = g.pc, pv = g.pv;
    const int ntx = (W + TXC - 1) / TXC, nty = (H + TYR - 1) / TYR;
    unsigned tile = xcd_contiguous(blockIdx.x, gridDim.x);
    const int tix = tile % ntx; tile /= ntx;
    const int tiy = tile % nty;
    const int b = tile / nty;
    const int x0 = tix * TXC, y0 = tiy * TYR;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *u2 = in.u + b * g.su, *v2 = in.v + b * g.sv, *d2 = in.d + b * g.sc;
    float *uo = out.u + b * g.su, *vo = out.v + b * g.sv, *dn = out.d + b * g.sc;
    float *fr = frames ? frames + (size_t)b * fsb : nullptr;
    const float dt = g.dt;

    // ---- stage the windows: every address clamped into its field (no load under a branch), all loads before the first LDS write
    {
        float ru[NST], rv[NST], rd[NST];
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            const int e0 = tid + it * NT, e = e0 < WR * WC ? e0 : WR * WC - 1;
            const int r = e / WC, c = e - r * WC;
            const int gy = y0 - 1 + r, gx = x0 - 1 + c;
            const int yc = clampi(gy, 0, H - 1), xc = clampi(gx, 0, W - 1);
            ru[it] = u2[(unsigned)(clampi(gy, 0, H) * pc + xc)];
            rv[it] = v2[(unsigned)(yc * pv + clampi(gx, 0, W))];
            rd[it] = d2[(unsigned)(yc * pc + xc)];
        }
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            const int e0 = tid + it * NT;
            const int r = e0 / WC, c = e0 - r * WC;
            if (e0 < WR * WC) { U2s[r * WP + c] = ru[it]; V2s[r * WP + c] = rv[it]; D2s[r * WP + c] = rd[it]; }
        }
    }
    __syncthreads();

    const int rb = wv * R, yb = y0 + rb;                                  // this wave's rows: yb .. yb+R-1 (+ row yb+R for Un, Vn)
    const int x = x0 + lane;
    const float fxl = (float)x;
    const int x4 = 4 * x;
    auto stb = [&](float *rowbase, float v) {     // one value of this lane's column into a row (uniform base): descriptor base = the row
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), __builtin_amdgcn_make_buffer_rsrc(rowbase, 0, 0x7fffffff, 0x00020000), x4, 0, 0);
    };
    const int wbase = (rb + 1) * WP + lane + 1;                           // window index of (row yb, column x); + r WP for row yb + r
    const int wex = (rb + 1 + (lane <= R ? lane : R)) * WP + TXC + 1;     // extra-column unit: lane = row, column x0 + TXC
    const float fxe = (float)(x0 + TXC);
    // is this wave's whole neighbourhood inside the grid?  (rows yb-1 .. yb+R+1 and columns x0-1 .. x0+TXC+1 exist in every field, the
    // sampling rules hold on all its units, and no coordinate below 2: (int)NaN = 0 must fail the neighbourhood test)
    const bool inner_w = yb >= 2 && yb + R + 1 <= H - 2 && x0 >= 2 && x0 + TXC + 1 <= W - 2;

    struct Prep { float wx0, wx1, wy0, wy1; int a; };
    // back-trace -> weights + the LDS address; returns "lands in the neighbourhood".  Field [Rf][Cf].
    auto prep = [&](auto edge, int Rf, int Cf, int widx, int y, int xx, float fx, float ui, float vi, bool exists, Prep &P) -> bool {
        constexpr bool EDGE = decltype(edge)::value;
        float px = fx - dt * ui, py = (float)y - dt * vi;
        if (EDGE) { px = clampf(px, 0.f, (float)(Cf - 1)); py = clampf(py, 0.f, (float)(Rf - 1)); }
        const float fx0 = floorf(px), fy0 = floorf(py);
        float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
        if (EDGE) { fx1 = fminf(fx1, (float)(Cf - 1)); fy1 = fminf(fy1, (float)(Rf - 1)); }
        P.wx0 = fx1 - px; P.wx1 = px - fx0; P.wy0 = fy1 - py; P.wy1 = py - fy0;
        int rx = (int)fx0 - xx, ry = (int)fy0 - y;
        bool fast = (unsigned)((rx + 1) | (ry + 1)) <= 1u;
        if (EDGE && !exists) { rx = 0; ry = 0; fast = true; }             // a lane without a cell reads its own (in-window) slot; result unused
        P.a = widx + ry * WP + rx;
        return fast;
    };
    auto finish = [&](const float *win, const Prep &P) -> float {
        const float t0 = win[P.a], t1 = win[P.a + 1], t2 = win[P.a + WP], t3 = win[P.a + WP + 1];
        float acc = (P.wx0 * P.wy0) * t0 + (P.wx1 * P.wy0) * t1;
        acc = acc + (P.wx0 * P.wy1) * t2;
        acc = acc + (P.wx1 * P.wy1) * t3;
        return acc;
    };

    float un[R + 1], unx[R + 1], vn[R + 1];
    auto body = [&](auto edge) {
        constexpr bool EDGE = decltype(edge)::value;
        float ui[BU], vi[BU], val[BU];
        Prep P[BU];
        bool ex[BU];
        // ---------------- Un: units 0 .. R = rows yb .. yb+R at column x; unit R+1 = the tile's extra column x0 + TXC (lane = row).  u is [H+1][W]
        float uex = 0.f;
#pragma unroll
        for (int b0 = 0; b0 <= R + 1; b0 += BU) {
            bool ok = true;
#pragma unroll
            for (int j = 0; j < BU; ++j) {
                const int r = b0 + j;
                if (r > R + 1) continue;
                const bool xt = r == R + 1;
                const int y = xt ? yb + lane : yb + r, xx = xt ? x0 + TXC : x, w0 = xt ? wex : wbase + r * WP;
                const float a = 0.5f * U2s[w0] + 0.5f * U2s[w0 + 1];
                const float c = 0.5f * V2s[w0] + 0.5f * V2s[w0 + WP];
                ex[j] = (!EDGE && !xt) || ((!xt || lane <= R) && y <= H && xx <= W - 1);
                ui[j] = ((!EDGE && !xt) || (y <= H - 1 && xx <= W - 2)) ? a : 0.f;
                vi[j] = ((!EDGE && !xt) || y <= H - 2) ? c : 0.f;
                if (xt) ok &= prep(std::true_type{}, H + 1, W, w0, y, xx, fxe, ui[j], vi[j], ex[j], P[j]);
                else ok &= prep(edge, H + 1, W, w0, y, xx, fxl, ui[j], vi[j], ex[j], P[j]);
            }
            if (__builtin_expect(__all(ok), 1)) {
#pragma unroll
                for (int j = 0; j < BU; ++j)
                    if (b0 + j <= R + 1) val[j] = finish(U2s, P[j]);
            } else {
#pragma unroll
                for (int j = 0; j < BU; ++j) {
                    const int r = b0 + j;
                    if (r > R + 1) continue;
                    const bool xt = r == R + 1;
                    val[j] = ex[j] ? far_value2(u2, pc, H + 1, W, dt, xt ? yb + lane : yb + r, xt ? x0 + TXC : x, ui[j], vi[j]) : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < BU; ++j) {
                const int r = b0 + j;
                if (r > R + 1) continue;
                if (r == R + 1) { uex = val[j]; continue; }
                un[r] = val[j];
                const int y = yb + r;
                if ((r < R || (EDGE && y == H)) && ex[j]) stb(uo + (size_t)y * pc, val[j]);
            }
        }
#pragma unroll
        for (int r = 0; r <= R; ++r)                                       // Un at x + 1: the next lane's, lane 63 takes the extra column's row r
            unx[r] = shl1_with(un[r], __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, uex), r)));
        // ---------------- Vn: rows 0 .. R.  v is [H][W+1] (x = W of a narrower last tile is one of these lanes)
#pragma unroll
        for (int b0 = 0; b0 <= R; b0 += BU) {
            bool ok = true;
#pragma unroll
            for (int j = 0; j < BU; ++j) {
                const int r = b0 + j;
                if (r > R) continue;
                const int y = yb + r, w0 = wbase + r * WP;
                const float a = 0.5f * un[r] + 0.5f * unx[r];
                const float c = 0.5f * V2s[w0] + 0.5f * V2s[w0 + WP];
                ex[j] = !EDGE || (y <= H - 1 && x <= W);
                ui[j] = (!EDGE || x <= W - 2) ? a : 0.f;
                vi[j] = (!EDGE || (y <= H - 2 && x <= W - 1)) ? c : 0.f;
                ok &= prep(edge, H, W + 1, w0, y, x, fxl, ui[j], vi[j], ex[j], P[j]);
            }
            if (__builtin_expect(__all(ok), 1)) {
#pragma unroll
                for (int j = 0; j < BU; ++j)
                    if (b0 + j <= R) val[j] = finish(V2s, P[j]);
            } else {
#pragma unroll
                for (int j = 0; j < BU; ++j)
                    if (b0 + j <= R) val[j] = ex[j] ? far_value2(v2, pv, H, W + 1, dt, yb + b0 + j, x, ui[j], vi[j]) : 0.f;
            }
#pragma unroll
            for (int j = 0; j < BU; ++j) {
                const int r = b0 + j;
                if (r > R) continue;
                vn[r] = val[j];
                if (r < R && ex[j]) stb(vo + (size_t)(yb + r) * pv, val[j]);
            }
        }
        if (EDGE && x0 + TXC == W) {                                       // the field's own extra column x = W (lane = row, rows 0 .. R-1)
            const int y = yb + lane;
            if (lane < R && y <= H - 1)                                    // (ui needs x <= W-2, vi x <= W-1: both zero)
                vo[(unsigned)(y * pv + W)] = far_value2(v2, pv, H, W + 1, dt, y, W, 0.f, 0.f);
        }
        // ---------------- density: rows 0 .. R-1 (+ decay, frame)
#pragma unroll
        for (int b0 = 0; b0 < R; b0 += BU) {
            bool ok = true;
#pragma unroll
            for (int j = 0; j < BU; ++j) {
                const int r = b0 + j;
                if (r >= R) continue;
                const int y = yb + r, w0 = wbase + r * WP;
                const float a = 0.5f * un[r] + 0.5f * unx[r];
                const float c = 0.5f * vn[r] + 0.5f * vn[r + 1];
                ex[j] = !EDGE || (y <= H - 1 && x <= W - 1);
                ui[j] = (!EDGE || x <= W - 2) ? a : 0.f;
                vi[j] = (!EDGE || y <= H - 2) ? c : 0.f;
                ok &= prep(edge, H, W, w0, y, x, fxl, ui[j], vi[j], ex[j], P[j]);
            }
            if (__builtin_expect(__all(ok), 1)) {
#pragma unroll
                for (int j = 0; j < BU; ++j)
                    if (b0 + j < R) val[j] = finish(D2s, P[j]);
            } else {
#pragma unroll
                for (int j = 0; j < BU; ++j)
                    if (b0 + j < R) val[j] = ex[j] ? far_value2(d2, pc, H, W, dt, yb + b0 + j, x, ui[j], vi[j]) : 0.f;
            }
#pragma unroll
            for (int j = 0; j < BU; ++j) {
                const int r = b0 + j;
                if (r >= R) continue;
                const int y = yb + r;
                if (!ex[j]) continue;
                const float v = val[j] * 0.995f;                              // :171
                if (fr) {
                    float f = v;
                    if (fractal) {                                            // fractal_generator.py:62 (F is [W][H], square)
                        float t = fint * fractal[(unsigned)(y * W + x)];
                        t = t * v;
                        f = v + t;
                    }
                    stb(fr + (size_t)y * W, f);
                }
                stb(dn + (size_t)y * pc, v);
            }
        }
    };
    if (inner_w) body(std::false_type{});
    else body(std::true_type{});
}

hipError_t launch_advect_fused(const Geom &g, StateView in, StateView out, float *frames, int64_t fsb, const float *fractal, float fint,
                               hipStream_t st) {
    // R x NW = 8 x 4 rows per workgroup (measured at configs[2] against 4 x 4, 4 x 8, 8 x 8, 16 x 2 rows and batches of 5 units: equal within
    // noise except 16 x 2, +7 %)
    constexpr int R = 8, NW = 4;
    const long long n = (long long)cdiv(g.W, 64) * cdiv(g.H, R * NW) * g.B;
    hipLaunchKernelGGL((k_advect_rows<R, NW, 3>), dim3((unsigned)n), dim3(NW * 64), 0, st, g, in, out, frames, fsb, fractal, fint);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the public interpolation helpers (navier_stokes.py:97-131)
// bilinear_interpolate / interpolate_velocity_u / interpolate_velocity_v as pure gathers on caller-given coordinates (any float:
// the reference floors to int64 and clamps, so coordinates far outside the field are legal).  floor() is saturated in float
// before the int conversion: every value below -2 / above dim + 1 clamps to the same indices as the int64 original.
__device__ __forceinline__ int floor_sat(float x, int dim) {
    float f = floorf(x);
    f = f < -2.0f ? -2.0f : f;
    f = f > (float)(dim + 1) ? (float)(dim + 1) : f;
    return (int)f;
}

// MODE 0: bilinear(field, y, x); 1: x <- clamp(x + 0.5, 0, w - 1) first (:97-102); 2: y <- clamp(y + 0.5, 0, h - 1) first (:104-109)
template <int MODE>
__global__ void k_interp(const float *field, int h, int w, int pitch, size_t fstride, const float *ys, const float *xs,
                         size_t cstride, size_t n, float *out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int b = blockIdx.y;
    const float *f = field + b * fstride;
    float y = ys[b * cstride + k], x = xs[b * cstride + k];
    if (MODE == 1) x = clampf(x + 0.5f, 0.f, (float)(w - 1));
    if (MODE == 2) y = clampf(y + 0.5f, 0.f, (float)(h - 1));
    int x0 = floor_sat(x, w), y0 = floor_sat(y, h);
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = clampi(x0, 0, w - 1); x1 = clampi(x1, 0, w - 1);
    y0 = clampi(y0, 0, h - 1); y1 = clampi(y1, 0, h - 1);
    const float fx0 = (float)x0, fx1 = (float)x1, fy0 = (float)y0, fy1 = (float)y1;
    const float wa = (fx1 - x) * (fy1 - y);
    const float wb = (x - fx0) * (fy1 - y);
    const float wc = (fx1 - x) * (y - fy0);
    const float wd = (x - fx0) * (y - fy0);
    float r = wa * f[(size_t)y0 * pitch + x0] + wb * f[(size_t)y0 * pitch + x1];
    r = r + wc * f[(size_t)y1 * pitch + x0];
    r = r + wd * f[(size_t)y1 * pitch + x1];
    out[(size_t)b * n + k] = r;
}

hipError_t launch_interp(int mode, const float *field, int B, int h, int w, int pitch, size_t fstride, const float *y,
                         const float *x, size_t cstride, size_t n, float *out, hipStream_t st) {
    dim3 grid((unsigned)((n + 255) / 256), B), block(256);
    if (mode == 0) hipLaunchKernelGGL(k_interp<0>, grid, block, 0, st, field, h, w, pitch, fstride, y, x, cstride, n, out);
    else if (mode == 1) hipLaunchKernelGGL(k_interp<1>, grid, block, 0, st, field, h, w, pitch, fstride, y, x, cstride, n, out);
    else hipLaunchKernelGGL(k_interp<2>, grid, block, 0, st, field, h, w, pitch, fstride, y, x, cstride, n, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- fractal constants (fractal_generator.py:12-51)
// torch.linspace fp32 CPU kernel: one rounding per element (FMA form), symmetric halves.
__device__ __forceinline__ float linspace_at(float start, float end, int steps, int i) {
    float step = __fdiv_rn(end - start, (float)(steps - 1));
    return i < steps / 2 ? __fmaf_rn(step, (float)i, start) : __fmaf_rn(-step, (float)(steps - i - 1), end);
}

// out index [i][j] over [W][H] with X = x[i], Y = y[j] (meshgrid 'ij' of (x,y)); N = H = W.
__global__ void k_fractal_constants(int N, float *perlin, float *mandel, float *field) {
    int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= N || j >= N) return;
    // perlin (:12-31): sum_{o<6} (amp*sin(f*x))*cos(f*y); (noise+1)/2
    float px = linspace_at(0.f, 10.f, N, i), py = linspace_at(0.f, 10.f, N, j);
    float noise = 0.f, amp = 1.f, freq = 1.f;
#pragma unroll
    for (int o = 0; o < 6; ++o) {
        float t = amp * sinf(freq * px);
        t = t * cosf(freq * py);
        noise = noise + t;
        amp *= 0.5f; freq *= 2.f;      // exact powers of two: same values as the python doubles
    }
    float per = __fdiv_rn(noise + 1.0f, 2.0f);
    // mandelbrot (:33-51): z <- z*z + c while |z| <= 2 (masked update == freeze after escape), count = last it
    float cr = linspace_at(-2.5f, 1.5f, N, i), ci = linspace_at(-1.5f, 1.5f, N, j);
    float zr = 0.f, zi = 0.f;
    int cnt = 0;
    for (int it = 0; it < 100; ++it) {
        float m = __fsqrt_rn(zr * zr + zi * zi);
        if (!(m <= 2.0f)) break;
        float rr = zr * zr - zi * zi;
        float ab = zr * zi;
        float ii = ab + ab;
        zr = rr + cr; zi = ii + ci;
        cnt = it;
    }
    float man = __fdiv_rn((float)cnt, 100.0f);
    size_t o = (size_t)i * N + j;
    perlin[o] = per;
    mandel[o] = man;
    field[o] = 0.7f * per + 0.3f * man;   // :58-59
}

hipError_t launch_fractal_constants(int N, float *perlin, float *mandel, float *field, hipStream_t st) {
    dim3 grid(cdiv(N, TX), cdiv(N, TY)), block(TX, TY);
    hipLaunchKernelGGL(k_fractal_constants, grid, block, 0, st, N, perlin, mandel, field);
    return hipGetLastError();
}

// field + (intensity*F)*field  (:62)
__global__ void k_apply_fractal(const float *in, float *out, const float *fractal, size_t per_field, size_t total, float fint) {
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t step = (size_t)gridDim.x * blockDim.x;
    for (; k < total; k += step) {
        float x = in[k];
        float t = fint * fractal[k % per_field];
        t = t * x;
        out[k] = x + t;
    }
}

hipError_t launch_apply_fractal(const float *in, float *out, const float *fractal, int n_fields, int N, float intensity,
                                hipStream_t st) {
    size_t per = (size_t)N * N, total = per * n_fields;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_apply_fractal, dim3(blocks), dim3(256), 0, st, in, out, fractal, per, total, intensity);
    return hipGetLastError();
}

}  // namespace smk
