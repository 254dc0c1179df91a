// Tangent-linear (forward-mode) derivative of one 2-D stable-fluids step (navier_stokes.py:151-173): the kernels behind smk_advect_tangent
// and smk_tangent_renorm.  DESIGN.md section 3.11.
//
// Buoyancy, the three diffusions, the divergence, the Jacobi sweeps and the gradient subtraction are linear and homogeneous in the state:
// their tangent is the stepper's own kernel applied to the tangent state.  Only the advection is non-linear, and its tangent is a gather at
// the forward's own taps -- there is nothing to transpose, so a back-trace may move any number of cells (no far case).
//
// Arithmetic rules (the project's gradient rules): fp32 throughout, every sum in one fixed order, no atomics, every output element written,
// results bit-identical from call to call and independent of T and of a grid's batch mates.  The back-trace positions, indices, clamp
// decisions and weights are formed by the forward's own expressions (csrc/fluid_trace.h, shared with csrc/fluid_grad.hip), so they are
// the forward's bit for bit.
#include "fluid_tangent.h"
#include "fluid_trace.h"

namespace smk {

namespace {

// ---------------------------------------------------------------- advection tangent
// out = adv(f; u, v) (times 0.995 for WHICH = 2).  One thread per destination cell (Y, X): it forms the forward's velocity samples, the
// back-trace, its clamp decisions, the four taps and weights and the slopes of the interpolant ONCE, keeps them in registers, and then
// loops over the T tangents of its grid:
//     r  = ((wa tf00 + wb tf01) + wc tf10) + wd tf11            the forward's gather of the tangent field
//     r  = r + sx * dpx,   dpx = -(dt * interp(tu)) where 0 <= X - dt ui <= C - 1 (bounds included), else 0
//     r  = r + sy * dpy,   dpy = -(dt * interp(tv)) likewise from Y - dt vi
//     sx = (fy1 - py)(f01 - f00) + (py - fy0)(f11 - f10),  sy = (fx1 - px)(f10 - f00) + (px - fx0)(f11 - f01)
// interp(tu), interp(tv): the forward's velocity samples of the tangent velocities, at the fixed sample coordinates (same taps, same
// weights, same order).  sx, sy are the derivatives of the weights as written, formed from the clamped indices: on the upper-edge quirk
// (x0 == x1) the two values are the same element and the slope is an exact 0.
template <int WHICH>
__global__ __launch_bounds__(FT_NT) void k_advect_tangent(Geom g, int T, const float *__restrict__ field, const float *__restrict__ u,
                                                          const float *__restrict__ v, const float *tfield, const float *tu,
                                                          const float *tv, float *__restrict__ tout) {
    constexpr bool IS_U = WHICH == 0, IS_V = WHICH == 1;
    const int R = IS_U ? g.H + 1 : g.H, C = IS_V ? g.W + 1 : g.W;
    const int pitch = IS_V ? g.pv : g.pc;
    const size_t fs = IS_U ? g.su : (IS_V ? g.sv : g.sc);
    const int b = blockIdx.z;
    const int X = blockIdx.x * FT_TX + threadIdx.x % FT_TX, Y = blockIdx.y * FT_TY + threadIdx.x / FT_TX;
    if (Y >= R || X >= C) return;
    const float *ub = u + (size_t)b * g.su, *vb = v + (size_t)b * g.sv, *fb = field + (size_t)b * fs;
    const Trace tr = trace_at(g, R, C, pitch, ub, vb, fb, Y, X);
    const Taps &su = tr.su, &sv = tr.sv, &t = tr.t;
    const size_t cell = (size_t)Y * pitch + X;
    for (int k = 0; k < T; ++k) {
        const size_t plane = (size_t)b * T + k;
        const float tui = gather(tu + plane * g.su, su), tvi = gather(tv + plane * g.sv, sv);
        const float dpx = tr.pass_x ? -(g.dt * tui) : 0.f, dpy = tr.pass_y ? -(g.dt * tvi) : 0.f;
        float r = gather(tfield + plane * fs, t);
        r = r + tr.sx * dpx;
        r = r + tr.sy * dpy;
        if (WHICH == 2) r = r * 0.995f;                                         // :171
        tout[plane * fs + cell] = r;
    }
}

// ---------------------------------------------------------------- norm and rescale of whole tangent states
// A tangent state is 4H + 1 rows: u's H + 1 of W, v's H of W + 1, p's H of W, density's H of W.
struct Row {
    float *p;
    int cols;
};
__device__ __forceinline__ Row ft_row(const Geom &g, float *tu, float *tv, float *tp, float *td, int bt, int r) {
    if (r <= g.H) return {tu + (size_t)bt * g.su + (size_t)r * g.pc, g.W};
    r -= g.H + 1;
    if (r < g.H) return {tv + (size_t)bt * g.sv + (size_t)r * g.pv, g.W + 1};
    r -= g.H;
    if (r < g.H) return {tp + (size_t)bt * g.sc + (size_t)r * g.pc, g.W};
    r -= g.H;
    return {td + (size_t)bt * g.sc + (size_t)r * g.pc, g.W};
}

// Level one: workgroup (p, bt) sums the squares of rows [p * rpg, (p + 1) * rpg) of tangent bt in fp64.  Wave w takes the rows
// w, w + 4, ... of the run, lane l their columns l, l + 64, ...; a thread adds its squares in that order, then the 256 sums are folded
// by halves (s = 128, 64, .. 1: x[i] += x[i + s]) -- one fixed order, whatever the machine.
__global__ __launch_bounds__(FT_NT) void k_tangent_sumsq(Geom g, int rpg, float *tu, float *tv, float *tp, float *td,
                                                         double *__restrict__ partial) {
    __shared__ double part[FT_NT];
    const int bt = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const int rows = 4 * g.H + 1, r0 = p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    double acc = 0.0;
    for (int r = r0 + (tid >> 6); r < r1; r += FT_NT / 64) {
        const Row row = ft_row(g, tu, tv, tp, td, bt, r);
        for (int c = tid & 63; c < row.cols; c += 64) {
            const double x = (double)row.p[c];
            acc = acc + x * x;
        }
    }
    part[tid] = acc;
    for (int s = FT_NT / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) part[tid] = part[tid] + part[tid + s];
    }
    if (tid == 0) partial[(size_t)bt * P + p] = part[0];
}

// Level two: every workgroup of tangent bt adds the P partial sums in ascending order (all get the same words), the first one reports
// the norm, and each divides its own rows by (float)norm with a true fp32 divide -- unless the norm is 0 or not finite (as fp64 or as fp32).
__global__ __launch_bounds__(FT_NT) void k_tangent_scale(Geom g, int rpg, float *tu, float *tv, float *tp, float *td,
                                                         const double *__restrict__ partial, double *__restrict__ norms) {
    __shared__ double total;
    const int bt = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    if (tid == 0) {
        double t = 0.0;
        for (int c = 0; c < P; ++c) t = t + partial[(size_t)bt * P + c];
        total = sqrt(t);
        if (p == 0) norms[bt] = total;
    }
    __syncthreads();
    const double norm = total;
    const float d = (float)norm;
    if (!(norm > 0.0) || !isfinite(norm) || !isfinite(d)) return;               // (workgroup-uniform; NaN fails the first test)
    const int rows = 4 * g.H + 1, r0 = p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    for (int r = r0 + (tid >> 6); r < r1; r += FT_NT / 64) {
        const Row row = ft_row(g, tu, tv, tp, td, bt, r);
        for (int c = tid & 63; c < row.cols; c += 64) row.p[c] = __fdiv_rn(row.p[c], d);
    }
}

}  // namespace

hipError_t launch_advect_tangent(const Geom &g, int T, int which, const float *field, const float *u, const float *v, const float *tfield,
                                 const float *tu, const float *tv, float *tout, hipStream_t st) {
    const int R = which == 0 ? g.H + 1 : g.H, C = which == 1 ? g.W + 1 : g.W;
    const dim3 grid((unsigned)cdiv(C, FT_TX), (unsigned)cdiv(R, FT_TY), (unsigned)g.B), block(FT_NT);
    if (which == 0) hipLaunchKernelGGL(k_advect_tangent<0>, grid, block, 0, st, g, T, field, u, v, tfield, tu, tv, tout);
    else if (which == 1) hipLaunchKernelGGL(k_advect_tangent<1>, grid, block, 0, st, g, T, field, u, v, tfield, tu, tv, tout);
    else hipLaunchKernelGGL(k_advect_tangent<2>, grid, block, 0, st, g, T, field, u, v, tfield, tu, tv, tout);
    return hipGetLastError();
}

hipError_t launch_tangent_renorm(const Geom &g, float *tu, float *tv, float *tp, float *td, double *norms, double *partial, hipStream_t st) {
    const int rpg = ft_rows_per_group(g.H);
    const dim3 grid((unsigned)ft_groups(g.H), (unsigned)g.B), block(FT_NT);
    hipLaunchKernelGGL(k_tangent_sumsq, grid, block, 0, st, g, rpg, tu, tv, tp, td, partial);
    hipLaunchKernelGGL(k_tangent_scale, grid, block, 0, st, g, rpg, tu, tv, tp, td, (const double *)partial, norms);
    return hipGetLastError();
}

}  // namespace smk

using namespace smk;

namespace {

bool ft_shape_ok(int32_t B, int32_t T, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v) {
    return fluid2d_shape_ok(B, H, W, pitch_c, pitch_v) &&
           T >= 1 && (int64_t)B * T <= 65535;                   // the tangents' planes are the launch grid's z
}
const char *const FT_SHAPE = "B, T >= 1, B * T <= 65535, 3 <= H, W <= 32766, pitch_c >= W, pitch_v >= W + 1";

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int smk_advect_tangent(int32_t which, const float *field, const float *u, const float *v, const float *tfield, const float *tu,
                       const float *tv, float *tout, int32_t B, int32_t T, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v,
                       double dt, void *stream) {
    SMK_REQUIRE(field && u && v && tfield && tu && tv && tout, "advect_tangent: null pointer");
    SMK_REQUIRE(which >= 0 && which <= 2, "advect_tangent: which in 0..2");
    SMK_REQUIRE(ft_shape_ok(B, T, H, W, pitch_c, pitch_v), FT_SHAPE);
    SMK_REQUIRE(tout != field && tout != u && tout != v && tout != tfield && tout != tu && tout != tv,
                "advect_tangent: the output aliases an input");
    const Geom g = fluid2d_geom(B, H, W, pitch_c, pitch_v, dt, 0.0);
    return check_launch(launch_advect_tangent(g, T, which, field, u, v, tfield, tu, tv, tout, (hipStream_t)stream), "advect_tangent");
}

int64_t smk_tangent_renorm_workspace(int32_t B, int32_t T, int32_t H, int32_t W) {
    if (!ft_shape_ok(B, T, H, W, W, W + 1)) return -1;
    return (int64_t)B * T * ft_groups(H) * (int64_t)sizeof(double);
}

int smk_tangent_renorm(float *tu, float *tv, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t H, int32_t W,
                       int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(tu && tv && tp && td && norms, "tangent_renorm: null pointer");
    SMK_REQUIRE(ft_shape_ok(B, T, H, W, pitch_c, pitch_v), FT_SHAPE);
    SMK_REQUIRE(workspace && workspace_bytes >= smk_tangent_renorm_workspace(B, T, H, W),
                "tangent_renorm: workspace smaller than smk_tangent_renorm_workspace(B, T, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)norms & 7) == 0, "tangent_renorm: workspace and norms must be 8-byte aligned");
    const Geom g = fluid2d_geom(B * T, H, W, pitch_c, pitch_v, 0.0, 0.0);
    return check_launch(launch_tangent_renorm(g, tu, tv, tp, td, norms, (double *)workspace, (hipStream_t)stream), "tangent_renorm");
}

}  // extern "C"
#pragma GCC visibility pop
