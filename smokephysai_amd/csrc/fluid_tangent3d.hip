// Tangent-linear (forward-mode) derivative of one 3-D stable-fluids step (SPEC_3D.md sections 3-6): the kernels behind
// smk_advect3d_tangent and smk_tangent3d_renorm.  DESIGN.md section 3.12; the 3-D counterpart of csrc/fluid_tangent.hip.
//
// Buoyancy, the four diffusions, the divergence, the Jacobi sweeps and the gradient subtraction are linear and homogeneous in the state:
// their tangent is the stepper's own kernel applied to the tangent state.  Only the advection is non-linear, and its tangent is a gather at
// the forward's own taps -- there is nothing to transpose, so a back-trace may move any number of cells (no far case).
//
// Arithmetic rules (the project's gradient rules): fp32 throughout, every sum in one fixed order, no atomics, every output element written,
// results bit-identical from call to call and independent of T and of a grid's batch mates.  The back-trace positions, indices, clamp
// decisions, weights and slopes are formed by the forward's own expressions (csrc/fluid_trace3d.h), so they are the forward's bit for bit.
#include "fluid_tangent3d.h"
#include "fluid_trace3d.h"

namespace smk {

namespace {

// ---------------------------------------------------------------- advection tangent
// out = adv(f; u, v, w) (times 0.995 for WHICH = 3).  One thread per destination cell (Z, Y, X); grid z = b * Df + Z as k3_advect has it,
// so workgroups that run together work on neighbouring planes and the z-taps meet in L2.  The thread forms the forward's velocity
// samples, the back-trace, its clamp decisions, the eight taps and weights and the three slopes of the interpolant ONCE, keeps them in
// registers, and then loops over the T tangents of its grid:
//     r   = interp3's eight-term sum over tfield: weights (wx wy) wz, z-low plane first, x fastest, low before high
//     r   = r + sx * dpx;  r = r + sy * dpy;  r = r + sz * dpz;           WHICH == 3: r = r * 0.995f
//     dpx = -(dt * vel3_at<2>(tu)) where 0 <= X - dt ui <= Wf - 1 (bounds included), else 0; dpy from tv with <1>, dpz from tw with <0>
// Every address comes from clamped indices or from behind vel3_at's guard: no input value can move one out of its volume.
template <int WHICH>
__global__ __launch_bounds__(FT3_NT) void k3_advect_tangent(Geom3 g, int T, const float *__restrict__ field, const float *__restrict__ u,
                                                            const float *__restrict__ v, const float *__restrict__ w, const float *tfield,
                                                            const float *tu, const float *tv, const float *tw, float *__restrict__ tout) {
    const int Df = g.D + (WHICH == 2), Hf = g.H + (WHICH == 0), Wf = g.W + (WHICH == 1);
    const int pitch = WHICH == 1 ? g.pv : g.pc;
    const size_t fs = WHICH == 0 ? g.su : (WHICH == 1 ? g.sv : (WHICH == 2 ? g.sw : g.sc));
    const int b = blockIdx.z / Df, Z = blockIdx.z % Df;
    const int X = blockIdx.x * FT3_TX + threadIdx.x % FT3_TX, Y = blockIdx.y * FT3_TY + threadIdx.x / FT3_TX;
    if (Y >= Hf || X >= Wf) return;
    const Trace3 tr = trace3_at(g, Df, Hf, Wf, pitch, u + b * g.su, v + b * g.sv, w + b * g.sw, field + b * fs, Z, Y, X);
    const size_t cell = ((size_t)Z * Hf + Y) * pitch + X;
    for (int k = 0; k < T; ++k) {
        const size_t grid = (size_t)b * T + k;
        const float tui = vel3_sample(tu + grid * g.su, tr.su), tvi = vel3_sample(tv + grid * g.sv, tr.sv);
        const float twi = vel3_sample(tw + grid * g.sw, tr.sw);
        const float dpx = tr.pass_x ? -(g.dt * tui) : 0.f, dpy = tr.pass_y ? -(g.dt * tvi) : 0.f, dpz = tr.pass_z ? -(g.dt * twi) : 0.f;
        float r = gather3(tfield + grid * fs, tr);
        r = r + tr.sx * dpx;
        r = r + tr.sy * dpy;
        r = r + tr.sz * dpz;
        if (WHICH == 3) r = r * 0.995f;                                         // the decay of step()
        tout[grid * fs + cell] = r;
    }
}

// ---------------------------------------------------------------- norm and rescale of whole tangent states
struct Row3 {
    float *p;
    int cols;
};
__device__ __forceinline__ Row3 ft3_row_ptr(const Geom3 &g, float *tu, float *tv, float *tw, float *tp, float *td, int bt, int64_t r) {
    const Ft3Row q = ft3_row(g.D, g.H, g.W, g.pc, g.pv, r);
    float *base = q.field == 0 ? tu + (size_t)bt * g.su
                : q.field == 1 ? tv + (size_t)bt * g.sv
                : q.field == 2 ? tw + (size_t)bt * g.sw
                : (q.field == 3 ? tp : td) + (size_t)bt * g.sc;
    return {base + q.offset, q.cols};
}

// Level one: workgroup (p, bt) sums the squares of rows [p * rpg, (p + 1) * rpg) of tangent bt in fp64.  Wave w takes the rows
// w, w + 4, ... of the run, lane l their columns l, l + 64, ...; a thread adds its squares in that order, then the 256 sums are folded
// by halves (s = 128, 64, .. 1: x[i] += x[i + s]) -- one fixed order, whatever the machine (k_tangent_sumsq's, csrc/fluid_tangent.hip).
__global__ __launch_bounds__(FT3_NT) void k3_tangent_sumsq(Geom3 g, int rpg, float *tu, float *tv, float *tw, float *tp, float *td,
                                                           double *__restrict__ partial) {
    __shared__ double part[FT3_NT];
    const int bt = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const int64_t rows = ft3_rows(g.D, g.H), r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    double acc = 0.0;
    for (int64_t r = r0 + (tid >> 6); r < r1; r += FT3_NT / 64) {
        const Row3 row = ft3_row_ptr(g, tu, tv, tw, tp, td, bt, r);
        for (int c = tid & 63; c < row.cols; c += 64) {
            const double x = (double)row.p[c];
            acc = acc + x * x;
        }
    }
    part[tid] = acc;
    for (int s = FT3_NT / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) part[tid] = part[tid] + part[tid + s];
    }
    if (tid == 0) partial[(size_t)bt * P + p] = part[0];
}

// Level two: every workgroup of tangent bt adds the P partial sums in ascending order (all get the same words), the first one reports
// the norm, and each divides its own rows by (float)norm with a true fp32 divide -- unless the norm is 0 or not finite (as fp64 or as fp32).
__global__ __launch_bounds__(FT3_NT) void k3_tangent_scale(Geom3 g, int rpg, float *tu, float *tv, float *tw, float *tp, float *td,
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
    const int64_t rows = ft3_rows(g.D, g.H), r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    for (int64_t r = r0 + (tid >> 6); r < r1; r += FT3_NT / 64) {
        const Row3 row = ft3_row_ptr(g, tu, tv, tw, tp, td, bt, r);
        for (int c = tid & 63; c < row.cols; c += 64) row.p[c] = __fdiv_rn(row.p[c], d);
    }
}

}  // namespace

hipError_t launch3_advect_tangent(const Geom3 &g, int T, int which, const float *field, const float *u, const float *v, const float *w,
                                  const float *tfield, const float *tu, const float *tv, const float *tw, float *tout, hipStream_t st) {
    const int Df = g.D + (which == 2), Hf = g.H + (which == 0), Wf = g.W + (which == 1);
    const dim3 grid((unsigned)cdiv(Wf, FT3_TX), (unsigned)cdiv(Hf, FT3_TY), (unsigned)(g.B * Df)), block(FT3_NT);
    switch (which) {
        case 0: hipLaunchKernelGGL(k3_advect_tangent<0>, grid, block, 0, st, g, T, field, u, v, w, tfield, tu, tv, tw, tout); break;
        case 1: hipLaunchKernelGGL(k3_advect_tangent<1>, grid, block, 0, st, g, T, field, u, v, w, tfield, tu, tv, tw, tout); break;
        case 2: hipLaunchKernelGGL(k3_advect_tangent<2>, grid, block, 0, st, g, T, field, u, v, w, tfield, tu, tv, tw, tout); break;
        default: hipLaunchKernelGGL(k3_advect_tangent<3>, grid, block, 0, st, g, T, field, u, v, w, tfield, tu, tv, tw, tout); break;
    }
    return hipGetLastError();
}

hipError_t launch3_tangent_renorm(const Geom3 &g, float *tu, float *tv, float *tw, float *tp, float *td, double *norms, double *partial,
                                  hipStream_t st) {
    const int rpg = ft3_rows_per_group(g.D, g.H);
    const dim3 grid((unsigned)ft3_groups(g.D, g.H), (unsigned)g.B), block(FT3_NT);
    hipLaunchKernelGGL(k3_tangent_sumsq, grid, block, 0, st, g, rpg, tu, tv, tw, tp, td, partial);
    hipLaunchKernelGGL(k3_tangent_scale, grid, block, 0, st, g, rpg, tu, tv, tw, tp, td, (const double *)partial, norms);
    return hipGetLastError();
}

}  // namespace smk

using namespace smk;

namespace {

// One limit for both entry points and for the stepper of B * T grids that runs the tangents' linear stages (smk_sim3d_create's
// B * (D + 1) <= 65535 at B * T grids): it covers the advection's launch grid, B * (D + 1) planes, and the renormalisation's, B * T.
bool ft3_shape_ok(int32_t B, int32_t T, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v) {
    return fluid3d_shape_ok(B, D, H, W, pitch_c, pitch_v) && T >= 1 && (int64_t)B * T * (D + 1) <= 65535;
}
const char *const FT3_SHAPE = "B, T >= 1, B * T * (D + 1) <= 65535, 3 <= D, H, W <= 32766, pitch_c >= W, pitch_v >= W + 1, one grid's field below 2^31 elements";

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int smk_advect3d_tangent(int32_t which, const float *field, const float *u, const float *v, const float *w, const float *tfield,
                         const float *tu, const float *tv, const float *tw, float *tout, int32_t B, int32_t T, int32_t D, int32_t H,
                         int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, void *stream) {
    SMK_REQUIRE(field && u && v && w && tfield && tu && tv && tw && tout, "advect3d_tangent: null pointer");
    SMK_REQUIRE(which >= 0 && which <= 3, "advect3d_tangent: which in 0..3");
    SMK_REQUIRE(ft3_shape_ok(B, T, D, H, W, pitch_c, pitch_v), FT3_SHAPE);
    SMK_REQUIRE(tout != field && tout != u && tout != v && tout != w && tout != tfield && tout != tu && tout != tv && tout != tw,
                "advect3d_tangent: the output aliases an input");
    const Geom3 g = fluid3d_geom(B, D, H, W, pitch_c, pitch_v, dt);
    return check_launch(launch3_advect_tangent(g, T, which, field, u, v, w, tfield, tu, tv, tw, tout, (hipStream_t)stream),
                        "advect3d_tangent");
}

int64_t smk_tangent3d_renorm_workspace(int32_t B, int32_t T, int32_t D, int32_t H, int32_t W) {
    if (!ft3_shape_ok(B, T, D, H, W, W, W + 1)) return -1;
    return (int64_t)B * T * ft3_groups(D, H) * (int64_t)sizeof(double);
}

int smk_tangent3d_renorm(float *tu, float *tv, float *tw, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t D, int32_t H,
                         int32_t W, int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(tu && tv && tw && tp && td && norms, "tangent3d_renorm: null pointer");
    SMK_REQUIRE(ft3_shape_ok(B, T, D, H, W, pitch_c, pitch_v), FT3_SHAPE);
    SMK_REQUIRE(workspace && workspace_bytes >= smk_tangent3d_renorm_workspace(B, T, D, H, W),
                "tangent3d_renorm: workspace smaller than smk_tangent3d_renorm_workspace(B, T, D, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)norms & 7) == 0, "tangent3d_renorm: workspace and norms must be 8-byte aligned");
    Geom3 g = fluid3d_geom(B, D, H, W, pitch_c, pitch_v, 0.0);
    g.B = B * T;                                                                // the launch's grids are the tangent states
    return check_launch(launch3_tangent_renorm(g, tu, tv, tw, tp, td, norms, (double *)workspace, (hipStream_t)stream), "tangent3d_renorm");
}

}  // extern "C"
#pragma GCC visibility pop
