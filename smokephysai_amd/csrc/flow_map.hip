// The flow map of the 2-D stepper and its finite-time Lyapunov exponent (FTLE): the kernels behind smk_flow_map_step and smk_ftle_field.
// DESIGN.md section 3.14.
//
// A displacement field disp = (dx, dy) at the cell centres, in cells, stands for the map x -> x + disp.  One smk_flow_map_step after every
// step(), with that step's output velocities (the ones its density advection sampled), composes the step's own first-order trace into it:
//   backward   x + disp is where the particle now at x was when the window began (semi-Lagrangian composition, in time order);
//   forward    x + disp is where the particle that began at x is now.
// smk_ftle_field turns a displacement field into the FTLE of its map, with the field's mean and maximum per grid.
//
// Arithmetic rules (the project's derivative rules): fp32 throughout (the statistics in fp64), one rounding per listed operation (the build
// keeps -ffp-contract=off), every sum in one fixed order, no atomics, every output element written, the pitch padding neither read nor
// written, results bit-identical from call to call and independent of a grid's batch mates.  The backward map's velocity samples,
// back-trace, clamp decisions, taps and weights are csrc/fluid_trace.h's, i.e. the density advection's bit for bit.
#include "flow_map.h"

namespace smk {

namespace {

// ---------------------------------------------------------------- one map step
// One thread per cell (Y, X), both components.
// DIR = FM_BACKWARD:  ax = X - dt su,  px = clamp(ax, 0, W - 1);  ix = -(dt su) where 0 <= ax <= W - 1 (bounds included), else px - X;
//                     dx' = interp(dx; py, px) + ix;  y likewise.  su, sv, (py, px), the taps and the weights: trace_at's; the two gathers
//                     share them.  The increment is never formed as px - X where the clamp passes: X + (-(dt su)) loses nothing of a small
//                     displacement, (X - dt su) - X rounds it to a multiple of ulp(X).
// DIR = FM_FORWARD:   qx = clamp(X + dx, 0, W - 1), qy likewise (sample positions only);  su, sv = u, v sampled at (qy, qx);
//                     dx' = min(max(dx + dt su, -X), W - 1 - X);  y likewise (the bounds are exact integers).
template <int DIR>
__global__ __launch_bounds__(FT_NT) void k_flow_map(Geom g, int pm, const float *__restrict__ u, const float *__restrict__ v,
                                                    const float *__restrict__ disp, float *__restrict__ out) {
    const int b = blockIdx.z;
    const int X = blockIdx.x * FT_TX + threadIdx.x % FT_TX, Y = blockIdx.y * FT_TY + threadIdx.x / FT_TX;
    if (Y >= g.H || X >= g.W) return;
    const size_t plane = (size_t)g.H * pm, cell = (size_t)Y * pm + X;
    const float *ub = u + (size_t)b * g.su, *vb = v + (size_t)b * g.sv;
    const float *dxb = disp + (size_t)b * 2 * plane, *dyb = dxb + plane;
    float *oxb = out + (size_t)b * 2 * plane, *oyb = oxb + plane;
    const float fX = (float)X, fY = (float)Y;
    if (DIR == FM_BACKWARD) {
        const Trace tr = trace_at(g, g.H, g.W, pm, ub, vb, dxb, Y, X);
        const float ix = tr.pass_x ? -(g.dt * tr.ui) : tr.px - fX;
        const float iy = tr.pass_y ? -(g.dt * tr.vi) : tr.py - fY;
        oxb[cell] = gather(dxb, tr.t) + ix;
        oyb[cell] = gather(dyb, tr.t) + iy;
    } else {
        const float hx = (float)(g.W - 1), hy = (float)(g.H - 1);
        const float dx = dxb[cell], dy = dyb[cell];
        const float qx = clampf(fX + dx, 0.f, hx), qy = clampf(fY + dy, 0.f, hy);
        const float su = gather(ub, u_taps_at(g, qy, qx)), sv = gather(vb, v_taps_at(g, qy, qx));
        oxb[cell] = clampf(dx + g.dt * su, -fX, hx - fX);
        oyb[cell] = clampf(dy + g.dt * sv, -fY, hy - fY);
    }
}

// ---------------------------------------------------------------- the FTLE of a displacement field
// Level one: workgroup (p, b) owns rows [p * rpg, (p + 1) * rpg) of grid b.  Wave w takes the rows w, w + 4, ... of the run, lane l their
// columns l, l + 64, ...  Per cell, with a = dx, b = dy and G = [[a_x, a_y], [b_x, b_y]] their differences, the Green-Lagrange strain
// E = (G + G^T + G^T G) / 2 formed so that the identity never enters, its larger eigenvalue, and
//     ftle = log1p(max(2 emax, lo)) / (2 horizon),   lo = the fp32 number next above -1.
// A thread adds its values in fp64 in that order and keeps their maximum, then the 256 sums and maxima are folded by halves
// (s = 128, 64, .. 1: x[i] += x[i + s]) -- smk_tangent_renorm's fixed order.
__global__ __launch_bounds__(FT_NT) void k_ftle(Geom g, int pm, int rpg, float two_horizon, const float *__restrict__ disp,
                                                float *__restrict__ ftle, double *__restrict__ partial) {
    __shared__ double part[FT_NT], top[FT_NT];
    const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const int r0 = p * rpg, r1 = r0 + rpg < g.H ? r0 + rpg : g.H;
    const size_t plane = (size_t)g.H * pm;
    const float *dxb = disp + (size_t)b * 2 * plane, *dyb = dxb + plane;
    float *fb = ftle + (size_t)b * plane;
    const float lo = -0.99999994f;                                               // -1 + 2^-24
    double acc = 0.0, best = -INFINITY;
    for (int r = r0 + (tid >> 6); r < r1; r += FT_NT / 64) {
        for (int c = tid & 63; c < g.W; c += 64) {
            const size_t cell = (size_t)r * pm + c;
            const float ax = diff_at(dxb + cell, c, g.W, 1), ay = diff_at(dxb + cell, r, g.H, (size_t)pm);
            const float bx = diff_at(dyb + cell, c, g.W, 1), by = diff_at(dyb + cell, r, g.H, (size_t)pm);
            const float exx = ax + 0.5f * (ax * ax + bx * bx);
            const float eyy = by + 0.5f * (ay * ay + by * by);
            const float exy = 0.5f * (ay + bx) + 0.5f * (ax * ay + bx * by);
            const float m = 0.5f * (exx + eyy), d = 0.5f * (exx - eyy);
            const float emax = m + sqrtf(d * d + exy * exy);
            float t = 2.0f * emax;
            t = t < lo ? lo : t;                                                 // (a NaN stays a NaN)
            const float f = __fdiv_rn(log1pf(t), two_horizon);
            fb[cell] = f;
            acc = acc + (double)f;
            best = nanmax(best, (double)f);
        }
    }
    part[tid] = acc;
    top[tid] = best;
    for (int s = FT_NT / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            part[tid] = part[tid] + part[tid + s];
            top[tid] = nanmax(top[tid], top[tid + s]);
        }
    }
    if (tid == 0) {
        partial[((size_t)b * P + p) * 2] = part[0];
        partial[((size_t)b * P + p) * 2 + 1] = top[0];
    }
}

// Level two: one thread per grid adds the P partial sums in ascending order and divides by the number of cells; the maximum likewise.
__global__ void k_ftle_stats(int B, int P, double cells, const double *__restrict__ partial, double *__restrict__ stats) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double t = 0.0, best = -INFINITY;
    for (int c = 0; c < P; ++c) {
        t = t + partial[((size_t)b * P + c) * 2];
        best = nanmax(best, partial[((size_t)b * P + c) * 2 + 1]);
    }
    stats[(size_t)b * 2] = t / cells;
    stats[(size_t)b * 2 + 1] = best;
}

}  // namespace

hipError_t launch_flow_map(const Geom &g, int pm, int dir, const float *u, const float *v, const float *disp, float *out, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(g.W, FT_TX), (unsigned)cdiv(g.H, FT_TY), (unsigned)g.B), block(FT_NT);
    if (dir == FM_BACKWARD) hipLaunchKernelGGL(k_flow_map<FM_BACKWARD>, grid, block, 0, st, g, pm, u, v, disp, out);
    else hipLaunchKernelGGL(k_flow_map<FM_FORWARD>, grid, block, 0, st, g, pm, u, v, disp, out);
    return hipGetLastError();
}

hipError_t launch_ftle_stats(int B, int P, double cells, const double *partial, double *stats, hipStream_t st) {
    hipLaunchKernelGGL(k_ftle_stats, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, B, P, cells, partial, stats);
    return hipGetLastError();
}

hipError_t launch_ftle(const Geom &g, int pm, float two_horizon, const float *disp, float *ftle, double *stats, double *partial,
                       hipStream_t st) {
    const int rpg = fm_rows_per_group(g.H), P = fm_groups(g.H);
    hipLaunchKernelGGL(k_ftle, dim3((unsigned)P, (unsigned)g.B), dim3(FT_NT), 0, st, g, pm, rpg, two_horizon, disp, ftle, partial);
    return launch_ftle_stats(g.B, P, (double)g.H * (double)g.W, partial, stats, st);
}

}  // namespace smk

using namespace smk;

namespace {

bool fm_shape_ok(int32_t B, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t pitch_m) {
    return fluid2d_shape_ok(B, H, W, pitch_c, pitch_v) && pitch_m >= W;
}
const char *const FM_SHAPE = "1 <= B <= 65535, 3 <= H, W <= 32766, pitch_c >= W, pitch_v >= W + 1, pitch_m >= W";

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int smk_flow_map_step(int32_t direction, const float *u, const float *v, const float *disp_in, float *disp_out, int32_t B, int32_t H,
                      int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t pitch_m, double dt, void *stream) {
    SMK_REQUIRE(u && v && disp_in && disp_out, "flow_map_step: null pointer");
    SMK_REQUIRE(direction == FM_BACKWARD || direction == FM_FORWARD, "flow_map_step: direction is 0 (backward) or 1 (forward)");
    SMK_REQUIRE(fm_shape_ok(B, H, W, pitch_c, pitch_v, pitch_m), FM_SHAPE);
    SMK_REQUIRE(disp_out != disp_in && disp_out != u && disp_out != v, "flow_map_step: the output aliases an input");
    const Geom g = fluid2d_geom(B, H, W, pitch_c, pitch_v, dt, 0.0);
    return check_launch(launch_flow_map(g, pitch_m, direction, u, v, disp_in, disp_out, (hipStream_t)stream), "flow_map_step");
}

int64_t smk_ftle_workspace(int32_t B, int32_t H, int32_t W) {
    if (!fm_shape_ok(B, H, W, W, W + 1, W)) return -1;
    return (int64_t)B * fm_groups(H) * 2 * (int64_t)sizeof(double);
}

int smk_ftle_field(const float *disp, float *ftle, double *stats, int32_t B, int32_t H, int32_t W, int32_t pitch_m, double horizon,
                   void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(disp && ftle && stats, "ftle_field: null pointer");
    SMK_REQUIRE(fm_shape_ok(B, H, W, W, W + 1, pitch_m), FM_SHAPE);
    SMK_REQUIRE(horizon > 0.0 && (float)(2.0 * horizon) > 0.f && isfinite((float)(2.0 * horizon)), "ftle_field: horizon > 0 (and finite as fp32)");
    SMK_REQUIRE(ftle != disp, "ftle_field: the output aliases the input");
    SMK_REQUIRE(workspace && workspace_bytes >= smk_ftle_workspace(B, H, W),
                "ftle_field: workspace smaller than smk_ftle_workspace(B, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "ftle_field: workspace and stats must be 8-byte aligned");
    const Geom g = fluid2d_geom(B, H, W, pitch_m, W + 1, 0.0, 0.0);
    return check_launch(launch_ftle(g, pitch_m, (float)(2.0 * horizon), disp, ftle, stats, (double *)workspace, (hipStream_t)stream),
                        "ftle_field");
}

}  // extern "C"
#pragma GCC visibility pop
