// The flow map of the 3-D stepper and its finite-time Lyapunov exponent (FTLE): the kernels behind smk_flow_map3d_step and
// smk_ftle3d_field.  DESIGN.md section 3.15; the 3-D counterpart of csrc/flow_map.hip.
//
// A displacement disp = (dx, dy, dz) at the cell centres, in cells, stands for the map x -> x + disp; component k acts along the axis
// velocity component k acts along.  One smk_flow_map3d_step after every step(), with that step's output velocities (the ones its density
// advection sampled), composes the step's own first-order trace into it, backward or forward as in 2-D.  smk_ftle3d_field turns a
// displacement into the FTLE of its map, with the field's mean and maximum per grid.
//
// Arithmetic rules (the project's derivative rules): fp32 throughout (the statistics in fp64), one rounding per listed operation (the build
// keeps -ffp-contract=off), every sum in one fixed order, no atomics, every output element written, the pitch padding neither read nor
// written, results bit-identical from call to call and independent of a grid's batch mates, every index clamped before use.  The backward
// map's velocity samples, back-trace, clamp decisions, taps and weights are the density advection's bit for bit (flow_map3d.h over
// fluid_trace3d.h's helpers).
#include "flow_map3d.h"

namespace smk {

namespace {

// ---------------------------------------------------------------- one map step
// One thread per cell (Z, Y, X) of plane blockIdx.z % D of grid blockIdx.z / D, all three components.
// DIR = FM_BACKWARD:  per axis a = X - dt s, p = clamp(a, 0, n - 1);  the increment -(dt s) where 0 <= a <= n - 1 (bounds included), else
//                     p - X;  d' = interp(d; pz, py, px) + increment.  The three gathers share the eight taps.  The increment is never
//                     formed as p - X where the clamp passes (csrc/flow_map.hip says why).
// DIR = FM_FORWARD:   per axis q = clamp(X + d, 0, n - 1) (sample positions only);  s = the component sampled at (qz, qy, qx);
//                     d' = min(max(d + dt s, -X), n - 1 - X) (the bounds are exact integers).
template <int DIR>
__global__ __launch_bounds__(FT3_NT) void k3_flow_map(Geom3 g, int pm, const float *__restrict__ u, const float *__restrict__ v,
                                                      const float *__restrict__ w, const float *__restrict__ disp,
                                                      float *__restrict__ out) {
    const int b = blockIdx.z / g.D, Z = blockIdx.z % g.D;
    const int X = blockIdx.x * FT3_TX + threadIdx.x % FT3_TX, Y = blockIdx.y * FT3_TY + threadIdx.x / FT3_TX;
    if (Y >= g.H || X >= g.W) return;
    const size_t vol = (size_t)g.D * g.H * pm, cell = ((size_t)Z * g.H + Y) * pm + X;
    const float *ub = u + (size_t)b * g.su, *vb = v + (size_t)b * g.sv, *wb = w + (size_t)b * g.sw;
    const float *dxb = disp + (size_t)b * 3 * vol, *dyb = dxb + vol, *dzb = dyb + vol;
    float *oxb = out + (size_t)b * 3 * vol, *oyb = oxb + vol, *ozb = oyb + vol;
    const float fX = (float)X, fY = (float)Y, fZ = (float)Z;
    if (DIR == FM_BACKWARD) {
        const MapTrace3 tr = map_trace3_at(g, ub, vb, wb, Z, Y, X);
        const Taps3 t = taps3_at(g.D, g.H, g.W, pm, tr.pz, tr.py, tr.px);
        const float ix = tr.pass_x ? -tr.tx : tr.px - fX;
        const float iy = tr.pass_y ? -tr.ty : tr.py - fY;
        const float iz = tr.pass_z ? -tr.tz : tr.pz - fZ;
        oxb[cell] = gather3(dxb, t) + ix;
        oyb[cell] = gather3(dyb, t) + iy;
        ozb[cell] = gather3(dzb, t) + iz;
    } else {
        const float hx = (float)(g.W - 1), hy = (float)(g.H - 1), hz = (float)(g.D - 1);
        const float dx = dxb[cell], dy = dyb[cell], dz = dzb[cell];
        const float qx = clampf3(fX + dx, 0.f, hx), qy = clampf3(fY + dy, 0.f, hy), qz = clampf3(fZ + dz, 0.f, hz);
        const float su = gather3(ub, stag3_taps_at<2>(g.D, g.H + 1, g.W, g.pc, qz, qy, qx));
        const float sv = gather3(vb, stag3_taps_at<1>(g.D, g.H, g.W + 1, g.pv, qz, qy, qx));
        const float sw = gather3(wb, stag3_taps_at<0>(g.D + 1, g.H, g.W, g.pc, qz, qy, qx));
        oxb[cell] = clampf3(dx + g.dt * su, -fX, hx - fX);
        oyb[cell] = clampf3(dy + g.dt * sv, -fY, hy - fY);
        ozb[cell] = clampf3(dz + g.dt * sw, -fZ, hz - fZ);
    }
}

// ---------------------------------------------------------------- the FTLE of a displacement volume
// One Jacobi rotation of a symmetric 3 x 3 matrix that annihilates a_pq (r: the third index), branch-free, the rule operation for
// operation:  theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), sign(theta) = +1 for theta >= 0;  where
// a_pq == 0 the divide is by 1 and t = 0 is selected;  c = 1 / sqrt(t^2 + 1), s = t c;  a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0;
// a_rp' = c a_rp - s a_rq, a_rq' = s a_rp + c a_rq.  Divides and square roots are the correctly rounded ones.
__device__ __forceinline__ void jacobi_rotate(float &app, float &aqq, float &apq, float &arp, float &arq) {
    const bool flat = apq == 0.f;
    const float theta = __fdiv_rn(aqq - app, flat ? 1.0f : 2.0f * apq);
    float t = __fdiv_rn(theta >= 0.f ? 1.0f : -1.0f, fabsf(theta) + __fsqrt_rn(theta * theta + 1.0f));
    t = flat ? 0.f : t;
    const float c = __fdiv_rn(1.0f, __fsqrt_rn(t * t + 1.0f));
    const float s = t * c;
    const float npp = app - t * apq, nqq = aqq + t * apq;
    const float nrp = c * arp - s * arq, nrq = s * arp + c * arq;
    app = npp; aqq = nqq; apq = 0.f; arp = nrp; arq = nrq;
}
// max in which a NaN wins (torch.maximum's convention)
__device__ __forceinline__ float nanmaxf(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}

constexpr int FM3_SWEEPS = 4;   // fixed, no early exit: 3 sweeps leave 4.7e-10 ||E||_F in fp64, and the fp64 rule is the tests' oracle

// Level one: workgroup (p, b) owns rows [p * rpg, (p + 1) * rpg) of grid b's D H rows (fm3_row: planes before rows).  Wave w takes the
// rows w, w + 4, ... of the run, lane l their columns l, l + 64, ...  Per cell, with g[k][j] the difference of component k along axis j
// (x, y, z), the Green-Lagrange strain formed so that the identity never enters,
//     E_ii = g[i][i] + 0.5 ((g[x][i]^2 + g[y][i]^2) + g[z][i]^2),
//     E_ij = 0.5 (g[i][j] + g[j][i]) + 0.5 ((g[x][i] g[x][j] + g[y][i] g[y][j]) + g[z][i] g[z][j]),
// its largest eigenvalue by FM3_SWEEPS cyclic Jacobi sweeps of rotations (x, y), (x, z), (y, z), and
//     ftle = log1p(max(2 emax, lo)) / (2 horizon),   lo = the fp32 number next above -1.
// A thread adds its values in fp64 in that order and keeps their maximum, then the 256 sums and maxima are folded by halves
// (s = 128, 64, .. 1: x[i] += x[i + s]) -- smk_tangent_renorm's fixed order.
__global__ __launch_bounds__(FT3_NT) void k3_ftle(Geom3 g, int pm, int rpg, float two_horizon, const float *__restrict__ disp,
                                                  float *__restrict__ ftle, double *__restrict__ partial) {
    __shared__ double part[FT3_NT], top[FT3_NT];
    const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const int64_t rows = fm3_rows(g.D, g.H);
    const int64_t r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
    const size_t vol = (size_t)g.D * g.H * pm, sy = (size_t)pm, sz = (size_t)g.H * pm;
    const float *d0 = disp + (size_t)b * 3 * vol;
    float *fb = ftle + (size_t)b * vol;
    const float lo = -0.99999994f;                                               // -1 + 2^-24
    double acc = 0.0, best = -INFINITY;
    for (int64_t r = r0 + (tid >> 6); r < r1; r += FT3_NT / 64) {
        const Fm3Row q = fm3_row(g.H, pm, r);
        for (int c = tid & 63; c < g.W; c += 64) {
            const size_t cell = (size_t)q.offset + c;
            float gr[3][3];                                                      // gr[k][j] = d disp_k / d axis_j
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float *f = d0 + k * vol + cell;
                gr[k][0] = diff_at(f, c, g.W, 1);
                gr[k][1] = diff_at(f, q.row, g.H, sy);
                gr[k][2] = diff_at(f, q.plane, g.D, sz);
            }
#define FM3_DOTS(i, j) ((gr[0][i] * gr[0][j] + gr[1][i] * gr[1][j]) + gr[2][i] * gr[2][j])
            float exx = gr[0][0] + 0.5f * FM3_DOTS(0, 0);
            float eyy = gr[1][1] + 0.5f * FM3_DOTS(1, 1);
            float ezz = gr[2][2] + 0.5f * FM3_DOTS(2, 2);
            float exy = 0.5f * (gr[0][1] + gr[1][0]) + 0.5f * FM3_DOTS(0, 1);
            float exz = 0.5f * (gr[0][2] + gr[2][0]) + 0.5f * FM3_DOTS(0, 2);
            float eyz = 0.5f * (gr[1][2] + gr[2][1]) + 0.5f * FM3_DOTS(1, 2);
#undef FM3_DOTS
#pragma unroll
            for (int sweep = 0; sweep < FM3_SWEEPS; ++sweep) {
                jacobi_rotate(exx, eyy, exy, exz, eyz);
                jacobi_rotate(exx, ezz, exz, exy, eyz);
                jacobi_rotate(eyy, ezz, eyz, exy, exz);
            }
            float t = 2.0f * nanmaxf(nanmaxf(exx, eyy), ezz);
            t = t < lo ? lo : t;                                                 // (a NaN stays a NaN)
            const float f = __fdiv_rn(log1pf(t), two_horizon);
            fb[cell] = f;
            acc = acc + (double)f;
            best = nanmax(best, (double)f);
        }
    }
    part[tid] = acc;
    top[tid] = best;
    for (int s = FT3_NT / 2; s >= 1; s >>= 1) {
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

}  // namespace

hipError_t launch3_flow_map(const Geom3 &g, int pm, int dir, const float *u, const float *v, const float *w, const float *disp, float *out,
                            hipStream_t st) {
    const dim3 grid((unsigned)cdiv(g.W, FT3_TX), (unsigned)cdiv(g.H, FT3_TY), (unsigned)(g.B * g.D)), block(FT3_NT);
    if (dir == FM_BACKWARD) hipLaunchKernelGGL(k3_flow_map<FM_BACKWARD>, grid, block, 0, st, g, pm, u, v, w, disp, out);
    else hipLaunchKernelGGL(k3_flow_map<FM_FORWARD>, grid, block, 0, st, g, pm, u, v, w, disp, out);
    return hipGetLastError();
}

hipError_t launch3_ftle(const Geom3 &g, int pm, float two_horizon, const float *disp, float *ftle, double *stats, double *partial,
                        hipStream_t st) {
    const int rpg = fm3_rows_per_group(g.D, g.H), P = fm3_groups(g.D, g.H);
    hipLaunchKernelGGL(k3_ftle, dim3((unsigned)P, (unsigned)g.B), dim3(FT3_NT), 0, st, g, pm, rpg, two_horizon, disp, ftle, partial);
    return launch_ftle_stats(g.B, P, (double)g.D * (double)g.H * (double)g.W, partial, stats, st);
}

}  // namespace smk

using namespace smk;

namespace {

bool fm3_shape_ok(int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t pitch_m) {
    return fluid3d_shape_ok(B, D, H, W, pitch_c, pitch_v) && fm3_pitch_ok(D, H, W, pitch_m);
}
const char *const FM3_SHAPE = "B >= 1, 3 <= D, H, W <= 32766, B * (D + 1) <= 65535, pitch_c >= W, pitch_v >= W + 1, pitch_m >= W, "
                              "(D + 1) * (H + 1) * pitch_c, ... * pitch_v and D * H * pitch_m < 2^31";

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int smk_flow_map3d_step(int32_t direction, const float *u, const float *v, const float *w, const float *disp_in, float *disp_out, int32_t B,
                        int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t pitch_m, double dt, void *stream) {
    SMK_REQUIRE(u && v && w && disp_in && disp_out, "flow_map3d_step: null pointer");
    SMK_REQUIRE(direction == FM_BACKWARD || direction == FM_FORWARD, "flow_map3d_step: direction is 0 (backward) or 1 (forward)");
    SMK_REQUIRE(fm3_shape_ok(B, D, H, W, pitch_c, pitch_v, pitch_m), FM3_SHAPE);
    SMK_REQUIRE(disp_out != disp_in && disp_out != u && disp_out != v && disp_out != w, "flow_map3d_step: the output aliases an input");
    const Geom3 g = fluid3d_geom(B, D, H, W, pitch_c, pitch_v, dt);
    return check_launch(launch3_flow_map(g, pitch_m, direction, u, v, w, disp_in, disp_out, (hipStream_t)stream), "flow_map3d_step");
}

int64_t smk_ftle3d_workspace(int32_t B, int32_t D, int32_t H, int32_t W) {
    if (!fm3_shape_ok(B, D, H, W, W, W + 1, W)) return -1;
    return fm3_workspace_bytes(B, D, H);
}

int smk_ftle3d_field(const float *disp, float *ftle, double *stats, int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_m,
                     double horizon, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(disp && ftle && stats, "ftle3d_field: null pointer");
    SMK_REQUIRE(fm3_shape_ok(B, D, H, W, W, W + 1, pitch_m), FM3_SHAPE);
    SMK_REQUIRE(horizon > 0.0 && (float)(2.0 * horizon) > 0.f && isfinite((float)(2.0 * horizon)),
                "ftle3d_field: horizon > 0 (and finite as fp32)");
    SMK_REQUIRE(ftle != disp, "ftle3d_field: the output aliases the input");
    SMK_REQUIRE(workspace && workspace_bytes >= smk_ftle3d_workspace(B, D, H, W),
                "ftle3d_field: workspace smaller than smk_ftle3d_workspace(B, D, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "ftle3d_field: workspace and stats must be 8-byte aligned");
    const Geom3 g = fluid3d_geom(B, D, H, W, pitch_m, W + 1, 0.0);
    return check_launch(launch3_ftle(g, pitch_m, (float)(2.0 * horizon), disp, ftle, stats, (double *)workspace, (hipStream_t)stream),
                        "ftle3d_field");
}

}  // extern "C"
#pragma GCC visibility pop
