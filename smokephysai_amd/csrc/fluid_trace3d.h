// The 3-D advection's back-trace as the tangent kernel re-forms it: included by csrc/fluid_tangent3d.hip; the
// counterpart of csrc/fluid_trace.h.  Positions, indices, clamp decisions, weights and slopes are formed by the forward's own expressions
// (csrc/stencil3d.hip: vel3_at, interp3, k3_advect; stencil3d.h: clampf3; the build keeps -ffp-contract=off) and, for the slopes, by
// k3_advect_backward's (csrc/fluid_grad3d.hip, which keeps its own copy of the same text), so they are the forward's and the adjoint's
// bit for bit.  Also the host-side geometry and shape check of the file's entry points.
#pragma once
#include "stencil3d.h"

#include <math.h>

namespace smk {

// What every 3-D derivative entry point takes: smk_sim3d_create's shapes (csrc/fluid_grad3d.hip: fg3_shape_ok).
inline bool fluid3d_shape_ok(int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v) {
    return B >= 1 && D >= 3 && H >= 3 && W >= 3 && D <= 32766 && H <= 32766 && W <= 32766 && pitch_c >= W && pitch_v >= W + 1 &&
           (int64_t)B * (D + 1) <= 65535 && (int64_t)(D + 1) * (H + 1) * pitch_v < (1LL << 31) &&
           (int64_t)(D + 1) * (H + 1) * pitch_c < (1LL << 31);
}
inline Geom3 fluid3d_geom(int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, double dt) {
    Geom3 g{};
    g.B = B; g.D = D; g.H = H; g.W = W; g.pc = pitch_c; g.pv = pitch_v;
    g.su = (size_t)D * (H + 1) * pitch_c; g.sv = (size_t)D * H * pitch_v; g.sw = (size_t)(D + 1) * H * pitch_c;
    g.sc = (size_t)D * H * pitch_c;
    g.dt = (float)dt;
    g.sixth = (float)(1.0 / 6.0);
    return g;
}

namespace {

// csrc/stencil3d.hip's vel3_at in two halves: where the sample taps (the guard: every index <= extent - 2, else the sample is exactly 0)
// and the element offset of its low tap, then 0.5 c[o] + 0.5 c[o + step] -- so the tangent velocities are sampled at the same two
// elements, in the same order, without forming the guard again.
struct Vel3Taps {
    bool live;
    int o, step;
};
template <int ACT>
__device__ __forceinline__ Vel3Taps vel3_taps(int Dc, int Hc, int Wc, int pitch, int z, int y, int x) {
    Vel3Taps t;
    t.live = !(z > Dc - 2 || y > Hc - 2 || x > Wc - 2);
    t.o = t.live ? (z * Hc + y) * pitch + x : 0;                 // in-grid offsets fit 32 bits (the shape check)
    t.step = ACT == 2 ? 1 : (ACT == 1 ? pitch : Hc * pitch);
    return t;
}
__device__ __forceinline__ float vel3_sample(const float *c, const Vel3Taps &t) {
    if (!t.live) return 0.f;
    return 0.5f * c[t.o] + 0.5f * c[t.o + t.step];
}

// Everything the derivative of out[Z][Y][X] = adv(f; u, v, w)[Z][Y][X] takes from the forward, for a destination cell of a
// [Df][Hf][Wf] field of the given pitch (ub, vb, wb, fb: the grid's volumes).
struct Trace3 {
    Vel3Taps su, sv, sw;         // the velocity samples' taps
    bool pass_x, pass_y, pass_z; // the clamp passes its derivative where lo <= x <= hi, bounds included (torch's convention)
    int o[8];                    // interp3's taps: element offsets, z-low plane first, x fastest, low before high
    float wt[8];                 // ... and weights (wx * wy) * wz
    float sx, sy, sz;            // d out / d px, py, pz: k3_advect_backward's four-term slopes of the interpolant
};
__device__ __forceinline__ Trace3 trace3_at(const Geom3 &g, int Df, int Hf, int Wf, int pitch, const float *ub, const float *vb,
                                            const float *wb, const float *fb, int Z, int Y, int X) {
    Trace3 r;
    r.su = vel3_taps<2>(g.D, g.H + 1, g.W, g.pc, Z, Y, X);
    r.sv = vel3_taps<1>(g.D, g.H, g.W + 1, g.pv, Z, Y, X);
    r.sw = vel3_taps<0>(g.D + 1, g.H, g.W, g.pc, Z, Y, X);
    const float ui = vel3_sample(ub, r.su), vi = vel3_sample(vb, r.sv), wi = vel3_sample(wb, r.sw);
    const float tx = g.dt * ui, ty = g.dt * vi, tz = g.dt * wi;
    const float pxu = (float)X - tx, pyu = (float)Y - ty, pzu = (float)Z - tz;                // k3_advect, before the clamp
    const float hx = (float)(Wf - 1), hy = (float)(Hf - 1), hz = (float)(Df - 1);
    const float px = clampf3(pxu, 0.f, hx), py = clampf3(pyu, 0.f, hy), pz = clampf3(pzu, 0.f, hz);
    r.pass_x = pxu >= 0.f && pxu <= hx; r.pass_y = pyu >= 0.f && pyu <= hy; r.pass_z = pzu >= 0.f && pzu <= hz;
    int x0 = (int)floorf(px), y0 = (int)floorf(py), z0 = (int)floorf(pz);                     // interp3
    int x1 = x0 + 1, y1 = y0 + 1, z1 = z0 + 1;
    x0 = clampi3(x0, 0, Wf - 1); x1 = clampi3(x1, 0, Wf - 1);
    y0 = clampi3(y0, 0, Hf - 1); y1 = clampi3(y1, 0, Hf - 1);
    z0 = clampi3(z0, 0, Df - 1); z1 = clampi3(z1, 0, Df - 1);
    const float wx0 = (float)x1 - px, wx1 = px - (float)x0;
    const float wy0 = (float)y1 - py, wy1 = py - (float)y0;
    const float wz0 = (float)z1 - pz, wz1 = pz - (float)z0;
    const int r00 = (z0 * Hf + y0) * pitch, r01 = (z0 * Hf + y1) * pitch;
    const int r10 = (z1 * Hf + y0) * pitch, r11 = (z1 * Hf + y1) * pitch;
    r.o[0] = r00 + x0; r.o[1] = r00 + x1; r.o[2] = r01 + x0; r.o[3] = r01 + x1;
    r.o[4] = r10 + x0; r.o[5] = r10 + x1; r.o[6] = r11 + x0; r.o[7] = r11 + x1;
    r.wt[0] = (wx0 * wy0) * wz0; r.wt[1] = (wx1 * wy0) * wz0; r.wt[2] = (wx0 * wy1) * wz0; r.wt[3] = (wx1 * wy1) * wz0;
    r.wt[4] = (wx0 * wy0) * wz1; r.wt[5] = (wx1 * wy0) * wz1; r.wt[6] = (wx0 * wy1) * wz1; r.wt[7] = (wx1 * wy1) * wz1;
    const float f000 = fb[r.o[0]], f001 = fb[r.o[1]], f010 = fb[r.o[2]], f011 = fb[r.o[3]];
    const float f100 = fb[r.o[4]], f101 = fb[r.o[5]], f110 = fb[r.o[6]], f111 = fb[r.o[7]];
    // slope of the interpolant along an axis: the other two axes' weights times (f_hi - f_lo), z-low plane first
    float sx = (wy0 * wz0) * (f001 - f000);
    sx = sx + (wy1 * wz0) * (f011 - f010);
    sx = sx + (wy0 * wz1) * (f101 - f100);
    sx = sx + (wy1 * wz1) * (f111 - f110);
    float sy = (wx0 * wz0) * (f010 - f000);
    sy = sy + (wx1 * wz0) * (f011 - f001);
    sy = sy + (wx0 * wz1) * (f110 - f100);
    sy = sy + (wx1 * wz1) * (f111 - f101);
    float sz = (wx0 * wy0) * (f100 - f000);
    sz = sz + (wx1 * wy0) * (f101 - f001);
    sz = sz + (wx0 * wy1) * (f110 - f010);
    sz = sz + (wx1 * wy1) * (f111 - f011);
    r.sx = sx; r.sy = sy; r.sz = sz;
    return r;
}
// interp3's eight-term sum over a volume at the trace's taps, in its order
__device__ __forceinline__ float gather3(const float *f, const Trace3 &t) {
    float acc = t.wt[0] * f[t.o[0]];
#pragma unroll
    for (int i = 1; i < 8; ++i) acc = acc + t.wt[i] * f[t.o[i]];
    return acc;
}

}  // namespace

}  // namespace smk
