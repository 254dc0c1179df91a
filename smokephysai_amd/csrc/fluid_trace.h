// The 2-D advection's back-trace as the derivative kernels re-form it: included by csrc/fluid_grad.hip (adjoint) and
// csrc/fluid_tangent.hip (tangent, section 3.11) only.  Positions, indices, clamp decisions and weights are formed by the forward's own
// expressions (csrc/stencil.hip: bilinear, k_advect; the build keeps -ffp-contract=off), so they are the forward's bit for bit.  Also the
// host-side geometry and shape check the two files' entry points share.
#pragma once
#include "common.h"

#include <math.h>

namespace smk {

// What every entry point of the two files takes: NavierStokesSimulator's shapes, within the launch grid's and the tap packing's reach.
inline bool fluid2d_shape_ok(int32_t B, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v) {
    return B >= 1 && B <= 65535 && H >= 3 && W >= 3 && H <= 32766 && W <= 32766 && pitch_c >= W && pitch_v >= W + 1;
}
inline Geom fluid2d_geom(int32_t B, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, double viscosity) {
    Geom g{};
    g.B = B; g.H = H; g.W = W; g.pc = pitch_c; g.pv = pitch_v;
    g.su = (size_t)(H + 1) * pitch_c; g.sv = (size_t)H * pitch_v; g.sc = (size_t)H * pitch_c;
    g.dt = (float)dt;
    g.coef_uv = (float)(dt * viscosity);
    g.coef_d = (float)(dt * (viscosity * 0.1));
    return g;
}

namespace {          // (per translation unit, as the two files kept them: the stepper has helpers of the same names)

__device__ __forceinline__ float clampf(float x, float lo, float hi) {
    float t = x < lo ? lo : x;   // torch.clamp = min(max(x, lo), hi)
    return t > hi ? hi : t;
}
__device__ __forceinline__ int clampi(int x, int lo, int hi) {
    int t = x < lo ? lo : x;
    return t > hi ? hi : t;
}

// bilinear_interpolate's taps and weights (navier_stokes.py:111-131) exactly as csrc/stencil.hip's bilinear() forms them: the clamped
// indices, and the element offsets of (y0,x0), (y0,x1), (y1,x0), (y1,x1) in a plane of the given pitch (a user keeps what it reads).
struct Taps {
    int x0, x1, y0, y1;
    size_t o00, o01, o10, o11;
    float wa, wb, wc, wd;        // weights of (y0,x0), (y0,x1), (y1,x0), (y1,x1)
    float fx0, fx1, fy0, fy1;
};
__device__ __forceinline__ Taps taps_at(int h, int w, int pitch, float y, float x) {
    Taps t;
    int x0 = (int)floorf(x), y0 = (int)floorf(y);
    int x1 = x0 + 1, y1 = y0 + 1;
    t.x0 = clampi(x0, 0, w - 1); t.x1 = clampi(x1, 0, w - 1);
    t.y0 = clampi(y0, 0, h - 1); t.y1 = clampi(y1, 0, h - 1);
    t.fx0 = (float)t.x0; t.fx1 = (float)t.x1; t.fy0 = (float)t.y0; t.fy1 = (float)t.y1;
    t.wa = (t.fx1 - x) * (t.fy1 - y);
    t.wb = (x - t.fx0) * (t.fy1 - y);
    t.wc = (t.fx1 - x) * (y - t.fy0);
    t.wd = (x - t.fx0) * (y - t.fy0);
    t.o00 = (size_t)t.y0 * pitch + t.x0; t.o01 = (size_t)t.y0 * pitch + t.x1;
    t.o10 = (size_t)t.y1 * pitch + t.x0; t.o11 = (size_t)t.y1 * pitch + t.x1;
    return t;
}
// ((wa f00 + wb f01) + wc f10) + wd f11: bilinear()'s sum, in its order
__device__ __forceinline__ float gather(const float *f, const Taps &t) {
    float r = t.wa * f[t.o00] + t.wb * f[t.o01];
    r = r + t.wc * f[t.o10];
    r = r + t.wd * f[t.o11];
    return r;
}
// interpolate_velocity_u at the cell (Y, X) (navier_stokes.py:97-102): taps of u [H+1][W] at (Y, clamp(X + 0.5)); _v likewise (:104-109).
__device__ __forceinline__ Taps u_sample_taps(const Geom &g, int Y, int X) {
    return taps_at(g.H + 1, g.W, g.pc, (float)Y, clampf((float)X + 0.5f, 0.f, (float)(g.W - 1)));
}
__device__ __forceinline__ Taps v_sample_taps(const Geom &g, int Y, int X) {
    return taps_at(g.H, g.W + 1, g.pv, clampf((float)Y + 0.5f, 0.f, (float)(g.H - 1)), (float)X);
}

// Everything the derivative of out[Y][X] = adv(f; u, v)[Y][X] takes from the forward, for a destination cell of an [R][C] field of the
// given pitch (ub, vb, fb: the grid's planes).
struct Trace {
    Taps su, sv;                 // the velocity samples' taps
    float ui, vi;                // ... and values
    float pxu, pyu, px, py;      // the back-trace before and after its clamp (navier_stokes.py:87-92)
    bool pass_x, pass_y;         // the clamp passes its derivative where lo <= x <= hi, bounds included (torch's convention)
    Taps t;                      // the field's taps at (py, px)
    float sx, sy;                // d out / d px, d out / d py: the derivatives of the weights as written, from the clamped indices (on
                                 // the upper-edge quirk, x0 == x1, both values are the same element and the slope is an exact 0)
};
__device__ __forceinline__ Trace trace_at(const Geom &g, int R, int C, int pitch, const float *ub, const float *vb, const float *fb,
                                          int Y, int X) {
    Trace r;
    const float fY = (float)Y, fX = (float)X;
    r.su = u_sample_taps(g, Y, X);
    r.sv = v_sample_taps(g, Y, X);
    r.ui = gather(ub, r.su);
    r.vi = gather(vb, r.sv);
    r.pxu = fX - g.dt * r.ui; r.pyu = fY - g.dt * r.vi;
    const float hx = (float)(C - 1), hy = (float)(R - 1);
    r.px = clampf(r.pxu, 0.f, hx); r.py = clampf(r.pyu, 0.f, hy);
    r.pass_x = r.pxu >= 0.f && r.pxu <= hx; r.pass_y = r.pyu >= 0.f && r.pyu <= hy;
    r.t = taps_at(R, C, pitch, r.py, r.px);
    const float f00 = fb[r.t.o00], f01 = fb[r.t.o01], f10 = fb[r.t.o10], f11 = fb[r.t.o11];
    r.sx = (r.t.fy1 - r.py) * (f01 - f00) + (r.py - r.t.fy0) * (f11 - f10);
    r.sy = (r.t.fx1 - r.px) * (f10 - f00) + (r.px - r.t.fx0) * (f11 - f01);
    return r;
}

}  // namespace

}  // namespace smk
