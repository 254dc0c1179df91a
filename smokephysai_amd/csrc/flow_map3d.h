// Flow-map kernels of the 3-D stepper (csrc/flow_map3d.hip): launch functions behind smk_flow_map3d_step and smk_ftle3d_field
// (include/smokehip.h), the back-trace record the backward map needs, and the staggered trilinear samples at a general position, which
// only the forward map needs.  DESIGN.md section 3.15 has the rule; the 3-D counterpart of csrc/flow_map.h.
//
// The first part is plain C++ for host and device: the row map and the group rule of smk_ftle3d_field, which the kernel, the launcher,
// the workspace query and the stand-alone host check (tests/host/ftle3d_rows_main.cpp) all compile.  The rest needs the HIP compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FM3_HD __host__ __device__ inline
#else
#define FM3_HD inline
#endif

namespace smk {

// smk_ftle3d_field: a grid's D H rows of W cells, planes before rows, are dealt to P workgroups in runs of consecutive rows, as
// smk_tangent3d_renorm deals a tangent state's: a run has at least FM3_ROWS rows and a grid at most FM3_MAX_P runs (level two adds the
// runs one after another in one thread, so their number is kept small).
constexpr int FM3_ROWS = 16, FM3_MAX_P = 256;

FM3_HD int64_t fm3_rows(int D, int H) { return (int64_t)D * H; }
FM3_HD int fm3_rows_per_group(int D, int H) {
    const int64_t most = (fm3_rows(D, H) + FM3_MAX_P - 1) / FM3_MAX_P;
    return most > FM3_ROWS ? (int)most : FM3_ROWS;
}
FM3_HD int fm3_groups(int D, int H) {
    const int rpg = fm3_rows_per_group(D, H);
    return (int)((fm3_rows(D, H) + rpg - 1) / rpg);
}
// The workspace of smk_ftle3d_field: per grid and run one (sum, maximum) pair of doubles.
FM3_HD int64_t fm3_workspace_bytes(int B, int D, int H) { return (int64_t)B * fm3_groups(D, H) * 2 * (int64_t)sizeof(double); }

// Row r of a grid, 0 <= r < fm3_rows(D, H): its plane and row, and the element offset of its first cell within one volume
// [D][H][pitch_m] (a displacement component's, or the FTLE's).
struct Fm3Row {
    int plane, row;
    int64_t offset;
};
FM3_HD Fm3Row fm3_row(int H, int pitch_m, int64_t r) {
    Fm3Row q;
    q.plane = (int)(r / H);
    q.row = (int)(r % H);
    q.offset = r * pitch_m;                       // (plane * H + row) * pitch_m
    return q;
}

// What both entry points ask of pitch_m beside fluid3d_shape_ok: rows that hold their W cells, and in-volume offsets within 31 bits.
FM3_HD bool fm3_pitch_ok(int D, int H, int W, int pitch_m) { return pitch_m >= W && (int64_t)D * H * pitch_m < (1LL << 31); }

}  // namespace smk

#if defined(__HIPCC__)
#include "flow_map.h"
#include "fluid_tangent3d.h"
#include "fluid_trace3d.h"

namespace smk {

// disp [B][3][D][H][pm] -> out likewise; dir: FM_BACKWARD / FM_FORWARD.  One launch, on fluid_tangent3d.h's 32 x 8 tile.
hipError_t launch3_flow_map(const Geom3 &g, int pm, int dir, const float *u, const float *v, const float *w, const float *disp, float *out,
                            hipStream_t st);
// disp [B][3][D][H][pm] -> ftle [B][D][H][pm], stats [B][2] (mean, max).  partial: g.B * fm3_groups(g.D, g.H) * 2 doubles.  Two launches.
hipError_t launch3_ftle(const Geom3 &g, int pm, float two_horizon, const float *disp, float *ftle, double *stats, double *partial,
                        hipStream_t st);

namespace {

// interp3's eight taps and weights (csrc/stencil3d.hip; the text of fluid_trace3d.h's trace3_at) at a position (pz, py, px) in a
// [Df][Hf][Wf] volume of the given pitch: floor, the INDICES clamped, weights from the clamped indices -- so any position, NaN and +-inf
// included, taps inside the volume, and a position on the last index reads 0.  Element offsets z-low plane first, x fastest, low before
// high; weights (wx * wy) * wz.
struct Taps3 {
    int o[8];
    float wt[8];
};
__device__ __forceinline__ Taps3 taps3_at(int Df, int Hf, int Wf, int pitch, float pz, float py, float px) {
    Taps3 r;
    int x0 = (int)floorf(px), y0 = (int)floorf(py), z0 = (int)floorf(pz);
    int x1 = x0 + 1, y1 = y0 + 1, z1 = z0 + 1;
    x0 = clampi3(x0, 0, Wf - 1); x1 = clampi3(x1, 0, Wf - 1);
    y0 = clampi3(y0, 0, Hf - 1); y1 = clampi3(y1, 0, Hf - 1);
    z0 = clampi3(z0, 0, Df - 1); z1 = clampi3(z1, 0, Df - 1);
    const float wx0 = (float)x1 - px, wx1 = px - (float)x0;
    const float wy0 = (float)y1 - py, wy1 = py - (float)y0;
    const float wz0 = (float)z1 - pz, wz1 = pz - (float)z0;
    const int r00 = (z0 * Hf + y0) * pitch, r01 = (z0 * Hf + y1) * pitch;           // in-volume offsets fit 32 bits (the shape check)
    const int r10 = (z1 * Hf + y0) * pitch, r11 = (z1 * Hf + y1) * pitch;
    r.o[0] = r00 + x0; r.o[1] = r00 + x1; r.o[2] = r01 + x0; r.o[3] = r01 + x1;
    r.o[4] = r10 + x0; r.o[5] = r10 + x1; r.o[6] = r11 + x0; r.o[7] = r11 + x1;
    r.wt[0] = (wx0 * wy0) * wz0; r.wt[1] = (wx1 * wy0) * wz0; r.wt[2] = (wx0 * wy1) * wz0; r.wt[3] = (wx1 * wy1) * wz0;
    r.wt[4] = (wx0 * wy0) * wz1; r.wt[5] = (wx1 * wy0) * wz1; r.wt[6] = (wx0 * wy1) * wz1; r.wt[7] = (wx1 * wy1) * wz1;
    return r;
}
// interp3's eight-term sum over a volume at those taps, in its order
__device__ __forceinline__ float gather3(const float *f, const Taps3 &t) {
    float acc = t.wt[0] * f[t.o[0]];
#pragma unroll
    for (int i = 1; i < 8; ++i) acc = acc + t.wt[i] * f[t.o[i]];
    return acc;
}

// What the backward map takes from the density advection of cell (Z, Y, X): trace3_at's expressions (vel3_taps, vel3_sample, clampf3,
// the clamp decisions) up to the clamped position, and with them what Trace3 does not keep -- the moves dt * sample and the clamped
// position -- but no slopes, so no field is loaded for them.  The taps of the position are taps3_at(g.D, g.H, g.W, pm, pz, py, px).
struct MapTrace3 {
    float tx, ty, tz;            // dt * (ui, vi, wi)
    float px, py, pz;            // the clamped back-trace position
    bool pass_x, pass_y, pass_z; // lo <= unclamped position <= hi, bounds included
};
__device__ __forceinline__ MapTrace3 map_trace3_at(const Geom3 &g, const float *ub, const float *vb, const float *wb, int Z, int Y, int X) {
    MapTrace3 r;
    const Vel3Taps su = vel3_taps<2>(g.D, g.H + 1, g.W, g.pc, Z, Y, X);
    const Vel3Taps sv = vel3_taps<1>(g.D, g.H, g.W + 1, g.pv, Z, Y, X);
    const Vel3Taps sw = vel3_taps<0>(g.D + 1, g.H, g.W, g.pc, Z, Y, X);
    const float ui = vel3_sample(ub, su), vi = vel3_sample(vb, sv), wi = vel3_sample(wb, sw);
    r.tx = g.dt * ui; r.ty = g.dt * vi; r.tz = g.dt * wi;
    const float pxu = (float)X - r.tx, pyu = (float)Y - r.ty, pzu = (float)Z - r.tz;           // k3_advect, before the clamp
    const float hx = (float)(g.W - 1), hy = (float)(g.H - 1), hz = (float)(g.D - 1);
    r.px = clampf3(pxu, 0.f, hx); r.py = clampf3(pyu, 0.f, hy); r.pz = clampf3(pzu, 0.f, hz);
    r.pass_x = pxu >= 0.f && pxu <= hx; r.pass_y = pyu >= 0.f && pyu <= hy; r.pass_z = pzu >= 0.f && pzu <= hz;
    return r;
}

// A staggered component sampled at a general position (qz, qy, qx) of the cell grid, as the rule's _sample forms it (SPEC_3D.md
// section 5): +0.5 along the axis the component acts on (ACT: 0 = z, 1 = y, 2 = x, vel3_taps' constants), that coordinate clamped to
// the component's extent [Dc][Hc][Wc], then interp3's taps.  (The other two coordinates come clamped to the cell grid, which lies inside
// the component's extent: their clamps would change nothing, a NaN included.)
template <int ACT>
__device__ __forceinline__ Taps3 stag3_taps_at(int Dc, int Hc, int Wc, int pitch, float qz, float qy, float qx) {
    if (ACT == 0) qz = clampf3(qz + 0.5f, 0.f, (float)(Dc - 1));
    if (ACT == 1) qy = clampf3(qy + 0.5f, 0.f, (float)(Hc - 1));
    if (ACT == 2) qx = clampf3(qx + 0.5f, 0.f, (float)(Wc - 1));
    return taps3_at(Dc, Hc, Wc, pitch, qz, qy, qx);
}

}  // namespace

}  // namespace smk
#endif
