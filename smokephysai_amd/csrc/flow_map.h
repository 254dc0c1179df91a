// Flow-map kernels of the 2-D stepper (csrc/flow_map.hip): launch functions behind smk_flow_map_step and smk_ftle_field
// (include/smokehip.h), and the staggered velocity samples at a general position, which only the forward map needs.  DESIGN.md section
// 3.14 has the rule.
#pragma once
#include "common.h"
#include "fluid_tangent.h"
#include "fluid_trace.h"

namespace smk {

constexpr int FM_BACKWARD = 0, FM_FORWARD = 1;

// smk_ftle_field deals a grid's H rows to P workgroups in runs of consecutive rows, as smk_tangent_renorm deals a tangent's: a run has at
// least FT_ROWS rows and a grid at most FT_MAX_P runs.
inline int fm_rows_per_group(int H) {
    const int most = cdiv(H, FT_MAX_P);
    return most > FT_ROWS ? most : FT_ROWS;
}
inline int fm_groups(int H) { return cdiv(H, fm_rows_per_group(H)); }

// disp [B][2][H][pm] -> out likewise; dir: FM_BACKWARD / FM_FORWARD.  One launch.
hipError_t launch_flow_map(const Geom &g, int pm, int dir, const float *u, const float *v, const float *disp, float *out, hipStream_t st);
// disp [B][2][H][pm] -> ftle [B][H][pm], stats [B][2] (mean, max).  partial: g.B * fm_groups(g.H) * 2 doubles.  Two launches.
hipError_t launch_ftle(const Geom &g, int pm, float two_horizon, const float *disp, float *ftle, double *stats, double *partial,
                       hipStream_t st);
// Level two of the FTLE's statistics, shared with csrc/flow_map3d.hip: partial [B][P][2] (sum, max) -> stats [B][2] (sum / cells, max),
// one thread per grid, the P runs in ascending order.  One launch.
hipError_t launch_ftle_stats(int B, int P, double cells, const double *partial, double *stats, hipStream_t st);

namespace {

// d f / d i at unit spacing, f pointing at element i of n, `stride` elements apart: central with a factor 0.5 inside, one-sided at both ends.
__device__ __forceinline__ float diff_at(const float *f, int i, int n, size_t stride) {
    if (i == 0) return f[stride] - f[0];
    if (i == n - 1) return f[0] - *(f - stride);
    return 0.5f * (f[stride] - *(f - stride));
}
// max in which a NaN wins (torch's convention), so a grid holding one reports it
__device__ __forceinline__ double nanmax(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}

// interpolate_velocity_u / _v (navier_stokes.py:97-109) at a position (y, x) in cells, as csrc/stencil.hip's k_interp forms them: the
// +0.5 shift along the axis the component acts on, that coordinate clamped to the component's extent, then bilinear()'s taps.  (The other
// coordinate comes clamped to the cell grid, which lies inside the component's extent: its clamp would change nothing.)
__device__ __forceinline__ Taps u_taps_at(const Geom &g, float y, float x) {
    return taps_at(g.H + 1, g.W, g.pc, y, clampf(x + 0.5f, 0.f, (float)(g.W - 1)));
}
__device__ __forceinline__ Taps v_taps_at(const Geom &g, float y, float x) {
    return taps_at(g.H, g.W + 1, g.pv, clampf(y + 0.5f, 0.f, (float)(g.H - 1)), x);
}

}  // namespace

}  // namespace smk
