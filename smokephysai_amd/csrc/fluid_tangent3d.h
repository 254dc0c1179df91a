// Tangent-linear (forward-mode) kernels of one 3-D stable-fluids step (csrc/fluid_tangent3d.hip): launch functions behind
// smk_advect3d_tangent and smk_tangent3d_renorm (include/smokehip.h).  DESIGN.md section 3.12 has the rule; the 3-D counterpart of
// csrc/fluid_tangent.h.
//
// The first part is plain C++ for host and device: the row map and the group rule of smk_tangent3d_renorm, which the two kernels, the
// launcher, the workspace query and the stand-alone host check (tests/host/tangent3d_rows_main.cpp) all compile.  The launch functions
// below it need the HIP compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FT3_HD __host__ __device__ inline
#else
#define FT3_HD inline
#endif

namespace smk {

// smk_tangent3d_renorm: a tangent state's rows -- u's D (H + 1) of W, v's D H of W + 1, w's (D + 1) H of W, p's D H of W, density's D H of
// W, in that order, planes before rows within a field -- are dealt to P workgroups in runs of consecutive rows; a run has at least
// FT3_ROWS rows and a tangent at most FT3_MAX_P runs (smk_tangent_renorm's two constants: level two adds the runs one after another in
// one thread, so their number is kept small).
constexpr int FT3_ROWS = 16, FT3_MAX_P = 256;

FT3_HD int64_t ft3_rows(int D, int H) {
    return (int64_t)D * (H + 1) + (int64_t)D * H + (int64_t)(D + 1) * H + 2 * (int64_t)D * H;
}
FT3_HD int ft3_rows_per_group(int D, int H) {
    const int64_t most = (ft3_rows(D, H) + FT3_MAX_P - 1) / FT3_MAX_P;
    return most > FT3_ROWS ? (int)most : FT3_ROWS;
}
FT3_HD int ft3_groups(int D, int H) {
    const int rpg = ft3_rows_per_group(D, H);
    return (int)((ft3_rows(D, H) + rpg - 1) / rpg);
}

// Row r of a tangent state, 0 <= r < ft3_rows(D, H): which field (0..4 = u, v, w, p, density), which plane and row of it, how many
// columns, and the element offset of the row's first column within the field's grid (pitch_c / pitch_v as the field asks).
struct Ft3Row {
    int field, plane, row, cols;
    int64_t offset;
};
FT3_HD Ft3Row ft3_row(int D, int H, int W, int pitch_c, int pitch_v, int64_t r) {
    const int64_t nu = (int64_t)D * (H + 1), nc = (int64_t)D * H, nw = (int64_t)(D + 1) * H;
    Ft3Row q;
    int rows_per_plane = H, pitch = pitch_c;
    q.cols = W;
    if (r < nu) { q.field = 0; rows_per_plane = H + 1; }
    else if ((r -= nu) < nc) { q.field = 1; q.cols = W + 1; pitch = pitch_v; }
    else if ((r -= nc) < nw) { q.field = 2; }
    else if ((r -= nw) < nc) { q.field = 3; }
    else { r -= nc; q.field = 4; }
    q.plane = (int)(r / rows_per_plane);
    q.row = (int)(r % rows_per_plane);
    q.offset = r * pitch;                       // (plane * rows_per_plane + row) * pitch
    return q;
}

}  // namespace smk

#if defined(__HIPCC__)
#include "stencil3d.h"

namespace smk {

// The tile of destination cells one workgroup of k3_advect_tangent owns in its plane: one thread per cell (k3_advect_backward's tile).
constexpr int FT3_TX = 32, FT3_TY = 8, FT3_NT = FT3_TX * FT3_TY;

// g.B = the number of grids; tangents [B][T] grids.  which: 0 field = u-shaped, 1 v-shaped, 2 w-shaped, 3 cell-shaped with the 0.995
// decay.  One launch.
hipError_t launch3_advect_tangent(const Geom3 &g, int T, int which, const float *field, const float *u, const float *v, const float *w,
                                  const float *tfield, const float *tu, const float *tv, const float *tw, float *tout, hipStream_t st);
// g.B = B * T tangent states.  partial: g.B * ft3_groups(g.D, g.H) doubles.  Two launches.
hipError_t launch3_tangent_renorm(const Geom3 &g, float *tu, float *tv, float *tw, float *tp, float *td, double *norms, double *partial,
                                  hipStream_t st);

}  // namespace smk
#endif
