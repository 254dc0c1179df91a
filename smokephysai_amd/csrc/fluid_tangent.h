// Tangent-linear (forward-mode) kernels of one 2-D stable-fluids step (csrc/fluid_tangent.hip): launch functions behind smk_advect_tangent
// and smk_tangent_renorm (include/smokehip.h).  DESIGN.md section 3.11 has the rule.
#pragma once
#include "common.h"

namespace smk {

// The tile of destination cells one workgroup of k_advect_tangent owns: one thread per cell (k_advect_backward's tile).
constexpr int FT_TX = 32, FT_TY = 8, FT_NT = FT_TX * FT_TY;
// smk_tangent_renorm: a tangent's 4H + 1 rows (u, v, p, density, in that order) are dealt to P workgroups in runs of consecutive rows;
// a run has at least FT_ROWS rows and a tangent at most FT_MAX_P runs.
constexpr int FT_ROWS = 16, FT_MAX_P = 256;

inline int ft_rows_per_group(int H) {
    const int rows = 4 * H + 1, most = cdiv(rows, FT_MAX_P);
    return most > FT_ROWS ? most : FT_ROWS;
}
inline int ft_groups(int H) { return cdiv(4 * H + 1, ft_rows_per_group(H)); }

// g.B = the number of grids; tangents [B][T] planes.  which: 0 field = u-shaped, 1 v-shaped, 2 cell-shaped with the 0.995 decay.
hipError_t launch_advect_tangent(const Geom &g, int T, int which, const float *field, const float *u, const float *v, const float *tfield,
                                 const float *tu, const float *tv, float *tout, hipStream_t st);
// g.B = B * T tangent states.  partial: g.B * ft_groups(g.H) doubles.  Two launches.
hipError_t launch_tangent_renorm(const Geom &g, float *tu, float *tv, float *tp, float *td, double *norms, double *partial, hipStream_t st);

}  // namespace smk
