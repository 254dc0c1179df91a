// Orthonormalisation of the T tangent states of a grid by modified Gram-Schmidt (csrc/tangent_qr.hip): launch functions behind
// smk_tangent_orthonormalize and smk_tangent3d_orthonormalize (include/smokehip.h).  DESIGN.md section 3.13 has the rule.
//
// The row maps, the run length and the number of runs are smk_tangent_renorm's and smk_tangent3d_renorm's (fluid_tangent.h,
// fluid_tangent3d.h), so with T = 1 the two launches are those kernels' sums and divides, word for word.
#pragma once
#include "fluid_tangent.h"
#include "fluid_tangent3d.h"

namespace smk {

constexpr int TQ_MAX_T = 8;                      // at most 7 later vectors: 7 fp64 accumulators per thread, 7 * 256 doubles of LDS (14 KB)
constexpr int TQ_NT = 256;                       // = FT_NT = FT3_NT: the renorm kernels' workgroup

// Launches per call: the sum of squares of vector 0, then per vector its norm-scale-dots pass and (but for the last) the update pass.
inline int tq_launches(int T) { return 2 * T; }

// g.B = the number of grids; tangents [B][T] grids.  work: B * T * runs doubles (per grid: the runs' partial sums of squares of the
// current vector, then (T - 1) * runs partial dot products).
hipError_t launch_tangent_orthonormalize(const Geom &g, int T, float *tu, float *tv, float *tp, float *td, double *norms, double *work,
                                         hipStream_t st);
hipError_t launch3_tangent_orthonormalize(const Geom3 &g, int T, float *tu, float *tv, float *tw, float *tp, float *td, double *norms,
                                          double *work, hipStream_t st);

}  // namespace smk
