// Backward (adjoint) kernels of one 2-D stable-fluids step (csrc/fluid_grad.hip): launch functions behind smk_advect_backward,
// smk_project_backward and smk_buoy_diffuse_backward (include/smokehip.h).  DESIGN.md section 3.9 has the derivation.
#pragma once
#include "common.h"

namespace smk {

// The tile of source cells one workgroup of k_advect_backward owns, and the tile + one-cell halo of destination records it forms in LDS.
constexpr int FG_TX = 32, FG_TY = 8, FG_NT = FG_TX * FG_TY;
constexpr int FG_HX = FG_TX + 2, FG_HY = FG_TY + 2, FG_REC = FG_HX * FG_HY;
// The projection's backward: transposed Jacobi sweeps per launch, and the square tile a workgroup keeps in LDS meanwhile.
constexpr int FG_PB_T = 4, FG_PB_TILE = 32;

// which: 0 field = u-shaped, 1 v-shaped, 2 cell-shaped with the 0.995 decay folded into gout.  far: int32 [B], cleared here first.
hipError_t launch_advect_backward(const Geom &g, int which, const float *field, const float *u, const float *v, const float *gout,
                                  float *dfield, float *du, float *dv, int32_t *far, hipStream_t st);
// ws: 3 * B * H * W floats (two planes of lambda, one of ddiv).  ceil(iters / FG_PB_T) + 2 launches.
hipError_t launch_project_backward(const Geom &g, const float *gu, const float *gv, const float *gp, float *du, float *dv, float *dp,
                                   int iters, float *ws, hipStream_t st);
hipError_t launch_buoy_diffuse_backward(const Geom &g, const float *gu, const float *gv, const float *gd, float *du, float *dv, float *dd,
                                        hipStream_t st);

}  // namespace smk
