// Backward (adjoint) kernels of one 3-D stable-fluids step (csrc/fluid_grad3d.hip): launch functions behind smk_advect3d_backward,
// smk_project3d_backward and smk_buoy_diffuse3d_backward (include/smokehip.h).  DESIGN.md section 3.10 has the derivation.
#pragma once
#include "stencil3d.h"

namespace smk {

// The tile of source cells one workgroup of k3_advect_backward owns in every plane of its z-march, and the tile + one-cell halo of
// destination records it forms in LDS; the ring holds the records of three consecutive planes.
constexpr int FG3_TX = 32, FG3_TY = 8, FG3_NT = FG3_TX * FG3_TY;
constexpr int FG3_HX = FG3_TX + 2, FG3_HY = FG3_TY + 2, FG3_REC = FG3_HX * FG3_HY, FG3_RING = 3;
// The projection's backward: transposed Jacobi sweeps per launch, and the brick of cells a workgroup keeps in LDS meanwhile.
constexpr int FG3_PB_T = 2, FG3_PB_Z = 8, FG3_PB_Y = 8, FG3_PB_X = 32;

// which: 0 field = u-shaped, 1 v-shaped, 2 w-shaped, 3 cell-shaped with the 0.995 decay folded into gout.  far: int32 [B], cleared here
// first.  One kernel launch.
hipError_t launch3_advect_backward(const Geom3 &g, int which, const float *field, const float *u, const float *v, const float *w,
                                   const float *gout, float *dfield, float *du, float *dv, float *dw, int32_t *far, hipStream_t st);
// ws: 3 * B * D * H * W floats (two volumes of lambda, one of ddiv).  ceil(iters / FG3_PB_T) + 2 launches.
hipError_t launch3_project_backward(const Geom3 &g, const float *gu, const float *gv, const float *gw, const float *gp, float *du,
                                    float *dv, float *dw, float *dp, int iters, float *ws, hipStream_t st);
hipError_t launch3_buoy_diffuse_backward(const Geom3 &g, const float *gu, const float *gv, const float *gw, const float *gd, float *du,
                                         float *dv, float *dw, float *dd, hipStream_t st);

}  // namespace smk
