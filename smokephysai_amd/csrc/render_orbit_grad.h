#pragma once
#include "orbit_grad_plan.h"
#include "render.h"

namespace smk {

// Workspace bytes of the orbit render's gradient.  SMK_LIGHT_NONE: K alone, min(n, 16) * H * W floats (one value per ray of at most 16
// volumes at one view), cut to 256 MiB.  SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y: the prefix along y and U, n*D*H*W floats each, then the
// per-sample scratch of orbit_grad_plan (at most 256 MiB).  The same for any number of views.
int64_t render_orbit_backward_workspace(int64_t n, int D, int H, int W, int light);

// cs: n * n_views (cos, sin) pairs on the host, volume-major.  G / Gt: planes v * n_views + k, either may be null (= zero).  out: dense
// [D][H][W] volumes ostride floats apart, every element written (view 0 writes, later views add in ascending order).
hipError_t launch_volume_render_orbit_backward(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light,
                                               const RenderParams &p, const float *cs, int n_views, const float *G, int64_t gstride,
                                               const float *Gt, int64_t tstride, float *out, int64_t ostride, float *workspace, hipStream_t st);

}  // namespace smk
