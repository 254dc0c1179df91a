#pragma once
#include "orbit_plan.h"
#include "render.h"

namespace smk {

constexpr int ORBIT_VIEWS_PER_LAUNCH = 16;     // (cos, sin) pairs that travel as launch arguments

// workspace: render_prefix_workspace (render.h).  cs: n * n_views (cos, sin) pairs on the host, volume-major.  Plane v * n_views + k of image / trans is view k of volume v.
hipError_t launch_volume_render_orbit(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                      const float *cs, int n_views, float *image, int64_t image_stride, float *trans, int64_t trans_stride,
                                      float *workspace, hipStream_t st);

}  // namespace smk
