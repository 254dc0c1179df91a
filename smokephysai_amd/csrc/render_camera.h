#pragma once
#include "camera_plan.h"
#include "render.h"

namespace smk {

constexpr int CAMERA_VIEWS_PER_LAUNCH = 16;    // view coefficient sets that travel as launch arguments

// workspace: render_prefix_workspace (render.h).  views: n * n_views coefficient sets on the host, volume-major.  Plane v * n_views + k of image / trans is view k of volume v.
hipError_t launch_volume_render_camera(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                       const CameraView *views, int n_views, float *image, int64_t image_stride, float *trans,
                                       int64_t trans_stride, float *workspace, hipStream_t st);

}  // namespace smk
