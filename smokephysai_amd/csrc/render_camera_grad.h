#pragma once
#include "camera_grad_plan.h"
#include "render.h"

namespace smk {

// Workspace bytes of the free-camera render's gradient.  SMK_LIGHT_NONE: K alone, one value per ray of the scratch's marched rows.
// SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y: the prefix along y and U, n*D*H*W floats each, then the banded per-sample scratch of
// camera_grad_plan (at most 256 MiB).  The same for any number of views.
int64_t render_camera_backward_workspace(int64_t n, int D, int H, int W, int light);

// views: n * n_views coefficient sets on the host, volume-major.  G / Gt: planes v * n_views + k, either may be null (= zero).  out: dense
// [D][H][W] volumes ostride floats apart, every element written (view 0 writes, later views add in ascending order).
hipError_t launch_volume_render_camera_backward(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light,
                                                const RenderParams &p, const CameraView *views, int n_views, const float *G, int64_t gstride,
                                                const float *Gt, int64_t tstride, float *out, int64_t ostride, float *workspace,
                                                hipStream_t st);

}  // namespace smk
