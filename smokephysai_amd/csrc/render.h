#pragma once
#include "common.h"

namespace smk {

constexpr int RENDER_MAX_DEPTH = 64;      // planes one lane keeps a running light sum for (registers)
constexpr int RENDER_SEG_ROWS = 16;       // rows per segment of the +-y light prefix (render.py: SEGMENT_ROWS)

// the settings of smk_render_desc, cast once on the host
struct RenderParams {
    float neg_sigma_view, neg_sigma_light, ambient, one_minus_ambient, gain;
};

// bytes of the segment-total workspace: 0 unless the light travels along y and the rows span more than one segment
int64_t render_workspace(int64_t n, int D, int H, int W, int light);
hipError_t launch_volume_render(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                float *image, int64_t image_stride, float *trans, int64_t trans_stride, float *workspace, hipStream_t st);

// the gradient of image and transmittance with respect to the volumes (G / Gt: their upstream gradients, either may be null = zero).
// Workspace bytes: 0 unless the light travels along y; then three segment arrays [n][segments][D][W] (also for one segment) + [n][H][W].
int64_t render_backward_workspace(int64_t n, int D, int H, int W, int light);
hipError_t launch_volume_render_backward(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                         const float *G, int64_t gstride, const float *Gt, int64_t tstride, float *out, int64_t ostride,
                                         float *workspace, hipStream_t st);

}  // namespace smk
