#pragma once
#include "common.h"

namespace smk {

constexpr int RENDER_MAX_DEPTH = 64;      // planes one lane keeps a running light sum for (registers)
constexpr int RENDER_SEG_ROWS = 16;       // rows per segment of the +-y light prefix (render.py: SEGMENT_ROWS)

// the settings of smk_render_desc, cast once on the host
struct RenderParams {
    float neg_sigma_view, neg_sigma_light, ambient, one_minus_ambient, gain;
};

// ---- device helpers shared by render.hip and render_orbit.hip
// Smoke volumes are mostly empty (the stepper's are 99.9 % zeros after 20 steps).  A voxel with rho == 0 adds (0 * L) * T = 0 exactly as
// long as L and T are finite, which A >= 0 and tau >= 0 guarantee (both factors are then in [0, 1]); with negative or NaN sums behind it the
// term is formed as written.  A wave whose 64 voxels are all of that kind skips the term: same bits, no exp.
__device__ __forceinline__ bool wave_has_term(float rho, float A, float tau) {
    return __builtin_amdgcn_ballot_w64(!(rho == 0.f && A >= 0.f && tau >= 0.f)) != 0;
}

// one term of the image sum
__device__ __forceinline__ float render_term(float rho, float A, float tau, const RenderParams &p, bool lit) {
    const float alpha = -expm1f(p.neg_sigma_view * rho);
    const float L = lit ? p.ambient + p.one_minus_ambient * __expf(p.neg_sigma_light * A) : 1.0f;
    return (alpha * L) * __expf(p.neg_sigma_view * tau);
}

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
