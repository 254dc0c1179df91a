#pragma once
#include <initializer_list>

#include "common.h"

namespace smk {

constexpr int RENDER_MAX_DEPTH = 64;      // planes one lane keeps a running light sum for (registers)
constexpr int RENDER_SEG_ROWS = 16;       // rows per segment of the +-y light prefix (render.py: SEGMENT_ROWS)

// the settings of smk_render_desc, cast once on the host
struct RenderParams {
    float neg_sigma_view, neg_sigma_light, ambient, one_minus_ambient, gain;
};

// ---- device helpers shared by render.hip, render_orbit.hip and render_camera.hip
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

// ---- the host-side checks that the four entry points share (smk_volume_render, _backward, _orbit, _camera)
constexpr int64_t RENDER_MAX_CELLS = (1LL << 31) - (1LL << 16);       // smk_volume_stats' limit: 32-bit offsets inside a volume
constexpr int64_t RENDER_MAX_PLANES = 1 << 20;                        // n * n_views of one call (the host forms a coefficient set for each)

// what one renderer is built for
struct RenderLimits {
    int max_depth, max_height, max_width;  // 0: the extent has no limit of its own
    const char *moving;                    // nullptr: the front view, every smk_light; else what the camera is called where the
                                           // world-fixed +z light is refused ("orbit views")
};

// one output or upstream-gradient buffer of n (n * n_views) planes, or of n volumes
struct RenderBuffer {
    const void *ptr;                       // may be null where the entry point allows it: then its stride is not looked at
    int64_t stride;
    bool volume;                           // at least D*H*W apart, not H*W
    const char *stride_name;
};

// n >= 1, the shape within `lim` and a light the renderer is built for: what the *_workspace queries answer -1 without
bool render_query_ok(const RenderLimits &lim, int32_t n, int32_t D, int32_t H, int32_t W, int32_t light);
// Everything between the entry point's null-pointer check and its angle checks, in that order: extents (n_views counts only for
// a moving camera), `lim`, the light and the ranges of desc, strides, 4-byte alignment.  `name`: the entry point without its "smk_".
// SMK_OK with *p filled, or the status with set_error called.
int render_check(const char *name, const RenderLimits &lim, int32_t n, int32_t D, int32_t H, int32_t W, int32_t n_views,
                 const smk_render_desc *desc, const void *vols, int64_t vol_stride, std::initializer_list<RenderBuffer> bufs,
                 const void *workspace, RenderParams *p);
// ... and the last one: `need` bytes of workspace are there
int render_check_workspace(const char *name, int64_t need, const void *workspace, int64_t workspace_bytes);
// what a failed launch leaves: SMK_OK, or SMK_ERR_HIP with "<name>: <hip's words>"
int render_launch_status(const char *name, hipError_t e);

// ---- the +-y light prefix on the voxel grid, for the renderers that interpolate it (render_orbit.hip, render_camera.hip)
// bytes: n volumes of D*H*W floats under SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y, 0 under SMK_LIGHT_NONE
int64_t render_prefix_workspace(int64_t n, int D, int H, int W, int light);
// workspace[v][z][y][x] = the sum of rho[z][y'][x] over the rows the light crosses before y (up: the light travels along +y)
hipError_t launch_render_prefix(const float *vols, int64_t stride, int64_t n, int D, int H, int W, bool up, float *workspace, hipStream_t st);
// The transpose, for the gradients of the moving cameras (render_orbit_grad.hip, render_camera_grad.hip): out[v][z][y][x] += the sum of
// U[v][z][y'][x] over the rows y' that y shadows, nearest row first.  U: n dense volumes; out: volumes ostride floats apart.
// render_grad_light_fits: the grid fits a launch (what a launcher asks before its first launch, so that an error leaves `out` untouched).
bool render_grad_light_fits(int64_t n, int D, int W);
hipError_t launch_render_grad_light(const float *U, float *out, int64_t ostride, int64_t n, int D, int H, int W, bool up, hipStream_t st);

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
