#pragma once
#include "orbit_plan.h"
#include "render.h"

namespace smk {

constexpr int ORBIT_VIEWS_PER_LAUNCH = 16;     // (cos, sin) pairs that travel as launch arguments

// bytes of the light-prefix workspace: n volumes of D*H*W floats under SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y, 0 under SMK_LIGHT_NONE
int64_t render_orbit_workspace(int64_t n, int D, int H, int W, int light);
// the +-y light prefix of n volumes on the voxel grid (k_orbit_prefix): workspace[v][z][y][x] = the sum of rho[z][y'][x] over the rows the
// light crosses before y (up: the light travels along +y).  Shared with render_camera.hip.
hipError_t launch_orbit_prefix(const float *vols, int64_t stride, int64_t n, int D, int H, int W, bool up, float *workspace, hipStream_t st);
// cs: n * n_views (cos, sin) pairs on the host, volume-major.  Plane v * n_views + k of image / trans is view k of volume v.
hipError_t launch_volume_render_orbit(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                      const float *cs, int n_views, float *image, int64_t image_stride, float *trans, int64_t trans_stride,
                                      float *workspace, hipStream_t st);

}  // namespace smk
