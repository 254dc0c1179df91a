// Free-camera render of n volumes [D][H][W]: an orthographic camera with an azimuth and an elevation per view (SPEC_3D.md section 10,
// "Free camera"; smk_volume_render_camera).  A pixel's ray is S samples along the view direction, each a trilinear interpolation of rho
// (outside the volume: 0), and the rule of the front view runs over the samples.  fp32, one fixed order per sum, no atomics; a pixel
// depends on its own volume and its own view only.
//
// The form.  A pitched ray leaves its row of the volume, so the orbit's per-row [z, x] box in LDS does not carry over, and the bounding
// box of a useful brick of samples in three dimensions does not fit LDS twice (DESIGN.md 8.5 has the arithmetic).  The eight taps of a
// sample are read from global memory instead: lanes lie along x', so at small azimuths neighbouring lanes read neighbouring addresses, and
// at any angle the taps of neighbouring samples, lanes and rows repeat in L1 / L2.  A wave owns CAMERA_TILE_W x CAMERA_TILE_H pixels and
// marches in chunks of CAMERA_CHUNK samples; a chunk whose brick of positions (camera_plan.h) cannot touch the volume is skipped whole.
// There is no LDS and no barrier: the waves of a workgroup are independent.  Every offset comes from camera_taps, which tests each tap
// against the volume; a tap outside it is not read (its lane reads cell 0 of its own volume and discards it).
//
// Light "+y" / "-y": A_s is the same interpolation of the voxel-grid prefix A[z][y][x], which k_render_prefix (render.hip) writes into
// the workspace once per call; the main kernel reads it beside rho at the same offsets.
//
// Views: the coefficients travel as launch arguments, CAMERA_VIEWS_PER_LAUNCH per launch; a launch orders its workgroups view-fastest.
#include "render_camera.h"

#include <cmath>
#include <new>
#include <vector>

namespace smk {

namespace {

constexpr int CV_NT = 64 * CAMERA_WAVES;
static_assert(CAMERA_TILE_W * CAMERA_TILE_H == 64, "a tile is one wave");

struct CameraViews {
    CameraView v[CAMERA_VIEWS_PER_LAUNCH];
};

// ---- one wave = CAMERA_TILE_W columns x CAMERA_TILE_H rows of one view; lanes along x'
template <bool LIT>
__global__ __launch_bounds__(CV_NT) void k_render_camera(const float *__restrict__ vols, int64_t stride, const float *__restrict__ prefix,
                                                         int D, int H, int W, int n_views, int pair0, int npairs, int nstrips,
                                                         CameraViews views, RenderParams p, float *__restrict__ image, int64_t istride,
                                                         float *__restrict__ trans, int64_t tstride) {
    unsigned id = blockIdx.x;
    const int pi = id % npairs; id /= npairs;
    const int strip = id % nstrips, yg = id / nstrips;
    const int pair = pair0 + pi, v = pair / n_views;
    const CameraView cv = views.v[pi];
    const CameraGeom g = camera_geom(D, H, W);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    const int xa = strip * CAMERA_TILE_W, xb = xa + CAMERA_TILE_W - 1 < W ? xa + CAMERA_TILE_W - 1 : W - 1;
    const int ya = (yg * CAMERA_WAVES + wave) * CAMERA_TILE_H;
    if (ya >= H) return;                                       // the whole wave: nothing below waits for it
    const int yb = ya + CAMERA_TILE_H - 1 < H ? ya + CAMERA_TILE_H - 1 : H - 1;
    const int y = ya + lane / CAMERA_TILE_W, xcol = xa + lane % CAMERA_TILE_W;
    const bool ok = y <= yb && xcol <= xb;                     // lanes past the image work on the tile's last row / column
    const float a = (float)(xcol <= xb ? xcol : xb) - g.cx, b = (float)(y <= yb ? y : yb) - g.cy;
    const float *vol = vols + (size_t)v * stride;
    const float *pre = LIT ? prefix + (size_t)v * D * H * W : nullptr;
    float tau = 0.f, img = 0.f;
    for (int s0 = 0; s0 < g.S; s0 += CAMERA_CHUNK) {
        const int s1 = s0 + CAMERA_CHUNK - 1 < g.S ? s0 + CAMERA_CHUNK - 1 : g.S - 1;
        if (!camera_brick_live(g, camera_brick(g, cv, xa, xb, ya, yb, s0, s1))) continue;      // the same for every lane of the wave
        for (int k = s0; k <= s1; ++k) {
            const float t = (float)k - g.tc;
            const float z = camera_sample_z(a, b, t, cv, g.cz), yy = camera_sample_y(b, t, cv, g.cy), x = camera_sample_x(a, b, t, cv, g.cx);
            const float zf = floorf(z), yf = floorf(yy), xf = floorf(x);
            int32_t off[8];
            camera_taps(g, (int)zf, (int)yf, (int)xf, off);
            float rv[8], av[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const int32_t o = off[n] < 0 ? 0 : off[n];     // in [0, D*H*W)
                rv[n] = vol[o];
                if constexpr (LIT) av[n] = pre[o];
            }
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                rv[n] = off[n] < 0 ? 0.f : rv[n];
                if constexpr (LIT) av[n] = off[n] < 0 ? 0.f : av[n];
            }
            const float fz = z - zf, fy = yy - yf, fx = x - xf;
            const float rho = camera_trilinear(rv, fz, fy, fx);
            const float A = LIT ? camera_trilinear(av, fz, fy, fx) : 0.f;
            if (wave_has_term(rho, A, tau)) img += render_term(rho, A, tau, p, LIT);
            tau += rho;
        }
    }
    if (!ok) return;
    const size_t pix = (size_t)y * W + xcol;
    image[(size_t)pair * istride + pix] = p.gain * img;
    if (trans != nullptr) trans[(size_t)pair * tstride + pix] = __expf(p.neg_sigma_view * tau);
}

}  // namespace

hipError_t launch_volume_render_camera(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                       const CameraView *cvs, int n_views, float *image, int64_t image_stride, float *trans,
                                       int64_t trans_stride, float *workspace, hipStream_t st) {
    const bool lit = light == SMK_LIGHT_POS_Y || light == SMK_LIGHT_NEG_Y;
    const int rows = CAMERA_WAVES * CAMERA_TILE_H;
    const int nstrips = (W + CAMERA_TILE_W - 1) / CAMERA_TILE_W, nyg = (H + rows - 1) / rows;
    const int64_t pairs = n * n_views, per_pair = (int64_t)nstrips * nyg;
    if (per_pair * CAMERA_VIEWS_PER_LAUNCH > 0x7fffffffLL || pairs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e;
    if (lit && (e = launch_render_prefix(vols, stride, n, D, H, W, light == SMK_LIGHT_POS_Y, workspace, st)) != hipSuccess) return e;
    for (int64_t p0 = 0; p0 < pairs; p0 += CAMERA_VIEWS_PER_LAUNCH) {
        const int np = (int)(pairs - p0 < CAMERA_VIEWS_PER_LAUNCH ? pairs - p0 : CAMERA_VIEWS_PER_LAUNCH);
        CameraViews views = {};
        for (int i = 0; i < np; ++i) views.v[i] = cvs[p0 + i];
        const unsigned grid = (unsigned)(per_pair * np);
        if (lit)
            hipLaunchKernelGGL(k_render_camera<true>, dim3(grid), dim3(CV_NT), 0, st, vols, stride, workspace, D, H, W, n_views, (int)p0, np,
                               nstrips, views, p, image, image_stride, trans, trans_stride);
        else
            hipLaunchKernelGGL(k_render_camera<false>, dim3(grid), dim3(CV_NT), 0, st, vols, stride, (const float *)nullptr, D, H, W, n_views,
                               (int)p0, np, nstrips, views, p, image, image_stride, trans, trans_stride);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace smk

using namespace smk;

#pragma GCC visibility push(default)
extern "C" {

static constexpr RenderLimits CAMERA = {CAMERA_MAX_DEPTH, CAMERA_MAX_HEIGHT, CAMERA_MAX_WIDTH, "a moving camera"};

int64_t smk_volume_render_camera_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light) {
    return render_query_ok(CAMERA, n, D, H, W, light) ? render_prefix_workspace(n, D, H, W, light) : -1;
}

int smk_volume_render_camera(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, const smk_render_desc *desc,
                             const double *azimuths, const double *elevations, int32_t n_views, float *image, int64_t image_stride,
                             float *transmittance, int64_t trans_stride, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(vols && desc && image && azimuths && elevations, "null pointer");
    RenderParams p;
    int rc = render_check("volume_render_camera", CAMERA, n, D, H, W, n_views, desc, vols, vol_stride,
                          {{image, image_stride, false, "image_stride"}, {transmittance, trans_stride, false, "trans_stride"}}, workspace, &p);
    if (rc != SMK_OK) return rc;
    const int64_t planes = (int64_t)n * n_views;
    for (int64_t i = 0; i < planes; ++i) {
        SMK_REQUIRE(std::isfinite(azimuths[i]), "azimuths: finite numbers of degrees");
        SMK_REQUIRE(std::isfinite(elevations[i]) && elevations[i] >= -90.0 && elevations[i] <= 90.0,
                    "elevations: finite numbers of degrees in [-90, 90]");
    }
    rc = render_check_workspace("volume_render_camera", render_prefix_workspace(n, D, H, W, desc->light), workspace, workspace_bytes);
    if (rc != SMK_OK) return rc;
    std::vector<CameraView> cvs;
    try {
        cvs.resize((size_t)planes);                            // up to 2^20 coefficient sets, 32 MB: no exception may cross the C boundary
    } catch (const std::bad_alloc &) {
        set_error("volume_render_camera: out of host memory for the view coefficients");
        return SMK_ERR_INVALID;
    }
    for (int64_t i = 0; i < planes; ++i) SMK_REQUIRE(camera_view(azimuths[i], elevations[i], &cvs[i]), "angles");
    return render_launch_status("volume_render_camera",
                                launch_volume_render_camera(vols, vol_stride, n, D, H, W, desc->light, p, cvs.data(), n_views, image,
                                                            image_stride, transmittance, trans_stride, (float *)workspace, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
