// Orbit-camera render of n volumes [D][H][W]: an orthographic camera turned about the vertical axis y by an azimuth per view
// (SPEC_3D.md section 10, "Orbit views"; smk_volume_render_orbit).  Image row y is volume row y; a pixel's ray is S samples in the
// (z, x) plane of that row, each a bilinear interpolation of rho (outside the volume: 0), and the rule of the front view runs over the
// samples.  fp32, one fixed order per sum, no atomics; a pixel depends on its own volume and its own view only.
//
// The staging.  At an oblique angle the 64 sample positions of a wave lie on a diagonal of the (z, x) plane, in up to 64 different rows
// of the volume, so nothing is sampled from global memory.  A workgroup of ORBIT_STRIP x ORBIT_ROWS threads owns a strip of image
// columns and a few rows y and marches the samples in chunks of ORBIT_CHUNK.  Per chunk it loads the bounding box of the chunk's
// positions (orbit_plan.h: at most 46 x 46 cells, clipped to the volume) of every one of its rows y into LDS with row-contiguous loads,
// and every lane then takes its four neighbours from LDS.  A chunk whose box misses the volume is skipped whole (its samples are zeros:
// they add 0 to every sum); at azimuth 0 that leaves D of the S samples.  The geometry does not depend on y: one box per chunk serves
// all the rows.
//
// Light "+y" / "-y": interpolation is linear and the positions do not depend on y, so the prefix of the samples along y is the
// interpolation of the voxel-grid prefix A[z][y][x].  k_render_prefix (render.hip) writes that prefix into the workspace (one read and one
// write of the volumes, lanes along x), and the main kernel stages it beside rho and interpolates both with the same weights.
//
// Views: the (cos, sin) pairs travel as launch arguments, ORBIT_VIEWS_PER_LAUNCH per launch; a launch orders its workgroups view-fastest,
// so the views of one (rows, strip) run together and meet in L2.  The prefix pass runs once per call, whatever the number of views.
#include "render_orbit.h"

#include <cmath>
#include <vector>

namespace smk {

namespace {

constexpr int OV_NT = ORBIT_STRIP * ORBIT_ROWS;       // 128 threads
constexpr int STAGE_U = 4;                            // box cells a lane loads ahead of their LDS stores

struct OrbitViews {
    float c[ORBIT_VIEWS_PER_LAUNCH], s[ORBIT_VIEWS_PER_LAUNCH];
};

// the four neighbours of one sample out of a staged box (rows of nx floats); a neighbour outside the box counts as 0
__device__ __forceinline__ float orbit_bilinear(const float *box, int iz, int ix, int nz, int nx, float fz, float fx) {
    const bool z0 = (unsigned)iz < (unsigned)nz, z1 = (unsigned)(iz + 1) < (unsigned)nz;
    const bool x0 = (unsigned)ix < (unsigned)nx, x1 = (unsigned)(ix + 1) < (unsigned)nx;
    const int i00 = iz * nx + ix;
    const float v00 = (z0 && x0) ? box[(z0 && x0) ? i00 : 0] : 0.f;
    const float v01 = (z0 && x1) ? box[(z0 && x1) ? i00 + 1 : 0] : 0.f;
    const float v10 = (z1 && x0) ? box[(z1 && x0) ? i00 + nx : 0] : 0.f;
    const float v11 = (z1 && x1) ? box[(z1 && x1) ? i00 + nx + 1 : 0] : 0.f;
    const float gx = 1.0f - fx;
    return (1.0f - fz) * (gx * v00 + fx * v01) + fz * (gx * v10 + fx * v11);
}

// ---- one workgroup = ORBIT_STRIP columns x ORBIT_ROWS rows of one view; lanes along x'
template <bool LIT>
__global__ __launch_bounds__(OV_NT) void k_render_orbit(const float *__restrict__ vols, int64_t stride, const float *__restrict__ prefix,
                                                        int D, int H, int W, int n_views, int pair0, int npairs, int nstrips, OrbitViews views,
                                                        RenderParams p, float *__restrict__ image, int64_t istride,
                                                        float *__restrict__ trans, int64_t tstride) {
    constexpr int PLANES = LIT ? 2 : 1;
    __shared__ float lds[ORBIT_ROWS * PLANES * ORBIT_BOX_FLOATS];
    unsigned id = blockIdx.x;
    const int pi = id % npairs; id /= npairs;
    const int strip = id % nstrips, yg = id / nstrips;
    const int pair = pair0 + pi, v = pair / n_views;
    const float c = views.c[pi], s = views.s[pi];
    const OrbitGeom g = orbit_geom(D, W);
    const int xa = strip * ORBIT_STRIP, xb = xa + ORBIT_STRIP - 1 < W ? xa + ORBIT_STRIP - 1 : W - 1;
    const int r = threadIdx.x / ORBIT_STRIP, j = threadIdx.x % ORBIT_STRIP;
    const int y = yg * ORBIT_ROWS + r, xcol = xa + j;
    const bool ok = y < H && xcol <= xb;                       // lanes past the image work on its last row / the strip's last column
    const float a = (float)(xcol <= xb ? xcol : xb) - g.cx;
    const size_t HW = (size_t)H * W;
    const float *vol = vols + (size_t)v * stride;
    const float *pre = LIT ? prefix + (size_t)v * D * HW : nullptr;
    const float *mine = lds + r * PLANES * ORBIT_BOX_FLOATS;
    size_t yoff[ORBIT_ROWS];                                   // the rows this workgroup stages (past the image: its last row again)
#pragma unroll
    for (int rr = 0; rr < ORBIT_ROWS; ++rr) yoff[rr] = (size_t)(yg * ORBIT_ROWS + rr < H ? yg * ORBIT_ROWS + rr : H - 1) * W;
    float tau = 0.f, img = 0.f;
    for (int s0 = 0; s0 < g.S; s0 += ORBIT_CHUNK) {
        const int s1 = s0 + ORBIT_CHUNK - 1 < g.S ? s0 + ORBIT_CHUNK - 1 : g.S - 1;
        const OrbitBox b = orbit_box(g, c, s, xa, xb, s0, s1);             // the same for every thread of the workgroup
        if (b.empty()) continue;
        const int nz = b.nz(), nx = b.nx(), cells = nz * nx;               // <= ORBIT_BOX_FLOATS (tests/host/orbit_plan_main.cpp)
        const float inv_nx = 1.0f / (float)nx;
        __syncthreads();                                                   // the previous chunk has been read
        const size_t corner = (size_t)b.z0 * HW + b.x0;
        for (int e0 = threadIdx.x; e0 < cells; e0 += OV_NT * STAGE_U) {       // STAGE_U x ORBIT_ROWS x PLANES loads in flight per lane
            float val[STAGE_U][ORBIT_ROWS][PLANES];
#pragma unroll
            for (int u = 0; u < STAGE_U; ++u) {
                const int e = e0 + u * OV_NT < cells ? e0 + u * OV_NT : cells - 1;       // past the box: its last cell again, not stored
                const int zr = orbit_box_row(e, inv_nx), xc = e - zr * nx;
                const size_t at = corner + (size_t)zr * HW + xc;            // (z0 + zr, ., x0 + xc) inside the volume
#pragma unroll
                for (int rr = 0; rr < ORBIT_ROWS; ++rr) {
                    val[u][rr][0] = vol[at + yoff[rr]];
                    if constexpr (LIT) val[u][rr][1] = pre[at + yoff[rr]];
                }
            }
#pragma unroll
            for (int u = 0; u < STAGE_U; ++u) {
                const int e = e0 + u * OV_NT;
                if (e < cells) {
#pragma unroll
                    for (int rr = 0; rr < ORBIT_ROWS; ++rr) {
                        lds[rr * PLANES * ORBIT_BOX_FLOATS + e] = val[u][rr][0];
                        if constexpr (LIT) lds[rr * PLANES * ORBIT_BOX_FLOATS + ORBIT_BOX_FLOATS + e] = val[u][rr][1];
                    }
                }
            }
        }
        __syncthreads();
        for (int k = s0; k <= s1; ++k) {
            const float t = (float)k - g.tc;
            const float z = orbit_sample_z(a, t, c, s, g.cz), x = orbit_sample_x(a, t, c, s, g.cx);
            const float zf = floorf(z), xf = floorf(x);
            const int iz = (int)zf - b.z0, ix = (int)xf - b.x0;
            const float fz = z - zf, fx = x - xf;
            const float rho = orbit_bilinear(mine, iz, ix, nz, nx, fz, fx);
            const float A = LIT ? orbit_bilinear(mine + ORBIT_BOX_FLOATS, iz, ix, nz, nx, fz, fx) : 0.f;
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

hipError_t launch_volume_render_orbit(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                      const float *cs, int n_views, float *image, int64_t image_stride, float *trans, int64_t trans_stride,
                                      float *workspace, hipStream_t st) {
    const bool lit = light == SMK_LIGHT_POS_Y || light == SMK_LIGHT_NEG_Y;
    const int nstrips = (W + ORBIT_STRIP - 1) / ORBIT_STRIP, nyg = (H + ORBIT_ROWS - 1) / ORBIT_ROWS;
    const int64_t pairs = n * n_views, per_pair = (int64_t)nstrips * nyg;
    if (per_pair * ORBIT_VIEWS_PER_LAUNCH > 0x7fffffffLL || pairs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipError_t e;
    if (lit && (e = launch_render_prefix(vols, stride, n, D, H, W, light == SMK_LIGHT_POS_Y, workspace, st)) != hipSuccess) return e;
    for (int64_t p0 = 0; p0 < pairs; p0 += ORBIT_VIEWS_PER_LAUNCH) {
        const int np = (int)(pairs - p0 < ORBIT_VIEWS_PER_LAUNCH ? pairs - p0 : ORBIT_VIEWS_PER_LAUNCH);
        OrbitViews views = {};
        for (int i = 0; i < np; ++i) {
            views.c[i] = cs[2 * (p0 + i)];
            views.s[i] = cs[2 * (p0 + i) + 1];
        }
        const unsigned grid = (unsigned)(per_pair * np);
        if (lit)
            hipLaunchKernelGGL(k_render_orbit<true>, dim3(grid), dim3(OV_NT), 0, st, vols, stride, workspace, D, H, W, n_views, (int)p0, np, nstrips,
                               views, p, image, image_stride, trans, trans_stride);
        else
            hipLaunchKernelGGL(k_render_orbit<false>, dim3(grid), dim3(OV_NT), 0, st, vols, stride, (const float *)nullptr, D, H, W, n_views,
                               (int)p0, np, nstrips, views, p, image, image_stride, trans, trans_stride);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace smk

using namespace smk;

#pragma GCC visibility push(default)
extern "C" {

static constexpr RenderLimits ORBIT = {ORBIT_MAX_DEPTH, 0, ORBIT_MAX_WIDTH, "orbit views"};

int64_t smk_volume_render_orbit_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light) {
    return render_query_ok(ORBIT, n, D, H, W, light) ? render_prefix_workspace(n, D, H, W, light) : -1;
}

int smk_volume_render_orbit(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, const smk_render_desc *desc,
                            const double *azimuths, int32_t n_views, float *image, int64_t image_stride, float *transmittance,
                            int64_t trans_stride, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(vols && desc && image && azimuths, "null pointer");
    RenderParams p;
    int rc = render_check("volume_render_orbit", ORBIT, n, D, H, W, n_views, desc, vols, vol_stride,
                          {{image, image_stride, false, "image_stride"}, {transmittance, trans_stride, false, "trans_stride"}}, workspace, &p);
    if (rc != SMK_OK) return rc;
    const int64_t planes = (int64_t)n * n_views;
    for (int64_t i = 0; i < planes; ++i) SMK_REQUIRE(std::isfinite(azimuths[i]), "azimuths: finite numbers of degrees");
    rc = render_check_workspace("volume_render_orbit", render_prefix_workspace(n, D, H, W, desc->light), workspace, workspace_bytes);
    if (rc != SMK_OK) return rc;
    std::vector<float> cs((size_t)planes * 2);
    for (int64_t i = 0; i < planes; ++i) orbit_cos_sin(azimuths[i], &cs[2 * i], &cs[2 * i + 1]);
    return render_launch_status("volume_render_orbit",
                                launch_volume_render_orbit(vols, vol_stride, n, D, H, W, desc->light, p, cs.data(), n_views, image, image_stride,
                                                           transmittance, trans_stride, (float *)workspace, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
