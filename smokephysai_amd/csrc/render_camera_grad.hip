// The gradient of the free-camera render with respect to the volumes (SPEC_3D.md section 10, "Free camera -- Gradient";
// smk_volume_render_camera_backward).  With rho_s, A_s the trilinear samples of rho and of its +-y prefix on the voxel grid, tau the
// exclusive prefix of rho_s over s, T = exp(-sv tau), alpha = -expm1(-sv rho_s), X = exp(-sl A_s), L = a + (1 - a) X, c = alpha L T, and
// G / Gt the upstream gradients of one view's image / transmittance:
//   Q[s,y',x'] = g G sv (exp(-sv rho_s) L T - sum_{s' > s} c) - sv Gt trans        R[s,y',x'] = g G alpha T (-sl (1 - a) X)
//   drho[z,y,x] = sum over the views of (B^T Q)[z,y,x] + the sum of (B^T R)[z,y'',x] over the voxel rows y'' that y shadows
// B^T: the transpose of the interpolation, the forward's eight weights.  fp32, one fixed order per sum, views in ascending order, no
// atomics: the transpose is a gather.
//
// Three kinds of launch (the plan, the bands and every index: camera_grad_plan.h):
//   k_camera_grad_rays   : the forward's march (its tiles, chunks, camera_brick_live, camera_taps) over the image rows of one band at
//                          one view; no LDS, no barrier.  The suffix sum is total - inclusive prefix, and the total is known only after
//                          the last sample, so a sample leaves Q' = g G sv (E + P) (E = exp(-sv rho_s) L T, P the inclusive prefix of c)
//                          and R, and the ray leaves K = g G sv (sum c) + sv Gt trans: Q = Q' - K, one march.  Unlit, Q = sv trans (g G - Gt)
//                          for every s: K alone, no per-sample scratch.  A skipped chunk writes nothing: none of its samples has a tap
//                          inside the volume, so no candidate with a weight reads what it would leave.  No wave skips a term: rho_s = 0
//                          has a gradient.
//   k_camera_grad_gather : one thread per voxel of the band's slab of voxel rows; a thread whose voxel the band does not own leaves.  An
//                          owner visits the 4 x 4 x 4 candidate (row, column, sample) triples about the voxel's ray coordinates in one
//                          fixed order, forms each one's position as the forward does and adds weight * Q where one of its taps is the
//                          voxel.  View 0 of a volume writes drho (and U = B^T R), later views add to it in view order: every voxel is
//                          owned by exactly one band of every view, so every element is written, a voxel no ray reaches with 0.
//   k_render_grad_light  : +-y only (render.hip).  drho[z,y,x] += the exclusive sum of U over the rows y shadows.
// Under a +-y light k_render_prefix (render.hip) runs first, as in the forward.  The walk: groups of up to 16 volumes; per group the views
// in ascending order; per view the bands.  Launches per call: 2 per unit (a group's band) and view, plus 2 under a +-y light.
#include "render_camera_grad.h"

#include <cmath>
#include <new>
#include <vector>

namespace smk {

namespace {

constexpr int CG_NT = 64 * CAMERA_WAVES;
constexpr int CG_FLAT = 256;                          // threads per workgroup of the gather
static_assert(CAMERA_TILE_W * CAMERA_TILE_H == 64, "a tile is one wave");

struct CameraGradViews {
    CameraView v[CAMERA_GRAD_VOLS_PER_LAUNCH];
};

// ---- one wave = CAMERA_TILE_W columns x CAMERA_TILE_H rows of one volume of the unit, rows counted from the band's first; lanes along x'
template <bool LIT>
__global__ __launch_bounds__(CG_NT) void k_camera_grad_rays(const float *__restrict__ vols, int64_t stride, const float *__restrict__ prefix,
                                                            int D, int H, int W, int n_views, int view, int64_t v0, int y0, int yend,
                                                            int nstrips, int nyg, CameraGradViews views, RenderParams p, CameraGradPlan plan,
                                                            const float *__restrict__ G, int64_t gstride, const float *__restrict__ Gt,
                                                            int64_t tstride, float *__restrict__ scratch) {
    unsigned id = blockIdx.x;
    const int strip = id % nstrips; id /= nstrips;
    const int yg = id % nyg, vi = id / nyg;
    const int64_t v = v0 + vi;
    const CameraView cv = views.v[vi];
    const CameraGeom g = camera_geom(D, H, W);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    const int xa = strip * CAMERA_TILE_W, xb = xa + CAMERA_TILE_W - 1 < W ? xa + CAMERA_TILE_W - 1 : W - 1;
    const int ya = y0 + (yg * CAMERA_WAVES + wave) * CAMERA_TILE_H;
    if (ya >= yend) return;                                    // the whole wave: nothing below waits for it
    const int yb = ya + CAMERA_TILE_H - 1 < yend ? ya + CAMERA_TILE_H - 1 : yend - 1;
    const int y = ya + lane / CAMERA_TILE_W, xcol = xa + lane % CAMERA_TILE_W;
    const bool ok = y <= yb && xcol <= xb;                     // lanes past the band / image work on the tile's last row / column
    const int yc = y <= yb ? y : yb, xc = xcol <= xb ? xcol : xb;
    const float a = (float)xc - g.cx, b = (float)yc - g.cy;
    const float *vol = vols + (size_t)v * stride;
    const float *pre = LIT ? prefix + (size_t)v * D * H * W : nullptr;
    const size_t plane = (size_t)(v * n_views + view), pix = (size_t)yc * W + xc;
    const float gG = G != nullptr ? p.gain * G[plane * gstride + pix] : 0.f;
    const float gt = Gt != nullptr ? Gt[plane * tstride + pix] : 0.f;
    const float sv = -p.neg_sigma_view, gs = gG * sv;
    const int64_t row = camera_grad_row(plan, vi, y0, yc);     // < max_vols * slots
    float tau = 0.f, P = 0.f;
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
            if constexpr (LIT) {
                const float A = camera_trilinear(av, fz, fy, fx);
                const float alpha = -expm1f(p.neg_sigma_view * rho);
                const float T = __expf(p.neg_sigma_view * tau);
                const float X = __expf(p.neg_sigma_light * A);
                const float LT = (p.ambient + p.one_minus_ambient * X) * T;
                P += alpha * LT;
                if (ok) {
                    scratch[camera_grad_at_q(plan, row, k, xc)] = gs * ((1.0f - alpha) * LT + P);
                    scratch[camera_grad_at_r(plan, row, k, xc)] = ((gG * alpha) * T) * ((p.neg_sigma_light * p.one_minus_ambient) * X);
                }
            }
            tau += rho;
        }
    }
    if (!ok) return;
    const float trans = __expf(p.neg_sigma_view * tau);
    scratch[camera_grad_at_k(plan, row, xc)] = LIT ? gs * P + (sv * gt) * trans : (sv * trans) * (gG - gt);
}

// ---- one thread per voxel of the unit's slab of voxel rows [ya, ya + ny): x fastest, then the row, then z, then the volume
template <bool LIT>
__global__ __launch_bounds__(CG_FLAT) void k_camera_grad_gather(int D, int H, int W, int64_t v0, int y0, int yend, int ya, int ny,
                                                                int64_t total, CameraGradViews views, CameraGradPlan plan,
                                                                const float *__restrict__ scratch, float *out, int64_t ostride, float *U,
                                                                int accumulate) {
    int64_t id = (int64_t)blockIdx.x * CG_FLAT + threadIdx.x;
    if (id >= total) return;
    const int x = (int)(id % W); id /= W;
    const int y = ya + (int)(id % ny); id /= ny;
    const int z = (int)(id % D), vi = (int)(id / D);
    const CameraView cv = views.v[vi];
    const CameraGeom g = camera_geom(D, H, W);
    float col, rowc, smp;
    camera_grad_invert(g, cv, z, y, x, &col, &rowc, &smp);
    const int owner = camera_grad_owner_row(rowc, H);
    if (owner < y0 || owner >= y0 + plan.band) return;         // another band writes this voxel
    const int r0 = camera_grad_first(rowc), x0 = camera_grad_first(col), k0 = camera_grad_first(smp);
    float accQ = 0.f, accR = 0.f;
    for (int i = 0; i < CAMERA_GRAD_WINDOW; ++i) {
        const int yr = r0 + i;
        if (yr < y0 || yr >= yend) continue;                   // not marched: outside the image (camera_grad_plan.h)
        const int64_t row = camera_grad_row(plan, vi, y0, yr);
#pragma unroll
        for (int j = 0; j < CAMERA_GRAD_WINDOW; ++j) {
            const int xc = x0 + j;
            if (xc < 0 || xc >= W) continue;
            const float K = scratch[camera_grad_at_k(plan, row, xc)];
#pragma unroll
            for (int kk = 0; kk < CAMERA_GRAD_WINDOW; ++kk) {
                const int k = k0 + kk;
                if (k < 0 || k >= g.S) continue;
                const float w = camera_grad_weight(g, cv, xc, yr, k, z, y, x);
                if (w == 0.f) continue;
                if constexpr (LIT) {
                    accQ += w * (scratch[camera_grad_at_q(plan, row, k, xc)] - K);
                    accR += w * scratch[camera_grad_at_r(plan, row, k, xc)];
                } else {
                    accQ += w * K;
                }
            }
        }
    }
    const size_t cell = ((size_t)z * H + (size_t)y) * W + x;   // < D * H * W
    float *o = out + (size_t)(v0 + vi) * ostride + cell;
    *o = accumulate ? *o + accQ : accQ;
    if constexpr (LIT) {
        float *u = U + (size_t)(v0 + vi) * D * H * W + cell;
        *u = accumulate ? *u + accR : accR;
    }
}

}  // namespace

int64_t render_camera_backward_workspace(int64_t n, int D, int H, int W, int light) {
    const bool lit = light == SMK_LIGHT_POS_Y || light == SMK_LIGHT_NEG_Y;
    const CameraGradPlan plan = camera_grad_plan(n, D, H, W, lit);
    return ((lit ? 2 * n * (int64_t)D * H * W : 0) + plan.scratch_floats) * (int64_t)sizeof(float);
}

hipError_t launch_volume_render_camera_backward(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light,
                                                const RenderParams &p, const CameraView *cvs, int n_views, const float *G, int64_t gstride,
                                                const float *Gt, int64_t tstride, float *out, int64_t ostride, float *workspace,
                                                hipStream_t st) {
    const bool lit = light == SMK_LIGHT_POS_Y || light == SMK_LIGHT_NEG_Y;
    const CameraGradPlan plan = camera_grad_plan(n, D, H, W, lit);
    const CameraGeom g = camera_geom(D, H, W);
    const int64_t cells = (int64_t)D * H * W;
    float *wsA = lit ? workspace : nullptr, *wsU = lit ? workspace + n * cells : nullptr;
    float *scratch = lit ? workspace + 2 * n * cells : workspace;
    const int rows = CAMERA_WAVES * CAMERA_TILE_H;
    const int nstrips = (W + CAMERA_TILE_W - 1) / CAMERA_TILE_W;
    // the largest grids of the walk, before the first launch: an error leaves `out` untouched
    const int64_t max_rays = (int64_t)plan.max_vols * ((plan.slots + rows - 1) / rows) * nstrips;
    const int64_t max_gather = ((int64_t)plan.max_vols * cells + CG_FLAT - 1) / CG_FLAT;
    if (max_rays > 0x7fffffffLL || max_gather > 0x7fffffffLL || (lit && !render_grad_light_fits(n, D, W))) return hipErrorInvalidValue;
    hipError_t e;
    if (lit && (e = launch_render_prefix(vols, stride, n, D, H, W, light == SMK_LIGHT_POS_Y, wsA, st)) != hipSuccess) return e;
    for (int64_t v0 = 0; v0 < n; v0 += plan.max_vols) {
        const int nv = (int)(n - v0 < plan.max_vols ? n - v0 : plan.max_vols);
        for (int k = 0; k < n_views; ++k) {
            CameraGradViews views = {};
            for (int i = 0; i < nv; ++i) views.v[i] = cvs[(v0 + i) * n_views + k];
            for (int y0 = 0; y0 < H; y0 += plan.band) {
                const int yend = camera_grad_march_end(plan, y0);
                int ya = H, yb = -1;                           // the union of the volumes' slabs
                for (int i = 0; i < nv; ++i) {
                    int a, b;
                    camera_grad_slab(g, views.v[i], plan, y0, &a, &b);
                    if (a <= b) {
                        ya = a < ya ? a : ya;
                        yb = b > yb ? b : yb;
                    }
                }
                if (ya > yb) continue;                         // the band owns no voxel at these views
                const int nyg = (yend - y0 + rows - 1) / rows, ny = yb - ya + 1;
                const int64_t grid_rays = (int64_t)nv * nyg * nstrips, total = (int64_t)nv * D * ny * W;
                const int64_t grid_gather = (total + CG_FLAT - 1) / CG_FLAT;
                if (lit) {
                    hipLaunchKernelGGL(k_camera_grad_rays<true>, dim3((unsigned)grid_rays), dim3(CG_NT), 0, st, vols, stride, wsA, D, H, W,
                                       n_views, k, v0, y0, yend, nstrips, nyg, views, p, plan, G, gstride, Gt, tstride, scratch);
                    if ((e = hipGetLastError()) != hipSuccess) return e;
                    hipLaunchKernelGGL(k_camera_grad_gather<true>, dim3((unsigned)grid_gather), dim3(CG_FLAT), 0, st, D, H, W, v0, y0, yend, ya,
                                       ny, total, views, plan, scratch, out, ostride, wsU, k > 0 ? 1 : 0);
                } else {
                    hipLaunchKernelGGL(k_camera_grad_rays<false>, dim3((unsigned)grid_rays), dim3(CG_NT), 0, st, vols, stride,
                                       (const float *)nullptr, D, H, W, n_views, k, v0, y0, yend, nstrips, nyg, views, p, plan, G, gstride, Gt,
                                       tstride, scratch);
                    if ((e = hipGetLastError()) != hipSuccess) return e;
                    hipLaunchKernelGGL(k_camera_grad_gather<false>, dim3((unsigned)grid_gather), dim3(CG_FLAT), 0, st, D, H, W, v0, y0, yend, ya,
                                       ny, total, views, plan, scratch, out, ostride, (float *)nullptr, k > 0 ? 1 : 0);
                }
                if ((e = hipGetLastError()) != hipSuccess) return e;
            }
        }
    }
    return lit ? launch_render_grad_light(wsU, out, ostride, n, D, H, W, light == SMK_LIGHT_POS_Y, st) : hipSuccess;
}

}  // namespace smk

using namespace smk;

#pragma GCC visibility push(default)
extern "C" {

static constexpr RenderLimits CAMERA_GRAD = {CAMERA_MAX_DEPTH, CAMERA_GRAD_MAX_HEIGHT, CAMERA_MAX_WIDTH, "a moving camera"};

int64_t smk_volume_render_camera_backward_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light) {
    return render_query_ok(CAMERA_GRAD, n, D, H, W, light) ? render_camera_backward_workspace(n, D, H, W, light) : -1;
}

int smk_volume_render_camera_backward(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W,
                                      const smk_render_desc *desc, const double *azimuths, const double *elevations, int32_t n_views,
                                      const float *grad_image, int64_t grad_image_stride, const float *grad_trans, int64_t grad_trans_stride,
                                      float *grad_vols, int64_t grad_vol_stride, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(vols && desc && grad_vols && azimuths && elevations, "null pointer");
    SMK_REQUIRE(grad_image || grad_trans, "grad_image and grad_trans are both null: there is no gradient to carry back");
    RenderParams p;
    int rc = render_check("volume_render_camera_backward", CAMERA_GRAD, n, D, H, W, n_views, desc, vols, vol_stride,
                          {{grad_vols, grad_vol_stride, true, "grad_vol_stride"},
                           {grad_image, grad_image_stride, false, "grad_image_stride"},
                           {grad_trans, grad_trans_stride, false, "grad_trans_stride"}}, workspace, &p);
    if (rc != SMK_OK) return rc;
    const int64_t planes = (int64_t)n * n_views;
    for (int64_t i = 0; i < planes; ++i) {
        SMK_REQUIRE(std::isfinite(azimuths[i]), "azimuths: finite numbers of degrees");
        SMK_REQUIRE(std::isfinite(elevations[i]) && elevations[i] >= -90.0 && elevations[i] <= 90.0,
                    "elevations: finite numbers of degrees in [-90, 90]");
    }
    rc = render_check_workspace("volume_render_camera_backward", render_camera_backward_workspace(n, D, H, W, desc->light), workspace,
                                workspace_bytes);
    if (rc != SMK_OK) return rc;
    std::vector<CameraView> cvs;
    try {
        cvs.resize((size_t)planes);                            // up to 2^20 coefficient sets, 32 MB: no exception may cross the C boundary
    } catch (const std::bad_alloc &) {
        set_error("volume_render_camera_backward: out of host memory for the view coefficients");
        return SMK_ERR_INVALID;
    }
    for (int64_t i = 0; i < planes; ++i) SMK_REQUIRE(camera_view(azimuths[i], elevations[i], &cvs[i]), "angles");
    return render_launch_status("volume_render_camera_backward",
                                launch_volume_render_camera_backward(vols, vol_stride, n, D, H, W, desc->light, p, cvs.data(), n_views,
                                                                     grad_image, grad_image_stride, grad_trans, grad_trans_stride, grad_vols,
                                                                     grad_vol_stride, (float *)workspace, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
