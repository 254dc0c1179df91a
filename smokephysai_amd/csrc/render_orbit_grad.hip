// The gradient of the orbit render with respect to the volumes (SPEC_3D.md section 10, "Orbit views -- Gradient";
// smk_volume_render_orbit_backward).  With rho_s, A_s the bilinear samples of rho and of its +-y prefix, tau the exclusive prefix of
// rho_s over s, T = exp(-sv tau), alpha = -expm1(-sv rho_s), X = exp(-sl A_s), L = a + (1 - a) X, c = alpha L T, and G / Gt the upstream
// gradients of one view's image / transmittance:
//   Q[s,y,x'] = g G sv (exp(-sv rho_s) L T - sum_{s' > s} c) - sv Gt trans        R[s,y,x'] = g G alpha T (-sl (1 - a) X)
//   drho[z,y,x] = sum over the views of (B^T Q)[z,y,x] + the sum of (B^T R)[z,y',x] over the rows y' that y shadows
// B^T: the transpose of the interpolation, the forward's four weights.  fp32, one fixed order per sum, views in ascending order, no
// atomics: the transpose is a gather.
//
// Three kinds of launch (the plan and every index: orbit_grad_plan.h):
//   k_orbit_grad_rays   : the forward's march (its strips, chunks, LDS boxes and orbit_box) over the rows of one unit at one view.  The
//                         suffix sum is total - inclusive prefix, and the total is known only after the last sample, so a sample leaves
//                         Q' = g G sv (E + P) (E = exp(-sv rho_s) L T, P the inclusive prefix of c) and R, and the ray leaves
//                         K = g G sv (sum c) + sv Gt trans: Q = Q' - K, one march.  Unlit, Q = sv trans (g G - Gt) for every s: K alone, no
//                         per-sample scratch.  A chunk whose box misses the volume is skipped as in the forward: none of its samples has a
//                         tap inside the volume, so nothing reads what it would leave.  No wave skips a term: rho_s = 0 has a gradient.
//   k_orbit_grad_gather : one thread per voxel (z, x) of a row.  It visits the 4 x 4 candidate (column, sample) pairs about the voxel's
//                         ray coordinates in one fixed order, forms each one's position as the forward does and adds weight * Q where one
//                         of its taps is the voxel.  View 0 of a volume writes drho (and U = B^T R), later views add to it in view order:
//                         every element is written, a voxel no ray reaches with 0.
//   k_render_grad_light : +-y only (render.hip, shared with the free camera's gradient).  drho[z,y,x] += the exclusive sum of U over the
//                         rows y shadows: a march along y, lanes along x.
// Under a +-y light k_render_prefix (render.hip) runs first, as in the forward.  Launches per call: 2 * n_views per unit, plus 2 under a
// +-y light; a unit is up to 16 volumes, fewer (down to a range of rows of one) where their rows exceed the scratch.
#include "render_orbit_grad.h"

#include <cmath>
#include <vector>

namespace smk {

namespace {

constexpr int OG_NT = ORBIT_STRIP * ORBIT_ROWS;       // 128 threads
constexpr int OG_FLAT = 256;                          // threads per workgroup of the gather
constexpr int STAGE_U = 4;                            // box cells a lane loads ahead of their LDS stores

struct OrbitGradViews {
    float c[ORBIT_GRAD_VOLS_PER_LAUNCH], s[ORBIT_GRAD_VOLS_PER_LAUNCH];
};

// the four neighbours of one sample out of a staged box (rows of nx floats); a neighbour outside the box counts as 0
__device__ __forceinline__ float box_bilinear(const float *box, int iz, int ix, int nz, int nx, float fz, float fx) {
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

// ---- one workgroup = ORBIT_STRIP columns x ORBIT_ROWS rows of one volume of the unit; lanes along x'
template <bool LIT>
__global__ __launch_bounds__(OG_NT) void k_orbit_grad_rays(const float *__restrict__ vols, int64_t stride, const float *__restrict__ prefix,
                                                           int D, int H, int W, int n_views, int view, int64_t v0, int y0, int ny, int nstrips,
                                                           int nyg, OrbitGradViews views, RenderParams p, OrbitGradPlan plan,
                                                           const float *__restrict__ G, int64_t gstride, const float *__restrict__ Gt,
                                                           int64_t tstride, float *__restrict__ scratch) {
    constexpr int PLANES = LIT ? 2 : 1;
    __shared__ float lds[ORBIT_ROWS * PLANES * ORBIT_BOX_FLOATS];
    unsigned id = blockIdx.x;
    const int strip = id % nstrips; id /= nstrips;
    const int yg = id % nyg, vi = id / nyg;
    const int64_t v = v0 + vi;
    const float c = views.c[vi], s = views.s[vi];
    const OrbitGeom g = orbit_geom(D, W);
    const int xa = strip * ORBIT_STRIP, xb = xa + ORBIT_STRIP - 1 < W ? xa + ORBIT_STRIP - 1 : W - 1;
    const int r = threadIdx.x / ORBIT_STRIP, j = threadIdx.x % ORBIT_STRIP;
    const int yend = y0 + ny;                                  // <= H
    const int y = y0 + yg * ORBIT_ROWS + r, xcol = xa + j;
    const bool ok = y < yend && xcol <= xb;                    // lanes past the unit work on its last row / the strip's last column
    const int yc = y < yend ? y : yend - 1, xc = xcol <= xb ? xcol : xb;
    const float a = (float)xc - g.cx;
    const size_t HW = (size_t)H * W;
    const float *vol = vols + (size_t)v * stride;
    const float *pre = LIT ? prefix + (size_t)v * D * HW : nullptr;
    const float *mine = lds + r * PLANES * ORBIT_BOX_FLOATS;
    size_t yoff[ORBIT_ROWS];
#pragma unroll
    for (int rr = 0; rr < ORBIT_ROWS; ++rr) {
        const int yr = y0 + yg * ORBIT_ROWS + rr;
        yoff[rr] = (size_t)(yr < yend ? yr : yend - 1) * W;
    }
    const size_t plane = (size_t)(v * n_views + view), pix = (size_t)yc * W + xc;
    const float gG = G != nullptr ? p.gain * G[plane * gstride + pix] : 0.f;
    const float gt = Gt != nullptr ? Gt[plane * tstride + pix] : 0.f;
    const float sv = -p.neg_sigma_view, gs = gG * sv;
    const int64_t row = (int64_t)vi * ny + (yc - y0);          // < cap_rows (orbit_grad_unit)
    float tau = 0.f, P = 0.f;
    for (int s0 = 0; s0 < g.S; s0 += ORBIT_CHUNK) {
        const int s1 = s0 + ORBIT_CHUNK - 1 < g.S ? s0 + ORBIT_CHUNK - 1 : g.S - 1;
        const OrbitBox b = orbit_box(g, c, s, xa, xb, s0, s1);             // the same for every thread of the workgroup
        if (b.empty()) continue;
        const int nz = b.nz(), nx = b.nx(), cells = nz * nx;               // <= ORBIT_BOX_FLOATS (tests/host/orbit_plan_main.cpp)
        const float inv_nx = 1.0f / (float)nx;
        __syncthreads();                                                   // the previous chunk has been read
        const size_t corner = (size_t)b.z0 * HW + b.x0;
        for (int e0 = threadIdx.x; e0 < cells; e0 += OG_NT * STAGE_U) {
            float val[STAGE_U][ORBIT_ROWS][PLANES];
#pragma unroll
            for (int u = 0; u < STAGE_U; ++u) {
                const int e = e0 + u * OG_NT < cells ? e0 + u * OG_NT : cells - 1;       // past the box: its last cell again, not stored
                const int zr = orbit_box_row(e, inv_nx), xo = e - zr * nx;
                const size_t at = corner + (size_t)zr * HW + xo;            // (z0 + zr, ., x0 + xo) inside the volume
#pragma unroll
                for (int rr = 0; rr < ORBIT_ROWS; ++rr) {
                    val[u][rr][0] = vol[at + yoff[rr]];
                    if constexpr (LIT) val[u][rr][1] = pre[at + yoff[rr]];
                }
            }
#pragma unroll
            for (int u = 0; u < STAGE_U; ++u) {
                const int e = e0 + u * OG_NT;
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
            const float rho = box_bilinear(mine, iz, ix, nz, nx, fz, fx);
            if constexpr (LIT) {
                const float A = box_bilinear(mine + ORBIT_BOX_FLOATS, iz, ix, nz, nx, fz, fx);
                const float alpha = -expm1f(p.neg_sigma_view * rho);
                const float T = __expf(p.neg_sigma_view * tau);
                const float X = __expf(p.neg_sigma_light * A);
                const float LT = (p.ambient + p.one_minus_ambient * X) * T;
                P += alpha * LT;
                if (ok) {
                    scratch[orbit_grad_at_q(plan, row, k, xc)] = gs * ((1.0f - alpha) * LT + P);
                    scratch[orbit_grad_at_r(plan, row, k, xc)] = ((gG * alpha) * T) * ((p.neg_sigma_light * p.one_minus_ambient) * X);
                }
            }
            tau += rho;
        }
    }
    if (!ok) return;
    const float trans = __expf(p.neg_sigma_view * tau);
    scratch[orbit_grad_at_k(plan, row, xc)] = LIT ? gs * P + (sv * gt) * trans : (sv * trans) * (gG - gt);
}

// ---- one thread per voxel of the unit's rows: x fastest, then z, then the row
template <bool LIT>
__global__ __launch_bounds__(OG_FLAT) void k_orbit_grad_gather(int D, int H, int W, int64_t v0, int y0, int ny, int64_t total,
                                                               OrbitGradViews views, OrbitGradPlan plan, const float *__restrict__ scratch,
                                                               float *out, int64_t ostride, float *U, int accumulate) {
    int64_t id = (int64_t)blockIdx.x * OG_FLAT + threadIdx.x;
    if (id >= total) return;
    const int x = (int)(id % W); id /= W;
    const int z = (int)(id % D); id /= D;
    const int yl = (int)(id % ny), vi = (int)(id / ny);
    const int64_t row = id;                                    // vi * ny + yl
    const float c = views.c[vi], s = views.s[vi];
    const OrbitGeom g = orbit_geom(D, W);
    float col, smp;
    orbit_grad_invert(g, c, s, z, x, &col, &smp);
    const int x0 = orbit_grad_first(col), k0 = orbit_grad_first(smp);
    float accQ = 0.f, accR = 0.f;
#pragma unroll
    for (int i = 0; i < ORBIT_GRAD_WINDOW; ++i) {
        const int xc = x0 + i;
        if (xc < 0 || xc >= W) continue;
        const float K = scratch[orbit_grad_at_k(plan, row, xc)];
#pragma unroll
        for (int jj = 0; jj < ORBIT_GRAD_WINDOW; ++jj) {
            const int k = k0 + jj;
            if (k < 0 || k >= g.S) continue;
            const float w = orbit_grad_weight(g, c, s, xc, k, z, x);
            if (w == 0.f) continue;
            if constexpr (LIT) {
                accQ += w * (scratch[orbit_grad_at_q(plan, row, k, xc)] - K);
                accR += w * scratch[orbit_grad_at_r(plan, row, k, xc)];
            } else {
                accQ += w * K;
            }
        }
    }
    const size_t cell = ((size_t)z * H + (size_t)(y0 + yl)) * W + x;       // < D * H * W
    float *o = out + (size_t)(v0 + vi) * ostride + cell;
    *o = accumulate ? *o + accQ : accQ;
    if constexpr (LIT) {
        float *u = U + (size_t)(v0 + vi) * D * H * W + cell;
        *u = accumulate ? *u + accR : accR;
    }
}

}  // namespace

int64_t render_orbit_backward_workspace(int64_t n, int D, int H, int W, int light) {
    const bool lit = light == SMK_LIGHT_POS_Y || light == SMK_LIGHT_NEG_Y;
    const OrbitGradPlan plan = orbit_grad_plan(n, D, H, W, lit);
    return ((lit ? 2 * n * (int64_t)D * H * W : 0) + plan.scratch_floats) * (int64_t)sizeof(float);
}

hipError_t launch_volume_render_orbit_backward(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light,
                                               const RenderParams &p, const float *cs, int n_views, const float *G, int64_t gstride,
                                               const float *Gt, int64_t tstride, float *out, int64_t ostride, float *workspace,
                                               hipStream_t st) {
    const bool lit = light == SMK_LIGHT_POS_Y || light == SMK_LIGHT_NEG_Y;
    const OrbitGradPlan plan = orbit_grad_plan(n, D, H, W, lit);
    const int64_t cells = (int64_t)D * H * W;
    float *wsA = lit ? workspace : nullptr, *wsU = lit ? workspace + n * cells : nullptr;
    float *scratch = lit ? workspace + 2 * n * cells : workspace;
    const int nstrips = (W + ORBIT_STRIP - 1) / ORBIT_STRIP;
    if (lit && !render_grad_light_fits(n, D, W)) return hipErrorInvalidValue;
    hipError_t e;
    if (lit && (e = launch_render_prefix(vols, stride, n, D, H, W, light == SMK_LIGHT_POS_Y, wsA, st)) != hipSuccess) return e;
    int64_t v0 = 0;
    int y0 = 0;
    for (bool more = true; more;) {
        const OrbitGradUnit u = orbit_grad_unit(plan, n, H, v0, y0);
        const int nyg = (u.ny + ORBIT_ROWS - 1) / ORBIT_ROWS;
        const int64_t grid_rays = (int64_t)u.nv * nyg * nstrips, total = (int64_t)u.nv * u.ny * D * W;
        const int64_t grid_gather = (total + OG_FLAT - 1) / OG_FLAT;
        if (grid_rays > 0x7fffffffLL || grid_gather > 0x7fffffffLL) return hipErrorInvalidValue;
        for (int k = 0; k < n_views; ++k) {
            OrbitGradViews views = {};
            for (int i = 0; i < u.nv; ++i) {
                views.c[i] = cs[2 * ((u.v0 + i) * n_views + k)];
                views.s[i] = cs[2 * ((u.v0 + i) * n_views + k) + 1];
            }
            if (lit) {
                hipLaunchKernelGGL(k_orbit_grad_rays<true>, dim3((unsigned)grid_rays), dim3(OG_NT), 0, st, vols, stride, wsA, D, H, W, n_views, k,
                                   u.v0, u.y0, u.ny, nstrips, nyg, views, p, plan, G, gstride, Gt, tstride, scratch);
                if ((e = hipGetLastError()) != hipSuccess) return e;
                hipLaunchKernelGGL(k_orbit_grad_gather<true>, dim3((unsigned)grid_gather), dim3(OG_FLAT), 0, st, D, H, W, u.v0, u.y0, u.ny, total,
                                   views, plan, scratch, out, ostride, wsU, k > 0 ? 1 : 0);
            } else {
                hipLaunchKernelGGL(k_orbit_grad_rays<false>, dim3((unsigned)grid_rays), dim3(OG_NT), 0, st, vols, stride, (const float *)nullptr,
                                   D, H, W, n_views, k, u.v0, u.y0, u.ny, nstrips, nyg, views, p, plan, G, gstride, Gt, tstride, scratch);
                if ((e = hipGetLastError()) != hipSuccess) return e;
                hipLaunchKernelGGL(k_orbit_grad_gather<false>, dim3((unsigned)grid_gather), dim3(OG_FLAT), 0, st, D, H, W, u.v0, u.y0, u.ny, total,
                                   views, plan, scratch, out, ostride, (float *)nullptr, k > 0 ? 1 : 0);
            }
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        more = orbit_grad_next(u, n, H, &v0, &y0);
    }
    return lit ? launch_render_grad_light(wsU, out, ostride, n, D, H, W, light == SMK_LIGHT_POS_Y, st) : hipSuccess;
}

}  // namespace smk

using namespace smk;

#pragma GCC visibility push(default)
extern "C" {

static constexpr RenderLimits ORBIT_GRAD = {ORBIT_MAX_DEPTH, 0, ORBIT_MAX_WIDTH, "orbit views"};

int64_t smk_volume_render_orbit_backward_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light) {
    return render_query_ok(ORBIT_GRAD, n, D, H, W, light) ? render_orbit_backward_workspace(n, D, H, W, light) : -1;
}

int smk_volume_render_orbit_backward(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W,
                                     const smk_render_desc *desc, const double *azimuths, int32_t n_views, const float *grad_image,
                                     int64_t grad_image_stride, const float *grad_trans, int64_t grad_trans_stride, float *grad_vols,
                                     int64_t grad_vol_stride, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(vols && desc && grad_vols && azimuths, "null pointer");
    SMK_REQUIRE(grad_image || grad_trans, "grad_image and grad_trans are both null: there is no gradient to carry back");
    RenderParams p;
    int rc = render_check("volume_render_orbit_backward", ORBIT_GRAD, n, D, H, W, n_views, desc, vols, vol_stride,
                          {{grad_vols, grad_vol_stride, true, "grad_vol_stride"},
                           {grad_image, grad_image_stride, false, "grad_image_stride"},
                           {grad_trans, grad_trans_stride, false, "grad_trans_stride"}}, workspace, &p);
    if (rc != SMK_OK) return rc;
    const int64_t planes = (int64_t)n * n_views;
    for (int64_t i = 0; i < planes; ++i) SMK_REQUIRE(std::isfinite(azimuths[i]), "azimuths: finite numbers of degrees");
    rc = render_check_workspace("volume_render_orbit_backward", render_orbit_backward_workspace(n, D, H, W, desc->light), workspace,
                                workspace_bytes);
    if (rc != SMK_OK) return rc;
    std::vector<float> cs((size_t)planes * 2);
    for (int64_t i = 0; i < planes; ++i) orbit_cos_sin(azimuths[i], &cs[2 * i], &cs[2 * i + 1]);
    return render_launch_status("volume_render_orbit_backward",
                                launch_volume_render_orbit_backward(vols, vol_stride, n, D, H, W, desc->light, p, cs.data(), n_views,
                                                                    grad_image, grad_image_stride, grad_trans, grad_trans_stride, grad_vols,
                                                                    grad_vol_stride, (float *)workspace, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
