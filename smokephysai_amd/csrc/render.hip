// Front-view single-scattering render of n volumes [D][H][W] to images [H][W] (SPEC_3D.md section 10; smk_volume_render).
//   tau[z]  = sum_{z' < z} rho[z']                       exclusive prefix toward the camera (plane 0 is nearest)
//   A[z,y]  = exclusive prefix of rho along the light's direction of travel (+y, -y, +z = tau, none = 0)
//   image   = gain * sum_z  -expm1(-sv rho) * (a + (1 - a) exp(-sl A)) * exp(-sv tau),   z ascending
//   trans   = exp(-sv * sum_z rho)
// fp32, one fixed order per sum, no atomics: bit-reproducible, and a volume's result does not depend on its neighbours in the batch.
//
// Light "none" and "+z" couple nothing across pixels: k_render_view, one pixel per lane (lanes along x), z marched in a loop, the
// volumes read once.
// Light "+y" / "-y": the prefix along y serialises a column.  One lane owns one column x and keeps the running sum of every plane in
// registers (D <= 64 floats); a wave owns 64 consecutive columns and RENDER_SEG_ROWS rows, so every load is 256 contiguous bytes.  The rows
// are cut into segments so that a volume gives (W / 64) * (H / 16) waves instead of W / 64:
//   k_render_seg_totals : per (segment, z, x) the sum of the segment's rows, in the light's order of travel      (read 1 of the volumes)
//   k_render_seg_scan   : exclusive scan of those totals over the segments, in place, in the order of travel     (workspace only)
//   k_render_lit<DMAX>  : starts every plane's sum from its scanned total and marches the segment's rows         (read 2 of the volumes)
// The workspace is [n][segments][D][W] floats = 1 / RENDER_SEG_ROWS of the volumes.  H <= RENDER_SEG_ROWS needs none (one segment).
//
// The gradient of both outputs with respect to the volumes (SPEC_3D.md section 10, "Gradient"; smk_volume_render_backward) is in the
// second half of this file: the same two mappings, the same segment kernels, every element of the result written exactly once.
//
// What the moving cameras share with the front view is here too (render.h): k_render_prefix, the whole +-y prefix on the voxel grid, which
// render_orbit.hip and render_camera.hip interpolate, its transpose k_render_grad_light for their gradients, and, at the end, the host-side checks of all four entry points.
#include "render.h"

namespace smk {

namespace {

constexpr int RV_NT = 256;                 // threads per workgroup of the three flat kernels
constexpr int SEG = RENDER_SEG_ROWS;

// ---- light none / +z: one pixel per lane, nothing shared
template <bool LIT_Z>
__global__ __launch_bounds__(RV_NT) void k_render_view(const float *__restrict__ vols, int64_t stride, int D, int HW, int bpv, RenderParams p,
                                                       float *__restrict__ image, int64_t istride, float *__restrict__ trans,
                                                       int64_t tstride) {
    const int v = blockIdx.x / bpv, pix = (blockIdx.x % bpv) * RV_NT + threadIdx.x;
    const bool ok = pix < HW;                                   // lanes past the plane read its last pixel and store nothing
    const float *f = vols + (size_t)v * stride + (ok ? pix : HW - 1);
    float tau = 0.f, img = 0.f;
    constexpr int U = 8;                                        // planes loaded ahead of their terms
    for (int z0 = 0; z0 < D; z0 += U) {
        float r[U];
#pragma unroll
        for (int j = 0; j < U; ++j) r[j] = z0 + j < D ? f[(size_t)(z0 + j) * HW] : 0.f;      // z * HW + pix < D * H * W
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (z0 + j < D) {                                   // wave-uniform
                if (wave_has_term(r[j], tau, tau)) img += render_term(r[j], tau, tau, p, LIT_Z);
                tau += r[j];
            }
        }
    }
    if (!ok) return;
    image[(size_t)v * istride + pix] = p.gain * img;
    if (trans != nullptr) trans[(size_t)v * tstride + pix] = __expf(p.neg_sigma_view * tau);
}

// rows [y0, y1) of segment s, and row i of it in the light's order of travel
__device__ __forceinline__ int seg_row(int s, int i, int H, int up, int *rows) {
    const int y0 = s * SEG, y1 = y0 + SEG < H ? y0 + SEG : H;
    *rows = y1 - y0;
    return up ? y0 + i : y1 - 1 - i;
}

// ---- light +-y, pass 1: ws[v][s][z][x] = sum of rho[z][y][x] over the rows of segment s, in the order of travel
__global__ __launch_bounds__(RV_NT) void k_render_seg_totals(const float *__restrict__ vols, int64_t stride, int D, int H, int W, int nseg,
                                                             int bpp, int up, float *__restrict__ ws) {
    unsigned id = blockIdx.x;
    const int q = (id % bpp) * RV_NT + threadIdx.x; id /= bpp;
    const int s = id % nseg, v = id / nseg;
    const int DW = D * W;
    if (q >= DW) return;
    const int z = q / W, x = q - z * W;
    const float *f = vols + (size_t)v * stride + (size_t)z * H * W + x;
    int rows;
    (void)seg_row(s, 0, H, up, &rows);
    float r[SEG];
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        int dummy;
        r[i] = i < rows ? f[(size_t)seg_row(s, i, H, up, &dummy) * W] : 0.f;
    }
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < SEG; ++i)
        if (i < rows) t += r[i];
    ws[((size_t)v * nseg + s) * DW + q] = t;
}

// ---- pass 2: exclusive scan over the segments, in place, in the order of travel
__global__ __launch_bounds__(RV_NT) void k_render_seg_scan(int DW, int nseg, int bpp, int up, float *__restrict__ ws) {
    const int v = blockIdx.x / bpp, q = (blockIdx.x % bpp) * RV_NT + threadIdx.x;
    if (q >= DW) return;
    float *w = ws + (size_t)v * nseg * DW + q;
    float run = 0.f;
    constexpr int U = 8;                                       // loads in flight (the stores alias them: read a group first)
    for (int k0 = 0; k0 < nseg; k0 += U) {
        float t[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int k = k0 + j, s = up ? k : nseg - 1 - k;
            t[j] = k < nseg ? w[(size_t)s * DW] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int k = k0 + j, s = up ? k : nseg - 1 - k;
            if (k < nseg) {
                w[(size_t)s * DW] = run;
                run += t[j];
            }
        }
    }
}

// ---- pass 3: one wave = 64 columns x one segment; A[z] lives in registers (the z loops are unrolled: static indices)
template <int DMAX>
__global__ __launch_bounds__(64, 2) void k_render_lit(const float *__restrict__ vols, int64_t stride, int D, int H, int W, int nseg, int nxc,
                                                   int up, RenderParams p, const float *__restrict__ ws, float *__restrict__ image,
                                                   int64_t istride, float *__restrict__ trans, int64_t tstride) {
    unsigned id = blockIdx.x;
    const int xc = id % nxc; id /= nxc;
    const int s = id % nseg, v = id / nseg;
    const int x = xc * 64 + threadIdx.x;
    const bool ok = x < W;
    // Every load is a wave-uniform 64-bit row address plus this lane's byte offset (at most 252): one register per lane serves all planes.
    // Lanes past the row load its last column and store nothing.
    const unsigned lane_b = 4u * (unsigned)(ok ? (int)threadIdx.x : W - 1 - xc * 64);
    const char *f = reinterpret_cast<const char *>(vols + (size_t)v * stride + xc * 64);
    float A[DMAX];
    const char *wrow = reinterpret_cast<const char *>(ws + ((size_t)v * nseg + s) * D * W + xc * 64);
#pragma unroll
    for (int z = 0; z < DMAX; ++z)
        A[z] = (ws != nullptr && z < D) ? *reinterpret_cast<const float *>(wrow + (size_t)z * W * 4 + lane_b) : 0.f;
    int rows;
    (void)seg_row(s, 0, H, up, &rows);
    for (int i = 0; i < rows; ++i) {
        int dummy;
        const int y = seg_row(s, i, H, up, &dummy);
        int Dr = D;
        asm volatile("" : "+s"(Dr));                           // D again, opaque per row: 64 scalar compares, not 64 saved lane masks
        const char *row = f + (size_t)y * W * 4;               // (z * H + y) * W + x < D * H * W
        float tau = 0.f, img = 0.f;
        constexpr int RC = DMAX < 16 ? DMAX : 16;              // planes loaded ahead of their terms
#pragma unroll
        for (int z0 = 0; z0 < DMAX; z0 += RC) {
            float r[RC];
#pragma unroll
            for (int j = 0; j < RC; ++j) {                     // planes past D load plane D - 1 again (never used)
                r[j] = *reinterpret_cast<const float *>(row + lane_b);
                row += z0 + j + 1 < Dr ? (size_t)H * W * 4 : 0;
            }
#pragma unroll
            for (int j = 0; j < RC; ++j) {
                if (z0 + j < Dr) {                             // wave-uniform
                    if (wave_has_term(r[j], A[z0 + j], tau)) img += render_term(r[j], A[z0 + j], tau, p, true);
                    tau += r[j];
                    A[z0 + j] += r[j];
                }
            }
        }
        if (ok) {
            image[(size_t)v * istride + (size_t)y * W + x] = p.gain * img;
            if (trans != nullptr) trans[(size_t)v * tstride + (size_t)y * W + x] = __expf(p.neg_sigma_view * tau);
        }
    }
}

inline int render_segments(int H) { return (H + SEG - 1) / SEG; }

// ---- light +-y for the moving cameras: ws[v][z][y][x] = sum of rho[z][y'][x] over the rows y' the light crosses before y, in the order
// of travel.  The whole prefix on the voxel grid, which they interpolate: one read and one write of the volumes, lanes along x.
__global__ __launch_bounds__(RV_NT) void k_render_prefix(const float *__restrict__ vols, int64_t stride, int D, int H, int W, int bpp, int up,
                                                         float *__restrict__ ws) {
    const int v = blockIdx.x / bpp, q = (blockIdx.x % bpp) * RV_NT + threadIdx.x;
    if (q >= D * W) return;
    const int z = q / W, x = q - z * W;
    const size_t base = (size_t)z * H * W + x;                 // + y * W < D * H * W
    const float *f = vols + (size_t)v * stride + base;
    float *o = ws + (size_t)v * D * H * W + base;
    float run = 0.f;
    constexpr int U = 8;                                       // rows loaded ahead of their sums
    for (int i0 = 0; i0 < H; i0 += U) {
        float r[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int i = i0 + j, y = up ? i : H - 1 - i;
            r[j] = i < H ? f[(size_t)y * W] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int i = i0 + j, y = up ? i : H - 1 - i;
            if (i < H) {
                o[(size_t)y * W] = run;
                run += r[j];
            }
        }
    }
}

// ---- light +-y, the gradients of the moving cameras: out[v][z][y][x] += the sum of U[v][z][y'][x] over the rows y' that y shadows (up:
// y' > y), nearest row first.  The transpose of k_render_prefix: a march along y, lanes along x.
__global__ __launch_bounds__(RV_NT) void k_render_grad_light(const float *__restrict__ U, float *out, int64_t ostride, int D, int H, int W,
                                                             int bpp, int up) {
    const int v = blockIdx.x / bpp, q = (blockIdx.x % bpp) * RV_NT + threadIdx.x;
    if (q >= D * W) return;
    const int z = q / W, x = q - z * W;
    const size_t base = (size_t)z * H * W + x;                 // + y * W < D * H * W
    const float *u = U + (size_t)v * D * H * W + base;
    float *o = out + (size_t)v * ostride + base;
    float run = 0.f;
    constexpr int UN = 8;                                      // rows loaded ahead of their sums
    for (int i0 = 0; i0 < H; i0 += UN) {
        float r[UN], d[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int i = i0 + j, y = up ? H - 1 - i : i;
            r[j] = i < H ? u[(size_t)y * W] : 0.f;
            d[j] = i < H ? o[(size_t)y * W] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const int i = i0 + j, y = up ? H - 1 - i : i;
            if (i < H) {
                o[(size_t)y * W] = d[j] + run;
                run += r[j];
            }
        }
    }
}

}  // namespace

int64_t render_prefix_workspace(int64_t n, int D, int H, int W, int light) {
    if (light != SMK_LIGHT_POS_Y && light != SMK_LIGHT_NEG_Y) return 0;
    return n * (int64_t)D * H * W * (int64_t)sizeof(float);
}

hipError_t launch_render_prefix(const float *vols, int64_t stride, int64_t n, int D, int H, int W, bool up, float *workspace, hipStream_t st) {
    const int64_t bpp = ((int64_t)D * W + RV_NT - 1) / RV_NT, grid = n * bpp;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_render_prefix, dim3((unsigned)grid), dim3(RV_NT), 0, st, vols, stride, D, H, W, (int)bpp, up ? 1 : 0, workspace);
    return hipGetLastError();
}

bool render_grad_light_fits(int64_t n, int D, int W) { return n * (((int64_t)D * W + RV_NT - 1) / RV_NT) <= 0x7fffffffLL; }

hipError_t launch_render_grad_light(const float *U, float *out, int64_t ostride, int64_t n, int D, int H, int W, bool up, hipStream_t st) {
    const int64_t bpp = ((int64_t)D * W + RV_NT - 1) / RV_NT, grid = n * bpp;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_render_grad_light, dim3((unsigned)grid), dim3(RV_NT), 0, st, U, out, ostride, D, H, W, (int)bpp, up ? 1 : 0);
    return hipGetLastError();
}

int64_t render_workspace(int64_t n, int D, int H, int W, int light) {
    if (light != SMK_LIGHT_POS_Y && light != SMK_LIGHT_NEG_Y) return 0;
    const int nseg = render_segments(H);
    if (nseg <= 1) return 0;
    return n * nseg * (int64_t)D * W * (int64_t)sizeof(float);
}

hipError_t launch_volume_render(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                float *image, int64_t image_stride, float *trans, int64_t trans_stride, float *workspace, hipStream_t st) {
    const int64_t HW = (int64_t)H * W, DW = (int64_t)D * W;
    if (light == SMK_LIGHT_NONE || light == SMK_LIGHT_POS_Z) {
        const int64_t bpv = (HW + RV_NT - 1) / RV_NT, grid = n * bpv;
        if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
        if (light == SMK_LIGHT_POS_Z)
            hipLaunchKernelGGL(k_render_view<true>, dim3((unsigned)grid), dim3(RV_NT), 0, st, vols, stride, D, (int)HW, (int)bpv, p, image,
                               image_stride, trans, trans_stride);
        else
            hipLaunchKernelGGL(k_render_view<false>, dim3((unsigned)grid), dim3(RV_NT), 0, st, vols, stride, D, (int)HW, (int)bpv, p, image,
                               image_stride, trans, trans_stride);
        return hipGetLastError();
    }
    const int up = light == SMK_LIGHT_POS_Y;
    const int nseg = render_segments(H), nxc = (W + 63) / 64;
    const int64_t bpp = (DW + RV_NT - 1) / RV_NT;
    const int64_t g1 = n * nseg * bpp, g2 = n * bpp, g3 = n * nseg * nxc;
    if (g1 > 0x7fffffffLL || g3 > 0x7fffffffLL) return hipErrorInvalidValue;
    float *ws = nseg > 1 ? workspace : nullptr;
    if (ws != nullptr) {
        hipLaunchKernelGGL(k_render_seg_totals, dim3((unsigned)g1), dim3(RV_NT), 0, st, vols, stride, D, H, W, nseg, (int)bpp, up, ws);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_render_seg_scan, dim3((unsigned)g2), dim3(RV_NT), 0, st, (int)DW, nseg, (int)bpp, up, ws);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
#define SMK_RENDER_LIT(DMAX)                                                                                                            \
    hipLaunchKernelGGL(k_render_lit<DMAX>, dim3((unsigned)g3), dim3(64), 0, st, vols, stride, D, H, W, nseg, nxc, up, p, ws, image, \
                       image_stride, trans, trans_stride)
    if (D <= 8) SMK_RENDER_LIT(8);
    else if (D <= 16) SMK_RENDER_LIT(16);
    else if (D <= 32) SMK_RENDER_LIT(32);
    else SMK_RENDER_LIT(64);
#undef SMK_RENDER_LIT
    return hipGetLastError();
}

// ================================================================================================================================
// The gradient.  With G / Gt the upstream gradients of image / transmittance (absent = zero), per voxel
//   T = exp(-sv tau), X = exp(-sl A), L = a + (1 - a) X, alpha = -expm1(-sv rho), c = alpha L T, E = (1 - alpha) L T,
//   S = g G alpha T (-sl (1 - a) X)                                        (what the voxel's image term gives back per unit of A)
//   drho[z,y,x] = g G sv (E - sum_{z' > z} c) - sv Gt trans + sum of S over the voxels this voxel shadows.
// Every suffix sum is formed as (total - inclusive prefix) in the forward's own direction, so tau and A are the forward's sums (a march
// in reverse would have to subtract them down from their end values, and sl * A then carries the rounding of the END value into the
// first, brightest voxels).  What a total costs is one rounding at the size of one term.  No wave skips a term here: rho = 0 has a
// gradient.
//   none : the first bracket telescopes to trans: drho = sv trans (g G - Gt) for every z.  k_render_grad_none, one read.
//   +z   : k_render_grad_view, one pixel per lane: march 1 for the totals of c and S, march 2 writes.  Two reads, one launch.
//   +-y  : k_render_seg_totals + k_render_seg_scan give A at every segment's start as in the forward (read 1);
//          k_render_grad_lit<DMAX, false> marches every segment and writes its total of S per (z, x), and per pixel
//          K = g G sv (sum_z c) + sv Gt trans, which every plane of the pixel subtracts and only the last plane completes (read 2);
//          k_render_grad_seg_scan sums those totals over the segments AFTER each one in the order of travel (workspace only);
//          k_render_grad_lit<DMAX, true> marches every segment again with, per plane, A and the S still to come in registers, and
//          writes drho = g G sv (E + prefix of c) + S to come - K plane by plane (read 3).
// Workspace of +-y: three arrays [n][segments][D][W] (A at the start, S totals, S of the later segments), also for a single segment, and
// K [n][H][W].
namespace {

struct GradTerm {
    float c, E, S;
};

__device__ __forceinline__ GradTerm grad_term(float rho, float A, float tau, float gG, const RenderParams &p) {
    const float alpha = -expm1f(p.neg_sigma_view * rho);
    const float T = __expf(p.neg_sigma_view * tau);
    const float X = __expf(p.neg_sigma_light * A);
    const float LT = (p.ambient + p.one_minus_ambient * X) * T;
    GradTerm t;
    t.c = alpha * LT;
    t.E = (1.0f - alpha) * LT;
    t.S = ((gG * alpha) * T) * ((p.neg_sigma_light * p.one_minus_ambient) * X);
    return t;
}

// the upstream pair of one pixel: gain * G and Gt (a null pointer is a zero gradient)
__device__ __forceinline__ void grad_upstream(const float *G, int64_t gstride, const float *Gt, int64_t tstride, int v, size_t pix, float gain,
                                              float *gG, float *gt) {
    *gG = G != nullptr ? gain * G[(size_t)v * gstride + pix] : 0.f;
    *gt = Gt != nullptr ? Gt[(size_t)v * tstride + pix] : 0.f;
}

// ---- light none: one pixel per lane, one read
__global__ __launch_bounds__(RV_NT) void k_render_grad_none(const float *__restrict__ vols, int64_t stride, int D, int HW, int bpv, RenderParams p,
                                                            const float *__restrict__ G, int64_t gstride, const float *__restrict__ Gt,
                                                            int64_t tstride, float *__restrict__ out, int64_t ostride) {
    const int v = blockIdx.x / bpv, pix = (blockIdx.x % bpv) * RV_NT + threadIdx.x;
    const bool ok = pix < HW;                                   // lanes past the plane read its last pixel and store nothing
    const float *f = vols + (size_t)v * stride + (ok ? pix : HW - 1);
    float tau = 0.f;
    constexpr int U = 8;
    for (int z0 = 0; z0 < D; z0 += U) {
        float r[U];
#pragma unroll
        for (int j = 0; j < U; ++j) r[j] = z0 + j < D ? f[(size_t)(z0 + j) * HW] : 0.f;
#pragma unroll
        for (int j = 0; j < U; ++j)
            if (z0 + j < D) tau += r[j];                        // the forward's order: the forward's transmittance
    }
    if (!ok) return;
    float gG, gt;
    grad_upstream(G, gstride, Gt, tstride, v, (size_t)pix, p.gain, &gG, &gt);
    const float d = (-p.neg_sigma_view * __expf(p.neg_sigma_view * tau)) * (gG - gt);
    float *o = out + (size_t)v * ostride + pix;
    for (int z = 0; z < D; ++z) o[(size_t)z * HW] = d;          // z * HW + pix < D * H * W
}

// ---- light +z: one pixel per lane, A = tau; two marches over z
__global__ __launch_bounds__(RV_NT) void k_render_grad_view(const float *__restrict__ vols, int64_t stride, int D, int HW, int bpv, RenderParams p,
                                                            const float *__restrict__ G, int64_t gstride, const float *__restrict__ Gt,
                                                            int64_t tstride, float *__restrict__ out, int64_t ostride) {
    const int v = blockIdx.x / bpv, pix = (blockIdx.x % bpv) * RV_NT + threadIdx.x;
    const bool ok = pix < HW;
    const int pc = ok ? pix : HW - 1;                           // lanes past the plane work on its last pixel and store nothing
    const float *f = vols + (size_t)v * stride + pc;
    float gG, gt;
    grad_upstream(G, gstride, Gt, tstride, v, (size_t)pc, p.gain, &gG, &gt);
    const float sv = -p.neg_sigma_view, gs = gG * sv;
    constexpr int U = 8;
    float tau = 0.f, C = 0.f, St = 0.f;
    for (int z0 = 0; z0 < D; z0 += U) {
        float r[U];
#pragma unroll
        for (int j = 0; j < U; ++j) r[j] = z0 + j < D ? f[(size_t)(z0 + j) * HW] : 0.f;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (z0 + j < D) {                                   // wave-uniform
                const GradTerm t = grad_term(r[j], tau, tau, gG, p);
                C += t.c;
                St += t.S;
                tau += r[j];
            }
        }
    }
    const float kt = (sv * gt) * __expf(p.neg_sigma_view * tau);
    float *o = out + (size_t)v * ostride + pc;
    float P = 0.f, Q = 0.f;
    tau = 0.f;
    for (int z0 = 0; z0 < D; z0 += U) {
        float r[U];
#pragma unroll
        for (int j = 0; j < U; ++j) r[j] = z0 + j < D ? f[(size_t)(z0 + j) * HW] : 0.f;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (z0 + j < D) {
                const GradTerm t = grad_term(r[j], tau, tau, gG, p);       // the same bits as in march 1
                P += t.c;
                Q += t.S;
                tau += r[j];
                const float d = (gs * ((t.E + P) - C) - kt) + (St - Q);
                if (ok) o[(size_t)(z0 + j) * HW] = d;
            }
        }
    }
}

// ---- light +-y: sum of in[s'] over the segments s' after s in the order of travel (out of place: the totals are used again)
__global__ __launch_bounds__(RV_NT) void k_render_grad_seg_scan(int DW, int nseg, int bpp, int up, const float *__restrict__ in,
                                                                float *__restrict__ out) {
    const int v = blockIdx.x / bpp, q = (blockIdx.x % bpp) * RV_NT + threadIdx.x;
    if (q >= DW) return;
    const size_t base = (size_t)v * nseg * DW + q;
    float run = 0.f;
#pragma unroll 4
    for (int k = 0; k < nseg; ++k) {
        const int s = up ? nseg - 1 - k : k;                   // against the order of travel
        out[base + (size_t)s * DW] = run;
        run += in[base + (size_t)s * DW];
    }
}

// ---- light +-y: one wave = 64 columns x one segment, as k_render_lit.  FINAL = false: wsS[v][s][z][x] = the segment's sum of S.
// and wsK[v][y][x] = K.  FINAL = true: drho of the segment's rows; Sl[z] is the S of everything the row's voxel shadows (the rows after
// it in this segment and all later segments).
template <int DMAX, bool FINAL>
__global__ __launch_bounds__(64) void k_render_grad_lit(const float *__restrict__ vols, int64_t stride, int D, int H, int W, int nseg, int nxc,
                                                        int up, RenderParams p, const float *__restrict__ wsA, float *wsS, const float *wsR,
                                                        float *wsK, const float *__restrict__ G, int64_t gstride, const float *__restrict__ Gt,
                                                        int64_t tstride, float *out, int64_t ostride) {
    unsigned id = blockIdx.x;
    const int xc = id % nxc; id /= nxc;
    const int s = id % nseg, v = id / nseg;
    const int x = xc * 64 + threadIdx.x;
    const bool ok = x < W;
    const int xl = ok ? (int)threadIdx.x : W - 1 - xc * 64;    // lanes past the row work on its last column and store nothing
    const unsigned lane_b = 4u * (unsigned)xl;
    const char *f = reinterpret_cast<const char *>(vols + (size_t)v * stride + xc * 64);
    const size_t wofs = ((size_t)v * nseg + s) * D * W + xc * 64;          // + z * W + xl < n * nseg * D * W
    float A[DMAX], Sl[DMAX];
#pragma unroll
    for (int z = 0; z < DMAX; ++z) {
        A[z] = z < D ? wsA[wofs + (size_t)z * W + xl] : 0.f;
        Sl[z] = (FINAL && z < D) ? wsS[wofs + (size_t)z * W + xl] + wsR[wofs + (size_t)z * W + xl] : 0.f;
    }
    const float sv = -p.neg_sigma_view;
    int rows;
    (void)seg_row(s, 0, H, up, &rows);
    for (int i = 0; i < rows; ++i) {
        int dummy;
        const int y = seg_row(s, i, H, up, &dummy);
        int Dr = D;
        asm volatile("" : "+s"(Dr));                           // D again, opaque per row (k_render_lit)
        float gG, gt;
        grad_upstream(G, gstride, Gt, tstride, v, (size_t)y * W + xc * 64 + xl, p.gain, &gG, &gt);
        const float gs = gG * sv;
        const char *row = f + (size_t)y * W * 4;               // (z * H + y) * W + x < D * H * W
        float tau = 0.f, P = 0.f;
        const size_t kofs = (size_t)v * H * W + (size_t)y * W + xc * 64 + xl;      // < n * H * W
        float K = 0.f;
        if constexpr (FINAL) K = wsK[kofs];
        float *o = out + (size_t)v * ostride + (size_t)y * W + x;
        constexpr int RC = DMAX < 16 ? DMAX : 16;              // planes loaded ahead of their terms
#pragma unroll
        for (int z0 = 0; z0 < DMAX; z0 += RC) {
            float r[RC];
#pragma unroll
            for (int j = 0; j < RC; ++j) {                     // planes past D load plane D - 1 again (never used)
                r[j] = *reinterpret_cast<const float *>(row + lane_b);
                row += z0 + j + 1 < Dr ? (size_t)H * W * 4 : 0;
            }
#pragma unroll
            for (int j = 0; j < RC; ++j) {
                if (z0 + j < Dr) {                             // wave-uniform
                    const GradTerm t = grad_term(r[j], A[z0 + j], tau, gG, p);
                    P += t.c;
                    if constexpr (FINAL) {
                        Sl[z0 + j] -= t.S;
                        if (ok) o[(size_t)(z0 + j) * H * W] = (gs * (t.E + P) + Sl[z0 + j]) - K;
                    } else {
                        Sl[z0 + j] += t.S;
                    }
                    tau += r[j];
                    A[z0 + j] += r[j];
                }
            }
        }
        if constexpr (!FINAL) {                                // what every plane of this pixel subtracts: known after the last plane only
            if (ok) wsK[kofs] = gs * P + (sv * gt) * __expf(p.neg_sigma_view * tau);
        }
    }
    if constexpr (!FINAL) {
#pragma unroll
        for (int z = 0; z < DMAX; ++z)
            if (z < D && ok) wsS[wofs + (size_t)z * W + xl] = Sl[z];
    }
}

}  // namespace

int64_t render_backward_workspace(int64_t n, int D, int H, int W, int light) {
    if (light != SMK_LIGHT_POS_Y && light != SMK_LIGHT_NEG_Y) return 0;
    return (3 * n * render_segments(H) * (int64_t)D * W + n * (int64_t)H * W) * (int64_t)sizeof(float);
}

hipError_t launch_volume_render_backward(const float *vols, int64_t stride, int64_t n, int D, int H, int W, int light, const RenderParams &p,
                                         const float *G, int64_t gstride, const float *Gt, int64_t tstride, float *out, int64_t ostride,
                                         float *workspace, hipStream_t st) {
    const int64_t HW = (int64_t)H * W, DW = (int64_t)D * W;
    if (light == SMK_LIGHT_NONE || light == SMK_LIGHT_POS_Z) {
        const int64_t bpv = (HW + RV_NT - 1) / RV_NT, grid = n * bpv;
        if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
        if (light == SMK_LIGHT_POS_Z)
            hipLaunchKernelGGL(k_render_grad_view, dim3((unsigned)grid), dim3(RV_NT), 0, st, vols, stride, D, (int)HW, (int)bpv, p, G, gstride, Gt,
                               tstride, out, ostride);
        else
            hipLaunchKernelGGL(k_render_grad_none, dim3((unsigned)grid), dim3(RV_NT), 0, st, vols, stride, D, (int)HW, (int)bpv, p, G, gstride, Gt,
                               tstride, out, ostride);
        return hipGetLastError();
    }
    const int up = light == SMK_LIGHT_POS_Y;
    const int nseg = render_segments(H), nxc = (W + 63) / 64;
    const int64_t bpp = (DW + RV_NT - 1) / RV_NT;
    const int64_t g1 = n * nseg * bpp, g2 = n * bpp, g3 = n * nseg * nxc;
    if (g1 > 0x7fffffffLL || g3 > 0x7fffffffLL) return hipErrorInvalidValue;
    float *wsA = workspace, *wsS = wsA + n * nseg * DW, *wsR = wsS + n * nseg * DW, *wsK = wsR + n * nseg * DW;
    hipError_t e;
    hipLaunchKernelGGL(k_render_seg_totals, dim3((unsigned)g1), dim3(RV_NT), 0, st, vols, stride, D, H, W, nseg, (int)bpp, up, wsA);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_render_seg_scan, dim3((unsigned)g2), dim3(RV_NT), 0, st, (int)DW, nseg, (int)bpp, up, wsA);
    if ((e = hipGetLastError()) != hipSuccess) return e;
#define SMK_RENDER_GRAD_LIT(DMAX, FINAL)                                                                                                  \
    hipLaunchKernelGGL((k_render_grad_lit<DMAX, FINAL>), dim3((unsigned)g3), dim3(64), 0, st, vols, stride, D, H, W, nseg, nxc, up, p, wsA, wsS, \
                       wsR, wsK, G, gstride, Gt, tstride, out, ostride)
#define SMK_RENDER_GRAD_PASS(FINAL)                                                                                                       \
    do {                                                                                                                                  \
        if (D <= 8) SMK_RENDER_GRAD_LIT(8, FINAL);                                                                                        \
        else if (D <= 16) SMK_RENDER_GRAD_LIT(16, FINAL);                                                                                 \
        else if (D <= 32) SMK_RENDER_GRAD_LIT(32, FINAL);                                                                                 \
        else SMK_RENDER_GRAD_LIT(64, FINAL);                                                                                              \
    } while (0)
    SMK_RENDER_GRAD_PASS(false);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_render_grad_seg_scan, dim3((unsigned)g2), dim3(RV_NT), 0, st, (int)DW, nseg, (int)bpp, up, wsS, wsR);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    SMK_RENDER_GRAD_PASS(true);
#undef SMK_RENDER_GRAD_PASS
#undef SMK_RENDER_GRAD_LIT
    return hipGetLastError();
}


// ================================================================================================================================
// The host-side checks of the four entry points (render.h).
bool render_query_ok(const RenderLimits &lim, int32_t n, int32_t D, int32_t H, int32_t W, int32_t light) {
    return n >= 1 && D >= 1 && D <= lim.max_depth && H >= 1 && (lim.max_height == 0 || H <= lim.max_height) && W >= 1 &&
           (lim.max_width == 0 || W <= lim.max_width) && (int64_t)D * H * W <= RENDER_MAX_CELLS && light >= SMK_LIGHT_NONE &&
           light <= (lim.moving ? SMK_LIGHT_NEG_Y : SMK_LIGHT_POS_Z);
}

int render_check(const char *name, const RenderLimits &lim, int32_t n, int32_t D, int32_t H, int32_t W, int32_t n_views,
                 const smk_render_desc *desc, const void *vols, int64_t vol_stride, std::initializer_list<RenderBuffer> bufs,
                 const void *workspace, RenderParams *p) {
    if (lim.moving) {
        SMK_REQUIRE(n >= 1 && D >= 1 && H >= 1 && W >= 1 && n_views >= 1, "n, D, H, W, n_views >= 1");
        SMK_REQUIRE((int64_t)n * n_views <= RENDER_MAX_PLANES, "n * n_views <= 2^20");
    } else {
        SMK_REQUIRE(n >= 1 && D >= 1 && H >= 1 && W >= 1, "n, D, H, W >= 1");
    }
    if (!render_query_ok(lim, n, D, H, W, SMK_LIGHT_NONE)) {
        set_error(std::string(name) + ": D <= " + std::to_string(lim.max_depth) +
                  (lim.max_height ? ", H <= " + std::to_string(lim.max_height) : "") +
                  (lim.max_width ? ", W <= " + std::to_string(lim.max_width) : "") + " and D*H*W <= 2^31 - 2^16 are built (got D=" +
                  std::to_string(D) + ", H=" + std::to_string(H) + ", W=" + std::to_string(W) + ")");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(desc->light >= SMK_LIGHT_NONE && desc->light <= SMK_LIGHT_POS_Z, "light: one of smk_light");
    if (lim.moving && desc->light == SMK_LIGHT_POS_Z) {
        set_error(std::string(name) + ": SMK_LIGHT_POS_Z is not built for " + lim.moving + " (a world-fixed +z light seen obliquely is "
                  "another prefix); SMK_LIGHT_NONE, SMK_LIGHT_POS_Y and SMK_LIGHT_NEG_Y are");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(desc->sigma_view >= 0 && desc->sigma_light >= 0 && desc->ambient >= 0 && desc->ambient <= 1 && desc->gain > 0,
                "sigma_view, sigma_light >= 0; 0 <= ambient <= 1; gain > 0");
    const int64_t cells = (int64_t)D * H * W, HW = (int64_t)H * W, planes = lim.moving ? (int64_t)n * n_views : n;
    SMK_REQUIRE(vol_stride >= cells || n == 1, "vol_stride >= D*H*W");
    uintptr_t low_bits = (uintptr_t)vols | (uintptr_t)workspace;
    for (const RenderBuffer &b : bufs) {
        SMK_REQUIRE(b.ptr == nullptr || b.stride >= (b.volume ? cells : HW) || (b.volume ? n : planes) == 1,
                    std::string(b.stride_name) + (b.volume ? " >= D*H*W" : " >= H*W"));
        low_bits |= (uintptr_t)b.ptr;
    }
    SMK_REQUIRE((low_bits & 3) == 0, "4-byte aligned pointers");
    p->neg_sigma_view = (float)-desc->sigma_view;
    p->neg_sigma_light = (float)-desc->sigma_light;
    p->ambient = (float)desc->ambient;
    p->one_minus_ambient = (float)(1.0 - desc->ambient);
    p->gain = (float)desc->gain;
    return SMK_OK;
}

int render_check_workspace(const char *name, int64_t need, const void *workspace, int64_t workspace_bytes) {
    SMK_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
                std::string("workspace smaller than smk_") + name + "_workspace(n, D, H, W, light)");
    return SMK_OK;
}

int render_launch_status(const char *name, hipError_t e) {
    if (e == hipSuccess) return SMK_OK;
    set_error(std::string(name) + ": " + hipGetErrorString(e));
    return SMK_ERR_HIP;
}

}  // namespace smk

using namespace smk;

#pragma GCC visibility push(default)
extern "C" {

static constexpr RenderLimits FRONT = {RENDER_MAX_DEPTH, 0, 0, nullptr};

int64_t smk_volume_render_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light) {
    return render_query_ok(FRONT, n, D, H, W, light) ? render_workspace(n, D, H, W, light) : -1;
}

int smk_volume_render(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, const smk_render_desc *desc,
                      float *image, int64_t image_stride, float *transmittance, int64_t trans_stride, void *workspace,
                      int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(vols && desc && image, "null pointer");
    RenderParams p;
    int rc = render_check("volume_render", FRONT, n, D, H, W, 0, desc, vols, vol_stride,
                          {{image, image_stride, false, "image_stride"}, {transmittance, trans_stride, false, "trans_stride"}}, workspace, &p);
    if (rc == SMK_OK) rc = render_check_workspace("volume_render", render_workspace(n, D, H, W, desc->light), workspace, workspace_bytes);
    if (rc != SMK_OK) return rc;
    return render_launch_status("volume_render", launch_volume_render(vols, vol_stride, n, D, H, W, desc->light, p, image, image_stride,
                                                                      transmittance, trans_stride, (float *)workspace, (hipStream_t)stream));
}

int64_t smk_volume_render_backward_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light) {
    return render_query_ok(FRONT, n, D, H, W, light) ? render_backward_workspace(n, D, H, W, light) : -1;
}

int smk_volume_render_backward(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, const smk_render_desc *desc,
                               const float *grad_image, int64_t grad_image_stride, const float *grad_trans, int64_t grad_trans_stride,
                               float *grad_vols, int64_t grad_vol_stride, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(vols && desc && grad_vols, "null pointer");
    SMK_REQUIRE(grad_image || grad_trans, "grad_image and grad_trans are both null: there is no gradient to carry back");
    RenderParams p;
    int rc = render_check("volume_render_backward", FRONT, n, D, H, W, 0, desc, vols, vol_stride,
                          {{grad_vols, grad_vol_stride, true, "grad_vol_stride"},
                           {grad_image, grad_image_stride, false, "grad_image_stride"},
                           {grad_trans, grad_trans_stride, false, "grad_trans_stride"}}, workspace, &p);
    if (rc == SMK_OK)
        rc = render_check_workspace("volume_render_backward", render_backward_workspace(n, D, H, W, desc->light), workspace, workspace_bytes);
    if (rc != SMK_OK) return rc;
    return render_launch_status("volume_render_backward",
                                launch_volume_render_backward(vols, vol_stride, n, D, H, W, desc->light, p, grad_image, grad_image_stride,
                                                              grad_trans, grad_trans_stride, grad_vols, grad_vol_stride, (float *)workspace,
                                                              (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
