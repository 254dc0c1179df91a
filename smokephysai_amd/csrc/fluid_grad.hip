// Adjoint of one 2-D stable-fluids step (navier_stokes.py:151-173) with respect to its state (u, v, p, density): the backward kernels
// behind smk_advect_backward, smk_project_backward and smk_buoy_diffuse_backward.  DESIGN.md section 3.9.
//
// Arithmetic rules (the project's gradient rules): fp32 throughout, every sum in one fixed order, no atomics, every output element written,
// results bit-identical from call to call and independent of a grid's batch mates.  The back-trace positions, indices, clamp decisions and
// weights are formed by the forward's own expressions (csrc/fluid_trace.h, shared with csrc/fluid_tangent.hip), so they are the forward's
// bit for bit and the backward is the transpose of what the forward used.
#include "fluid_grad.h"
#include "fluid_trace.h"

namespace smk {

namespace {

// ---------------------------------------------------------------- advection backward
// out = adv(f; u, v).  A workgroup owns a FG_TY x FG_TX tile of SOURCE cells of the union domain [H+1][W+1] (it holds u [H+1][W], v [H][W+1]
// and the field [R][C]).  Pass 1 forms, for every DESTINATION cell of the tile plus a one-cell halo, the record the forward's own arithmetic
// gives -- the four clamped taps, the four weights times g, and -dt * gpx, -dt * gpy -- into LDS.  Pass 2 gathers: dfield[j] from the 3 x 3
// destinations around j (row-major, taps wa, wb, wc, wd), du[j] from the destinations (y, x-1), (y, x), dv[j] from (y-1, x), (y, x), whose
// velocity samples are the only ones that can tap j.  Taps are matched by comparing coordinates, never used as LDS indices, so a far
// back-trace (|displacement| >= 1 cell) only loses terms: it raises the grid's far word and the caller discards the grid.
template <int WHICH>
__global__ __launch_bounds__(FG_NT) void k_advect_backward(Geom g, const float *__restrict__ field, const float *__restrict__ u,
                                                           const float *__restrict__ v, const float *__restrict__ gout,
                                                           float *__restrict__ dfield, float *__restrict__ du, float *__restrict__ dv,
                                                           int32_t *far) {
    constexpr bool IS_U = WHICH == 0, IS_V = WHICH == 1;
    const int R = IS_U ? g.H + 1 : g.H, C = IS_V ? g.W + 1 : g.W;
    const int pitch = IS_V ? g.pv : g.pc;
    const size_t fs = IS_U ? g.su : (IS_V ? g.sv : g.sc);
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * FG_TX, ty0 = blockIdx.y * FG_TY;
    const float *ub = u + b * g.su, *vb = v + b * g.sv, *fb = field + b * fs, *gb = gout + b * fs;

    __shared__ float s_w[4][FG_REC];          // weight * g of the taps (y0,x0), (y0,x1), (y1,x0), (y1,x1)
    __shared__ float s_tx[FG_REC], s_ty[FG_REC];      // -dt * gpx, -dt * gpy
    __shared__ int s_x[FG_REC], s_y[FG_REC];  // x0 | x1 << 16, y0 | y1 << 16; -1: no such destination

    const int tid = threadIdx.x;
    for (int r = tid; r < FG_REC; r += FG_NT) {
        const int Y = ty0 - 1 + r / FG_HX, X = tx0 - 1 + r % FG_HX;
        float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f, tx = 0.f, ty = 0.f;
        int xs = -1, ys = -1;
        if (Y >= 0 && Y < R && X >= 0 && X < C) {
            const Trace tr = trace_at(g, R, C, pitch, ub, vb, fb, Y, X);
            if (!(fabsf(tr.pxu - (float)X) < 1.0f) || !(fabsf(tr.pyu - (float)Y) < 1.0f)) far[b] = 1;   // (NaN included; every writer stores the same 1)
            const Taps &t = tr.t;
            float gi = gb[(size_t)Y * pitch + X];
            if (WHICH == 2) gi = gi * 0.995f;                                   // :171
            w0 = gi * t.wa; w1 = gi * t.wb; w2 = gi * t.wc; w3 = gi * t.wd;
            const float gpx = tr.pass_x ? gi * tr.sx : 0.f;
            const float gpy = tr.pass_y ? gi * tr.sy : 0.f;
            tx = -(g.dt * gpx); ty = -(g.dt * gpy);
            xs = t.x0 | (t.x1 << 16); ys = t.y0 | (t.y1 << 16);
        }
        s_w[0][r] = w0; s_w[1][r] = w1; s_w[2][r] = w2; s_w[3][r] = w3;
        s_tx[r] = tx; s_ty[r] = ty; s_x[r] = xs; s_y[r] = ys;
    }
    __syncthreads();

    const int lx = tid % FG_TX, ly = tid / FG_TX;
    const int x = tx0 + lx, y = ty0 + ly;
    const int rc = (ly + 1) * FG_HX + (lx + 1);          // this cell's own record
    if (y < R && x < C) {
        float acc = 0.f;
        for (int dy = -1; dy <= 1; ++dy) {
            for (int dx = -1; dx <= 1; ++dx) {
                const int r = rc + dy * FG_HX + dx;
                const int xs = s_x[r], ys = s_y[r];
                if (xs < 0) continue;
                const bool mx0 = (xs & 0xffff) == x, mx1 = (xs >> 16) == x, my0 = (ys & 0xffff) == y, my1 = (ys >> 16) == y;
                if (my0 && mx0) acc = acc + s_w[0][r];
                if (my0 && mx1) acc = acc + s_w[1][r];
                if (my1 && mx0) acc = acc + s_w[2][r];
                if (my1 && mx1) acc = acc + s_w[3][r];
            }
        }
        dfield[b * fs + (size_t)y * pitch + x] = acc;
    }
    if (y <= g.H && x < g.W) {                           // du[y][x]: the u samples of the destinations (y, x-1) and (y, x)
        float acc = 0.f;
        for (int dx = -1; dx <= 0; ++dx) {
            const int X = x + dx;
            if (y >= R || X < 0 || X >= C) continue;
            const Taps t = u_sample_taps(g, y, X);       // row y0 = y carries the whole sample: the weights of row y1 are exact zeros
            const float tpx = s_tx[rc + dx];
            if (t.y0 == y && t.x0 == x) acc = acc + tpx * t.wa;
            if (t.y0 == y && t.x1 == x) acc = acc + tpx * t.wb;
        }
        du[b * g.su + (size_t)y * g.pc + x] = acc;
    }
    if (y < g.H && x <= g.W) {                           // dv[y][x]: the v samples of the destinations (y-1, x) and (y, x)
        float acc = 0.f;
        for (int dy = -1; dy <= 0; ++dy) {
            const int Y = y + dy;
            if (x >= C || Y < 0 || Y >= R) continue;
            const Taps t = v_sample_taps(g, Y, x);       // column x0 = x carries the whole sample
            const float tpy = s_ty[rc + dy * FG_HX];
            if (t.x0 == x && t.y0 == y) acc = acc + tpy * t.wa;
            if (t.x0 == x && t.y1 == y) acc = acc + tpy * t.wc;
        }
        dv[b * g.sv + (size_t)y * g.pv + x] = acc;
    }
}

// ---------------------------------------------------------------- projection backward
// lambda = gp with the gradient subtraction's transpose added (navier_stokes.py:148-149); ddiv = 0.  lam, ddiv: dense [B][H][W].
__global__ void k_project_backward_init(Geom g, const float *__restrict__ gu, const float *__restrict__ gv, const float *__restrict__ gp,
                                        float *__restrict__ lam, float *__restrict__ ddiv) {
    const int b = blockIdx.z, x = blockIdx.x * FG_TX + threadIdx.x % FG_TX, y = blockIdx.y * FG_TY + threadIdx.x / FG_TX;
    if (y >= g.H || x >= g.W) return;
    const float *gub = gu + b * g.su, *gvb = gv + b * g.sv;
    float l = gp[b * g.sc + (size_t)y * g.pc + x];
    if (y >= 1) l = l - g.dt * gub[(size_t)y * g.pc + x];
    if (y <= g.H - 2) l = l + g.dt * gub[(size_t)(y + 1) * g.pc + x];
    if (x >= 1) l = l - g.dt * gvb[(size_t)y * g.pv + x];
    if (x <= g.W - 2) l = l + g.dt * gvb[(size_t)y * g.pv + x + 1];
    const size_t o = ((size_t)b * g.H + y) * g.W + x;
    lam[o] = l;
    ddiv[o] = 0.f;
}

// T <= FG_PB_T transposed Jacobi sweeps (navier_stokes.py:139-145) in one launch.  One sweep: m = lambda on the interior, 0 on the ring;
// ddiv -= 0.25 m; lambda' = 0.25 (up + down + left + right) of m on all cells, cells outside the grid counting 0.  A workgroup owns a
// 32 x 32 tile: it loads the masked lambda of the tile plus a halo of T cells into LDS, sweeps T times between two LDS planes (the region
// that is still exact shrinks by one cell per sweep and ends as the tile), keeps its cells' ddiv in registers meanwhile, and writes lambda
// and ddiv once.  Per cell the operations and their order are those of a single sweep, so the result does not depend on T.
__global__ __launch_bounds__(FG_NT) void k_project_backward_sweeps(int H, int W, int T, const float *__restrict__ lam_in,
                                                                   float *__restrict__ lam_out, float *__restrict__ ddiv) {
    constexpr int PT = FG_PB_TILE, RS = PT + 2 * FG_PB_T, CELLS = PT * PT / FG_NT;
    __shared__ float buf[2][RS * RS];
    const int b = blockIdx.z, tx0 = blockIdx.x * PT, ty0 = blockIdx.y * PT, tid = threadIdx.x;
    const size_t plane = (size_t)b * H * W;
    const float *l = lam_in + plane;
    const int rs = PT + 2 * T;                                   // side of the region loaded; its origin is (ty0 - T, tx0 - T)
    auto interior = [&](int ry, int rx) {
        const int y = ty0 - T + ry, x = tx0 - T + rx;
        return y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2;
    };
    for (int i = tid; i < rs * rs; i += FG_NT) {
        const int ry = i / rs, rx = i % rs;
        buf[0][ry * RS + rx] = interior(ry, rx) ? l[(size_t)(ty0 - T + ry) * W + (tx0 - T + rx)] : 0.f;
    }
    float acc[CELLS];
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const int c = tid + k * FG_NT, y = ty0 + c / PT, x = tx0 + c % PT;
        acc[k] = (y < H && x < W) ? ddiv[plane + (size_t)y * W + x] : 0.f;
    }
    auto swept = [&](const float *c, int ry, int rx) {           // 0.25 (up + down + left + right) at a region cell
        float s = c[(ry - 1) * RS + rx] + c[(ry + 1) * RS + rx];
        s = s + c[ry * RS + rx - 1];
        s = s + c[ry * RS + rx + 1];
        return 0.25f * s;
    };
    int cur = 0;
    for (int s = 0; s < T; ++s) {
        __syncthreads();
        const float *c = buf[cur];
#pragma unroll
        for (int k = 0; k < CELLS; ++k) {
            const int cell = tid + k * FG_NT;
            acc[k] = acc[k] - 0.25f * c[(cell / PT + T) * RS + cell % PT + T];
        }
        if (s < T - 1) {
            float *n = buf[cur ^ 1];
            const int lo = s + 1, side = rs - 2 * lo;
            for (int i = tid; i < side * side; i += FG_NT) {
                const int ry = lo + i / side, rx = lo + i % side;
                const float v = swept(c, ry, rx);
                n[ry * RS + rx] = interior(ry, rx) ? v : 0.f;
            }
            cur ^= 1;
        } else {
#pragma unroll
            for (int k = 0; k < CELLS; ++k) {
                const int cell = tid + k * FG_NT, y = ty0 + cell / PT, x = tx0 + cell % PT;
                if (y < H && x < W) lam_out[plane + (size_t)y * W + x] = swept(c, cell / PT + T, cell % PT + T);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const int c = tid + k * FG_NT, y = ty0 + c / PT, x = tx0 + c % PT;
        if (y < H && x < W) ddiv[plane + (size_t)y * W + x] = acc[k];
    }
}

// dp = lambda; with gd = ddiv / dt (the divergence's true divide, navier_stokes.py:136): du = gu + gd[y-1] - gd[y], dv = gv + gd[x-1] - gd[x].
__global__ void k_project_backward_final(Geom g, const float *__restrict__ gu, const float *__restrict__ gv, const float *__restrict__ lam,
                                         const float *__restrict__ ddiv, float *__restrict__ du, float *__restrict__ dv,
                                         float *__restrict__ dp) {
    const int b = blockIdx.z, x = blockIdx.x * FG_TX + threadIdx.x % FG_TX, y = blockIdx.y * FG_TY + threadIdx.x / FG_TX;
    const float *dd = ddiv + (size_t)b * g.H * g.W;
    if (y < g.H && x < g.W) dp[b * g.sc + (size_t)y * g.pc + x] = lam[((size_t)b * g.H + y) * g.W + x];
    if (y <= g.H && x < g.W) {
        float r = gu[b * g.su + (size_t)y * g.pc + x];
        if (y >= 1) r = r + __fdiv_rn(dd[(size_t)(y - 1) * g.W + x], g.dt);
        if (y <= g.H - 1) r = r - __fdiv_rn(dd[(size_t)y * g.W + x], g.dt);
        du[b * g.su + (size_t)y * g.pc + x] = r;
    }
    if (y < g.H && x <= g.W) {
        float r = gv[b * g.sv + (size_t)y * g.pv + x];
        if (x >= 1) r = r + __fdiv_rn(dd[(size_t)y * g.W + x - 1], g.dt);
        if (x <= g.W - 1) r = r - __fdiv_rn(dd[(size_t)y * g.W + x], g.dt);
        dv[b * g.sv + (size_t)y * g.pv + x] = r;
    }
}

// ---------------------------------------------------------------- diffusion + buoyancy backward
// diffusion_step with replicate padding is symmetric (navier_stokes.py:50-72): its transpose is itself.
__device__ __forceinline__ float fg_diffuse_at(const float *f, int R, int C, int pitch, int i, int j, float coef) {
    const int iu = i > 0 ? i - 1 : 0, id = i < R - 1 ? i + 1 : R - 1;
    const int jl = j > 0 ? j - 1 : 0, jr = j < C - 1 ? j + 1 : C - 1;
    const float c = f[(size_t)i * pitch + j];
    float lap = f[(size_t)iu * pitch + j] + f[(size_t)id * pitch + j];
    lap = lap + f[(size_t)i * pitch + jl];
    lap = lap + f[(size_t)i * pitch + jr];
    lap = lap - 4.0f * c;
    return c + coef * lap;
}

// du = Diff_nu(gu); dv = Diff_nu(gv); ddensity = Diff_{0.1 nu}(gd) + 0.1 (dt dv[:, :-1])  (buoyancy, navier_stokes.py:154-155).
__global__ void k_buoy_diffuse_backward(Geom g, const float *__restrict__ gu, const float *__restrict__ gv, const float *__restrict__ gd,
                                        float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dd) {
    const int b = blockIdx.z, x = blockIdx.x * FG_TX + threadIdx.x % FG_TX, y = blockIdx.y * FG_TY + threadIdx.x / FG_TX;
    if (y <= g.H && x < g.W)
        du[b * g.su + (size_t)y * g.pc + x] = fg_diffuse_at(gu + b * g.su, g.H + 1, g.W, g.pc, y, x, g.coef_uv);
    if (y < g.H && x <= g.W) {
        const float r = fg_diffuse_at(gv + b * g.sv, g.H, g.W + 1, g.pv, y, x, g.coef_uv);
        dv[b * g.sv + (size_t)y * g.pv + x] = r;
        if (x < g.W) {
            const float t = g.dt * r;
            dd[b * g.sc + (size_t)y * g.pc + x] = fg_diffuse_at(gd + b * g.sc, g.H, g.W, g.pc, y, x, g.coef_d) + t * 0.1f;
        }
    }
}

dim3 union_grid(const Geom &g) { return dim3((unsigned)cdiv(g.W + 1, FG_TX), (unsigned)cdiv(g.H + 1, FG_TY), (unsigned)g.B); }
dim3 cell_grid(const Geom &g) { return dim3((unsigned)cdiv(g.W, FG_TX), (unsigned)cdiv(g.H, FG_TY), (unsigned)g.B); }

}  // namespace

hipError_t launch_advect_backward(const Geom &g, int which, const float *field, const float *u, const float *v, const float *gout,
                                  float *dfield, float *du, float *dv, int32_t *far, hipStream_t st) {
    hipError_t e = hipMemsetAsync(far, 0, (size_t)g.B * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const dim3 grid = union_grid(g), block(FG_NT);
    if (which == 0) hipLaunchKernelGGL(k_advect_backward<0>, grid, block, 0, st, g, field, u, v, gout, dfield, du, dv, far);
    else if (which == 1) hipLaunchKernelGGL(k_advect_backward<1>, grid, block, 0, st, g, field, u, v, gout, dfield, du, dv, far);
    else hipLaunchKernelGGL(k_advect_backward<2>, grid, block, 0, st, g, field, u, v, gout, dfield, du, dv, far);
    return hipGetLastError();
}

hipError_t launch_project_backward(const Geom &g, const float *gu, const float *gv, const float *gp, float *du, float *dv, float *dp,
                                   int iters, float *ws, hipStream_t st) {
    const size_t n = (size_t)g.B * g.H * g.W;
    float *lam = ws, *lam2 = ws + n, *ddiv = ws + 2 * n;
    const dim3 block(FG_NT);
    hipLaunchKernelGGL(k_project_backward_init, cell_grid(g), block, 0, st, g, gu, gv, gp, lam, ddiv);
    const dim3 tiles((unsigned)cdiv(g.W, FG_PB_TILE), (unsigned)cdiv(g.H, FG_PB_TILE), (unsigned)g.B);
    for (int done = 0; done < iters; done += FG_PB_T) {
        const int T = iters - done < FG_PB_T ? iters - done : FG_PB_T;
        hipLaunchKernelGGL(k_project_backward_sweeps, tiles, block, 0, st, g.H, g.W, T, (const float *)lam, lam2, ddiv);
        float *t = lam; lam = lam2; lam2 = t;
    }
    hipLaunchKernelGGL(k_project_backward_final, union_grid(g), block, 0, st, g, gu, gv, (const float *)lam, (const float *)ddiv, du, dv, dp);
    return hipGetLastError();
}

hipError_t launch_buoy_diffuse_backward(const Geom &g, const float *gu, const float *gv, const float *gd, float *du, float *dv, float *dd,
                                        hipStream_t st) {
    hipLaunchKernelGGL(k_buoy_diffuse_backward, union_grid(g), dim3(FG_NT), 0, st, g, gu, gv, gd, du, dv, dd);
    return hipGetLastError();
}

}  // namespace smk

using namespace smk;

namespace {

// Shapes every entry point of this file takes: fluid_trace.h's.
const char *const FG_SHAPE = "1 <= B <= 65535, 3 <= H, W <= 32766, pitch_c >= W, pitch_v >= W + 1";

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int smk_advect_backward(int32_t which, const float *field, const float *u, const float *v, const float *gout, float *dfield, float *du,
                        float *dv, int32_t *far, int32_t B, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, double dt,
                        void *stream) {
    SMK_REQUIRE(field && u && v && gout && dfield && du && dv && far, "advect_backward: null pointer");
    SMK_REQUIRE(which >= 0 && which <= 2, "advect_backward: which in 0..2");
    SMK_REQUIRE(fluid2d_shape_ok(B, H, W, pitch_c, pitch_v), FG_SHAPE);
    SMK_REQUIRE(dfield != field && dfield != gout && dfield != u && dfield != v && du != u && du != field && du != gout && dv != v &&
                    dv != field && dv != gout && dfield != du && dfield != dv && du != dv,
                "advect_backward: an output aliases an input or another output");
    const Geom g = fluid2d_geom(B, H, W, pitch_c, pitch_v, dt, 0.0);
    return check_launch(launch_advect_backward(g, which, field, u, v, gout, dfield, du, dv, far, (hipStream_t)stream), "advect_backward");
}

int64_t smk_project_backward_workspace(int32_t B, int32_t H, int32_t W) {
    if (!fluid2d_shape_ok(B, H, W, W, W + 1)) return -1;
    return (int64_t)3 * B * H * W * (int64_t)sizeof(float);
}

int smk_project_backward(const float *gu, const float *gv, const float *gp, float *du, float *dv, float *dp, int32_t B, int32_t H,
                         int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t jacobi_iters, double dt, void *workspace,
                         int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(gu && gv && gp && du && dv && dp, "project_backward: null pointer");
    SMK_REQUIRE(fluid2d_shape_ok(B, H, W, pitch_c, pitch_v), FG_SHAPE);
    SMK_REQUIRE(jacobi_iters >= 0, "project_backward: jacobi_iters >= 0");
    SMK_REQUIRE(dt != 0.0, "project_backward: dt != 0");
    SMK_REQUIRE(du != gu && dv != gv && dp != gp, "project_backward: an output aliases its input");
    SMK_REQUIRE(workspace && workspace_bytes >= smk_project_backward_workspace(B, H, W),
                "project_backward: workspace smaller than smk_project_backward_workspace(B, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 3) == 0, "project_backward: workspace must be 4-byte aligned");
    const Geom g = fluid2d_geom(B, H, W, pitch_c, pitch_v, dt, 0.0);
    return check_launch(launch_project_backward(g, gu, gv, gp, du, dv, dp, jacobi_iters, (float *)workspace, (hipStream_t)stream),
                     "project_backward");
}

int smk_buoy_diffuse_backward(const float *gu, const float *gv, const float *gd, float *du, float *dv, float *dd, int32_t B, int32_t H,
                              int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, double viscosity, void *stream) {
    SMK_REQUIRE(gu && gv && gd && du && dv && dd, "buoy_diffuse_backward: null pointer");
    SMK_REQUIRE(fluid2d_shape_ok(B, H, W, pitch_c, pitch_v), FG_SHAPE);
    SMK_REQUIRE(du != gu && dv != gv && dd != gd, "buoy_diffuse_backward: an output aliases its input");
    const Geom g = fluid2d_geom(B, H, W, pitch_c, pitch_v, dt, viscosity);
    return check_launch(launch_buoy_diffuse_backward(g, gu, gv, gd, du, dv, dd, (hipStream_t)stream), "buoy_diffuse_backward");
}

}  // extern "C"
#pragma GCC visibility pop
