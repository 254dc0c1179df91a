// Adjoint of one 3-D stable-fluids step (SPEC_3D.md sections 3-6) with respect to its state (u, v, w, p, density): the backward kernels
// behind smk_advect3d_backward, smk_project3d_backward and smk_buoy_diffuse3d_backward.  DESIGN.md section 3.10; the 3-D counterpart of
// csrc/fluid_grad.hip.
//
// Arithmetic rules (the project's gradient rules): fp32 throughout, every sum in one fixed order, no atomics, every output element written,
// results bit-identical from call to call and independent of a grid's batch mates.  The back-trace positions, indices, clamp decisions and
// weights are formed by copies of the forward's own expressions (csrc/stencil3d.hip: vel3_at, interp3, k3_advect; stencil3d.h: clampf3;
// the build keeps -ffp-contract=off), so they are the forward's bit for bit and the backward is the transpose of what the forward used.
#include "fluid_grad3d.h"

#include <math.h>

namespace smk {

namespace {

// csrc/stencil3d.hip's vel3_at: the component sampled at a field's integer index, 0.5 c[lo] + 0.5 c[hi] along the acting axis where every
// index is <= extent - 2, exactly 0 otherwise.
template <int ACT>
__device__ __forceinline__ float fg3_vel_at(const float *c, int Dc, int Hc, int Wc, int pitch, int z, int y, int x) {
    if (z > Dc - 2 || y > Hc - 2 || x > Wc - 2) return 0.f;
    const int o = (z * Hc + y) * pitch + x;
    const int step = ACT == 2 ? 1 : (ACT == 1 ? pitch : Hc * pitch);
    return 0.5f * c[o] + 0.5f * c[o + step];
}

// ---------------------------------------------------------------- advection backward
// out = adv(f; u, v, w).  A workgroup owns an FG3_TY x FG3_TX tile of SOURCE cells of the union domain [D+1][H+1][W+1] (it holds
// u [D][H+1][W], v [D][H][W+1], w [D+1][H][W] and the field [Df][Hf][Wf]) and marches it through the planes z = 0 .. D.  For every
// DESTINATION cell of the tile plus a one-cell halo it forms the record the forward's own arithmetic gives -- the packed clamped taps, the
// six per-axis weights, g, and -dt * gpx, -dt * gpy, -dt * gpz -- into a ring of three planes in LDS: planes z - 1, z, z + 1 while plane z
// is gathered.  The gather: dfield[j] from the 3 x 3 x 3 destinations around j (z slowest, x fastest; taps in interp3's order), du[j] from
// the destinations (z, y, x-1), (z, y, x), dv[j] from (z, y-1, x), (z, y, x), dw[j] from (z-1, y, x), (z, y, x), whose velocity samples are
// the only ones that can tap j (vel3_at's guard).  Taps are matched by comparing coordinates, never used as LDS indices, so a far
// back-trace (|displacement| >= 1 cell on an axis) only loses terms: it raises the grid's far word and the caller discards the grid.
template <int WHICH>
__global__ __launch_bounds__(FG3_NT) void k3_advect_backward(Geom3 g, const float *__restrict__ field, const float *__restrict__ u,
                                                             const float *__restrict__ v, const float *__restrict__ w,
                                                             const float *__restrict__ gout, float *__restrict__ dfield,
                                                             float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                             int32_t *far) {
    const int Df = g.D + (WHICH == 2), Hf = g.H + (WHICH == 0), Wf = g.W + (WHICH == 1);
    const int pitch = WHICH == 1 ? g.pv : g.pc;
    const size_t fs = WHICH == 0 ? g.su : (WHICH == 1 ? g.sv : (WHICH == 2 ? g.sw : g.sc));
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * FG3_TX, ty0 = blockIdx.y * FG3_TY;
    const float *ub = u + b * g.su, *vb = v + b * g.sv, *wb = w + b * g.sw, *fb = field + b * fs, *gb = gout + b * fs;

    __shared__ int s_x[FG3_RING][FG3_REC], s_y[FG3_RING][FG3_REC], s_z[FG3_RING][FG3_REC];     // lo | hi << 16; s_x = -1: no such destination
    __shared__ float s_wx[2][FG3_RING][FG3_REC], s_wy[2][FG3_RING][FG3_REC], s_wz[2][FG3_RING][FG3_REC];   // [0]: low tap's weight
    __shared__ float s_g[FG3_RING][FG3_REC];
    __shared__ float s_tx[FG3_RING][FG3_REC], s_ty[FG3_RING][FG3_REC], s_tz[FG3_RING][FG3_REC];            // -dt * gp per axis

    const int tid = threadIdx.x;
    auto slot_of = [](int Z) { return (Z + FG3_RING) % FG3_RING; };      // Z >= -1
    auto form_plane = [&](int Z) {
        const int sl = slot_of(Z);
        for (int r = tid; r < FG3_REC; r += FG3_NT) {
            const int Y = ty0 - 1 + r / FG3_HX, X = tx0 - 1 + r % FG3_HX;
            float wx0 = 0.f, wx1 = 0.f, wy0 = 0.f, wy1 = 0.f, wz0 = 0.f, wz1 = 0.f, gi = 0.f, ttx = 0.f, tty = 0.f, ttz = 0.f;
            int xs = -1, ys = -1, zs = -1;
            if (Z >= 0 && Z < Df && Y >= 0 && Y < Hf && X >= 0 && X < Wf) {
                const float ui = fg3_vel_at<2>(ub, g.D, g.H + 1, g.W, g.pc, Z, Y, X);
                const float vi = fg3_vel_at<1>(vb, g.D, g.H, g.W + 1, g.pv, Z, Y, X);
                const float wi = fg3_vel_at<0>(wb, g.D + 1, g.H, g.W, g.pc, Z, Y, X);
                const float tx = g.dt * ui, ty = g.dt * vi, tz = g.dt * wi;
                const float fX = (float)X, fY = (float)Y, fZ = (float)Z;
                const float pxu = fX - tx, pyu = fY - ty, pzu = fZ - tz;                          // k3_advect, before the clamp
                const float hx = (float)(Wf - 1), hy = (float)(Hf - 1), hz = (float)(Df - 1);
                const float px = clampf3(pxu, 0.f, hx), py = clampf3(pyu, 0.f, hy), pz = clampf3(pzu, 0.f, hz);
                // (NaN included; every writer stores the same 1)
                if (!(fabsf(pxu - fX) < 1.0f) || !(fabsf(pyu - fY) < 1.0f) || !(fabsf(pzu - fZ) < 1.0f)) far[b] = 1;
                int x0 = (int)floorf(px), y0 = (int)floorf(py), z0 = (int)floorf(pz);             // interp3
                int x1 = x0 + 1, y1 = y0 + 1, z1 = z0 + 1;
                x0 = clampi3(x0, 0, Wf - 1); x1 = clampi3(x1, 0, Wf - 1);
                y0 = clampi3(y0, 0, Hf - 1); y1 = clampi3(y1, 0, Hf - 1);
                z0 = clampi3(z0, 0, Df - 1); z1 = clampi3(z1, 0, Df - 1);
                wx0 = (float)x1 - px; wx1 = px - (float)x0;
                wy0 = (float)y1 - py; wy1 = py - (float)y0;
                wz0 = (float)z1 - pz; wz1 = pz - (float)z0;
                const int r00 = (z0 * Hf + y0) * pitch, r01 = (z0 * Hf + y1) * pitch;
                const int r10 = (z1 * Hf + y0) * pitch, r11 = (z1 * Hf + y1) * pitch;
                const float f000 = fb[r00 + x0], f001 = fb[r00 + x1], f010 = fb[r01 + x0], f011 = fb[r01 + x1];
                const float f100 = fb[r10 + x0], f101 = fb[r10 + x1], f110 = fb[r11 + x0], f111 = fb[r11 + x1];
                gi = gb[(Z * Hf + Y) * pitch + X];
                if (WHICH == 3) gi = gi * 0.995f;                                                 // the decay of step()
                // slope of the interpolant along an axis: the other two axes' weights times (f_hi - f_lo), z-low plane first
                float sx = (wy0 * wz0) * (f001 - f000);
                sx = sx + (wy1 * wz0) * (f011 - f010);
                sx = sx + (wy0 * wz1) * (f101 - f100);
                sx = sx + (wy1 * wz1) * (f111 - f110);
                float sy = (wx0 * wz0) * (f010 - f000);
                sy = sy + (wx1 * wz0) * (f011 - f001);
                sy = sy + (wx0 * wz1) * (f110 - f100);
                sy = sy + (wx1 * wz1) * (f111 - f101);
                float sz = (wx0 * wy0) * (f100 - f000);
                sz = sz + (wx1 * wy0) * (f101 - f001);
                sz = sz + (wx0 * wy1) * (f110 - f010);
                sz = sz + (wx1 * wy1) * (f111 - f011);
                // clamp passes its gradient where lo <= x <= hi, bounds included (torch's convention)
                const float gpx = (pxu >= 0.f && pxu <= hx) ? gi * sx : 0.f;
                const float gpy = (pyu >= 0.f && pyu <= hy) ? gi * sy : 0.f;
                const float gpz = (pzu >= 0.f && pzu <= hz) ? gi * sz : 0.f;
                ttx = -(g.dt * gpx); tty = -(g.dt * gpy); ttz = -(g.dt * gpz);
                xs = x0 | (x1 << 16); ys = y0 | (y1 << 16); zs = z0 | (z1 << 16);
            }
            s_x[sl][r] = xs; s_y[sl][r] = ys; s_z[sl][r] = zs;
            s_wx[0][sl][r] = wx0; s_wx[1][sl][r] = wx1; s_wy[0][sl][r] = wy0; s_wy[1][sl][r] = wy1;
            s_wz[0][sl][r] = wz0; s_wz[1][sl][r] = wz1;
            s_g[sl][r] = gi; s_tx[sl][r] = ttx; s_ty[sl][r] = tty; s_tz[sl][r] = ttz;
        }
    };

    const int lx = tid % FG3_TX, ly = tid / FG3_TX;
    const int x = tx0 + lx, y = ty0 + ly;
    const int rc = (ly + 1) * FG3_HX + (lx + 1);          // this cell's own record
    form_plane(-1);
    form_plane(0);
    for (int z = 0; z <= g.D; ++z) {
        form_plane(z + 1);                                // over plane z - 2's slot, which the gather of plane z - 1 has left
        __syncthreads();
        const int sc = slot_of(z);
        if (z < Df && y < Hf && x < Wf) {
            float acc = 0.f;
            for (int dz = -1; dz <= 1; ++dz) {
                const int sl = slot_of(z + dz);
                for (int dy = -1; dy <= 1; ++dy) {
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int r = rc + dy * FG3_HX + dx;
                        const int xs = s_x[sl][r];
                        if (xs < 0) continue;
                        const int ys = s_y[sl][r], zs = s_z[sl][r];
                        const bool mx[2] = {(xs & 0xffff) == x, (xs >> 16) == x};
                        const bool my[2] = {(ys & 0xffff) == y, (ys >> 16) == y};
                        const bool mz[2] = {(zs & 0xffff) == z, (zs >> 16) == z};
                        if (!((mx[0] || mx[1]) && (my[0] || my[1]) && (mz[0] || mz[1]))) continue;
                        const float gi = s_g[sl][r];
                        const float wx[2] = {s_wx[0][sl][r], s_wx[1][sl][r]};
                        const float wy[2] = {s_wy[0][sl][r], s_wy[1][sl][r]};
                        const float wz[2] = {s_wz[0][sl][r], s_wz[1][sl][r]};
#pragma unroll
                        for (int k = 0; k < 2; ++k)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
#pragma unroll
                                for (int i = 0; i < 2; ++i)
                                    if (mz[k] && my[j] && mx[i]) acc = acc + gi * ((wx[i] * wy[j]) * wz[k]);
                    }
                }
            }
            dfield[b * fs + (size_t)((z * Hf + y) * pitch + x)] = acc;
        }
        if (z < g.D && y <= g.H && x < g.W) {             // du[z][y][x]: the u samples of the destinations (z, y, x-1) and (z, y, x)
            float acc = 0.f;
            for (int dx = -1; dx <= 0; ++dx) {
                const int X = x + dx;
                if (X < 0 || X > g.W - 2 || y > g.H - 1 || z > g.D - 2 || s_x[sc][rc + dx] < 0) continue;
                acc = acc + 0.5f * s_tx[sc][rc + dx];
            }
            du[b * g.su + (size_t)((z * (g.H + 1) + y) * g.pc + x)] = acc;
        }
        if (z < g.D && y < g.H && x <= g.W) {             // dv[z][y][x]: the v samples of the destinations (z, y-1, x) and (z, y, x)
            float acc = 0.f;
            for (int dy = -1; dy <= 0; ++dy) {
                const int Y = y + dy;
                if (Y < 0 || Y > g.H - 2 || x > g.W - 1 || z > g.D - 2 || s_x[sc][rc + dy * FG3_HX] < 0) continue;
                acc = acc + 0.5f * s_ty[sc][rc + dy * FG3_HX];
            }
            dv[b * g.sv + (size_t)((z * g.H + y) * g.pv + x)] = acc;
        }
        if (y < g.H && x < g.W) {                         // dw[z][y][x], z <= D: the w samples of the destinations (z-1, y, x) and (z, y, x)
            float acc = 0.f;
            for (int dz = -1; dz <= 0; ++dz) {
                const int Z = z + dz, sl = slot_of(Z);
                if (Z < 0 || Z > g.D - 1 || y > g.H - 2 || x > g.W - 2 || s_x[sl][rc] < 0) continue;
                acc = acc + 0.5f * s_tz[sl][rc];
            }
            dw[b * g.sw + (size_t)((z * g.H + y) * g.pc + x)] = acc;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- projection backward
// lambda = gp with the gradient subtraction's transpose added (SPEC_3D.md section 4, last bullet); ddiv = 0.  lam, ddiv: dense [B][D][H][W].
__global__ void k3_project_backward_init(Geom3 g, const float *__restrict__ gu, const float *__restrict__ gv, const float *__restrict__ gw,
                                         const float *__restrict__ gp, float *__restrict__ lam, float *__restrict__ ddiv) {
    const int b = blockIdx.z / g.D, z = blockIdx.z % g.D;
    const int x = blockIdx.x * FG3_TX + threadIdx.x % FG3_TX, y = blockIdx.y * FG3_TY + threadIdx.x / FG3_TX;
    if (y >= g.H || x >= g.W) return;
    const float *gub = gu + b * g.su, *gvb = gv + b * g.sv, *gwb = gw + b * g.sw;
    float l = gp[b * g.sc + (size_t)((z * g.H + y) * g.pc + x)];
    if (y >= 1) l = l - g.dt * gub[(z * (g.H + 1) + y) * g.pc + x];
    if (y <= g.H - 2) l = l + g.dt * gub[(z * (g.H + 1) + y + 1) * g.pc + x];
    if (x >= 1) l = l - g.dt * gvb[(z * g.H + y) * g.pv + x];
    if (x <= g.W - 2) l = l + g.dt * gvb[(z * g.H + y) * g.pv + x + 1];
    if (z >= 1) l = l - g.dt * gwb[(z * g.H + y) * g.pc + x];
    if (z <= g.D - 2) l = l + g.dt * gwb[((z + 1) * g.H + y) * g.pc + x];
    const size_t o = (((size_t)b * g.D + z) * g.H + y) * g.W + x;
    lam[o] = l;
    ddiv[o] = 0.f;
}

// T <= FG3_PB_T transposed Jacobi sweeps (SPEC_3D.md section 4) in one launch (T a template parameter: the region's sides are constants).  One sweep: m = lambda on the interior, 0 on the boundary
// shell; ddiv -= (1/6) m; lambda' = (1/6) (up + down + left + right + front + back) of m on all cells, cells outside the grid counting 0.
// A workgroup owns an 8 x 8 x 32 brick: it loads the masked lambda of the brick plus a halo of T cells into LDS, sweeps T times between two
// LDS volumes (the region that is still exact shrinks by one cell per sweep and ends as the brick), keeps its cells' ddiv in registers
// meanwhile, and writes lambda and ddiv once.  Per cell the operations and their order are those of a single sweep, so the result does not
// depend on T.  (m_{k+1} = mask (1/6) nbsum(m_k) is the forward sweep with div = 0; ddiv is the running sum of the iterates.)
template <int T>
__global__ __launch_bounds__(FG3_NT) void k3_project_backward_sweeps(int D, int H, int W, float sixth, const float *__restrict__ lam_in,
                                                                     float *__restrict__ lam_out, float *__restrict__ ddiv) {
    static_assert(T >= 1 && T <= FG3_PB_T, "the LDS volumes hold a halo of FG3_PB_T cells");
    constexpr int PZ = FG3_PB_Z, PY = FG3_PB_Y, PX = FG3_PB_X;
    constexpr int SX = PX + 2 * FG3_PB_T, SY = PY + 2 * FG3_PB_T, SZ = PZ + 2 * FG3_PB_T, CELLS = PZ * PY * PX / FG3_NT;
    __shared__ float buf[2][SZ * SY * SX];
    const int tiles_z = (D + PZ - 1) / PZ;
    const int b = blockIdx.z / tiles_z, tz0 = (blockIdx.z % tiles_z) * PZ, ty0 = blockIdx.y * PY, tx0 = blockIdx.x * PX, tid = threadIdx.x;
    const size_t vol = (size_t)b * D * H * W;
    const float *l = lam_in + vol;
    constexpr int rx = PX + 2 * T, ry = PY + 2 * T, rz = PZ + 2 * T;   // the region loaded; its origin is (tz0 - T, ty0 - T, tx0 - T)
    auto interior = [&](int qz, int qy, int qx) {
        const int z = tz0 - T + qz, y = ty0 - T + qy, x = tx0 - T + qx;
        return z >= 1 && z <= D - 2 && y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2;
    };
    for (int i = tid; i < rz * ry * rx; i += FG3_NT) {
        const int qx = i % rx, qy = (i / rx) % ry, qz = i / (rx * ry);
        buf[0][(qz * SY + qy) * SX + qx] =
            interior(qz, qy, qx) ? l[((size_t)(tz0 - T + qz) * H + (ty0 - T + qy)) * W + (tx0 - T + qx)] : 0.f;
    }
    // this thread's cells of the brick: (lz = k, ly, lx)
    const int lx = tid % PX, ly = tid / PX, x = tx0 + lx, y = ty0 + ly;
    float acc[CELLS];
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const int z = tz0 + k;
        acc[k] = (z < D && y < H && x < W) ? ddiv[vol + ((size_t)z * H + y) * W + x] : 0.f;
    }
    auto swept = [&](const float *c, int qz, int qy, int qx) {      // (1/6) (up + down + left + right + front + back) at a region cell
        const int o = (qz * SY + qy) * SX + qx;
        float s = c[o - SX] + c[o + SX];
        s = s + c[o - 1];
        s = s + c[o + 1];
        s = s + c[o - SY * SX];
        s = s + c[o + SY * SX];
        return sixth * s;
    };
    int cur = 0;
#pragma unroll
    for (int s = 0; s < T; ++s) {
        __syncthreads();
        const float *c = buf[cur];
#pragma unroll
        for (int k = 0; k < CELLS; ++k) acc[k] = acc[k] - sixth * c[((k + T) * SY + ly + T) * SX + lx + T];
        if (s < T - 1) {
            float *n = buf[cur ^ 1];
            const int lo = s + 1, nx = rx - 2 * lo, ny = ry - 2 * lo, nz = rz - 2 * lo;
            for (int i = tid; i < nz * ny * nx; i += FG3_NT) {
                const int qx = lo + i % nx, qy = lo + (i / nx) % ny, qz = lo + i / (nx * ny);
                const float val = swept(c, qz, qy, qx);
                n[(qz * SY + qy) * SX + qx] = interior(qz, qy, qx) ? val : 0.f;
            }
            cur ^= 1;
        } else {
#pragma unroll
            for (int k = 0; k < CELLS; ++k) {
                const int z = tz0 + k;
                if (z < D && y < H && x < W) lam_out[vol + ((size_t)z * H + y) * W + x] = swept(c, k + T, ly + T, lx + T);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const int z = tz0 + k;
        if (z < D && y < H && x < W) ddiv[vol + ((size_t)z * H + y) * W + x] = acc[k];
    }
}

// dp = lambda; with gd = ddiv / dt (the divergence's true divide): du = gu + gd[y-1] - gd[y], dv = gv + gd[x-1] - gd[x],
// dw = gw + gd[z-1] - gd[z].
__global__ void k3_project_backward_final(Geom3 g, const float *__restrict__ gu, const float *__restrict__ gv, const float *__restrict__ gw,
                                          const float *__restrict__ lam, const float *__restrict__ ddiv, float *__restrict__ du,
                                          float *__restrict__ dv, float *__restrict__ dw, float *__restrict__ dp) {
    const int b = blockIdx.z / (g.D + 1), z = blockIdx.z % (g.D + 1);
    const int x = blockIdx.x * FG3_TX + threadIdx.x % FG3_TX, y = blockIdx.y * FG3_TY + threadIdx.x / FG3_TX;
    const float *dd = ddiv + (size_t)b * g.D * g.H * g.W;
    const size_t HW = (size_t)g.H * g.W;
    if (z < g.D && y < g.H && x < g.W) dp[b * g.sc + (size_t)((z * g.H + y) * g.pc + x)] = lam[(size_t)b * g.D * HW + z * HW + (size_t)y * g.W + x];
    if (z < g.D && y <= g.H && x < g.W) {
        const size_t o = b * g.su + (size_t)((z * (g.H + 1) + y) * g.pc + x);
        float r = gu[o];
        if (y >= 1) r = r + __fdiv_rn(dd[z * HW + (size_t)(y - 1) * g.W + x], g.dt);
        if (y <= g.H - 1) r = r - __fdiv_rn(dd[z * HW + (size_t)y * g.W + x], g.dt);
        du[o] = r;
    }
    if (z < g.D && y < g.H && x <= g.W) {
        const size_t o = b * g.sv + (size_t)((z * g.H + y) * g.pv + x);
        float r = gv[o];
        if (x >= 1) r = r + __fdiv_rn(dd[z * HW + (size_t)y * g.W + x - 1], g.dt);
        if (x <= g.W - 1) r = r - __fdiv_rn(dd[z * HW + (size_t)y * g.W + x], g.dt);
        dv[o] = r;
    }
    if (y < g.H && x < g.W) {
        const size_t o = b * g.sw + (size_t)((z * g.H + y) * g.pc + x);
        float r = gw[o];
        if (z >= 1) r = r + __fdiv_rn(dd[(z - 1) * HW + (size_t)y * g.W + x], g.dt);
        if (z <= g.D - 1) r = r - __fdiv_rn(dd[z * HW + (size_t)y * g.W + x], g.dt);
        dw[o] = r;
    }
}

// ---------------------------------------------------------------- diffusion + buoyancy backward
// diffusion_step with replicate padding on six faces is symmetric (SPEC_3D.md section 3): its transpose is itself.
__device__ __forceinline__ float fg3_diffuse_at(const float *f, int P, int R, int C, int pitch, int k, int i, int j, float coef) {
    const int iu = i > 0 ? i - 1 : 0, id = i < R - 1 ? i + 1 : R - 1;
    const int jl = j > 0 ? j - 1 : 0, jr = j < C - 1 ? j + 1 : C - 1;
    const int kf = k > 0 ? k - 1 : 0, kb = k < P - 1 ? k + 1 : P - 1;
    const float c = f[(k * R + i) * pitch + j];
    float lap = f[(k * R + iu) * pitch + j] + f[(k * R + id) * pitch + j];
    lap = lap + f[(k * R + i) * pitch + jl];
    lap = lap + f[(k * R + i) * pitch + jr];
    lap = lap + f[(kf * R + i) * pitch + j];
    lap = lap + f[(kb * R + i) * pitch + j];
    lap = lap - 6.0f * c;
    return c + coef * lap;
}

// du = Diff_nu(gu); dv = Diff_nu(gv); dw = Diff_nu(gw); ddensity = Diff_{0.1 nu}(gd) + 0.1 (dt dv[:, :, :-1])  (buoyancy, section 6.1).
__global__ void k3_buoy_diffuse_backward(Geom3 g, const float *__restrict__ gu, const float *__restrict__ gv, const float *__restrict__ gw,
                                         const float *__restrict__ gd, float *__restrict__ du, float *__restrict__ dv,
                                         float *__restrict__ dw, float *__restrict__ dd) {
    const int b = blockIdx.z / (g.D + 1), z = blockIdx.z % (g.D + 1);
    const int x = blockIdx.x * FG3_TX + threadIdx.x % FG3_TX, y = blockIdx.y * FG3_TY + threadIdx.x / FG3_TX;
    if (z < g.D && y <= g.H && x < g.W)
        du[b * g.su + (size_t)((z * (g.H + 1) + y) * g.pc + x)] = fg3_diffuse_at(gu + b * g.su, g.D, g.H + 1, g.W, g.pc, z, y, x, g.coef_uv);
    if (z < g.D && y < g.H && x <= g.W) {
        const float r = fg3_diffuse_at(gv + b * g.sv, g.D, g.H, g.W + 1, g.pv, z, y, x, g.coef_uv);
        dv[b * g.sv + (size_t)((z * g.H + y) * g.pv + x)] = r;
        if (x < g.W) {
            const float t = g.dt * r;
            dd[b * g.sc + (size_t)((z * g.H + y) * g.pc + x)] = fg3_diffuse_at(gd + b * g.sc, g.D, g.H, g.W, g.pc, z, y, x, g.coef_d) + t * 0.1f;
        }
    }
    if (y < g.H && x < g.W)
        dw[b * g.sw + (size_t)((z * g.H + y) * g.pc + x)] = fg3_diffuse_at(gw + b * g.sw, g.D + 1, g.H, g.W, g.pc, z, y, x, g.coef_uv);
}

// one workgroup per FG3_TY x FG3_TX tile of the union rows and columns; grid.z carries the batch times the planes
dim3 union_planes(const Geom3 &g, int planes) {
    return dim3((unsigned)cdiv(g.W + 1, FG3_TX), (unsigned)cdiv(g.H + 1, FG3_TY), (unsigned)(g.B * planes));
}

}  // namespace

hipError_t launch3_advect_backward(const Geom3 &g, int which, const float *field, const float *u, const float *v, const float *w,
                                   const float *gout, float *dfield, float *du, float *dv, float *dw, int32_t *far, hipStream_t st) {
    hipError_t e = hipMemsetAsync(far, 0, (size_t)g.B * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const dim3 grid = union_planes(g, 1), block(FG3_NT);
    switch (which) {
        case 0: hipLaunchKernelGGL(k3_advect_backward<0>, grid, block, 0, st, g, field, u, v, w, gout, dfield, du, dv, dw, far); break;
        case 1: hipLaunchKernelGGL(k3_advect_backward<1>, grid, block, 0, st, g, field, u, v, w, gout, dfield, du, dv, dw, far); break;
        case 2: hipLaunchKernelGGL(k3_advect_backward<2>, grid, block, 0, st, g, field, u, v, w, gout, dfield, du, dv, dw, far); break;
        default: hipLaunchKernelGGL(k3_advect_backward<3>, grid, block, 0, st, g, field, u, v, w, gout, dfield, du, dv, dw, far); break;
    }
    return hipGetLastError();
}

hipError_t launch3_project_backward(const Geom3 &g, const float *gu, const float *gv, const float *gw, const float *gp, float *du,
                                    float *dv, float *dw, float *dp, int iters, float *ws, hipStream_t st) {
    const size_t n = (size_t)g.B * g.D * g.H * g.W;
    float *lam = ws, *lam2 = ws + n, *ddiv = ws + 2 * n;
    const dim3 block(FG3_NT);
    const dim3 cells((unsigned)cdiv(g.W, FG3_TX), (unsigned)cdiv(g.H, FG3_TY), (unsigned)(g.B * g.D));
    hipLaunchKernelGGL(k3_project_backward_init, cells, block, 0, st, g, gu, gv, gw, gp, lam, ddiv);
    const dim3 bricks((unsigned)cdiv(g.W, FG3_PB_X), (unsigned)cdiv(g.H, FG3_PB_Y), (unsigned)(g.B * cdiv(g.D, FG3_PB_Z)));
    for (int done = 0; done < iters; done += FG3_PB_T) {
        static_assert(FG3_PB_T == 2, "the launcher dispatches T = FG3_PB_T and a last launch of T = 1");
        if (iters - done >= FG3_PB_T)
            hipLaunchKernelGGL(k3_project_backward_sweeps<FG3_PB_T>, bricks, block, 0, st, g.D, g.H, g.W, g.sixth, (const float *)lam, lam2, ddiv);
        else
            hipLaunchKernelGGL(k3_project_backward_sweeps<1>, bricks, block, 0, st, g.D, g.H, g.W, g.sixth, (const float *)lam, lam2, ddiv);
        float *t = lam; lam = lam2; lam2 = t;
    }
    hipLaunchKernelGGL(k3_project_backward_final, union_planes(g, g.D + 1), block, 0, st, g, gu, gv, gw, (const float *)lam,
                       (const float *)ddiv, du, dv, dw, dp);
    return hipGetLastError();
}

hipError_t launch3_buoy_diffuse_backward(const Geom3 &g, const float *gu, const float *gv, const float *gw, const float *gd, float *du,
                                         float *dv, float *dw, float *dd, hipStream_t st) {
    hipLaunchKernelGGL(k3_buoy_diffuse_backward, union_planes(g, g.D + 1), dim3(FG3_NT), 0, st, g, gu, gv, gw, gd, du, dv, dw, dd);
    return hipGetLastError();
}

}  // namespace smk

using namespace smk;

namespace {

// Shapes every entry point of this file takes: smk_sim3d_create's, within the tap packing's reach.
bool fg3_shape_ok(int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v) {
    return B >= 1 && D >= 3 && H >= 3 && W >= 3 && D <= 32766 && H <= 32766 && W <= 32766 && pitch_c >= W && pitch_v >= W + 1 &&
           (int64_t)B * (D + 1) <= 65535 && (int64_t)(D + 1) * (H + 1) * pitch_v < (1LL << 31) &&
           (int64_t)(D + 1) * (H + 1) * pitch_c < (1LL << 31);
}
const char *const FG3_SHAPE = "B >= 1, 3 <= D, H, W <= 32766, pitch_c >= W, pitch_v >= W + 1, B * (D + 1) <= 65535, one grid's field below 2^31 elements";

Geom3 fg3_geom(int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, double viscosity) {
    Geom3 g{};
    g.B = B; g.D = D; g.H = H; g.W = W; g.pc = pitch_c; g.pv = pitch_v;
    g.su = (size_t)D * (H + 1) * pitch_c; g.sv = (size_t)D * H * pitch_v; g.sw = (size_t)(D + 1) * H * pitch_c;
    g.sc = (size_t)D * H * pitch_c;
    g.dt = (float)dt;
    g.coef_uv = (float)(dt * viscosity);
    g.coef_d = (float)(dt * (viscosity * 0.1));
    g.sixth = (float)(1.0 / 6.0);
    return g;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int smk_advect3d_backward(int32_t which, const float *field, const float *u, const float *v, const float *w, const float *gout,
                          float *dfield, float *du, float *dv, float *dw, int32_t *far, int32_t B, int32_t D, int32_t H, int32_t W,
                          int32_t pitch_c, int32_t pitch_v, double dt, void *stream) {
    SMK_REQUIRE(field && u && v && w && gout && dfield && du && dv && dw && far, "advect3d_backward: null pointer");
    SMK_REQUIRE(which >= 0 && which <= 3, "advect3d_backward: which in 0..3");
    SMK_REQUIRE(fg3_shape_ok(B, D, H, W, pitch_c, pitch_v), FG3_SHAPE);
    const float *ins[] = {field, u, v, w, gout};
    float *outs[] = {dfield, du, dv, dw};
    bool alias = false;
    for (int i = 0; i < 4; ++i) {
        for (const float *in : ins) alias |= outs[i] == in;
        for (int j = i + 1; j < 4; ++j) alias |= outs[i] == outs[j];
    }
    SMK_REQUIRE(!alias, "advect3d_backward: an output aliases an input or another output");
    const Geom3 g = fg3_geom(B, D, H, W, pitch_c, pitch_v, dt, 0.0);
    return check_launch(launch3_advect_backward(g, which, field, u, v, w, gout, dfield, du, dv, dw, far, (hipStream_t)stream),
                        "advect3d_backward");
}

int64_t smk_project3d_backward_workspace(int32_t B, int32_t D, int32_t H, int32_t W) {
    if (!fg3_shape_ok(B, D, H, W, W, W + 1)) return -1;
    return (int64_t)3 * B * D * H * W * (int64_t)sizeof(float);
}

int smk_project3d_backward(const float *gu, const float *gv, const float *gw, const float *gp, float *du, float *dv, float *dw, float *dp,
                           int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t jacobi_iters, double dt,
                           void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(gu && gv && gw && gp && du && dv && dw && dp, "project3d_backward: null pointer");
    SMK_REQUIRE(fg3_shape_ok(B, D, H, W, pitch_c, pitch_v), FG3_SHAPE);
    SMK_REQUIRE(jacobi_iters >= 0, "project3d_backward: jacobi_iters >= 0");
    SMK_REQUIRE(dt != 0.0, "project3d_backward: dt != 0");
    SMK_REQUIRE(du != gu && dv != gv && dw != gw && dp != gp, "project3d_backward: an output aliases its input");
    SMK_REQUIRE(workspace && workspace_bytes >= smk_project3d_backward_workspace(B, D, H, W),
                "project3d_backward: workspace smaller than smk_project3d_backward_workspace(B, D, H, W) bytes");
    SMK_REQUIRE(((uintptr_t)workspace & 3) == 0, "project3d_backward: workspace must be 4-byte aligned");
    const Geom3 g = fg3_geom(B, D, H, W, pitch_c, pitch_v, dt, 0.0);
    return check_launch(launch3_project_backward(g, gu, gv, gw, gp, du, dv, dw, dp, jacobi_iters, (float *)workspace, (hipStream_t)stream),
                        "project3d_backward");
}

int smk_buoy_diffuse3d_backward(const float *gu, const float *gv, const float *gw, const float *gd, float *du, float *dv, float *dw,
                                float *dd, int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, double dt,
                                double viscosity, void *stream) {
    SMK_REQUIRE(gu && gv && gw && gd && du && dv && dw && dd, "buoy_diffuse3d_backward: null pointer");
    SMK_REQUIRE(fg3_shape_ok(B, D, H, W, pitch_c, pitch_v), FG3_SHAPE);
    SMK_REQUIRE(du != gu && dv != gv && dw != gw && dd != gd, "buoy_diffuse3d_backward: an output aliases its input");
    const Geom3 g = fg3_geom(B, D, H, W, pitch_c, pitch_v, dt, viscosity);
    return check_launch(launch3_buoy_diffuse_backward(g, gu, gv, gw, gd, du, dv, dw, dd, (hipStream_t)stream), "buoy_diffuse3d_backward");
}

}  // extern "C"
#pragma GCC visibility pop
