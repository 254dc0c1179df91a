// Stand-alone host check of the gather plan of the free-camera render's gradient (smokephysai_amd/csrc/camera_grad_plan.h, the text the
// kernels compile).  For every shape and view of the device test (tests/render_camera_oracle.py GPU_SHAPES x GPU_VIEWS):
//   (a) every pixel, sample and tap as the ray pass forms them: every tap that is a voxel of the volume finds the sample inside that
//       voxel's 4 x 4 x 4 candidate window, the window is the integers within reach, and camera_grad_weight gives the tap's forward
//       weight (0 for a voxel that is no tap);
//   (b) for every band height from 1 to H and both kinds of scratch: every voxel is owned by exactly one band, lies in that band's slab
//       of voxel rows, and every candidate of it with a non-zero weight lies in an image row the band marches and in a chunk that
//       camera_brick_live keeps, whichever of the tiles that a band can lay over that row holds it;
//   (c) every scratch offset formed for such a candidate, and the extremes of every band's rows, lie below scratch_floats.
//   (d) At the limit shapes, for the image's four corner tiles and its centre tile at three near-exact views: (a) again, and the number
//       of marched rows that fit the scratch is at least 4.
// Built with -fsanitize=address,undefined where the toolchain has the runtimes; prints one summary line, exit status 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "camera_grad_plan.h"

using namespace smk;

static long long samples = 0, taps = 0, violations = 0, voxels = 0, bands = 0, candidates = 0, limit_taps = 0, min_fit = 1LL << 40;
static double max_reach = 0.0;

static void fail(const char *what, const CameraGeom &g, double phi, double theta, long long a, long long b, long long c) {
    if (++violations <= 20) std::printf("VIOLATION %s (%d,%d,%d) view=(%.6f,%.6f) %lld %lld %lld\n", what, g.D, g.H, g.W, phi, theta, a, b, c);
}

// (a) for the pixels [xa, xb] x [ya, yb]
static void walk_pixels(const CameraGeom &g, const CameraView &v, double phi, double theta, int xa, int xb, int ya, int yb, long long *ntaps) {
    for (int yr = ya; yr <= yb; ++yr)
        for (int xcol = xa; xcol <= xb; ++xcol) {
            const float a = (float)xcol - g.cx, b = (float)yr - g.cy;
            for (int k = 0; k < g.S; ++k) {
                const float t = (float)k - g.tc;
                const float pz = camera_sample_z(a, b, t, v, g.cz), py = camera_sample_y(b, t, v, g.cy), px = camera_sample_x(a, b, t, v, g.cx);
                const float zf = floorf(pz), yf = floorf(py), xf = floorf(px), fz = pz - zf, fy = py - yf, fx = px - xf;
                ++samples;
                bool any = false;
                for (int n = 0; n < 8; ++n) {
                    const int dz = n >> 2, dy = (n >> 1) & 1, dx = n & 1;
                    const int zi = (int)zf + dz, yi = (int)yf + dy, xi = (int)xf + dx;
                    if (zi < 0 || zi >= g.D || yi < 0 || yi >= g.H || xi < 0 || xi >= g.W) continue;
                    ++*ntaps;
                    any = true;
                    float col, row, smp;
                    camera_grad_invert(g, v, zi, yi, xi, &col, &row, &smp);
                    const int x0 = camera_grad_first(col), r0 = camera_grad_first(row), k0 = camera_grad_first(smp);
                    if (xcol < x0 || xcol >= x0 + CAMERA_GRAD_WINDOW || yr < r0 || yr >= r0 + CAMERA_GRAD_WINDOW || k < k0 ||
                        k >= k0 + CAMERA_GRAD_WINDOW)
                        fail("a sample that touches a voxel is outside its window", g, phi, theta, xcol, yr, k);
                    for (const float *p : {&col, &row, &smp}) {
                        const int f = camera_grad_first(*p);
                        if (!((float)(f + CAMERA_GRAD_WINDOW) > *p + CAMERA_GRAD_REACH && (float)(f - 1) < *p - CAMERA_GRAD_REACH))
                            fail("the window is not the integers within reach", g, phi, theta, xcol, yr, k);
                    }
                    for (double d : {std::fabs((double)xcol - (double)col), std::fabs((double)yr - (double)row), std::fabs((double)k - (double)smp)})
                        if (d > max_reach) max_reach = d;
                    const float want = (dz ? fz : 1.0f - fz) * ((dy ? fy : 1.0f - fy) * (dx ? fx : 1.0f - fx));
                    if (camera_grad_weight(g, v, xcol, yr, k, zi, yi, xi) != want)
                        fail("camera_grad_weight is not the forward's weight", g, phi, theta, xcol, yr, k);
                }
                if (any && (camera_grad_weight(g, v, xcol, yr, k, (int)zf + 2, (int)yf, (int)xf) != 0.f ||
                            camera_grad_weight(g, v, xcol, yr, k, (int)zf, (int)yf - 1, (int)xf) != 0.f ||
                            camera_grad_weight(g, v, xcol, yr, k, (int)zf, (int)yf, (int)xf + 2) != 0.f))
                    fail("camera_grad_weight of a voxel that is no tap", g, phi, theta, xcol, yr, k);
            }
        }
}

// (b), (c)
static void walk_voxels(const CameraGeom &g, const CameraView &v, double phi, double theta) {
    const int H = g.H;
    // the plans and slabs of every band height, lit and unlit
    struct Banding { CameraGradPlan p; std::vector<int> ya, yb; };
    std::vector<Banding> bandings;
    for (int lit = 0; lit < 2; ++lit)
        for (int R = 1; R <= H; ++R) {
            Banding bd;
            bd.p = camera_grad_plan(2, g.D, g.H, g.W, lit != 0, R);
            const CameraGradPlan &p = bd.p;
            if (p.band != R || p.slots != (R + 3 < H ? R + 3 : H) || p.max_vols != 2 || p.scratch_floats > CAMERA_GRAD_SCRATCH_FLOATS ||
                p.scratch_floats != (int64_t)p.max_vols * p.slots * p.row_floats)
                fail("plan", g, phi, theta, R, lit, p.band);
            for (int y0 = 0; y0 < H; y0 += p.band) {
                ++bands;
                int a, b;
                camera_grad_slab(g, v, p, y0, &a, &b);
                bd.ya.push_back(a);
                bd.yb.push_back(b);
                const int yend = camera_grad_march_end(p, y0);
                if (yend <= y0 || yend > H || yend - y0 > p.slots) fail("marched rows", g, phi, theta, R, y0, yend);
                const int64_t lo = camera_grad_row(p, 0, y0, y0) * p.row_floats;
                const int64_t top = camera_grad_row(p, p.max_vols - 1, y0, yend - 1);
                const int64_t k1 = camera_grad_at_k(p, top, g.W - 1);
                bool ok = lo == 0 && k1 < p.scratch_floats && k1 == (top + 1) * p.row_floats - 1;
                if (lit) ok = ok && camera_grad_at_q(p, top, 0, 0) == top * p.row_floats &&
                              camera_grad_at_q(p, top, g.S - 1, g.W - 1) + 1 == camera_grad_at_r(p, top, 0, 0) &&
                              camera_grad_at_r(p, top, g.S - 1, g.W - 1) + 1 == camera_grad_at_k(p, top, 0);
                else ok = ok && camera_grad_at_k(p, top, 0) == top * p.row_floats;
                if (!ok) fail("scratch row extremes", g, phi, theta, R, y0, lit);
            }
            bandings.push_back(bd);
        }
    for (int z = 0; z < g.D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < g.W; ++x) {
                ++voxels;
                float col, row, smp;
                camera_grad_invert(g, v, z, y, x, &col, &row, &smp);
                const int x0 = camera_grad_first(col), r0 = camera_grad_first(row), k0 = camera_grad_first(smp);
                const int owner = camera_grad_owner_row(row, H);
                // the candidates with a weight: their rows, columns and samples, and that every tile a band can lay over them is live
                int rmin = 1 << 30, rmax = -(1 << 30), cmin = 1 << 30, cmax = -1, kmin = 1 << 30, kmax = -1;
                for (int i = 0; i < CAMERA_GRAD_WINDOW; ++i)
                    for (int j = 0; j < CAMERA_GRAD_WINDOW; ++j)
                        for (int kk = 0; kk < CAMERA_GRAD_WINDOW; ++kk) {
                            const int yr = r0 + i, xc = x0 + j, k = k0 + kk;
                            if (yr < 0 || yr >= H || xc < 0 || xc >= g.W || k < 0 || k >= g.S) continue;
                            if (camera_grad_weight(g, v, xc, yr, k, z, y, x) == 0.f) continue;
                            ++candidates;
                            rmin = yr < rmin ? yr : rmin; rmax = yr > rmax ? yr : rmax;
                            cmin = xc < cmin ? xc : cmin; cmax = xc > cmax ? xc : cmax;
                            kmin = k < kmin ? k : kmin;   kmax = k > kmax ? k : kmax;
                            const int xa = xc / CAMERA_TILE_W * CAMERA_TILE_W, xb = xa + CAMERA_TILE_W - 1 < g.W ? xa + CAMERA_TILE_W - 1 : g.W - 1;
                            const int s0 = k / CAMERA_CHUNK * CAMERA_CHUNK, s1 = s0 + CAMERA_CHUNK - 1 < g.S ? s0 + CAMERA_CHUNK - 1 : g.S - 1;
                            // a band's tiles start at its first row: the row is a tile's first (alone where the band ends, or with the
                            // next row) or its second
                            const int tiles[3][2] = {{yr, yr}, {yr, yr + 1}, {yr - 1, yr}};
                            for (const int *tl : tiles) {
                                if (tl[0] < 0 || tl[1] >= H) continue;
                                if (!camera_brick_live(g, camera_brick(g, v, xa, xb, tl[0], tl[1], s0, s1)))
                                    fail("a candidate with a weight lies in a skipped chunk", g, phi, theta, xc, yr, k);
                            }
                        }
                for (const Banding &bd : bandings) {
                    const CameraGradPlan &p = bd.p;
                    int owners = 0, mine = -1, bi = 0, at = -1;
                    for (int y0 = 0; y0 < H; y0 += p.band, ++bi)
                        if (owner >= y0 && owner < y0 + p.band) { ++owners; mine = y0; at = bi; }
                    if (owners != 1) { fail("a voxel is not owned by exactly one band", g, phi, theta, z, y, x); continue; }
                    if (y < bd.ya[at] || y > bd.yb[at]) fail("an owned voxel lies outside its band's slab", g, phi, theta, z, y, x);
                    if (rmax < 0) continue;                    // no candidate with a weight: the voxel is written with 0
                    const int yend = camera_grad_march_end(p, mine);
                    if (rmin < mine || rmax >= yend) { fail("a candidate with a weight lies in a row its band does not march", g, phi, theta, z, y, x); continue; }
                    const int64_t hi = camera_grad_row(p, p.max_vols - 1, mine, rmax), lo = camera_grad_row(p, 0, mine, rmin);
                    const int64_t first = p.lit ? camera_grad_at_q(p, lo, kmin, cmin) : camera_grad_at_k(p, lo, cmin);
                    const int64_t last = camera_grad_at_k(p, hi, cmax), lastr = p.lit ? camera_grad_at_r(p, hi, kmax, cmax) : last;
                    if (first < 0 || last >= p.scratch_floats || lastr >= p.scratch_floats || lastr < 0)
                        fail("scratch offset", g, phi, theta, z, y, x);
                }
            }
}

static int run_walk() {
    const int shapes[][3] = {{1, 1, 1}, {3, 5, 7}, {6, 5, 8}, {5, 33, 36}, {24, 70, 64}, {64, 40, 48}, {16, 64, 130}};
    const double views[][2] = {{0.0, 0.0}, {37.5, 30.0}, {-123.0, -60.0}, {200.25, 12.5}, {90.0, 90.0}, {0.0, -90.0}, {720.001, 45.0}, {45.0, 0.001}};
    int nshapes = 0, nviews = 0;
    for (const auto &sh : shapes) {
        ++nshapes;
        const CameraGeom g = camera_geom(sh[0], sh[1], sh[2]);
        for (const auto &vw : views) {
            ++nviews;
            CameraView v;
            if (!camera_view(vw[0], vw[1], &v)) { fail("camera_view", g, vw[0], vw[1], 0, 0, 0); continue; }
            walk_pixels(g, v, vw[0], vw[1], 0, g.W - 1, 0, g.H - 1, &taps);
            walk_voxels(g, v, vw[0], vw[1]);
        }
    }
    // (d) the limits
    const int limits[][3] = {{64, 4096, 1024}, {1, 4096, 1024}, {64, 1, 1024}};
    const double near_exact[][2] = {{720.001, 45.0}, {45.0, 0.001}, {200.25, 89.999}};
    for (const auto &sh : limits) {
        const CameraGeom g = camera_geom(sh[0], sh[1], sh[2]);
        if (!camera_grad_shape_ok(sh[0], sh[1], sh[2]) || camera_grad_shape_ok(sh[0], CAMERA_GRAD_MAX_HEIGHT + 1, sh[2]))
            fail("camera_grad_shape_ok", g, 0, 0, 0, 0, 0);
        for (int lit = 0; lit < 2; ++lit) {
            const CameraGradPlan p = camera_grad_plan(3, sh[0], sh[1], sh[2], lit != 0);
            if (p.fit_rows < min_fit) min_fit = p.fit_rows;
            if (p.fit_rows < 4 || p.band < 1 || p.slots > p.fit_rows || p.scratch_floats > CAMERA_GRAD_SCRATCH_FLOATS ||
                p.row_floats * 4 >= 35000000LL)
                fail("the plan at the limits", g, 0, 0, p.fit_rows, p.band, p.slots);
        }
        const int tx[3] = {0, (g.W - 1) / CAMERA_TILE_W * CAMERA_TILE_W, g.W / 2 / CAMERA_TILE_W * CAMERA_TILE_W};
        const int ty[3] = {0, (g.H - 1) / CAMERA_TILE_H * CAMERA_TILE_H, g.H / 2 / CAMERA_TILE_H * CAMERA_TILE_H};
        const int tiles[5][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {2, 2}};
        for (const auto &vw : near_exact) {
            CameraView v;
            if (!camera_view(vw[0], vw[1], &v)) { fail("camera_view", g, vw[0], vw[1], 0, 0, 0); continue; }
            for (const auto &tl : tiles) {
                const int xa = tx[tl[0]], ya = ty[tl[1]];
                const int xb = xa + CAMERA_TILE_W - 1 < g.W ? xa + CAMERA_TILE_W - 1 : g.W - 1;
                const int yb = ya + CAMERA_TILE_H - 1 < g.H ? ya + CAMERA_TILE_H - 1 : g.H - 1;
                walk_pixels(g, v, vw[0], vw[1], xa, xb, ya, yb, &limit_taps);
            }
        }
    }
    std::printf("SHAPES %d VIEWS %d SAMPLES %lld TAPS %lld MAX_REACH %.6f WINDOW %d VOXELS %lld BANDS %lld CANDIDATES %lld LIMIT_TAPS %lld "
                "MIN_FIT %lld VIOLATIONS %lld\n", nshapes, nviews, samples, taps, max_reach, CAMERA_GRAD_WINDOW, voxels, bands, candidates,
                limit_taps, min_fit, violations);
    return violations == 0 ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "walk") == 0) return run_walk();
    std::fprintf(stderr, "usage: camera_grad_plan walk\n");
    return 2;
}
