// Stand-alone host check of the gather plan of the orbit render's gradient (smokephysai_amd/csrc/orbit_grad_plan.h, the text the kernels
// compile).
//   orbit_grad_plan walk : for every shape and azimuth below, every strip, chunk, image column and sample as the ray pass marches them
//                          (the forward's plan, orbit_plan.h):
//                            * every tap of a sample that is a voxel (z, x) of the volume finds the sample inside that voxel's candidate
//                              window, and orbit_grad_weight gives the tap's forward weight for it (and 0 for a voxel that is no tap);
//                            * the window is the stated maximum: the ORBIT_GRAD_WINDOW candidates cover [p - reach, p + reach];
//                            * the LDS index of every tap that is read lies inside the staged box;
//                          and for a list of (n, D, H, W, light) that the units of a call tile the batch exactly once in order, that no
//                          unit holds more rows than the scratch, and that every scratch index of every (row, sample, column) lies in
//                          the scratch, every cell hit at most once (walked cell by cell for the small plans, at the extremes of every
//                          row for the large ones).
// Built with -fsanitize=address,undefined where the toolchain has the runtimes; prints one summary line, exit status 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbit_grad_plan.h"

using namespace smk;

struct Shape {
    int D, W;
    double step;       // azimuth grid in degrees
};

static long long samples = 0, taps = 0, violations = 0, units = 0, cells_walked = 0;
static double max_reach = 0.0;

static void fail(const char *what, long long a, long long b, double phi, long long c, long long d) {
    if (++violations <= 20) std::printf("VIOLATION %s %lld %lld phi=%.6f %lld %lld\n", what, a, b, phi, c, d);
}

static void walk(int D, int W, double phi) {
    float c, s;
    orbit_cos_sin(phi, &c, &s);
    const OrbitGeom g = orbit_geom(D, W);
    std::vector<unsigned char> lds(ORBIT_BOX_FLOATS);          // indexed as the kernel indexes its box: the sanitizer watches the bounds
    for (int xa = 0; xa < W; xa += ORBIT_STRIP) {
        const int xb = xa + ORBIT_STRIP - 1 < W ? xa + ORBIT_STRIP - 1 : W - 1;
        for (int s0 = 0; s0 < g.S; s0 += ORBIT_CHUNK) {
            const int s1 = s0 + ORBIT_CHUNK - 1 < g.S ? s0 + ORBIT_CHUNK - 1 : g.S - 1;
            const OrbitBox b = orbit_box(g, c, s, xa, xb, s0, s1);
            const bool empty = b.empty();
            const int nz = empty ? 0 : b.nz(), nx = empty ? 0 : b.nx();
            if (!empty && nz * nx > ORBIT_BOX_FLOATS) { fail("box too large", D, W, phi, xa, s0); continue; }
            for (int xcol = xa; xcol <= xb; ++xcol) {
                const float a = (float)xcol - g.cx;
                for (int k = s0; k <= s1; ++k) {
                    const float t = (float)k - g.tc;
                    const float z = orbit_sample_z(a, t, c, s, g.cz), x = orbit_sample_x(a, t, c, s, g.cx);
                    const float zf = floorf(z), xf = floorf(x), fz = z - zf, fx = x - xf;
                    ++samples;
                    for (int n = 0; n < 4; ++n) {
                        const int zi = (int)zf + (n >> 1), xi = (int)xf + (n & 1);
                        if (zi < 0 || zi >= D || xi < 0 || xi >= W) continue;
                        ++taps;
                        if (empty) { fail("a skipped chunk has a tap inside the volume", D, W, phi, xcol, k); continue; }
                        const int iz = zi - b.z0, ix = xi - b.x0;
                        if ((unsigned)iz < (unsigned)nz && (unsigned)ix < (unsigned)nx) lds[(size_t)(iz * nx + ix)] = 1;
                        else fail("a tap inside the volume is outside the box", D, W, phi, xcol, k);
                        // the gather's side: voxel (zi, xi) looks for this sample
                        float col, smp;
                        orbit_grad_invert(g, c, s, zi, xi, &col, &smp);
                        const int x0 = orbit_grad_first(col), k0 = orbit_grad_first(smp);
                        if (xcol < x0 || xcol >= x0 + ORBIT_GRAD_WINDOW || k < k0 || k >= k0 + ORBIT_GRAD_WINDOW)
                            fail("a sample that touches a voxel is outside its window", D, W, phi, xcol, k);
                        if (!((float)(x0 + ORBIT_GRAD_WINDOW) > col + ORBIT_GRAD_REACH && (float)(x0 - 1) < col - ORBIT_GRAD_REACH &&
                              (float)(k0 + ORBIT_GRAD_WINDOW) > smp + ORBIT_GRAD_REACH && (float)(k0 - 1) < smp - ORBIT_GRAD_REACH))
                            fail("the window is not the integers within reach", D, W, phi, xcol, k);
                        const double dc = std::fabs((double)xcol - (double)col), dk = std::fabs((double)k - (double)smp);
                        if (dc > max_reach) max_reach = dc;
                        if (dk > max_reach) max_reach = dk;
                        const float want = ((n >> 1) ? fz : 1.0f - fz) * ((n & 1) ? fx : 1.0f - fx);
                        if (orbit_grad_weight(g, c, s, xcol, k, zi, xi) != want) fail("orbit_grad_weight is not the forward's weight", D, W, phi, xcol, k);
                    }
                    // a voxel that is no tap of the sample has weight 0
                    if (orbit_grad_weight(g, c, s, xcol, k, (int)zf + 2, (int)xf) != 0.f || orbit_grad_weight(g, c, s, xcol, k, (int)zf, (int)xf - 1) != 0.f)
                        fail("orbit_grad_weight of a voxel that is no tap", D, W, phi, xcol, k);
                }
            }
        }
    }
}

static void walk_units(long long n, int D, int H, int W, bool lit) {
    const OrbitGradPlan p = orbit_grad_plan(n, D, H, W, lit);
    if (p.cap_rows < 1 || p.scratch_floats > ORBIT_GRAD_SCRATCH_FLOATS || p.scratch_floats != p.cap_rows * p.row_floats)
        fail("plan", n, D, 0.0, H, W);
    const bool full = p.scratch_floats <= (1LL << 24);
    std::vector<unsigned char> hit(full ? (size_t)p.scratch_floats : 1);
    int64_t v0 = 0, want_v = 0;
    int y0 = 0, want_y = 0;
    for (bool more = true; more;) {
        const OrbitGradUnit u = orbit_grad_unit(p, n, H, v0, y0);
        ++units;
        if (u.v0 != want_v || u.y0 != want_y || u.nv < 1 || u.ny < 1 || u.nv > ORBIT_GRAD_VOLS_PER_LAUNCH || u.v0 + u.nv > n ||
            u.y0 + u.ny > H || (u.nv > 1 && (u.y0 != 0 || u.ny != H)) || (int64_t)u.nv * u.ny > p.cap_rows)
            fail("unit", n, H, 0.0, u.v0, u.y0);
        const int64_t rows = (int64_t)u.nv * u.ny;
        if (full) {
            std::fill(hit.begin(), hit.end(), 0);
            for (int64_t row = 0; row < rows; ++row)
                for (int x = 0; x < W; ++x) {
                    for (int k = 0; k < (lit ? p.S : 0); ++k)
                        for (int64_t at : {orbit_grad_at_q(p, row, k, x), orbit_grad_at_r(p, row, k, x)}) {
                            if (at < 0 || at >= p.scratch_floats) { fail("scratch index", n, H, 0.0, row, k); continue; }
                            if (hit[(size_t)at]++) fail("scratch cell hit twice", n, H, 0.0, row, k);
                            ++cells_walked;
                        }
                    const int64_t at = orbit_grad_at_k(p, row, x);
                    if (at < 0 || at >= p.scratch_floats) { fail("scratch index of K", n, H, 0.0, row, x); continue; }
                    if (hit[(size_t)at]++) fail("scratch cell of K hit twice", n, H, 0.0, row, x);
                    ++cells_walked;
                }
        } else {
            for (int64_t row : {(int64_t)0, rows - 1}) {
                const int64_t lo = row * p.row_floats, hi = lo + p.row_floats;
                const int64_t k0 = orbit_grad_at_k(p, row, 0), k1 = orbit_grad_at_k(p, row, W - 1);
                bool ok = lo >= 0 && hi <= p.scratch_floats && k1 == hi - 1 && k0 >= lo;
                if (lit) {
                    const int64_t q0 = orbit_grad_at_q(p, row, 0, 0), q1 = orbit_grad_at_q(p, row, p.S - 1, W - 1);
                    const int64_t r0 = orbit_grad_at_r(p, row, 0, 0), r1 = orbit_grad_at_r(p, row, p.S - 1, W - 1);
                    ok = ok && q0 == lo && q1 + 1 == r0 && r1 + 1 == k0;
                } else {
                    ok = ok && k0 == lo;
                }
                if (!ok) fail("scratch row extremes", n, H, 0.0, row, 0);
            }
        }
        if (u.y0 + u.ny < H) { want_v = u.v0; want_y = u.y0 + u.ny; }
        else { want_v = u.v0 + u.nv; want_y = 0; }
        more = orbit_grad_next(u, n, H, &v0, &y0);
    }
    if (want_v != n || want_y != 0) fail("the units do not end at the batch's end", n, H, 0.0, want_v, want_y);
}

static int run_walk() {
    const Shape shapes[] = {{1, 1, 2.5},   {3, 7, 2.5},    {6, 8, 2.5},     {5, 36, 2.5},  {24, 64, 2.5},   {64, 48, 2.5},  {16, 130, 2.5},
                            {8, 32, 2.5},  {64, 64, 2.5},  {64, 512, 22.5},  {1, 1024, 22.5}, {64, 1024, 45.0}, {64, 1, 2.5},  {33, 1000, 45.0},
                            {2, 33, 2.5},  {63, 65, 2.5}};
    int nshapes = 0, nangles = 0;
    for (const Shape &sh : shapes) {
        ++nshapes;
        for (double phi = -360.0; phi <= 720.0; phi += sh.step) {
            walk(sh.D, sh.W, phi + (sh.step > 20.0 ? 7.3 : 0.0));          // the coarse grids: off the quarter turns, which follow
            ++nangles;
        }
        for (int q = -4; q <= 8; ++q)
            for (double d : {-1e-3, 0.0, 1e-3}) {
                walk(sh.D, sh.W, 90.0 * q + d);
                ++nangles;
            }
    }
    struct Call { long long n; int D, H, W; bool lit; };
    const Call calls[] = {{1, 1, 1, 1, false}, {1, 1, 1, 1, true}, {2, 24, 70, 64, false}, {2, 24, 70, 64, true}, {40, 3, 5, 7, true},
                          {17, 64, 40, 48, true}, {17, 64, 40, 48, false}, {3, 64, 100, 1024, true}, {1, 64, 2000, 1024, true},
                          {8, 64, 512, 512, true}, {8, 64, 512, 512, false}, {20, 1, 1 << 20, 1024, false}, {2, 16, 64, 130, true},
                          {1000, 2, 3, 5, false}, {33, 5, 33, 36, true}};
    for (const Call &cl : calls) walk_units(cl.n, cl.D, cl.H, cl.W, cl.lit);
    std::printf("SHAPES %d ANGLES %d SAMPLES %lld TAPS %lld MAX_REACH %.6f WINDOW %d UNITS %lld CELLS %lld VIOLATIONS %lld\n", nshapes, nangles,
                samples, taps, max_reach, ORBIT_GRAD_WINDOW, units, cells_walked, violations);
    return violations == 0 ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "walk") == 0) return run_walk();
    std::fprintf(stderr, "usage: orbit_grad_plan walk\n");
    return 2;
}
