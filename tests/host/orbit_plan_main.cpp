// Stand-alone host check of the orbit render's staging plan (smokephysai_amd/csrc/orbit_plan.h, the text the kernel compiles).
//   orbit_plan walk   : for every shape and azimuth below, every strip of image columns and every chunk of samples, forms the box the
//                       kernel would stage and walks every sample of it exactly as the kernel does (the same fp32 position functions):
//                         * a neighbour inside the volume lies inside the box (or the box is empty and no neighbour is inside the volume);
//                         * the box is inside the volume, at most ORBIT_BOX_SIDE rows and columns, at most ORBIT_BOX_FLOATS cells;
//                         * the LDS index of every neighbour that is read lies in [0, cells);
//                       and, apart from the walk, that orbit_box_row splits every element index of every row length correctly and that
//                       S covers hypot(D, W) with the parity of D.
//   orbit_plan angles : prints (cos, sin) of the angle rule for the azimuths given on the command line, as hex floats.
// Built with -fsanitize=address,undefined where the toolchain has the runtimes; prints one summary line, exit status 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbit_plan.h"

using namespace smk;

struct Shape {
    int D, W;
    double step;       // azimuth grid in degrees
};

static long long samples = 0, boxes = 0, empties = 0, violations = 0;
static int max_cells = 0, max_side = 0;

static void fail(const char *what, int D, int W, double phi, int xa, int s0) {
    if (++violations <= 20) std::printf("VIOLATION %s D=%d W=%d phi=%.6f strip=%d chunk=%d\n", what, D, W, phi, xa, s0);
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
            int nz = 0, nx = 0;
            if (empty) {
                ++empties;
            } else {
                ++boxes;
                nz = b.nz(); nx = b.nx();
                if (b.z0 < 0 || b.x0 < 0 || b.z1 > D - 1 || b.x1 > W - 1) fail("box outside the volume", D, W, phi, xa, s0);
                if (nz > ORBIT_BOX_SIDE || nx > ORBIT_BOX_SIDE || nz * nx > ORBIT_BOX_FLOATS) { fail("box too large", D, W, phi, xa, s0); continue; }
                if (nz * nx > max_cells) max_cells = nz * nx;
                if (nz > max_side) max_side = nz;
                if (nx > max_side) max_side = nx;
            }
            for (int xcol = xa; xcol <= xb; ++xcol) {
                const float a = (float)xcol - g.cx;
                for (int k = s0; k <= s1; ++k) {
                    const float t = (float)k - g.tc;
                    const float z = orbit_sample_z(a, t, c, s, g.cz), x = orbit_sample_x(a, t, c, s, g.cx);
                    const float zf = floorf(z), xf = floorf(x);
                    ++samples;
                    for (int n = 0; n < 4; ++n) {
                        const int zi = (int)zf + (n >> 1), xi = (int)xf + (n & 1);
                        const bool in_volume = zi >= 0 && zi < D && xi >= 0 && xi < W;
                        if (empty) {
                            if (in_volume) fail("a skipped chunk has a neighbour inside the volume", D, W, phi, xa, s0);
                            continue;
                        }
                        const int iz = zi - b.z0, ix = xi - b.x0;
                        const bool in_box = (unsigned)iz < (unsigned)nz && (unsigned)ix < (unsigned)nx;
                        if (in_volume && !in_box) fail("a neighbour inside the volume is outside the box", D, W, phi, xa, s0);
                        if (in_box && !in_volume) fail("the box holds a cell outside the volume", D, W, phi, xa, s0);
                        if (in_box) lds[(size_t)(iz * nx + ix)] = 1;
                    }
                }
            }
        }
    }
}

static int run_walk() {
    const Shape shapes[] = {{1, 1, 0.5},   {3, 7, 0.5},    {6, 8, 0.5},     {5, 36, 0.5},  {24, 64, 0.5},   {64, 48, 0.5},  {16, 130, 0.5},
                            {8, 32, 0.5},  {64, 64, 0.5},  {64, 512, 7.5},  {1, 1024, 22.5}, {64, 1024, 15.0}, {64, 1, 0.5},  {33, 1000, 22.5},
                            {2, 33, 0.5},  {63, 65, 0.5}};
    int nshapes = 0, nangles = 0;
    for (const Shape &sh : shapes) {
        ++nshapes;
        for (double phi = -360.0; phi <= 720.0; phi += sh.step) {
            walk(sh.D, sh.W, phi);
            ++nangles;
        }
        for (int q = -4; q <= 8; ++q)
            for (double d : {-1e-3, 1e-3}) {
                walk(sh.D, sh.W, 90.0 * q + d);
                ++nangles;
            }
    }
    // orbit_box_row: every element of every row length the kernel can meet
    for (int nx = 1; nx <= ORBIT_BOX_SIDE; ++nx) {
        const float inv = 1.0f / (float)nx;
        for (int e = 0; e < ORBIT_BOX_FLOATS; ++e)
            if (orbit_box_row(e, inv) != e / nx) fail("orbit_box_row", nx, e, 0.0, 0, 0);
    }
    // S: covers the diagonal, has D's parity, and is the smallest such integer
    for (int D = 1; D <= ORBIT_MAX_DEPTH; ++D)
        for (int W = 1; W <= ORBIT_MAX_WIDTH; ++W) {
            const long long S = orbit_samples(D, W), q = (long long)D * D + (long long)W * W;
            const bool ok = S * S >= q && ((S - D) & 1) == 0 && (S < 2 || (S - 2) * (S - 2) < q);
            if (!ok) fail("orbit_samples", D, W, 0.0, 0, 0);
        }
    std::printf("SHAPES %d ANGLES %d SAMPLES %lld BOXES %lld EMPTY %lld MAX_CELLS %d MAX_SIDE %d VIOLATIONS %lld\n", nshapes, nangles, samples,
                boxes, empties, max_cells, max_side, violations);
    return violations == 0 ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "walk") == 0) return run_walk();
    if (argc >= 3 && std::strcmp(argv[1], "angles") == 0) {
        for (int i = 2; i < argc; ++i) {
            float c, s;
            orbit_cos_sin(std::atof(argv[i]), &c, &s);
            std::printf("ANGLE %s %a %a\n", argv[i], (double)c, (double)s);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: orbit_plan walk | angles PHI...\n");
    return 2;
}
