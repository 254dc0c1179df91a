// Stand-alone host check of the free-camera render's march plan (smokephysai_amd/csrc/camera_plan.h, the text the kernel compiles).
//   camera_plan walk   : for every shape and view below, every tile of image pixels and every chunk of samples, forms the brick the kernel
//                        would test and walks every sample of it exactly as the kernel does (the same fp32 position functions, the same
//                        camera_taps):
//                          * a skipped chunk has no tap inside the volume, so no tap inside the volume is ever missed;
//                          * every position lies inside its brick's extremes (the corner argument of camera_plan.h);
//                          * every offset camera_taps answers is -1 for a tap outside the volume and otherwise the tap's own offset
//                            (camera_tap_offset), inside [0, D*H*W): it indexes a buffer of that size here, under the sanitizer;
//                          * the floors stay far from the range of int.
//                        and, apart from the walk, that S covers the diagonal with the parity of D.
//   camera_plan angles : prints the eight view coefficients of the angle rule for the (azimuth, elevation) pairs given on the command
//                        line, as hex floats ("INVALID" for a pair the rule refuses).
// Built with -fsanitize=address,undefined where the toolchain has the runtimes; prints one summary line, exit status 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "camera_plan.h"

using namespace smk;

struct Shape {
    int D, H, W;
};

struct View {
    double phi, theta;
};

// the walk is shared among a few threads by (shape, view); every thread counts for itself
static thread_local long long samples = 0, live = 0, skipped = 0, taps_in = 0;
static std::atomic<long long> violations{0};

static void fail(const char *what, const Shape &sh, const View &v, int xa, int ya, int s0) {
    if (++violations <= 20)
        std::printf("VIOLATION %s D=%d H=%d W=%d phi=%.6f theta=%.6f tile=(%d,%d) chunk=%d\n", what, sh.D, sh.H, sh.W, v.phi, v.theta, xa, ya, s0);
}

static void walk(const Shape &sh, const View &view) {
    CameraView cv;
    if (!camera_view(view.phi, view.theta, &cv)) { fail("camera_view refuses a valid view", sh, view, 0, 0, 0); return; }
    const CameraGeom g = camera_geom(sh.D, sh.H, sh.W);
    const size_t cells = (size_t)sh.D * sh.H * sh.W;
    std::vector<unsigned char> volume(cells);                  // indexed as the kernel indexes a volume: the sanitizer watches the bounds
    for (int ya = 0; ya < sh.H; ya += CAMERA_TILE_H) {
        const int yb = ya + CAMERA_TILE_H - 1 < sh.H ? ya + CAMERA_TILE_H - 1 : sh.H - 1;
        for (int xa = 0; xa < sh.W; xa += CAMERA_TILE_W) {
            const int xb = xa + CAMERA_TILE_W - 1 < sh.W ? xa + CAMERA_TILE_W - 1 : sh.W - 1;
            for (int s0 = 0; s0 < g.S; s0 += CAMERA_CHUNK) {
                const int s1 = s0 + CAMERA_CHUNK - 1 < g.S ? s0 + CAMERA_CHUNK - 1 : g.S - 1;
                const CameraBrick k = camera_brick(g, cv, xa, xb, ya, yb, s0, s1);
                const bool is_live = camera_brick_live(g, k);
                ++(is_live ? live : skipped);
                for (int y = ya; y <= yb; ++y) {
                    const float b = (float)y - g.cy;
                    for (int xcol = xa; xcol <= xb; ++xcol) {
                        const float a = (float)xcol - g.cx;
                        for (int s = s0; s <= s1; ++s) {
                            const float t = (float)s - g.tc;
                            const float z = camera_sample_z(a, b, t, cv, g.cz), yy = camera_sample_y(b, t, cv, g.cy),
                                        x = camera_sample_x(a, b, t, cv, g.cx);
                            ++samples;
                            if (!(z >= k.zmin && z <= k.zmax && yy >= k.ymin && yy <= k.ymax && x >= k.xmin && x <= k.xmax))
                                fail("a position outside its brick", sh, view, xa, ya, s0);
                            const float zf = floorf(z), yf = floorf(yy), xf = floorf(x);
                            if (!(fabsf(zf) < 262144.f && fabsf(yf) < 262144.f && fabsf(xf) < 262144.f)) {
                                fail("a floor beyond 2^18", sh, view, xa, ya, s0);
                                continue;
                            }
                            const int iz = (int)zf, iy = (int)yf, ix = (int)xf;
                            int32_t off[8];
                            camera_taps(g, iz, iy, ix, off);
                            for (int n = 0; n < 8; ++n) {
                                const int tz = iz + (n >> 2), ty = iy + ((n >> 1) & 1), tx = ix + (n & 1);
                                const bool in_volume = tz >= 0 && tz < sh.D && ty >= 0 && ty < sh.H && tx >= 0 && tx < sh.W;
                                const int32_t want = in_volume ? (int32_t)(((long long)tz * sh.H + ty) * sh.W + tx) : -1;
                                if (off[n] != want || camera_tap_offset(g, tz, ty, tx) != want) {
                                    fail("a tap's offset is not its own", sh, view, xa, ya, s0);
                                    continue;
                                }
                                if (!in_volume) continue;
                                ++taps_in;
                                if (!is_live) fail("a skipped chunk has a tap inside the volume", sh, view, xa, ya, s0);
                                else if ((size_t)off[n] >= cells) fail("an offset outside the volume", sh, view, xa, ya, s0);
                                else volume[(size_t)off[n]] = 1;
                            }
                        }
                    }
                }
            }
        }
    }
}

static int run_walk() {
    // the shapes of tests/test_hip_render_camera.py, then single planes, rows and columns, then the limits D = 64, W = 1024 and a tall H;
    // every shape walks every view
    const Shape shapes[] = {{1, 1, 1},   {3, 5, 7},  {6, 5, 8},  {5, 33, 36}, {24, 70, 64}, {64, 40, 48},   {16, 64, 130}, {6, 8, 8},    {1, 9, 13},
                            {7, 1, 11},  {9, 12, 1}, {1, 1, 40}, {1, 40, 1},  {64, 1, 1},   {64, 2, 1024}, {2, 1024, 2},  {64, 1024, 1}};
    std::vector<View> views;
    for (double phi = -180.0; phi < 180.0; phi += 45.0)
        for (double theta = -90.0; theta <= 90.0; theta += 30.0) views.push_back({phi + 0.37, theta});
    // every exact quarter turn and 1e-3 degrees to either side of it, level and pitched; every exact right angle of the elevation and
    // 1e-3 degrees inside it, at two azimuths; and every quarter turn with every right angle
    for (int q = -1; q <= 4; ++q)
        for (double dp : {-1e-3, 0.0, 1e-3})
            for (double theta : {0.0, 33.0}) views.push_back({90.0 * q + dp, theta});
    for (double theta : {-90.0, -90.0 + 1e-3, -1e-3, 1e-3, 90.0 - 1e-3, 90.0})
        for (double phi : {0.0, 37.5}) views.push_back({phi, theta});
    for (int q = 0; q < 4; ++q)
        for (double theta : {-90.0, 90.0}) views.push_back({90.0 * q, theta});
    int nshapes = 0;
    struct Job { const Shape *sh; const View *v; };
    std::vector<Job> jobs;
    for (const Shape &sh : shapes) {
        ++nshapes;
        for (const View &v : views) jobs.push_back({&sh, &v});
    }
    const int nviews = (int)jobs.size();
    std::atomic<size_t> next{0};
    std::atomic<long long> all_samples{0}, all_live{0}, all_skipped{0}, all_taps{0};
    std::vector<std::thread> pool;
    for (int i = 0; i < 4; ++i)
        pool.emplace_back([&] {
            for (size_t j = next++; j < jobs.size(); j = next++) walk(*jobs[j].sh, *jobs[j].v);
            all_samples += samples; all_live += live; all_skipped += skipped; all_taps += taps_in;
        });
    for (std::thread &t : pool) t.join();
    // S: covers the diagonal, has D's parity, and is the smallest such integer
    for (int D = 1; D <= CAMERA_MAX_DEPTH; D += 3)
        for (int H = 1; H <= CAMERA_MAX_HEIGHT; H = H * 2 + (D & 1))
            for (int W = 1; W <= CAMERA_MAX_WIDTH; W += 7) {
                const long long S = camera_samples(D, H, W), q = (long long)D * D + (long long)H * H + (long long)W * W;
                const bool ok = S * S >= q && ((S - D) & 1) == 0 && (S < 2 || (S - 2) * (S - 2) < q);
                if (!ok) { Shape sh = {D, H, W}; View v = {0.0, 0.0}; fail("camera_samples", sh, v, 0, 0, 0); }
            }
    std::printf("SHAPES %d VIEWS %d SAMPLES %lld LIVE %lld SKIPPED %lld TAPS_INSIDE %lld VIOLATIONS %lld\n", nshapes, nviews, all_samples.load(), all_live.load(),
                all_skipped.load(), all_taps.load(), violations.load());
    return violations.load() == 0 ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "walk") == 0) return run_walk();
    if (argc >= 4 && std::strcmp(argv[1], "angles") == 0 && argc % 2 == 0) {
        for (int i = 2; i + 1 < argc; i += 2) {
            CameraView v;
            if (!camera_view(std::atof(argv[i]), std::atof(argv[i + 1]), &v)) {
                std::printf("ANGLE %s %s INVALID\n", argv[i], argv[i + 1]);
                continue;
            }
            std::printf("ANGLE %s %s %a %a %a %a %a %a %a %a\n", argv[i], argv[i + 1], (double)v.rx, (double)v.rz, (double)v.ex, (double)v.ey,
                        (double)v.ez, (double)v.dx, (double)v.dy, (double)v.dz);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: camera_plan walk | angles PHI THETA [PHI THETA ...]\n");
    return 2;
}
