// The sample geometry and the march plan of the free-camera render (SPEC_3D.md section 10, "Free camera"; csrc/render_camera.hip).  Plain
// C++ for host and device: the kernel, its launcher and the stand-alone host check (tests/host/camera_plan_main.cpp) compile this text.
//
// A wave renders a tile of CAMERA_TILE_W image columns x CAMERA_TILE_H rows and marches the S samples of its rays in chunks of
// CAMERA_CHUNK.  The samples of (tile, chunk) are a rotated brick; camera_brick bounds its positions per axis.  A brick none of whose
// positions can have a tap inside the volume is skipped whole (its samples are zeros).  Inside a marched chunk every one of a sample's
// eight taps is read from global memory at camera_tap_offset, which answers -1 for a tap outside the volume (it counts as 0) and an
// offset in [0, D*H*W) otherwise: no index is formed from a position without that test.  What the host check proves by walking is that a
// skipped chunk has no tap inside the volume, and that every offset that is read lies inside the volume and is the tap's own.
//
// Every position is formed in fp32 by camera_sample_x / _y / _z and nowhere else.  Each is monotone in a, in b and in t with the other two
// fixed (every operation rounds monotonically), so over a brick of (a, b, t) the extremes are at its eight corners: no margin is needed.
#pragma once
#include <stdint.h>

#include "view_plan.h"                     // the azimuth rule (orbit_cos_sin), ray_samples

namespace smk {

constexpr int CAMERA_TILE_W = 32;          // image columns per wave (lanes along x')
constexpr int CAMERA_TILE_H = 2;           // image rows per wave
constexpr int CAMERA_WAVES = 4;            // waves per workgroup, stacked along y': a workgroup owns 32 x 8 pixels
constexpr int CAMERA_CHUNK = 16;           // samples per skip decision
constexpr int CAMERA_MAX_DEPTH = 64;
constexpr int CAMERA_MAX_WIDTH = 1024;
// With pitch the image row enters the positions: b = y' - c_y and t must be exact fp32 numbers and floor(position) an int far from
// overflow.  H <= 2^16 keeps every |position| below 2^18.
constexpr int CAMERA_MAX_HEIGHT = 65536;

// the view coefficients, fp32 (r_y is 0 and is not carried)
struct CameraView {
    float rx, rz;                          // right  r = ( c,     0,  -s    )
    float ex, ey, ez;                      // up     e = ( s se,  ce,  c se )
    float dx, dy, dz;                      // view   d = ( s ce, -se,  c ce )
};

// The angle rule.  Azimuth: the orbit's rule (orbit_cos_sin, view_plan.h: exact at multiples of 90, cast to fp32 once), read back as
// doubles.  Elevation: 0, 90, -90 give exactly (1,0), (0,1), (0,-1), anything else cos / sin of radians in double.  The nine coefficients
// are formed in double and cast to fp32 once.  false: a non-finite angle or |elevation| > 90 (*v untouched).  Host only.
inline bool camera_view(double azimuth_deg, double elevation_deg, CameraView *v) {
    if (!isfinite(azimuth_deg) || !isfinite(elevation_deg) || elevation_deg < -90.0 || elevation_deg > 90.0) return false;
    float cf, sf;
    orbit_cos_sin(azimuth_deg, &cf, &sf);
    double ce, se;
    if (elevation_deg == 0.0) { ce = 1.0; se = 0.0; }
    else if (elevation_deg == 90.0) { ce = 0.0; se = 1.0; }
    else if (elevation_deg == -90.0) { ce = 0.0; se = -1.0; }
    else {
        const double rad = elevation_deg * (3.14159265358979323846 / 180.0);
        ce = cos(rad);
        se = sin(rad);
    }
    const double c = (double)cf, s = (double)sf;
    v->rx = (float)c;        v->rz = (float)-s;
    v->ex = (float)(s * se); v->ey = (float)ce;  v->ez = (float)(c * se);
    v->dx = (float)(s * ce); v->dy = (float)-se; v->dz = (float)(c * ce);
    return true;
}

// S: the smallest integer >= sqrt(D^2 + H^2 + W^2) with the parity of D
VIEW_HD int camera_samples(int D, int H, int W) { return ray_samples((long long)D * D + (long long)H * H + (long long)W * W, D); }

struct CameraGeom {
    int D, H, W, S;
    float cz, cy, cx, tc;                  // (D - 1) / 2, (H - 1) / 2, (W - 1) / 2, (S - 1) / 2: half-integers, exact
};

VIEW_HD CameraGeom camera_geom(int D, int H, int W) {
    CameraGeom g;
    g.D = D; g.H = H; g.W = W; g.S = camera_samples(D, H, W);
    g.cz = 0.5f * (float)(D - 1); g.cy = 0.5f * (float)(H - 1); g.cx = 0.5f * (float)(W - 1); g.tc = 0.5f * (float)(g.S - 1);
    return g;
}

// a = x' - c_x, b = y' - c_y, t = s - (S - 1) / 2 (all exact); one rounding per operation: compile with -ffp-contract=off (csrc/Makefile
// does, and so does the host check)
VIEW_HD float camera_sample_x(float a, float b, float t, const CameraView &v, float cx) { return cx + ((a * v.rx + b * v.ex) + t * v.dx); }
VIEW_HD float camera_sample_y(float b, float t, const CameraView &v, float cy) { return cy + (b * v.ey + t * v.dy); }
VIEW_HD float camera_sample_z(float a, float b, float t, const CameraView &v, float cz) { return cz + ((a * v.rz + b * v.ez) + t * v.dz); }

// the extremes of the positions of image columns [xa, xb], rows [ya, yb] and samples [s0, s1], per axis
struct CameraBrick {
    float zmin, zmax, ymin, ymax, xmin, xmax;
};

VIEW_HD CameraBrick camera_brick(const CameraGeom &g, const CameraView &v, int xa, int xb, int ya, int yb, int s0, int s1) {
    const float a0 = (float)xa - g.cx, a1 = (float)xb - g.cx, b0 = (float)ya - g.cy, b1 = (float)yb - g.cy;
    const float t0 = (float)s0 - g.tc, t1 = (float)s1 - g.tc;
    CameraBrick k = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 8; ++i) {
        const float a = (i & 1) ? a1 : a0, b = (i & 2) ? b1 : b0, t = (i & 4) ? t1 : t0;
        const float z = camera_sample_z(a, b, t, v, g.cz), y = camera_sample_y(b, t, v, g.cy), x = camera_sample_x(a, b, t, v, g.cx);
        if (i == 0 || z < k.zmin) k.zmin = z;
        if (i == 0 || z > k.zmax) k.zmax = z;
        if (i == 0 || y < k.ymin) k.ymin = y;
        if (i == 0 || y > k.ymax) k.ymax = y;
        if (i == 0 || x < k.xmin) k.xmin = x;
        if (i == 0 || x > k.xmax) k.xmax = x;
    }
    return k;
}

// A position p has the taps floor(p) and floor(p) + 1; one of them is in [0, N) exactly when -1 <= p < N.  A brick is live when, on
// every axis, its interval of positions meets [-1, N); a brick that is not live has no tap inside the volume.
VIEW_HD bool camera_brick_live(const CameraGeom &g, const CameraBrick &k) {
    return k.zmax >= -1.0f && k.zmin < (float)g.D && k.ymax >= -1.0f && k.ymin < (float)g.H && k.xmax >= -1.0f && k.xmin < (float)g.W;
}

// the offset of voxel (z, y, x) inside its volume, in [0, D*H*W) (below 2^31 - 2^16), or -1 for a tap outside the volume
VIEW_HD int32_t camera_tap_offset(const CameraGeom &g, int z, int y, int x) {
    const bool in = (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H && (unsigned)x < (unsigned)g.W;
    return in ? (int32_t)(((int64_t)z * g.H + y) * g.W + x) : -1;
}

// The eight taps of the sample whose floors are (iz, iy, ix), tap n = (iz + (n >> 2), iy + ((n >> 1) & 1), ix + (n & 1)): off[n] is
// camera_tap_offset of that tap, formed from one base offset.  The base is formed in unsigned arithmetic (it wraps for floors far outside
// the volume and is then never used); for a tap inside the volume the sum is the tap's own offset, below 2^31.  This is what the kernel
// calls; the host check holds it equal to camera_tap_offset tap by tap.
VIEW_HD void camera_taps(const CameraGeom &g, int iz, int iy, int ix, int32_t off[8]) {
    const bool zin[2] = {(unsigned)iz < (unsigned)g.D, (unsigned)(iz + 1) < (unsigned)g.D};
    const bool yin[2] = {(unsigned)iy < (unsigned)g.H, (unsigned)(iy + 1) < (unsigned)g.H};
    const bool xin[2] = {(unsigned)ix < (unsigned)g.W, (unsigned)(ix + 1) < (unsigned)g.W};
    const uint32_t W = (uint32_t)g.W, HW = (uint32_t)g.H * W;
    const uint32_t base = ((uint32_t)iz * (uint32_t)g.H + (uint32_t)iy) * W + (uint32_t)ix;
    for (int n = 0; n < 8; ++n) {
        const int dz = n >> 2, dy = (n >> 1) & 1, dx = n & 1;
        const uint32_t o = base + (dz ? HW : 0u) + (dy ? W : 0u) + (uint32_t)dx;
        off[n] = (zin[dz] && yin[dy] && xin[dx]) ? (int32_t)o : -1;
    }
}

// the trilinear combination in the spec's order; v[n]: tap n of camera_taps (0 for a tap outside the volume)
VIEW_HD float camera_trilinear(const float v[8], float fz, float fy, float fx) {
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float p0 = gy * (gx * v[0] + fx * v[1]) + fy * (gx * v[2] + fx * v[3]);
    const float p1 = gy * (gx * v[4] + fx * v[5]) + fy * (gx * v[6] + fx * v[7]);
    return (1.0f - fz) * p0 + fz * p1;
}

}  // namespace smk
