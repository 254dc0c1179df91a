// The gather plan of the free-camera render's gradient (SPEC_3D.md section 10, "Free camera -- Gradient"; csrc/render_camera_grad.hip).
// Plain C++ for host and device, built on camera_plan.h: the kernels, their launcher and the stand-alone host check
// (tests/host/camera_grad_plan_main.cpp) compile this text.
//
// The transpose of the interpolation is a gather: a thread owns voxel (z, y, x), inverts the rotation to the ray coordinates (column, row,
// sample) of the voxel's centre and visits the samples within CAMERA_GRAD_REACH of it on each ray axis.  r, e, d are orthonormal up to
// fp32 rounding, so the inversion is three dot products.  A sample one of whose eight taps is the voxel lies within 1 of it per volume
// axis, so within sqrt(3) = 1.7321 in each ray coordinate; the window reaches 1.75 on either side.  The margin, 0.018, has to cover the
// fp32 error of the inversion and of the candidate's position: each is a sum of three products of magnitude at most 2112 * 1 (half the
// longest ray at the backward's limits, D <= 64, H <= 4096, W <= 1024), so below 6 * 2^-24 * 2112 * 3 < 2.3e-3 each, plus the
// coefficients' departure from orthonormality (2^-24 per coefficient against offsets up to 2112: another 1.2e-3).  That is why the backward
// has a height limit of its own: at the forward's H = 65536 the same sums reach 0.04.  The closed interval [p - 1.75, p + 1.75] holds at
// most four integers: CAMERA_GRAD_WINDOW candidates per axis, first = ceil(p - 1.75).  Every candidate's position is formed again by
// camera_sample_x / _y / _z, as the forward forms it, and the candidate counts with the forward's weight when one of its taps is the voxel:
// what the window decides is only which samples are looked at (the host check proves that none is missed), never a weight.
//
// The per-sample scratch.  The ray pass leaves, for every image row it marches, two planes [S][W] (Q', R) and one row [W] (K) under a +-y
// light, or the row K alone unlit; Q = Q' - K (render_camera_grad.hip).  The scratch is capped at CAMERA_GRAD_SCRATCH_FLOATS (256 MiB).
//
// Bands.  With pitch a voxel's candidates lie in up to four image rows that depend on (z, y, x) and on the view, so no cut of the image
// rows keeps a voxel's samples together.  Instead a band of `band` image rows starting at y0 OWNS the voxels whose first row candidate,
// clamped to [0, H - 1], lies in [y0, y0 + band), and marches the rows [y0, y0 + band + 3) n [0, H): every candidate row of every voxel it
// owns.  The bands tile [0, H), so every voxel is written by exactly one band per view, from all of its candidates in one fixed order,
// and the result does not depend on the band height or on how many volumes share a launch.  A unit of the walk is up to
// CAMERA_GRAD_VOLS_PER_LAUNCH volumes x one band.
#pragma once
#include <stdint.h>

#include "camera_plan.h"

namespace smk {

constexpr int CAMERA_GRAD_WINDOW = 4;                      // candidates per axis
constexpr float CAMERA_GRAD_REACH = 1.75f;
constexpr int CAMERA_GRAD_VOLS_PER_LAUNCH = 16;            // coefficient sets that travel as launch arguments
constexpr int64_t CAMERA_GRAD_SCRATCH_FLOATS = 1LL << 26;  // 256 MiB
constexpr int CAMERA_GRAD_BAND_ROWS = 32;                  // image rows a band owns (low on purpose: small shapes run several bands)
constexpr int CAMERA_GRAD_MAX_HEIGHT = 4096;               // the margin of the window (above); a marched row stays below 35 MB

// the ray coordinates of the centre of voxel (z, y, x), as image column, image row and sample index (fractional)
VIEW_HD void camera_grad_invert(const CameraGeom &g, const CameraView &v, int z, int y, int x, float *col, float *row, float *smp) {
    const float px = (float)x - g.cx, py = (float)y - g.cy, pz = (float)z - g.cz;
    *col = g.cx + (px * v.rx + pz * v.rz);
    *row = g.cy + ((px * v.ex + py * v.ey) + pz * v.ez);
    *smp = g.tc + ((px * v.dx + py * v.dy) + pz * v.dz);
}

// the first of the CAMERA_GRAD_WINDOW candidates about p
VIEW_HD int camera_grad_first(float p) { return (int)ceilf(p - CAMERA_GRAD_REACH); }

// the image row that decides which band owns a voxel: its first row candidate, clamped to the image
VIEW_HD int camera_grad_owner_row(float row, int H) {
    const int f = camera_grad_first(row);
    return f < 0 ? 0 : f > H - 1 ? H - 1 : f;
}

// The weight with which voxel (z, y, x) enters sample k of pixel (yrow, xcol): the forward's, 0 when none of the sample's taps is the
// voxel.  One fixed product order.
VIEW_HD float camera_grad_weight(const CameraGeom &g, const CameraView &v, int xcol, int yrow, int k, int z, int y, int x) {
    const float a = (float)xcol - g.cx, b = (float)yrow - g.cy, t = (float)k - g.tc;
    const float pz = camera_sample_z(a, b, t, v, g.cz), py = camera_sample_y(b, t, v, g.cy), px = camera_sample_x(a, b, t, v, g.cx);
    const float zf = floorf(pz), yf = floorf(py), xf = floorf(px);
    // floors far outside the volume (|position| < 2^18) give differences that are not 0 or 1
    const int dz = z - (int)zf, dy = y - (int)yf, dx = x - (int)xf;
    if ((unsigned)dz > 1u || (unsigned)dy > 1u || (unsigned)dx > 1u) return 0.f;
    const float fz = pz - zf, fy = py - yf, fx = px - xf;
    return (dz ? fz : 1.0f - fz) * ((dy ? fy : 1.0f - fy) * (dx ? fx : 1.0f - fx));
}

// whether the backward takes this shape: the forward's limits and H <= CAMERA_GRAD_MAX_HEIGHT
VIEW_HD bool camera_grad_shape_ok(int D, int H, int W) {
    return D >= 1 && D <= CAMERA_MAX_DEPTH && H >= 1 && H <= CAMERA_GRAD_MAX_HEIGHT && W >= 1 && W <= CAMERA_MAX_WIDTH;
}

// ---- the scratch
struct CameraGradPlan {
    int S, H, W, lit;
    int band;                                              // image rows a band owns
    int slots;                                             // image rows a band marches at most: min(band + 3, H)
    int max_vols;                                          // volumes that share a unit at most
    int64_t row_floats;                                    // what one marched image row leaves
    int64_t fit_rows;                                      // marched rows the cap holds (>= 7 within the limits)
    int64_t scratch_floats;
};

// band_rows: CAMERA_GRAD_BAND_ROWS on the device; the host check walks every height
VIEW_HD CameraGradPlan camera_grad_plan(int64_t n, int D, int H, int W, bool lit, int band_rows = CAMERA_GRAD_BAND_ROWS) {
    CameraGradPlan p;
    p.S = camera_samples(D, H, W); p.H = H; p.W = W; p.lit = lit ? 1 : 0;
    p.row_floats = lit ? (2 * (int64_t)p.S + 1) * W : (int64_t)W;
    p.fit_rows = CAMERA_GRAD_SCRATCH_FLOATS / p.row_floats;
    int64_t band = p.fit_rows - (CAMERA_GRAD_WINDOW - 1);
    if (band > band_rows) band = band_rows;
    if (band > H) band = H;
    if (band < 1) band = 1;                                // not within the limits (camera_grad_shape_ok)
    p.band = (int)band;
    p.slots = p.band + CAMERA_GRAD_WINDOW - 1 < H ? p.band + CAMERA_GRAD_WINDOW - 1 : H;
    int64_t nv = p.fit_rows / p.slots;
    if (nv > CAMERA_GRAD_VOLS_PER_LAUNCH) nv = CAMERA_GRAD_VOLS_PER_LAUNCH;
    if (nv > n) nv = n;
    if (nv < 1) nv = 1;
    p.max_vols = (int)nv;
    p.scratch_floats = nv * p.slots * p.row_floats;
    return p;
}

// the image rows [y0, *yend) that the band starting at y0 marches
VIEW_HD int camera_grad_march_end(const CameraGradPlan &p, int y0) { return y0 + p.slots < p.H ? y0 + p.slots : p.H; }

// element offsets into the scratch; vi: the volume's number inside its unit, in [0, max_vols); yrow in [y0, camera_grad_march_end)
VIEW_HD int64_t camera_grad_row(const CameraGradPlan &p, int vi, int y0, int yrow) { return (int64_t)vi * p.slots + (yrow - y0); }
VIEW_HD int64_t camera_grad_at_q(const CameraGradPlan &p, int64_t row, int k, int xcol) { return row * p.row_floats + (int64_t)k * p.W + xcol; }
VIEW_HD int64_t camera_grad_at_r(const CameraGradPlan &p, int64_t row, int k, int xcol) {
    return row * p.row_floats + ((int64_t)p.S + k) * p.W + xcol;
}
VIEW_HD int64_t camera_grad_at_k(const CameraGradPlan &p, int64_t row, int xcol) {
    return row * p.row_floats + (p.lit ? 2 * (int64_t)p.S * p.W : 0) + xcol;
}

// A slab of voxel rows [*ya, *yb] outside which the band at y0 owns nothing at this view (empty: *ya > *yb).  The row coordinate is
// c_y + e . (p - c) with e_y >= 0: over (z, x) it varies by at most |e_x| c_x + |e_z| c_z about its value at the row's centre, and it
// does not fall with y.  An owned voxel's row lies in (y0 - 1 + 1.75, y0 + band - 1 + 1.75], without a lower end for the first band and
// without an upper end for the last; the slab is wider than that by CAMERA_GRAD_SLAB_MARGIN, far above the fp32 error of the row
// coordinate (2.3e-3, above).  The slab only sizes the gather's grid: ownership is decided voxel by voxel.
constexpr float CAMERA_GRAD_SLAB_MARGIN = 0.125f;
VIEW_HD void camera_grad_slab(const CameraGeom &g, const CameraView &v, const CameraGradPlan &p, int y0, int *ya, int *yb) {
    const float spread = fabsf(v.ex) * g.cx + fabsf(v.ez) * g.cz + CAMERA_GRAD_SLAB_MARGIN;
    const bool first = y0 == 0, last = y0 + p.band >= g.H;
    const float lo = (float)y0 + (CAMERA_GRAD_REACH - 1.0f), hi = (float)(y0 + p.band) + (CAMERA_GRAD_REACH - 1.0f);
    int a = 0, b = g.H - 1;
    if (!first) while (a <= b && g.cy + ((float)a - g.cy) * v.ey + spread < lo) ++a;
    if (!last) while (b >= a && g.cy + ((float)b - g.cy) * v.ey - spread > hi) --b;
    *ya = a; *yb = b;
}

}  // namespace smk
