// The gather plan of the orbit render's gradient (SPEC_3D.md section 10, "Orbit views -- Gradient"; csrc/render_orbit_grad.hip).  Plain
// C++ for host and device, built on orbit_plan.h: the kernels, their launcher and the stand-alone host check
// (tests/host/orbit_grad_plan_main.cpp) compile this text.
//
// The transpose of the interpolation is a gather: a thread owns voxel (z, x) of one row y, inverts the rotation to the ray coordinates
// (a*, t*) of the voxel's centre and visits the image columns x' and samples s within ORBIT_GRAD_REACH of it.  A sample one of whose four
// taps is the voxel lies within 1 of it in z and in x, so within sqrt(2) in a and in t; the window is 1.5 wide on either side, and the
// fp32 error of a position at W = 1024 is about 1e-4.  The closed interval [p - 1.5, p + 1.5] holds at most four integers:
// ORBIT_GRAD_WINDOW candidates per axis, first = ceil(p - 1.5).  Every candidate's position is formed again by orbit_sample_z /
// orbit_sample_x, as the forward forms it, and the candidate counts with the forward's weight when one of its taps is the voxel: what the
// window decides is only which samples are looked at (the host check proves that none is missed), never a weight.
//
// The per-sample scratch.  The ray pass leaves, for every image row it marches, ORBIT_GRAD_PLANES = 2 planes [S][W] (Q', R) and one row
// [W] (K) under a +-y light, or the row K alone unlit; Q = Q' - K (render_orbit_grad.hip).  The scratch holds as many rows as fit into
// ORBIT_GRAD_SCRATCH_FLOATS (256 MiB: the scratch of one step stays in the last-level cache), at least one, at most
// ORBIT_GRAD_VOLS_PER_LAUNCH volumes' worth; the launcher walks the batch in units of whole volumes, or of row ranges of one volume
// where a volume's rows do not fit.
#pragma once
#include <stdint.h>

#include "orbit_plan.h"

namespace smk {

constexpr int ORBIT_GRAD_WINDOW = 4;                       // candidates per axis
constexpr float ORBIT_GRAD_REACH = 1.5f;
constexpr int ORBIT_GRAD_VOLS_PER_LAUNCH = 16;             // (cos, sin) pairs that travel as launch arguments
constexpr int64_t ORBIT_GRAD_SCRATCH_FLOATS = 1LL << 26;   // 256 MiB

// the ray coordinates of the centre of voxel (z, x), as image column and sample index (fractional)
VIEW_HD void orbit_grad_invert(const OrbitGeom &g, float c, float s, int z, int x, float *col, float *smp) {
    const float dx = (float)x - g.cx, dz = (float)z - g.cz;
    *col = g.cx + (dx * c - dz * s);
    *smp = g.tc + (dx * s + dz * c);
}

// the first of the ORBIT_GRAD_WINDOW candidates about p
VIEW_HD int orbit_grad_first(float p) { return (int)ceilf(p - ORBIT_GRAD_REACH); }

// The weight with which voxel (z, x) enters sample (xcol, k): the forward's, 0 when none of the sample's taps is the voxel.
VIEW_HD float orbit_grad_weight(const OrbitGeom &g, float c, float s, int xcol, int k, int z, int x) {
    const float a = (float)xcol - g.cx, t = (float)k - g.tc;
    const float pz = orbit_sample_z(a, t, c, s, g.cz), px = orbit_sample_x(a, t, c, s, g.cx);
    const float zf = floorf(pz), xf = floorf(px);
    const int dz = z - (int)zf, dx = x - (int)xf;
    if ((unsigned)dz > 1u || (unsigned)dx > 1u) return 0.f;
    const float fz = pz - zf, fx = px - xf;
    return (dz ? fz : 1.0f - fz) * (dx ? fx : 1.0f - fx);
}

// ---- the scratch
struct OrbitGradPlan {
    int S, W, lit;
    int64_t row_floats;                                    // what one image row leaves
    int64_t cap_rows;                                      // rows the scratch holds
    int64_t scratch_floats;
};

VIEW_HD OrbitGradPlan orbit_grad_plan(int64_t n, int D, int H, int W, bool lit) {
    OrbitGradPlan p;
    p.S = orbit_samples(D, W); p.W = W; p.lit = lit ? 1 : 0;
    p.row_floats = lit ? (2 * (int64_t)p.S + 1) * W : (int64_t)W;
    const int64_t want = (n < ORBIT_GRAD_VOLS_PER_LAUNCH ? n : ORBIT_GRAD_VOLS_PER_LAUNCH) * (int64_t)H;
    const int64_t fit = ORBIT_GRAD_SCRATCH_FLOATS / p.row_floats;      // >= 31: a row is at most (2 * 1028 + 1) * 1024 floats
    p.cap_rows = want < fit ? want : fit;
    p.scratch_floats = p.cap_rows * p.row_floats;
    return p;
}

// element offsets into the scratch; row: the row's number inside its unit (volume-major), in [0, cap_rows)
VIEW_HD int64_t orbit_grad_at_q(const OrbitGradPlan &p, int64_t row, int k, int xcol) { return row * p.row_floats + (int64_t)k * p.W + xcol; }
VIEW_HD int64_t orbit_grad_at_r(const OrbitGradPlan &p, int64_t row, int k, int xcol) {
    return row * p.row_floats + ((int64_t)p.S + k) * p.W + xcol;
}
VIEW_HD int64_t orbit_grad_at_k(const OrbitGradPlan &p, int64_t row, int xcol) {
    return row * p.row_floats + (p.lit ? 2 * (int64_t)p.S * p.W : 0) + xcol;
}

// ---- the units of one call: volumes [v0, v0 + nv) x rows [y0, y0 + ny); nv > 1 only with all H rows
struct OrbitGradUnit {
    int64_t v0;
    int nv, y0, ny;
};

// the unit that starts at (v0, y0)
VIEW_HD OrbitGradUnit orbit_grad_unit(const OrbitGradPlan &p, int64_t n, int H, int64_t v0, int y0) {
    OrbitGradUnit u;
    u.v0 = v0; u.y0 = y0;
    if (y0 == 0 && (int64_t)H <= p.cap_rows) {
        int64_t nv = p.cap_rows / H;
        if (nv > ORBIT_GRAD_VOLS_PER_LAUNCH) nv = ORBIT_GRAD_VOLS_PER_LAUNCH;
        if (nv > n - v0) nv = n - v0;
        u.nv = (int)nv; u.ny = H;
    } else {
        u.nv = 1;
        u.ny = (int64_t)(H - y0) < p.cap_rows ? H - y0 : (int)p.cap_rows;
    }
    return u;
}

// where the next unit starts; false after the last
VIEW_HD bool orbit_grad_next(const OrbitGradUnit &u, int64_t n, int H, int64_t *v0, int *y0) {
    if (u.y0 + u.ny < H) { *v0 = u.v0; *y0 = u.y0 + u.ny; }
    else { *v0 = u.v0 + u.nv; *y0 = 0; }
    return *v0 < n;
}

}  // namespace smk
