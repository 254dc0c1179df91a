// The sample geometry and the staging plan of the orbit render (SPEC_3D.md section 10, "Orbit views"; csrc/render_orbit.hip).  Plain
// C++ for host and device: the kernel, its launcher and the stand-alone host check (tests/host/orbit_plan_main.cpp) compile this text.
//
// A workgroup renders a strip of ORBIT_STRIP image columns x' for ORBIT_ROWS rows y and marches the S samples of its rays in chunks of
// ORBIT_CHUNK.  The samples of (strip, chunk) are a rotated rectangle in the (z, x) plane; what the workgroup stages in LDS is that
// rectangle's bounding box, clipped to the volume, [z0, z1] x [x0, x1] with rows of nx = x1 - x0 + 1 floats.  A neighbour of a sample is
// read from the box when it lies in it and counts as 0 otherwise, so an index can never leave the box; what the host check proves is
// that no neighbour INSIDE the volume is ever outside the box (the image would be wrong, not the memory access) and that no box is
// larger than ORBIT_BOX_FLOATS.
//
// Every position is formed in fp32 by orbit_sample_z / orbit_sample_x and nowhere else.  Both are monotone in a for fixed t and in t for
// fixed a (each operation rounds monotonically), so over a rectangle of (a, t) the extremes are at its corners: the box needs no margin.
#pragma once
#include "view_plan.h"                     // the angle rule (orbit_cos_sin), ray_samples

namespace smk {

constexpr int ORBIT_STRIP = 32;            // image columns per workgroup
constexpr int ORBIT_ROWS = 4;              // image rows per workgroup (threads = ORBIT_STRIP * ORBIT_ROWS)
constexpr int ORBIT_CHUNK = 32;            // samples marched per staged box
constexpr int ORBIT_BOX_SIDE = 46;         // floor(hypot(STRIP - 1, CHUNK - 1)) + 3 rows or columns at most
constexpr int ORBIT_BOX_FLOATS = ORBIT_BOX_SIDE * ORBIT_BOX_SIDE;
constexpr int ORBIT_MAX_DEPTH = 64;
constexpr int ORBIT_MAX_WIDTH = 1024;

struct OrbitGeom {
    int D, W, S;
    float cz, cx, tc;                      // (D - 1) / 2, (W - 1) / 2, (S - 1) / 2: half-integers, exact
};

// S: the smallest integer >= hypot(D, W) with the parity of D
VIEW_HD int orbit_samples(int D, int W) { return ray_samples((long long)D * D + (long long)W * W, D); }

VIEW_HD OrbitGeom orbit_geom(int D, int W) {
    OrbitGeom g;
    g.D = D; g.W = W; g.S = orbit_samples(D, W);
    g.cz = 0.5f * (float)(D - 1); g.cx = 0.5f * (float)(W - 1); g.tc = 0.5f * (float)(g.S - 1);
    return g;
}

// a = x' - c_x, t = s - (S - 1) / 2 (both exact); one rounding per operation: compile with -ffp-contract=off (csrc/Makefile does, and
// so does the host check)
VIEW_HD float orbit_sample_x(float a, float t, float c, float s, float cx) { return cx + (a * c + t * s); }
VIEW_HD float orbit_sample_z(float a, float t, float c, float s, float cz) { return cz + (t * c - a * s); }

struct OrbitBox {
    int z0, z1, x0, x1;                    // inclusive, clipped to the volume; empty when z0 > z1 or x0 > x1
    VIEW_HD bool empty() const { return z0 > z1 || x0 > x1; }
    VIEW_HD int nz() const { return z1 - z0 + 1; }
    VIEW_HD int nx() const { return x1 - x0 + 1; }
};

// the box of image columns [xa, xb] and samples [s0, s1]
VIEW_HD OrbitBox orbit_box(const OrbitGeom &g, float c, float s, int xa, int xb, int s0, int s1) {
    const float a0 = (float)xa - g.cx, a1 = (float)xb - g.cx, t0 = (float)s0 - g.tc, t1 = (float)s1 - g.tc;
    float zmin = 0.f, zmax = 0.f, xmin = 0.f, xmax = 0.f;
    for (int k = 0; k < 4; ++k) {
        const float a = (k & 1) ? a1 : a0, t = (k & 2) ? t1 : t0;
        const float z = orbit_sample_z(a, t, c, s, g.cz), x = orbit_sample_x(a, t, c, s, g.cx);
        if (k == 0 || z < zmin) zmin = z;
        if (k == 0 || z > zmax) zmax = z;
        if (k == 0 || x < xmin) xmin = x;
        if (k == 0 || x > xmax) xmax = x;
    }
    OrbitBox b;
    b.z0 = (int)floorf(zmin); b.z1 = (int)floorf(zmax) + 1;
    b.x0 = (int)floorf(xmin); b.x1 = (int)floorf(xmax) + 1;
    if (b.z0 < 0) b.z0 = 0;
    if (b.x0 < 0) b.x0 = 0;
    if (b.z1 > g.D - 1) b.z1 = g.D - 1;
    if (b.x1 > g.W - 1) b.x1 = g.W - 1;
    return b;
}

// element e of a box with rows of nx floats -> its row; inv_nx = 1.0f / nx.  Exact for the boxes built here: (e + 0.5) / nx is at least
// 0.5 / ORBIT_BOX_SIDE away from an integer, far more than the rounding of one fp32 product (the host check walks every e and nx).
VIEW_HD int orbit_box_row(int e, float inv_nx) { return (int)(((float)e + 0.5f) * inv_nx); }

}  // namespace smk
