#pragma once
// The launch plan of the 3-D Jacobi sweeps (launch3_jacobi, stencil3d.hip): how `iters` sweeps are cut into launches and which kernel a
// launch takes.  Plain C++ with no HIP type in it: a host program compiles exactly this text (tests/test_jacobi3d_plan_host.py).
#include <cstddef>
#include <cstdio>
#include <string>

namespace smk {

// What the plan depends on.  align: the alignment in bytes (a power of two, 4 .. 16) common to the base pointers of p, p2, p3 (where
// there is one) and div.
struct Jacobi3Geom {
    int B, W, pc;
    size_t sc;           // per-grid stride of a cell field: D H pc
    int align;
    bool third;          // a third pressure buffer exists
};

struct Jacobi3Plan {
    // rows of W cells as whole quads: W and the pitch in multiples of 4
    bool vec = false;
    // ... and every quad 16-byte aligned: base pointers and the grid stride too (the plane stride H pc follows from the pitch).  The
    // four-cells-per-thread kernels (k3_jacobi_v4, k3_jacobi4) access p, pn and div as float4 and run only where this holds.
    bool quad = false;
    int n4 = 0, n2 = 0, n1 = 0;      // launches of 4, 2 and 1 sweeps, in this order
};

inline Jacobi3Plan plan3_jacobi(const Jacobi3Geom &g, int iters) {
    Jacobi3Plan pl;
    pl.vec = g.W % 4 == 0 && g.pc % 4 == 0;
    pl.quad = pl.vec && g.align % 16 == 0 && g.sc % 4 == 0;
    // temporally blocked launches of at most 4 sweeps first, single sweeps for the rest.  The result must end in p without a copy.  Two
    // buffers ping-pong, so an even launch count does; an odd count of three or more goes p -> p2 -> p3 -> p2 -> ... -> p through the
    // third buffer (J = 20: five 4-sweep launches); without a third buffer one 4-sweep launch is traded for two 2-sweep ones
    int left = iters < 0 ? 0 : iters, n = 0;
    const bool blocked = g.B <= 65535;
    int n4 = blocked ? left / 4 : 0;
    if (n4 > 60) n4 = 60;
    if (!g.third && left % 4 == 0 && (n4 & 1) && n4 * 4 == left) --n4;
    n = n4;
    left -= 4 * n4;
    if (blocked)
        for (; left >= 2 && n < 62; left -= 2) { ++n; ++pl.n2; }
    pl.n4 = n4;
    pl.n1 = left;
    return pl;
}

// The kernel of a temporally blocked launch and of a single sweep.
inline const char *plan3_blocked_form(const Jacobi3Plan &pl) { return pl.quad ? "quad v4<T>" : "xt"; }
inline const char *plan3_sweep_form(const Jacobi3Plan &pl) { return pl.quad ? "quad per-sweep" : "per-sweep"; }

// The members "jacobi" (the form of the blocked launches; of the single sweeps where there is no blocked launch), "jacobi_sweep" (the
// form of the single sweeps, null without one), "jacobi_launches" and "alignment" of smk_sim3d_describe's JSON object.
inline std::string describe_plan3(const Jacobi3Plan &pl, const Jacobi3Geom &g) {
    char buf[512];
    const bool any_blocked = pl.n4 + pl.n2 > 0;
    std::string sweep = pl.n1 > 0 ? std::string("\"") + plan3_sweep_form(pl) + "\"" : std::string("null");
    snprintf(buf, sizeof buf,
             "\"jacobi\": \"%s\", \"jacobi_sweep\": %s, \"jacobi_launches\": {\"four_sweeps\": %d, \"two_sweeps\": %d, \"one_sweep\": %d}, "
             "\"alignment\": {\"pressure_bytes\": %d, \"pitch_c\": %d, \"stride_c\": %zu, \"vec\": %s, \"quad\": %s}",
             any_blocked ? plan3_blocked_form(pl) : plan3_sweep_form(pl), sweep.c_str(), pl.n4, pl.n2, pl.n1, g.align, g.pc, g.sc,
             pl.vec ? "true" : "false", pl.quad ? "true" : "false");
    return buf;
}

}  // namespace smk
