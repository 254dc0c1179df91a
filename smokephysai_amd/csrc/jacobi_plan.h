#pragma once
// The launch plan of the 2-D pressure projection (k_jacobi_band, stencil.hip): which rows a band owns, how the sweeps are cut into runs, which
// form a call takes and with which kernel -- each worked out here once, for the kernel, its launchers and describe_projection alike.  Plain
// C++ with no HIP type in it: a host program compiles exactly this text (tests/test_projection_plan_host.py).
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMK_PLAN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SMK_PLAN_HD inline
#endif
namespace smk {

constexpr int JB_NW = 16;                                     // waves of a band's workgroup: a tile is JB_NW * rpw rows

// The integers of a Geom (common.h) that the shape plan depends on.
struct PlanGeom {
    int H, W, B;
    int pc, pv;          // row pitches of the cell fields and of v
    size_t sc;           // plane stride of a cell field
};
// What the alignment gates need to know beyond the PlanGeom: the other grid strides and the addresses a call runs on.
struct PlanLayout {
    size_t su, sv;       // plane strides of u (H + 1 rows of pc) and of v (H rows of pv)
    // Alignment in bytes (a power of two, 4 .. 16: ptr_align) common to the base pointers of
    int in_align;        //   the state a step reads: the caller's u, v and density (k_buoy_diffuse4, the prologue of a plan that folds)
    int uv_align;        //   the u and v the projection's gradient rewrites (the tail of k_jacobi_band)
};
// The strides smk_sim_create derives from the pitches; 16-byte aligned pointers unless said otherwise.
inline PlanLayout plan_layout_of(const struct PlanGeom &g, int in_align = 16, int uv_align = 16) {
    return PlanLayout{(size_t)(g.H + 1) * g.pc, (size_t)g.H * g.pv, in_align, uv_align};
}
// The alignment the addresses OR-ed into `bits` share, capped at the 16 bytes of the widest access any stepper kernel makes.
inline int ptr_align(unsigned long long bits) { return (bits & 15) == 0 ? 16 : ((bits & 7) == 0 ? 8 : 4); }

// ---- the alignment gates (DESIGN "Stepper state layouts") ----------------------------------------------------------------------------
// A row access of `bytes` (4, 8 or 16) at base + grid * stride + row * pitch + j0, with j0 a multiple of bytes / 4 floats, is naturally
// aligned for every grid and row exactly when base, pitch and grid stride are multiples of it.
inline bool rows_aligned(int bytes, int pitch, size_t stride, int base_align) {
    const int n = bytes / 4;
    return pitch % n == 0 && stride % (size_t)n == 0 && base_align % bytes == 0;
}
// The widest row access of k_jacobi_band<vec, ...>: ldv / stv move a lane's `vec` cells as float, float2 or float4 (VecT, stencil.hip).
SMK_PLAN_HD constexpr int jb_access_bytes(int vec) { return vec >= 4 ? 16 : 4 * vec; }
// The exchange buffers of the persistent form (the handle's own allocations: 256-byte aligned): pitch pc, stride sc.
inline bool jb_cell_rows_aligned(const PlanGeom &g, int vec) { return rows_aligned(jb_access_bytes(vec), g.pc, g.sc, 16); }
// The gradient epilogue's whole-row read-modify-write of u and v (jacobi_band_tail.h).
inline bool jb_tail_aligned(const PlanGeom &g, const PlanLayout &l, int vec) {
    const int a = jb_access_bytes(vec);
    return rows_aligned(a, g.pc, l.su, l.uv_align) && rows_aligned(a, g.pv, l.sv, l.uv_align);
}
// The folded prologue's row loads of the step's input u, v, density (its stores go where the tail's do: jb_tail_aligned).
inline bool jb_fold_aligned(const PlanGeom &g, const PlanLayout &l, int vec) {
    const int a = jb_access_bytes(vec);
    return rows_aligned(a, g.pc, l.su, l.in_align) && rows_aligned(a, g.pv, l.sv, l.in_align) && rows_aligned(a, g.pc, g.sc, l.in_align);
}
// The buoyancy + diffusion stage as a launch of its own: four columns per thread (k_buoy_diffuse4: 16-byte row accesses on the step's input
// u, v, density and on the handle's scratch state, which has the same pitches and strides) or one (k_buoy_diffuse).
inline bool buoy_diffuse_vec4(const PlanGeom &g, const PlanLayout &l) {
    return g.W % 4 == 0 && rows_aligned(16, g.pc, l.su, l.in_align) && rows_aligned(16, g.pv, l.sv, l.in_align) &&
           rows_aligned(16, g.pc, g.sc, l.in_align);
}

// Bands own unequal row ranges: the first and last band of a grid need a halo only on their inner side (the other side is the physical
// boundary), so they own TR - halo rows and the middle bands TR - 2 halo.  One band: the whole grid.  [own0, own1) are the rows the band
// owns, row0 the first row of its tile of TR rows.
struct BandRows { int own0, own1, row0; };
SMK_PLAN_HD BandRows jb_band_rows(int H, int TR, int halo, int nb, int band) {
    const int e_rows = TR - halo, m_rows = TR - 2 * halo;
    const int own0 = band == 0 ? 0 : e_rows + (band - 1) * m_rows;
    int own1 = band == nb - 1 ? H : e_rows + band * m_rows;
    own1 = own1 < H ? own1 : H;
    int r0 = band == 0 ? 0 : (band == nb - 1 ? H - TR : own0 - halo);
    if (r0 > H - TR) r0 = H - TR;
    if (r0 < 0) r0 = 0;
    return {own0, own1, r0};
}

// `iters` sweeps in `parts` nearly equal runs (ceil first, then floor): the sweeps of run c when `done` have been made.
SMK_PLAN_HD int jb_run_sweeps(int iters, int done, int parts, int c) { return (iters - done + (parts - c) - 1) / (parts - c); }

// Which order a sweep of k_jacobi_band takes (see `sweep` there), and how its interior rows split around the barrier.
// The persistent 4 x 8 instantiations sit at the 128-VGPR cap of a 1024-thread workgroup and would spill more in the pipelined order.
SMK_PLAN_HD constexpr bool jb_pipelined(int vec, int rpw, bool persist) { return !(persist && vec == 4 && rpw == 8); }

// Whether an instantiation carries both forms of the cell (stencil.h) and the guard that picks one per launch and workgroup: the form of
// the 256^2 x 64 step alone (persistent with the prologue, 4 cells per lane, 6 rows per wave), whose registers, scratch and occupancy stay
// where they were with the second sweep loop (125 -> 126 VGPRs) and which has been timed with it.  Every other instantiation has the
// exact cell only and compiles to the instructions it had before: with two loops the multi-launch forms took 4 - 28 more registers (three
// of them past the 64 that let two workgroups share a CU), 8 x 3 and 4 x 6 persistent went to the 128 cap, and the 32-cell forms spilled
// more.
SMK_PLAN_HD constexpr bool jb_two_forms(int vec, int rpw, bool persist, bool fold) { return persist && fold && vec == 4 && rpw == 6; }
// Whether the pipelined sweep of an instantiation steps its wave priority down between two barriers (`sweep`, jacobi_band_tail.h): 3 over
// the reads and the first interior rows behind the barrier, 2 over the last of them, 1 over the next sweep's edge rows and their publish, 0
// over the row ahead of the barrier and everywhere outside a sweep.  Issue goes to the highest priority first and among equals to the oldest
// wave, so with one level the four waves of a SIMD finish a sweep one after the other and wait at the barrier (profiles/r07); with the
// staircase whichever wave is behind wins the slot.  Arithmetic, LDS traffic and synchronisation are the same instructions in the same
// order.  True only for forms that have been timed with it (profiles/r34): the form of the 256^2 x 64 step.  Every other instantiation
// compiles to the instructions it had.
SMK_PLAN_HD constexpr bool jb_prio_stairs(int vec, int rpw, bool persist, bool fold) { return persist && fold && vec == 4 && rpw == 6; }
// Interior rows computed ahead of the barrier (they cover the publish); the others follow the reads.  Measured at 6 and 8 rows per wave
// (profiles/r07): one row ahead is the fastest split at 4 cells per lane; with none the stores are exposed, with all of them the reads.
// Under the staircase those rows run at the lowest priority and two of them are faster than one or none (profiles/r34/ab_variants.json).
SMK_PLAN_HD constexpr int jb_rows_before_barrier(int rpw, bool stairs = false) { return stairs ? 2 : (rpw > 2 ? 1 : 0); }
// The keep buffer of the PERSIST && FOLD form: the diffused u2 / v2 rows a band owns wait in LDS between the prologue and the gradient
// epilogue instead of going to HBM and back.  Beside `edge` (64 rows) and the flag word a workgroup, alone on its CU anyway, may declare
// the rest of the 160 KiB: that many rows of 64 * vec floats, at most the 2 * 16 * rpw a band can own.
constexpr int JB_LDS_BYTES = 163840;
SMK_PLAN_HD constexpr int jb_keep_rows(int vec, int rpw) {
    if (vec == 4 && rpw == 8) return 0;                       // at the 128-VGPR cap already (see jb_pipelined): the slot arithmetic would add spills
    const int row_bytes = 256 * vec, fit = (JB_LDS_BYTES - 64 * row_bytes - 4 * JB_NW - 16) / row_bytes;
    return fit < 2 * JB_NW * rpw ? fit : 2 * JB_NW * rpw;
}
// A band's owned rows are numbered v(own0), u(own0), v(own0 + 1), ... (u row 0 of the grid, which the gradient leaves alone, has no
// number): n of them.  With more rows than slots every (n / slots)-th row, in 16.16 fixed point, goes without one, so the rows that
// stay on the HBM path are spread evenly over the waves of the band rather than falling on its last waves.  The scale is rounded up,
// which for n <= 256 rows uses every slot and none twice.
SMK_PLAN_HD constexpr int jb_keep_rows_numbered(int own0, int own1) { return (own1 - (own0 > 1 ? own0 : 1)) + (own1 - own0); }
SMK_PLAN_HD constexpr int jb_keep_scale(int n, int slots) { return n <= slots ? 65536 : (slots * 65536 + n - 1) / n; }
SMK_PLAN_HD constexpr int jb_keep_slot(int idx, int scale) {  // the row's slot, or -1: no slot
    const int s = (idx * scale) >> 16;
    return (((idx + 1) * scale) >> 16) > s ? s : -1;
}

// What one projection launches.
enum class ProjectionForm {
    sweeps,        // no band plan: divergence, one k_jacobi_sweep launch per sweep, gradient
    bands,         // `parts` launches of k_jacobi_band, each a run of sweeps on register-resident tiles
    persistent,    // one launch of k_jacobi_band per grids_per_launch grids; the bands hand halo rows over between `parts` chunks
};
struct ProjectionPlan {
    ProjectionForm form = ProjectionForm::sweeps;
    int vec = 0, rpw = 0;          // cells per lane, rows per wave: the kernel's VEC, RPW
    int nb = 0, halo = 0;          // bands per grid; redundant rows on every inner side of a band (one band: none needed, 1 << 20)
    int parts = 0;                 // runs of sweeps between two refreshes of the halo rows: launches (bands) or chunks (persistent)
    int grids_per_launch = 0;      // persistent: grids whose bands are all co-resident (one 1024-thread workgroup per CU)
    bool folds = false;            // persistent: a step's buoyancy + diffusion stage can run as the launch's prologue
    bool two_forms = false;        // the kernel a whole step launches has both cell forms (jb_two_forms)
    bool pipelined = false;        // jb_pipelined
    bool prio_stairs = false;      // jb_prio_stairs
};

// Chunks of the persistent form: sizes are ceil / floor of iters / chunks (jb_run_sweeps), the largest <= halo, the last <= halo - 1 (the
// fused gradient needs the row above the owned range exact); two or more bands need two or more chunks (the first hand-off orders the
// final stores behind the neighbours' initial loads).  For iters >= 2 the count stays <= iters: one sweep per chunk passes both tests.
inline int jb_chunks(int iters, int halo) {
    int chunks = (iters + halo - 1) / halo;
    if (chunks < 2) chunks = 2;
    while (chunks < iters && ((iters + chunks - 1) / chunks > halo || iters / chunks > halo - 1)) ++chunks;
    return chunks;
}

// The band plan (vec, rpw, nb, halo) of the least estimated time; false -> no band plan: the generic per-sweep kernel.
// persist: cost the plan for the single-launch form (a hand-off between chunks instead of a relaunch), in which every band must own more
// rows than the halo: a band's halo rows then lie in its direct neighbour's owned range, and the u / v rows a neighbour's divergence
// reads are not rewritten before it has published once.  Its hand-off flags hold 64 bands per grid.
inline bool jb_search_bands(const PlanGeom &g, int iters, bool persist, ProjectionPlan &pp) {
    if (g.W % 64 != 0 || g.W / 64 > 8 || (g.W / 64 & (g.W / 64 - 1)) || g.pc % 4 != 0) return false;
    pp.vec = g.W / 64;
    // candidates: rows/wave; pick the plan with the least estimated time ~ launches*(t0 + iters*waves_of_work)
    const int rpws[] = {2, 3, 4, 6, 8};
    double best = 1e30;
    bool ok = false;
    for (int rpw : rpws) {
        if (pp.vec * rpw > 32) continue;                      // register budget (p + div)
        const int TR = JB_NW * rpw;
        if (TR > g.H) continue;
        for (int nb = 1; nb <= g.H / 8; ++nb) {
            // nb bands of TR rows cover H owned rows with a halo on every inner side: 2 (TR - h) + (nb - 2)(TR - 2h) >= H
            int halo = nb == 1 ? 1 << 20 : (nb * TR - g.H) / (2 * nb - 2);
            if (nb == 1 && TR != g.H) continue;
            if (nb * TR < g.H || halo < 2) continue;
            if (nb > 1) {
                if (halo > 64) halo = 64;
                if (halo > (TR - 1) / 2) halo = (TR - 1) / 2;          // middle bands keep at least one owned row
                if ((TR - halo) + (nb - 2) * (TR - 2 * halo) >= g.H) continue;   // a smaller halo than the cover needs: the last band would own nothing
            }
            if (persist && nb > 1) {
                auto owned = [&](int band) { const BandRows r = jb_band_rows(g.H, TR, halo, nb, band); return r.own1 - r.own0; };
                if (owned(0) <= halo || owned(nb - 1) <= halo || (nb > 2 && owned(1) <= halo) || nb > 64) continue;   // (middle bands own alike)
            }
            const double wgs = (double)nb * g.B, rounds = std::ceil(wgs / 256.0);
            // measured on MI355X with the pipelined sweep (profiles/r07/planner_fit.json: 256 rows x 64 grids at 6 rows per wave, J = 20 / 40 /
            // 60 / 100, and the nearest plans of 128^2 x 32 / x 64 at J = 20): a sweep of a 96-row workgroup takes 0.32 / 0.51 / 0.83 us at 1 / 2 /
            // 4 cells per lane, roughly linear in the rows a CU owns; prologue, loads and the gradient cost a row about 13 sweeps' worth; a
            // hand-off inside the persistent launch (2 * halo rows per band through sc1 stores / flag / sc1 loads) 2.8 us; a launch ~6 us, and
            // a relaunch reloads the band's p and div (~6 us with the boundary)
            const double cost_per_sweep = rounds * TR * ((0.15 + 0.17 * pp.vec) / 96.0), launch = 6.0, handoff = 2.8, fixed_sweeps = 13.0;
            const int chunks = persist && nb > 1 ? jb_chunks(iters, halo) : 1;
            const double cost = persist ? launch + (chunks - 1) * handoff + (iters + fixed_sweeps) * cost_per_sweep
                                        : 2 * std::ceil(0.5 * iters / halo) * launch + iters * cost_per_sweep;
            if (cost < best) { best = cost; pp.rpw = rpw; pp.nb = nb; pp.halo = halo; ok = true; }
        }
    }
    return ok;
}

// The plan of one projection of `iters` sweeps on `num_cu` compute units.  allow_persist: the run-time state permits the persistent form
// (a handle with hand-off flags that has seen no time-out, the switch on, no stream capture).  with_gradient: divergence and gradient
// run inside the first and last run (launch_project), so a run is at most halo - 1 sweeps; without it (launch_jacobi) at most halo.
inline ProjectionPlan plan_projection(const PlanGeom &g, int iters, int num_cu, bool allow_persist, bool with_gradient) {
    ProjectionPlan pp;
    // (x0 / x1 of the hand-off are addressed through 32-bit buffer offsets)
    if (with_gradient && allow_persist && iters >= 2 && jb_search_bands(g, iters, true, pp) && pp.halo >= 3 && pp.nb <= num_cu &&
        (pp.nb == 1 || (size_t)g.B * g.sc * sizeof(float) < (1ull << 31))) {
        pp.form = ProjectionForm::persistent;
        pp.parts = pp.nb == 1 ? 1 : jb_chunks(iters, pp.halo);
        pp.grids_per_launch = num_cu / pp.nb;
        if (pp.grids_per_launch >= 8) pp.grids_per_launch &= ~7;      // (whole rounds of the 8 XCDs: k_jacobi_band's block numbering)
        // 16-byte row accesses: pitches in multiples of 4; up to 4 cells per lane (with 8 the prologue's row windows do not fit)
        pp.folds = pp.vec <= 4 && g.pv % 4 == 0 && g.pc % 4 == 0;
    } else if ((with_gradient && iters < 2) || !jb_search_bands(g, iters, false, pp) || (with_gradient && pp.halo < 3)) {
        return ProjectionPlan{};
    } else {
        pp.form = ProjectionForm::bands;
        // an even number of nearly equal runs (global ping-pong ends back in p)
        const int cap = with_gradient ? pp.halo - 1 : pp.halo;
        pp.parts = !with_gradient && iters == 1 ? 1 : 2 * ((iters + 2 * cap - 1) / (2 * cap));
    }
    const bool persist = pp.form == ProjectionForm::persistent;
    pp.two_forms = jb_two_forms(pp.vec, pp.rpw, persist, pp.folds);
    pp.pipelined = jb_pipelined(pp.vec, pp.rpw, persist);
    pp.prio_stairs = jb_prio_stairs(pp.vec, pp.rpw, persist, pp.folds);
    return pp;
}

// The plan a launch takes: the shape plan above, held to the layout it is to run on.  plan_projection works the bands out from the grid's
// shape on the assumption that every row access of the band kernel is aligned; here a band plan whose accesses (jb_access_bytes(vec) wide)
// would not be naturally aligned under `l` gives way to the per-sweep kernel, and a plan folds only where the prologue's loads of the
// step's input are aligned too.  All band candidates of a shape have the same cells per lane, so no other band plan could pass instead.
inline ProjectionPlan plan_projection_on(const PlanGeom &g, const PlanLayout &l, int iters, int num_cu, bool allow_persist, bool with_gradient) {
    ProjectionPlan pp = plan_projection(g, iters, num_cu, allow_persist, with_gradient);
    if (pp.form == ProjectionForm::sweeps) return pp;
    if (!jb_cell_rows_aligned(g, pp.vec) || (with_gradient && !jb_tail_aligned(g, l, pp.vec))) return ProjectionPlan{};
    const bool persist = pp.form == ProjectionForm::persistent;
    pp.folds = pp.folds && jb_fold_aligned(g, l, pp.vec);
    pp.two_forms = jb_two_forms(pp.vec, pp.rpw, persist, pp.folds);
    pp.prio_stairs = jb_prio_stairs(pp.vec, pp.rpw, persist, pp.folds);
    return pp;
}

// The persistent launch with the folded prologue keeps a band's diffused u / v rows in LDS (k_jacobi_band, KEEP): slots per band, the
// rows of one grid that get a slot, and the most rows any band leaves on the HBM path.  All 0 for a plan without that form.
struct KeepStats { int slots, kept_per_grid, max_overflow; };
inline KeepStats keep_stats(const ProjectionPlan &pp, int H) {
    if (pp.form != ProjectionForm::persistent || !pp.folds) return {0, 0, 0};
    KeepStats ks{jb_keep_rows(pp.vec, pp.rpw), 0, 0};
    for (int band = 0; band < pp.nb; ++band) {
        const BandRows r = jb_band_rows(H, JB_NW * pp.rpw, pp.halo, pp.nb, band);
        const int n = jb_keep_rows_numbered(r.own0, r.own1), scale = jb_keep_scale(n, ks.slots);
        int kept = 0;
        for (int idx = 0; idx < n; ++idx) kept += jb_keep_slot(idx, scale) >= 0;
        ks.kept_per_grid += kept;
        if (n - kept > ks.max_overflow) ks.max_overflow = n - kept;
    }
    return ks;
}

// What the plan launches, as a JSON object (bench.py reports it as the stencil pass's on-chip bound: the Jacobi sweeps never touch HBM,
// so what limits them is sweeps x rows per workgroup x vector-issue time, not bytes).
inline std::string describe_plan(const ProjectionPlan &pp, int iters, const PlanGeom &g, int num_cu) {
    char buf[2048];
    if (pp.form == ProjectionForm::sweeps) {
        snprintf(buf, sizeof buf, "{\"kernel\": \"k_jacobi_sweep\", \"launches\": %d, \"sweeps\": %d, \"bound\": \"hbm (one pass over p and div per sweep)\"}",
                 iters + 2, iters);
        return buf;
    }
    const bool persist = pp.form == ProjectionForm::persistent;
    const int TR = JB_NW * pp.rpw;
    const int launches = persist ? (g.B + pp.grids_per_launch - 1) / pp.grids_per_launch : pp.parts;
    const double wgs = (double)pp.nb * g.B, rounds = std::ceil(wgs / num_cu);
    // measured (tools/probes/valu_probe, 4 waves per SIMD): a sweep row of 64 VEC-cell lanes = ~18 vector instructions of which 2 are DPP
    // wave shifts, ~2.6 cycles per instruction and SIMD -> TR rows on 4 SIMDs.  The edge-row exchange (publish -> s_barrier -> read) is
    // software-pipelined under those rows; what the in-kernel stamps show beyond the estimate is the four waves of a SIMD taking turns at its
    // vector issue, the youngest last, with the others waiting for it at the sweep's barrier (profiles/r07)
    // (with both cell forms a row is one instruction per cell shorter on the fused cell, which all but a trajectory's first steps take)
    const double valu_us_per_sweep = rounds * (TR / 4.0) * (18.0 - (pp.two_forms ? pp.vec : 0)) * 2.6 / 2100.0;
    const KeepStats ks = keep_stats(pp, g.H);
    snprintf(buf, sizeof buf,
             "{\"kernel\": \"k_jacobi_band<%d,%d>\", \"persistent\": %s, \"bands_per_grid\": %d, \"rows_per_workgroup\": %d, \"halo_rows\": %d, "
             "\"workgroups\": %d, \"launches\": %d, \"halo_handoffs\": %d, \"sweeps\": %d, \"sweeps_per_chunk\": %d, \"redundant_row_factor\": %.3f, "
             "\"keep_rows_per_band\": %d, \"keep_overflow_rows_max\": %d, \"keep_rows_per_grid\": %d, \"cell_forms_of_a_step\": %d, "
             "\"vector_issue_us_per_sweep_estimate\": %.3f, \"vector_issue_us_total_estimate\": %.1f, "
             "\"bound\": \"on-chip: sweeps x vector issue of rows_per_workgroup rows, one barrier per sweep (%s); p and div are "
             "register-resident %s\"}",
             pp.vec, pp.rpw, persist ? "true" : "false", pp.nb, TR, pp.halo, (int)wgs, launches, persist ? pp.parts - 1 : 0, iters,
             jb_run_sweeps(iters, 0, pp.parts, 0), (double)pp.nb * TR / g.H, ks.slots, ks.max_overflow, ks.kept_per_grid,
             pp.two_forms ? 2 : 1, valu_us_per_sweep, valu_us_per_sweep * iters,
             pp.pipelined
                 ? "the LDS edge-row exchange is pipelined over two sweeps: a wave's two edge rows and their publish come first, the interior rows "
                   "cover the stores and the read of the next sweep's neighbour rows"
                 : "plain order at the register cap: publish, interior rows, barrier, read of the neighbour rows, the two edge rows",
             persist ? "for the whole projection; bands hand halo rows to their neighbours through HBM between chunks" : "within a launch");
    return buf;
}

}  // namespace smk
