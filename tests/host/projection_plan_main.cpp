// Host check of the projection's launch plan (smokephysai_amd/csrc/jacobi_plan.h), built and run by tests/test_projection_plan_host.py:
// the very text the launchers and the kernel compile.
//   projection_plan invariants       what every shape plan (plan_projection) must satisfy, over a sweep of geometries; prints the counts and each violation
//   projection_plan table FILE       recomputes every PLAN / DESC line of FILE from its nine inputs and prints the file as it should read
//   projection_plan wrapper          the plans of the simulator classes' own layout (rows padded to 32 floats, 16-byte aligned pointers) at every
//                                    shape bench.py and tests/test_hip_physics.py step, against the plans recorded before the alignment gates
//   projection_plan alignment        over pitches W .. W+9, pointer offsets 0 / 4 / 8 / 12 and odd and even H: every wide access of the
//                                    selected forms (DESIGN "Stepper state layouts") is naturally aligned, by address arithmetic
//   projection_plan forms H W B pc pv in_off uv_off iters allow     the form strings smk_sim_describe reports for one layout
#include "jacobi_plan.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace smk;

static PlanGeom geom(int H, int W, int pc, int pv, int B) { return PlanGeom{H, W, B, pc, pv, (size_t)H * pc}; }
static int up32(int x) { return (x + 31) / 32 * 32; }

static int violations = 0;
#define REQUIRE(cond, ...)                                                                        \
    do {                                                                                          \
        if (!(cond) && ++violations <= 20) {                                                      \
            printf("VIOLATION %s: %s -- ", what, #cond);                                          \
            printf(__VA_ARGS__);                                                                  \
            printf("\n");                                                                         \
        }                                                                                         \
    } while (0)

static void check_plan(const PlanGeom &g, int iters, int num_cu, bool with_gradient, const ProjectionPlan &pp, const char *what) {
    const int H = g.H, TR = JB_NW * pp.rpw, nb = pp.nb, halo = pp.halo;
    const bool persist = pp.form == ProjectionForm::persistent;
    // the bands: owned ranges tile [0, H), tiles lie in the grid and hold the owned rows and the halo rows (those the grid has) of each inner side
    int next = 0;
    for (int band = 0; band < nb; ++band) {
        const BandRows r = jb_band_rows(H, TR, halo, nb, band);
        REQUIRE(r.own0 == next && r.own1 > r.own0, "band %d of %d owns [%d, %d), the one before ends at %d", band, nb, r.own0, r.own1, next);
        next = r.own1;
        REQUIRE(r.row0 >= 0 && r.row0 + TR <= H, "band %d: tile [%d, %d) of H = %d", band, r.row0, r.row0 + TR, H);
        const int need0 = band == 0 ? 0 : (r.own0 - halo > 0 ? r.own0 - halo : 0), need1 = band == nb - 1 ? H : (r.own1 + halo < H ? r.own1 + halo : H);
        REQUIRE(r.row0 <= need0 && r.row0 + TR >= need1, "band %d: tile [%d, %d) needs [%d, %d)", band, r.row0, r.row0 + TR, need0, need1);
        if (persist && nb > 1) REQUIRE(r.own1 - r.own0 > halo, "band %d owns %d rows, halo %d", band, r.own1 - r.own0, halo);
    }
    REQUIRE(next == H, "the bands end at row %d of %d", next, H);
    // the runs
    int done = 0, last = 0;
    for (int c = 0; c < pp.parts; ++c) {
        last = jb_run_sweeps(iters, done, pp.parts, c);
        REQUIRE(last >= 1 && last <= halo, "run %d of %d has %d sweeps, halo %d", c, pp.parts, last, halo);
        done += last;
    }
    REQUIRE(done == iters, "%d runs make %d of %d sweeps", pp.parts, done, iters);
    if (with_gradient) REQUIRE(last <= halo - 1, "the last run has %d sweeps, halo %d", last, halo);
    if (!persist) REQUIRE(pp.parts % 2 == 0 || (pp.parts == 1 && iters == 1 && !with_gradient), "%d launches", pp.parts);
    if (persist) {
        REQUIRE(nb <= 64 && nb <= num_cu, "%d bands on %d CUs", nb, num_cu);
        REQUIRE(pp.parts >= 2 || nb == 1, "%d bands in %d chunk", nb, pp.parts);
        REQUIRE(pp.grids_per_launch >= 1 && pp.grids_per_launch * nb <= num_cu, "%d grids of %d bands on %d CUs", pp.grids_per_launch, nb, num_cu);
    }
    // the keep buffer: walk every band's numbered rows through the slot function
    const KeepStats ks = keep_stats(pp, H);
    if (persist && pp.folds) {
        int kept_all = 0, overflow_max = 0;
        std::vector<char> used;
        for (int band = 0; band < nb; ++band) {
            const BandRows r = jb_band_rows(H, TR, halo, nb, band);
            const int n = jb_keep_rows_numbered(r.own0, r.own1), scale = jb_keep_scale(n, ks.slots);
            used.assign(ks.slots > 0 ? ks.slots : 1, 0);
            int kept = 0;
            for (int idx = 0; idx < n; ++idx) {
                const int s = jb_keep_slot(idx, scale);
                if (s < 0) continue;
                REQUIRE(s < ks.slots && !used[s < ks.slots ? s : 0], "band %d: row %d takes slot %d of %d", band, idx, s, ks.slots);
                if (s < ks.slots) used[s] = 1;
                ++kept;
            }
            kept_all += kept;
            if (n - kept > overflow_max) overflow_max = n - kept;
        }
        REQUIRE(ks.kept_per_grid == kept_all && ks.max_overflow == overflow_max, "keep_stats %d kept, %d over; walked %d, %d", ks.kept_per_grid,
                ks.max_overflow, kept_all, overflow_max);
    } else {
        REQUIRE(ks.slots == 0 && ks.kept_per_grid == 0 && ks.max_overflow == 0, "keep rows without the folded persistent form");
    }
}

static int invariants() {
    const int Hs[] = {32, 40, 48, 64, 72, 96, 100, 128, 136, 192, 200, 256, 300, 384, 500, 512, 640, 768, 1000, 1024};
    const int Ws[] = {64, 96, 128, 192, 256, 512};
    long plans = 0, bands = 0, persistent = 0, folding = 0;
    char what[160];
    for (int H : Hs)
        for (int W : Ws)
            for (int pitch = 0; pitch < 3; ++pitch)           // the simulator's pitches; a v pitch, then a cell pitch, that is no multiple of 4
                for (int B : {1, 8, 64, 300})
                    for (int iters : {1, 2, 3, 5, 20, 40, 100})
                        for (int num_cu : {32, 256})
                            for (int allow = 0; allow < 2; ++allow)
                                for (int grad = 0; grad < 2; ++grad) {
                                    const PlanGeom g = geom(H, W, pitch == 2 ? W + 2 : up32(W), pitch == 1 ? W + 1 : up32(W + 1), B);
                                    const ProjectionPlan pp = plan_projection(g, iters, num_cu, allow != 0, grad != 0);
                                    ++plans;
                                    if (pp.form == ProjectionForm::sweeps) continue;
                                    ++bands;
                                    persistent += pp.form == ProjectionForm::persistent;
                                    folding += pp.form == ProjectionForm::persistent && pp.folds;
                                    snprintf(what, sizeof what, "H=%d W=%d pc=%d pv=%d B=%d iters=%d cu=%d allow=%d grad=%d", H, W, g.pc, g.pv, B, iters,
                                             num_cu, allow, grad);
                                    check_plan(g, iters, num_cu, grad != 0, pp, what);
                                }
    printf("PLANS %ld BAND_KERNEL %ld PERSISTENT %ld FOLDING %ld VIOLATIONS %d\n", plans, bands, persistent, folding, violations);
    return 0;
}

static int table(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    static char line[4096];
    while (fgets(line, sizeof line, f)) {
        int H, W, pc, pv, B, iters, cu, allow, grad;
        const bool plan = !strncmp(line, "PLAN ", 5), desc = !strncmp(line, "DESC ", 5);
        if (!plan && !desc) { fputs(line, stdout); continue; }
        if (sscanf(line + 5, "%d %d %d %d %d %d %d %d %d", &H, &W, &pc, &pv, &B, &iters, &cu, &allow, &grad) != 9) { fclose(f); return 3; }
        const PlanGeom g = geom(H, W, pc, pv, B);
        const ProjectionPlan pp = plan_projection(g, iters, cu, allow != 0, grad != 0);
        printf("%s %d %d %d %d %d %d %d %d %d | ", plan ? "PLAN" : "DESC", H, W, pc, pv, B, iters, cu, allow, grad);
        if (desc) { printf("%s\n", describe_plan(pp, iters, g, cu).c_str()); continue; }
        const KeepStats ks = keep_stats(pp, H);
        const char *form = pp.form == ProjectionForm::persistent ? "persistent" : (pp.form == ProjectionForm::bands ? "bands" : "sweeps");
        printf("%s %d %d %d %d %d %d %d %d %d %d %d\n", form, pp.vec, pp.rpw, pp.nb, pp.halo, pp.parts, pp.grids_per_launch, (int)pp.two_forms,
               (int)pp.pipelined, ks.slots, ks.kept_per_grid, ks.max_overflow);
    }
    fclose(f);
    return 0;
}

// {H, W, B, iters, allow_persist | form, vec, rpw, nb, halo, parts, grids_per_launch, folds, two_forms, pipelined, buoy_diffuse vec4}: what the
// planner and launch_buoy_diffuse chose for these geometries on 256 compute units before pointer and stride terms entered the gates.
static const int WRAPPER_PLANS[][16] = {
    {256, 256, 64, 100, 1, 2, 4, 6, 4, 21, 5, 64, 1, 1, 1, 1},
    {256, 256, 64, 100, 0, 1, 4, 6, 4, 21, 6, 0, 0, 0, 1, 1},
    {128, 128, 32, 20, 1, 2, 2, 3, 5, 14, 2, 48, 1, 0, 1, 1},
    {128, 128, 32, 20, 0, 1, 2, 3, 4, 10, 4, 0, 0, 0, 1, 1},
    {128, 128, 64, 20, 1, 2, 2, 4, 3, 16, 2, 80, 1, 0, 1, 1},
    {128, 128, 64, 20, 0, 1, 2, 3, 4, 10, 4, 0, 0, 0, 1, 1},
    {256, 256, 64, 20, 1, 2, 4, 6, 4, 21, 2, 64, 1, 1, 1, 1},
    {256, 256, 64, 20, 0, 1, 4, 6, 4, 21, 2, 0, 0, 0, 1, 1},
    {64, 64, 1, 20, 1, 2, 1, 4, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {64, 64, 1, 20, 0, 1, 1, 2, 4, 10, 4, 0, 0, 0, 1, 1},
    {40, 56, 1, 20, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {40, 56, 1, 20, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {48, 48, 1, 20, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {48, 48, 1, 20, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {128, 128, 1, 20, 1, 2, 2, 3, 5, 14, 2, 48, 1, 0, 1, 1},
    {128, 128, 1, 20, 0, 1, 2, 2, 9, 10, 4, 0, 0, 0, 1, 1},
    {256, 256, 1, 20, 1, 2, 4, 2, 14, 7, 3, 16, 1, 0, 1, 1},
    {256, 256, 1, 20, 0, 1, 4, 2, 20, 10, 4, 0, 0, 0, 1, 1},
    {64, 64, 8, 20, 1, 2, 1, 4, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {64, 64, 8, 20, 0, 1, 1, 2, 4, 10, 4, 0, 0, 0, 1, 1},
    {48, 48, 5, 7, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {48, 48, 5, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {512, 512, 2, 37, 1, 2, 8, 2, 41, 10, 4, 6, 0, 0, 1, 1},
    {512, 512, 2, 37, 0, 1, 8, 3, 48, 19, 4, 0, 0, 0, 1, 1},
    {128, 256, 2, 45, 1, 2, 4, 2, 9, 10, 5, 24, 1, 0, 1, 1},
    {128, 256, 2, 45, 0, 1, 4, 2, 13, 12, 6, 0, 0, 0, 1, 1},
    {320, 64, 2, 100, 1, 2, 1, 3, 17, 15, 7, 8, 1, 0, 1, 1},
    {320, 64, 2, 100, 0, 1, 1, 4, 20, 25, 6, 0, 0, 0, 1, 1},
    {192, 128, 2, 21, 1, 2, 2, 3, 7, 12, 2, 32, 1, 0, 1, 1},
    {192, 128, 2, 21, 0, 1, 2, 2, 17, 11, 4, 0, 0, 0, 1, 1},
    {256, 256, 2, 7, 1, 2, 4, 2, 11, 4, 2, 16, 1, 0, 1, 1},
    {256, 256, 2, 7, 0, 1, 4, 2, 11, 4, 4, 0, 0, 0, 1, 1},
    {64, 64, 2, 100, 1, 2, 1, 4, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {64, 64, 2, 100, 0, 1, 1, 4, 1, 1048576, 2, 0, 0, 0, 1, 1},
    {33, 50, 2, 20, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {33, 50, 2, 20, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {70, 131, 2, 9, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {70, 131, 2, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {45, 70, 2, 6, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {45, 70, 2, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {32, 64, 2, 4, 1, 2, 1, 2, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {32, 64, 2, 4, 0, 1, 1, 2, 1, 1048576, 2, 0, 0, 0, 1, 1},
    {96, 192, 2, 8, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {96, 192, 2, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {67, 129, 2, 5, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {67, 129, 2, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {40, 128, 2, 3, 1, 2, 2, 2, 2, 12, 2, 128, 1, 0, 1, 1},
    {40, 128, 2, 3, 0, 1, 2, 2, 2, 12, 2, 0, 0, 0, 1, 1},
    {64, 64, 2, 5, 1, 2, 1, 4, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {64, 64, 2, 5, 0, 1, 1, 2, 3, 8, 2, 0, 0, 0, 1, 1},
    {31, 63, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {31, 63, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {33, 65, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {33, 65, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {8, 200, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {8, 200, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {130, 66, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {130, 66, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {256, 256, 32, 20, 1, 2, 4, 3, 8, 9, 3, 32, 1, 0, 1, 1},
    {256, 256, 32, 20, 0, 1, 4, 4, 6, 12, 2, 0, 0, 0, 1, 1},
    {192, 128, 64, 40, 1, 2, 2, 4, 4, 10, 5, 64, 1, 0, 1, 1},
    {192, 128, 64, 40, 0, 1, 2, 6, 3, 24, 2, 0, 0, 0, 1, 1},
    {320, 64, 64, 100, 1, 2, 1, 8, 4, 32, 4, 64, 1, 0, 1, 1},
    {320, 64, 64, 100, 0, 1, 1, 8, 4, 32, 4, 0, 0, 0, 1, 1},
    {128, 128, 128, 20, 1, 2, 2, 6, 2, 32, 2, 128, 1, 0, 1, 1},
    {128, 128, 128, 20, 0, 1, 2, 3, 4, 10, 4, 0, 0, 0, 1, 1},
    {128, 256, 64, 8, 1, 2, 4, 3, 4, 10, 2, 64, 1, 0, 1, 1},
    {128, 256, 64, 8, 0, 1, 4, 3, 3, 4, 4, 0, 0, 0, 1, 1},
    {512, 256, 32, 24, 1, 2, 4, 6, 7, 13, 2, 32, 1, 1, 1, 1},
    {512, 256, 32, 24, 0, 1, 4, 6, 7, 13, 2, 0, 0, 0, 1, 1},
    {32, 48, 1, 20, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {32, 48, 1, 20, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
    {64, 64, 3, 20, 1, 2, 1, 4, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {64, 64, 3, 20, 0, 1, 1, 2, 4, 10, 4, 0, 0, 0, 1, 1},
    {48, 64, 1, 20, 1, 2, 1, 3, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {48, 64, 1, 20, 0, 1, 1, 2, 3, 12, 2, 0, 0, 0, 1, 1},
    {48, 64, 3, 20, 1, 2, 1, 3, 1, 1048576, 1, 256, 1, 0, 1, 1},
    {48, 64, 3, 20, 0, 1, 1, 2, 3, 12, 2, 0, 0, 0, 1, 1},
};

static int wrapper() {
    int n = 0, bad = 0;
    for (const auto &r : WRAPPER_PLANS) {
        const PlanGeom g = geom(r[0], r[1], up32(r[1]), up32(r[1] + 1), r[2]);
        const PlanLayout l = plan_layout_of(g);
        const ProjectionPlan pp = plan_projection_on(g, l, r[3], 256, r[4] != 0, true);
        const int got[11] = {(int)pp.form, pp.vec, pp.rpw, pp.nb, pp.halo, pp.parts, pp.grids_per_launch, (int)pp.folds, (int)pp.two_forms,
                             (int)pp.pipelined, (int)buoy_diffuse_vec4(g, l)};
        ++n;
        if (memcmp(got, r + 5, sizeof got)) {
            ++bad;
            printf("MISMATCH H=%d W=%d B=%d iters=%d allow=%d: form %d vec %d rpw %d nb %d halo %d parts %d gpl %d folds %d two %d pipe %d vec4 %d\n", r[0],
                   r[1], r[2], r[3], r[4], got[0], got[1], got[2], got[3], got[4], got[5], got[6], got[7], got[8], got[9], got[10]);
        }
    }
    printf("WRAPPER %d MISMATCH %d\n", n, bad);
    return 0;
}

// One wide access of a selected form: `bytes` at base_off + 4 (grid * stride + row * pitch + j0) for every grid, row and lane start j0 (a
// multiple of `cells`).  Checked by the addresses themselves, not by the predicate the gate uses.
static long misaligned(int bytes, int base_off, int B, size_t stride, int rows, int pitch, int W, int cells) {
    long bad = 0;
    for (int b = 0; b < B; ++b)
        for (int row = 0; row < rows; ++row)
            for (int j0 = 0; j0 < W; j0 += cells) bad += (base_off + 4 * (b * stride + (size_t)row * pitch + j0)) % bytes != 0;
    return bad;
}

static int alignment() {
    const int Hs[] = {33, 64, 65, 96, 97, 128, 129}, Ws[] = {50, 52, 64, 128, 131, 256, 512}, offs[] = {0, 4, 8, 12};
    long cases = 0, bad = 0, n_vec4 = 0, n_scalar = 0, n_fold = 0, n_band[9] = {0}, n_sweeps = 0;
    for (int H : Hs)
        for (int W : Ws)
            for (int pc = W; pc <= W + 9; ++pc)
                for (int pv = W + 1; pv <= W + 10; ++pv)
                    for (int in_off : offs)
                        for (int uv_off : offs)
                            for (int B : {1, 3})
                                for (int iters : {6, 20})
                                    for (int allow = 0; allow < 2; ++allow) {
                                        // (the worst case: one of the pointers has the offset, the others are 16-byte aligned)
                                        const PlanGeom g = geom(H, W, pc, pv, B);
                                        const PlanLayout l = plan_layout_of(g, ptr_align((unsigned long long)in_off), ptr_align((unsigned long long)uv_off));
                                        const ProjectionPlan pp = plan_projection_on(g, l, iters, 256, allow != 0, true);
                                        ++cases;
                                        long m = 0;
                                        const bool fold = pp.form == ProjectionForm::persistent && pp.folds;
                                        if (!fold && buoy_diffuse_vec4(g, l)) {
                                            // k_buoy_diffuse4: float4 on u (H+1 rows), v, density of the input; the same on the scratch state (offset 0)
                                            ++n_vec4;
                                            for (int off : {in_off, 0})
                                                m += misaligned(16, off, B, l.su, H + 1, pc, W, 4) + misaligned(16, off, B, l.sv, H, pv, W, 4) +
                                                     misaligned(16, off, B, g.sc, H, pc, W, 4);
                                        } else if (!fold) {
                                            ++n_scalar;
                                        }
                                        if (pp.form == ProjectionForm::sweeps) { ++n_sweeps; bad += m; continue; }
                                        ++n_band[pp.vec];
                                        const int a = jb_access_bytes(pp.vec), cells = pp.vec;
                                        // the tail: ldv / stv of u and v rows (the projected u, v: uv_off); each float4 of an 8-cell lane is its own access
                                        m += misaligned(a, uv_off, B, l.su, H, pc, W, cells > 4 ? 4 : cells) + misaligned(a, uv_off, B, l.sv, H, pv, W, cells > 4 ? 4 : cells);
                                        if (pp.form == ProjectionForm::persistent)      // the hand-off rows in the exchange buffers (the handle's own: offset 0)
                                            m += misaligned(a, 0, B, g.sc, H, pc, W, cells > 4 ? 4 : cells);
                                        if (fold) {
                                            ++n_fold;
                                            m += misaligned(a, in_off, B, l.su, H + 1, pc, W, cells) + misaligned(a, in_off, B, l.sv, H, pv, W, cells) +
                                                 misaligned(a, in_off, B, g.sc, H, pc, W, cells);
                                        }
                                        if (m && bad < 20)
                                            printf("MISALIGNED H=%d W=%d pc=%d pv=%d in_off=%d uv_off=%d B=%d iters=%d allow=%d: %ld accesses (vec %d)\n", H, W, pc, pv,
                                                   in_off, uv_off, B, iters, allow, m, pp.vec);
                                        bad += m;
                                    }
    printf("ALIGNMENT CASES %ld VEC4 %ld SCALAR %ld FOLD %ld BAND1 %ld BAND2 %ld BAND4 %ld BAND8 %ld SWEEPS %ld MISALIGNED %ld\n", cases, n_vec4, n_scalar, n_fold,
           n_band[1], n_band[2], n_band[4], n_band[8], n_sweeps, bad);
    return 0;
}

static int forms(char **a) {
    const int H = atoi(a[0]), W = atoi(a[1]), B = atoi(a[2]), pc = atoi(a[3]), pv = atoi(a[4]), in_off = atoi(a[5]), uv_off = atoi(a[6]),
              iters = atoi(a[7]), allow = atoi(a[8]);
    const PlanGeom g = geom(H, W, pc, pv, B);
    const PlanLayout l = plan_layout_of(g, ptr_align((unsigned long long)in_off), ptr_align((unsigned long long)uv_off));
    const ProjectionPlan pp = plan_projection_on(g, l, iters, 256, allow != 0, true);
    const bool fold = pp.form == ProjectionForm::persistent && pp.folds;
    char kernel[64];
    if (pp.form == ProjectionForm::sweeps) snprintf(kernel, sizeof kernel, "k_jacobi_sweep");
    else snprintf(kernel, sizeof kernel, "k_jacobi_band<%d,%d>", pp.vec, pp.rpw);
    printf("%s|%s|%s|%s\n", kernel, pp.form == ProjectionForm::persistent ? "persistent" : "launches",
           fold ? "folded into the projection" : (buoy_diffuse_vec4(g, l) ? "vec4" : "scalar"), buoy_diffuse_vec4(g, l) ? "vec4" : "scalar");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "wrapper")) return wrapper();
    if (argc == 2 && !strcmp(argv[1], "alignment")) return alignment();
    if (argc == 11 && !strcmp(argv[1], "forms")) return forms(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "invariants")) return invariants();
    if (argc == 3 && !strcmp(argv[1], "table")) return table(argv[2]);
    fprintf(stderr, "usage: %s invariants | table FILE | wrapper | alignment | forms H W B pc pv in_off uv_off iters allow\n", argv[0]);
    return 2;
}
