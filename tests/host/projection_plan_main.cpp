// Host check of the projection's launch plan (smokephysai_amd/csrc/jacobi_plan.h), built and run by tests/test_projection_plan_host.py:
// the very text the launchers and the kernel compile.
//   projection_plan invariants       what every plan must satisfy, over a sweep of geometries; prints the counts and each violation
//   projection_plan table FILE       recomputes every PLAN / DESC line of FILE from its nine inputs and prints the file as it should read
#include "jacobi_plan.h"

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

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "invariants")) return invariants();
    if (argc == 3 && !strcmp(argv[1], "table")) return table(argv[2]);
    fprintf(stderr, "usage: %s invariants | table FILE\n", argv[0]);
    return 2;
}
