// Host-side view of the sweep's priority staircase (jb_prio_stairs, smokephysai_amd/csrc/jacobi_plan.h), for
// tests/test_jacobi_prio_stairs_host.py: the trait over every (vec, rpw, persist, fold) that has a kernel, the plan of the headline
// shape, and the smallest batch and sweep count at 256 x 256 whose plan has the staircase.
#include <cstdio>

#include "jacobi_plan.h"

using namespace smk;

static PlanGeom geom(int H, int W, int B) {
    const int pc = (W + 31) / 32 * 32, pv = (W + 32) / 32 * 32;           // the simulator classes' pitches: rows padded to 32 floats
    return PlanGeom{H, W, B, pc, pv, (size_t)H * pc};
}

static void print_plan(const char *tag, int H, int W, int B, int iters, bool allow_persist) {
    const ProjectionPlan pp = plan_projection(geom(H, W, B), iters, 256, allow_persist, true);
    const char *form = pp.form == ProjectionForm::persistent ? "persistent" : (pp.form == ProjectionForm::bands ? "bands" : "sweeps");
    printf("%s %d %d %d %d %d | %s %d %d %d %d %d %d %d\n", tag, H, W, B, iters, (int)allow_persist, form, pp.vec, pp.rpw, pp.nb,
           (int)pp.folds, (int)pp.two_forms, (int)pp.pipelined, (int)pp.prio_stairs);
}

int main() {
    const int vecs[] = {1, 2, 4, 8}, rpws[] = {2, 3, 4, 6, 8};
    for (int vec : vecs)
        for (int rpw : rpws)
            for (int persist = 0; persist < 2; ++persist)
                for (int fold = 0; fold < 2; ++fold)
                    printf("TRAIT %d %d %d %d | %d\n", vec, rpw, persist, fold, (int)jb_prio_stairs(vec, rpw, persist != 0, fold != 0));
    print_plan("PLAN", 256, 256, 64, 100, true);
    print_plan("PLAN", 256, 256, 64, 100, false);
    print_plan("PLAN", 128, 128, 32, 20, true);
    print_plan("PLAN", 128, 128, 64, 20, true);
    // the smallest batch, and for it the smallest sweep count, at which a 256 x 256 simulator takes the form with the staircase
    for (int B = 1; B <= 64; ++B)
        for (int iters = 2; iters <= 100; ++iters) {
            const ProjectionPlan pp = plan_projection(geom(256, 256, B), iters, 256, true, true);
            if (pp.prio_stairs && pp.nb >= 2) {
                print_plan("SMALLEST", 256, 256, B, iters, true);
                return 0;
            }
        }
    printf("SMALLEST none\n");
    return 0;
}
