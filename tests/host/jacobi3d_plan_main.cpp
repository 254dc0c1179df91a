// Host check of the 3-D Jacobi launch plan (smokephysai_amd/csrc/jacobi3d_plan.h), built and run by tests/test_jacobi3d_plan_host.py: the very
// text launch3_jacobi compiles.
//   jacobi3d_plan alignment     over pitches W .. W+9, pointer offsets 0 / 4 / 8 / 12, odd and even H and D: the launches add up to the
//                               sweeps and fit the launcher's array, and where the four-cells-per-thread kernels are selected every float4 of p, pn and div is aligned
//   jacobi3d_plan wrapper       the simulator class's own layout keeps the plans recorded before the gate moved here
//   jacobi3d_plan forms B D H W pc off iters third      the Jacobi members of smk_sim3d_describe for one layout
#include "jacobi3d_plan.h"

#include <cstdlib>
#include <cstring>

using namespace smk;

static int up32(int x) { return (x + 31) / 32 * 32; }
static int align_of(int off) { return off % 16 == 0 ? 16 : (off % 8 == 0 ? 8 : 4); }

static int alignment() {
    long cases = 0, bad = 0, n_quad = 0, n_vec_only = 0, n_narrow = 0;
    for (int D : {4, 9})
        for (int H : {16, 21})
            for (int W : {19, 28, 64})
                for (int pc = W; pc <= W + 9; ++pc)
                    for (int off : {0, 4, 8, 12})
                        for (int B : {1, 2, 3})
                            for (int iters : {0, 1, 2, 3, 4, 6, 7, 12, 20})
                                for (int third = 0; third < 2; ++third) {
                                    const size_t sc = (size_t)D * H * pc;
                                    const Jacobi3Geom g{B, W, pc, sc, align_of(off), third != 0};
                                    const Jacobi3Plan pl = plan3_jacobi(g, iters);
                                    ++cases;
                                    long m = 4 * pl.n4 + 2 * pl.n2 + pl.n1 != iters;
                                    m += pl.n4 > 60 || pl.n4 + pl.n2 > 62 || pl.n4 < 0 || pl.n2 < 0 || pl.n1 < 0;      // (launch3_jacobi's plan array holds 64)
                                    if (pl.quad) {
                                        ++n_quad;
                                        // k3_jacobi_v4 / k3_jacobi4: float4 at base + grid sc + (z H + y) pc + x, x a multiple of 4, on p, pn, div
                                        for (int b = 0; b < B; ++b)
                                            for (int z = 0; z < D; ++z)
                                                for (int y = 0; y < H; ++y)
                                                    for (int x = 0; x < W; x += 4) m += (off + 4 * (b * sc + ((size_t)z * H + y) * pc + x)) % 16 != 0;
                                        m += W % 4 != 0;
                                    } else if (pl.vec) {
                                        ++n_vec_only;
                                    } else {
                                        ++n_narrow;
                                    }
                                    if (m && bad < 20) printf("VIOLATION D=%d H=%d W=%d pc=%d off=%d B=%d iters=%d third=%d: %ld\n", D, H, W, pc, off, B, iters, third, m);
                                    bad += m;
                                }
    printf("ALIGNMENT3D CASES %ld QUAD %ld VEC_NOT_QUAD %ld NARROW %ld VIOLATIONS %ld\n", cases, n_quad, n_vec_only, n_narrow, bad);
    return 0;
}

// {B, D, H, W, iters, third | quad, four_sweeps, two_sweeps, one_sweep}: launch3_jacobi's choice for the simulator class's layout (rows padded
// to 32 floats, 16-byte aligned pointers; a third buffer where smk_sim3d_create allocates one) before the gate moved into the header.
static const int WRAPPER_PLANS[][10] = {
    {8, 64, 512, 512, 20, 1, 1, 5, 0, 0}, {2, 4, 16, 64, 4, 0, 1, 0, 2, 0},  {2, 9, 20, 28, 7, 0, 1, 1, 1, 1},   {2, 13, 22, 19, 6, 0, 0, 1, 1, 0},
    {1, 16, 32, 32, 20, 1, 1, 5, 0, 0},   {1, 16, 32, 32, 12, 1, 1, 3, 0, 0}, {1, 16, 32, 32, 8, 0, 1, 2, 0, 0},  {1, 16, 32, 32, 3, 0, 1, 0, 1, 1},
    {1, 16, 32, 32, 1, 0, 1, 0, 0, 1},    {1, 16, 32, 30, 5, 0, 0, 1, 0, 1},
};

static int wrapper() {
    int n = 0, bad = 0;
    for (const auto &r : WRAPPER_PLANS) {
        const int pc = up32(r[3]);
        const Jacobi3Geom g{r[0], r[3], pc, (size_t)r[1] * r[2] * pc, 16, r[5] != 0};
        const Jacobi3Plan pl = plan3_jacobi(g, r[4]);
        ++n;
        if ((int)pl.quad != r[6] || pl.n4 != r[7] || pl.n2 != r[8] || pl.n1 != r[9]) {
            ++bad;
            printf("MISMATCH B=%d D=%d H=%d W=%d iters=%d third=%d: quad %d launches %d %d %d\n", r[0], r[1], r[2], r[3], r[4], r[5], (int)pl.quad, pl.n4,
                   pl.n2, pl.n1);
        }
    }
    printf("WRAPPER3D %d MISMATCH %d\n", n, bad);
    return 0;
}

static int forms(char **a) {
    const int B = atoi(a[0]), D = atoi(a[1]), H = atoi(a[2]), W = atoi(a[3]), pc = atoi(a[4]), off = atoi(a[5]), iters = atoi(a[6]), third = atoi(a[7]);
    const Jacobi3Geom g{B, W, pc, (size_t)D * H * pc, align_of(off), third != 0};
    printf("{%s}\n", describe_plan3(plan3_jacobi(g, iters), g).c_str());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "alignment")) return alignment();
    if (argc == 2 && !strcmp(argv[1], "wrapper")) return wrapper();
    if (argc == 10 && !strcmp(argv[1], "forms")) return forms(argv + 2);
    fprintf(stderr, "usage: %s alignment | wrapper | forms B D H W pc off iters third\n", argv[0]);
    return 2;
}
