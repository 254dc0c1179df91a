// Host check of the two Jacobi cell forms and their guard (smokephysai_amd/csrc/stencil.h), built and run by
// tests/test_jacobi_cell_forms.py: the very text the kernel compiles, on operand pairs (S, d) chosen to stress the identity
//     fma(S, 0.25, -0.25 * d) == 0.25 * fl(S - d)        for every d the guard accepts.
// S enters the cells as `up` with -0 for the three other neighbours: x + (-0) == x for every x, zeros of both signs included.
#define SMK_CELL_FORMS_ONLY
#include "stencil.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

using smk::jacobi_cell_exact;
using smk::jacobi_cell_fused;
using smk::jacobi_cell_guard;
using smk::jacobi_cell_nd;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static inline uint64_t next64() {                              // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static inline float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static inline float any_finite() {                             // every finite bit pattern, denormals and both zeros included
    for (;;) {
        const uint32_t u = (uint32_t)next64();
        if ((u & 0x7f800000u) != 0x7f800000u) return from_bits(u);
    }
}
// a d the guard accepts: 2^-100 <= |d| <= 2^100, exponent uniform over e_lo .. e_hi (biased: 27 .. 227)
static inline float guarded_d(uint32_t e_lo = 27, uint32_t e_hi = 227) {
    const uint64_t r = next64();
    const uint32_t e = e_lo + (uint32_t)((r >> 32) % (e_hi - e_lo + 1));
    const uint32_t m = e == 227 ? 0u : (uint32_t)r & 0x007fffffu;
    return from_bits(((uint32_t)(r >> 63) << 31) | (e << 23) | m);
}

static unsigned long long pairs = 0, differing = 0, guard_rejected = 0;
static void pair(float S, float d) {
    if (!jacobi_cell_guard(d)) { ++guard_rejected; return; }
    const float nz = -0.0f;
    const float a = jacobi_cell_exact(S, nz, nz, nz, d), b = jacobi_cell_fused(S, nz, nz, nz, jacobi_cell_nd(d));
    ++pairs;
    if (bits(a) != bits(b)) {
        if (differing < 10) printf("DIFF S=%a d=%a exact=%a fused=%a\n", S, d, a, b);
        ++differing;
    }
}

int main() {
    // 1. S over all finite bit patterns, d over the whole guarded range
    for (int i = 0; i < 40000000; ++i) pair(any_finite(), guarded_d());
    // 2. S within +-16 ulp of d, S == d among them (the cancelling pairs), across the range and crowded at its lower end
    for (int i = 0; i < 1500000; ++i) {
        const float d = (i & 1) ? guarded_d() : guarded_d(27, 52);
        for (int k = -16; k <= 16; ++k) {
            const uint32_t u = bits(d) + (uint32_t)k;
            if ((u & 0x7f800000u) != 0x7f800000u) pair(from_bits(u), d);
        }
    }
    // 3. S denormal, d over the range and crowded at its lower end
    for (int i = 0; i < 20000000; ++i) {
        const uint64_t r = next64();
        const float S = from_bits(((uint32_t)(r >> 63) << 31) | ((uint32_t)r & 0x007fffffu));
        pair(S, (i & 1) ? guarded_d() : guarded_d(27, 30));
    }
    // 4. d = +-0 with any S; all sign combinations of zero explicitly
    for (int i = 0; i < 10000000; ++i) pair(any_finite(), (i & 1) ? 0.0f : -0.0f);
    for (int s = 0; s < 2; ++s)
        for (int t = 0; t < 2; ++t) pair(s ? -0.0f : 0.0f, t ? -0.0f : 0.0f);
    // 5. S within a factor 4 of d (results that may land in the denormal range): same sign and opposite
    for (int i = 0; i < 20000000; ++i) {
        const float d = (i & 3) ? guarded_d(27, 34) : guarded_d();
        const uint64_t r = next64();
        uint32_t e = (bits(d) >> 23 & 0xffu) + (uint32_t)(r >> 40) % 5u - 2u;
        if (e > 254u) e = 254u;
        pair(from_bits(((uint32_t)(r >> 63) << 31) | (e << 23) | ((uint32_t)r & 0x007fffffu)), d);
    }
    // 6. whole cells: four ordinary neighbours, d guarded
    unsigned long long cell_diff = 0;
    for (int i = 0; i < 10000000; ++i) {
        float n[4];
        for (float &x : n) x = from_bits(((uint32_t)next64() & 0x807fffffu) | ((100u + (uint32_t)(next64() % 56u)) << 23));
        const float d = (i & 1) ? guarded_d(90, 160) : 0.0f;
        ++pairs;
        if (bits(jacobi_cell_exact(n[0], n[1], n[2], n[3], d)) != bits(jacobi_cell_fused(n[0], n[1], n[2], n[3], jacobi_cell_nd(d)))) ++cell_diff;
    }
    differing += cell_diff;
    printf("PAIRS %llu DIFFERING %llu REJECTED_BY_GUARD %llu\n", pairs, differing, guard_rejected);

    // the guard's edges
    const float lo = std::ldexp(1.0f, -100), hi = std::ldexp(1.0f, 100);
    const float below = from_bits(bits(lo) - 1u), above = from_bits(bits(hi) + 1u);
    printf("GUARD nan=%d -nan=%d inf=%d -inf=%d below=%d -below=%d above=%d -above=%d lo=%d -lo=%d hi=%d -hi=%d zero=%d -zero=%d denormal=%d\n",
           jacobi_cell_guard(NAN), jacobi_cell_guard(-NAN), jacobi_cell_guard(INFINITY), jacobi_cell_guard(-INFINITY),
           jacobi_cell_guard(below), jacobi_cell_guard(-below), jacobi_cell_guard(above), jacobi_cell_guard(-above),
           jacobi_cell_guard(lo), jacobi_cell_guard(-lo), jacobi_cell_guard(hi), jacobi_cell_guard(-hi),
           jacobi_cell_guard(0.0f), jacobi_cell_guard(-0.0f), jacobi_cell_guard(std::ldexp(1.0f, -140)));

    // without the guard the forms differ: S = 2^-149, d = -2^-148
    const float S = std::ldexp(1.0f, -149), d = -std::ldexp(1.0f, -148), nz = -0.0f;
    const float a = jacobi_cell_exact(S, nz, nz, nz, d), b = jacobi_cell_fused(S, nz, nz, nz, jacobi_cell_nd(d));
    printf("COUNTEREXAMPLE guard=%d exact_bits=%08x fused_bits=%08x\n", jacobi_cell_guard(d), bits(a), bits(b));
    return 0;
}
