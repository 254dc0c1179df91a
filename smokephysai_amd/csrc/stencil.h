#pragma once
// The two forms of a Jacobi cell and the guard that chooses between them (k_jacobi_band, stencil.hip).  Plain C++ with no HIP type in
// it: a host program that defines SMK_CELL_FORMS_ONLY before including this file compiles exactly this text (tests/test_jacobi_cell_forms.py).
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMK_CELL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SMK_CELL_HD inline
#endif
namespace smk {
// navier_stokes.py:141-145: p_new = 0.25 * (up + dn + l + r - div), one rounding per operation, in this order.
SMK_CELL_HD float jacobi_cell_exact(float up, float dn, float l, float r, float d) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    float sm = up + dn;
    sm = sm + l;
    sm = sm + r;
    sm = sm - d;
    return 0.25f * sm;
}
// The same cell with nd = jacobi_cell_nd(d) formed once per launch: three adds and one fused multiply-add.  Scaling by 0.25 is exact in the
// normal range, so the single rounding of fma(S, 0.25, -d/4) is that of 0.25 * fl(S - d) -- as long as -0.25 * d is exact and the result
// cannot be rounded twice on its way into the denormal range.  jacobi_cell_guard(d) holds for exactly the d where both are certain:
// d = +-0 (both forms round S / 4 once; the signs of zero agree), or 2^-100 <= |d| <= 2^100 (a result below 2^-124 then needs S within a
// factor 2 of d, where S - d is exact by Sterbenz).  NaN and Inf fail it.  Without it the forms differ: S = 2^-149, d = -2^-148 gives
// 2^-149 exactly and 0 fused.
SMK_CELL_HD float jacobi_cell_nd(float d) { return -0.25f * d; }
SMK_CELL_HD float jacobi_cell_fused(float up, float dn, float l, float r, float nd) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    float sm = up + dn;
    sm = sm + l;
    sm = sm + r;
    return __builtin_fmaf(sm, 0.25f, nd);
}
SMK_CELL_HD bool jacobi_cell_guard(float d) {
    constexpr unsigned LO = (127u - 100u) << 23, HI = (127u + 100u) << 23;     // the bits of 2^-100 and 2^100
    const unsigned a = __builtin_bit_cast(unsigned, d) & 0x7fffffffu;
    return a == 0u || a - LO <= HI - LO;
}
}  // namespace smk

#ifndef SMK_CELL_FORMS_ONLY
#include "common.h"

namespace smk {

// All launchers enqueue on `st` and return a hipError_t from hipGetLastError().
hipError_t launch_zero_state(const Geom &g, StateView s, const uint8_t *dev_mask, hipStream_t st);
// device-side source record: denom = (float)(2*(radius/3)^2), fint = (float)intensity (host-computed doubles)
struct SrcDev { int x, y, radius; float denom, fint; };
// dev_first[b]..dev_first[b+1] indexes the sources of grid b (stable order).
hipError_t launch_add_sources(const Geom &g, float *density, const SrcDev *dev_src, const int *dev_first, hipStream_t st);
hipError_t launch_buoy_diffuse(const Geom &g, StateView in, StateView out, hipStream_t st);
hipError_t launch_diffuse(const float *in, float *out, int B, int R, int C, int pitch, float coef, hipStream_t st);
hipError_t launch_divergence(const Geom &g, const float *u, const float *v, float *div, int div_pitch, size_t div_stride,
                             hipStream_t st);
// `iters` Jacobi sweeps; result ends in p. p2 is scratch of the same layout as p.
hipError_t launch_jacobi(const Geom &g, float *p, float *p2, const float *div, int iters, hipStream_t st);
// Per-handle state of the single-launch (persistent) projection: hand-off flags of the bands (device), a host-visible status word
// the kernel sets when a bounded wait times out, and the running hand-off count the flags are compared with.
struct ProjectSync {
    unsigned *flags = nullptr;
    volatile unsigned *status = nullptr;
    unsigned seq = 0;
    int flags_len = 0;
    bool disabled = false;
    // which cell form the sweeps of each (grid, band) took in the handle's latest projection (device; 1 fused, 0 exact: see the cell
    // forms above), rewritten by every launch of a kernel that has both forms (forms_two; the others take the exact cell and write nothing);
    // forms_nb: bands per grid of that projection, 0 when it ran without the band kernel
    unsigned *forms = nullptr;    // (inside the flags allocation, behind the abort word)
    int forms_nb = 0;
    bool forms_two = false;
};
hipError_t project_sync_create(ProjectSync &ps, int B);
void project_sync_destroy(ProjectSync &ps);
// true exactly once after a persistent launch of this handle reported a timed-out hand-off (acknowledges the word, disables the persistent form)
bool project_sync_take_timeout(ProjectSync &ps);
// divergence + `iters` Jacobi sweeps + gradient subtraction on (u, v, p); p2 and div are scratch.  With `ps` the projection runs as one
// persistent launch where the plan allows (stencil.hip: k_jacobi_band<..., PERSIST>); returns hipErrorLaunchTimeOut once if an earlier
// persistent launch reported a timed-out wait, and uses the multi-launch form afterwards.
hipError_t launch_project(const Geom &g, float *u, float *v, float *p, float *p2, float *div, int iters, hipStream_t st,
                          ProjectSync *ps = nullptr);
// buoyancy + diffusion (in -> out.u, out.v, out.d) followed by the projection of (out.u, out.v) with p: where the plan is persistent and
// folds (jacobi_plan.h), the first stage runs as the prologue of that one launch.
hipError_t launch_buoy_project(const Geom &g, StateView in, StateView out, float *p, float *div, int iters, hipStream_t st, ProjectSync *ps);
// JSON description of what launch_project does for this geometry (kernel, bands, launches, sweeps per launch, on-chip estimates).
// in / out: the state a step reads and the scratch state its projection rewrites (their alignment is part of the plan); null: aligned.
std::string describe_projection(const Geom &g, int iters, const ProjectSync *ps = nullptr, const StateView *in = nullptr,
                                const StateView *out = nullptr);
// "buoy_diffuse": the form a step's buoyancy + diffusion takes ("vec4", "scalar", "folded into the projection"), "buoy_diffuse_stage":
// the form of the stage run alone (smk_sim_run_stage), "alignment": what the gates were given -- members of smk_sim_describe's object.
std::string describe_step_forms(const Geom &g, int iters, const ProjectSync *ps, const StateView &in, const StateView &out);
hipError_t launch_grad_subtract(const Geom &g, float *u, float *v, const float *p, hipStream_t st);
// kind 0: field=u (H+1 x W), 1: field=v (H x W+1), 2: density (H x W) with *0.995 decay and optional frame emit.
hipError_t launch_advect(const Geom &g, int kind, const float *field, float *out, const float *u, const float *v,
                         float *frames, int64_t frame_stride_b, const float *fractal, float fractal_intensity,
                         int32_t *x0, int32_t *y0, hipStream_t st);
// The three advections of one step (u, v, density with decay + frame emit) as one launch: in = (u2, v2, -, d2), out = (u, v, -, density).
hipError_t launch_advect_fused(const Geom &g, StateView in, StateView out, float *frames, int64_t frame_stride_b, const float *fractal,
                               float fractal_intensity, hipStream_t st);
// mode 0 bilinear_interpolate, 1 interpolate_velocity_u, 2 interpolate_velocity_v on n caller-given coordinates per field
// (cstride 0: the B fields share one coordinate list).
hipError_t launch_interp(int mode, const float *field, int B, int h, int w, int pitch, size_t fstride, const float *y,
                         const float *x, size_t cstride, size_t n, float *out, hipStream_t st);
hipError_t launch_fractal_constants(int N, float *perlin, float *mandel, float *field, hipStream_t st);
hipError_t launch_apply_fractal(const float *in, float *out, const float *fractal, int n_fields, int N, float intensity,
                                hipStream_t st);

}  // namespace smk
#endif  // SMK_CELL_FORMS_ONLY
