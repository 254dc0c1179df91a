/*
 * smokehip.h -- C ABI of libsmokehip.so: the MI355X (gfx950) implementation of the SmokePhysAI hot path.
 *
 * The reference (MengAiDev/SmokePhysAI) has no FFI: its boundary for this path is the Python class API
 *   src/physics/navier_stokes.py:6-173   NavierStokesSimulator
 *   src/physics/smoke_simulator.py:8-45  SmokeSimulator.{add_incense_source,simulate_step}
 *   src/physics/fractal_generator.py:5-62 FractalGenerator
 *   src/models/smokephys_net.py:24-32,87-91  SmokePhysNet.input_encoder (+ pooling)
 * Each entry point below names the reference interface it replaces.  Callers are the drop-in Python
 * classes in smokephysai_amd/ (ctypes); INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success, <0 = smk_status; smk_last_error() gives a thread-local message;
 *  - all device memory for state/frames/weights/features is CALLER-OWNED (torch tensors): the library never
 *    frees or reallocates it; library-owned scratch lives in the handle and dies with smk_sim_destroy;
 *  - all work is enqueued on the caller-supplied hipStream_t (passed as void*), no implicit sync;
 *  - a handle is not thread-safe; distinct handles are independent;
 *  - fields are fp32, batch-major [B][rows][pitch] with explicit row pitches (in floats):
 *        u [B][H+1][pitch_c]  v [B][H][pitch_v]  p,density [B][H][pitch_c]     pitch_c >= W, pitch_v >= W+1
 *    (the reference's shapes are u[H+1,W], v[H,W+1], p/density[H,W]: navier_stokes.py:27-32).
 *  - state layouts (smk_sim, smk_sim3d and the stateless field helpers alike; DESIGN.md "Stepper state layouts"):
 *      * every pitch_c >= W and pitch_v >= W+1 is accepted, the reference's dense pitch_c = W, pitch_v = W+1 included;
 *      * u, v, (w,) p, density and frames need 4-byte alignment and nothing more;
 *      * every frame_stride_b and frame_stride_t under which the [H][W] ([D][H][W]) frames do not overlap is accepted, gaps and a
 *        transposed order (frame_stride_t < frame_stride_b) included;
 *      * results are bit-identical across all accepted layouts: a kernel form that accesses rows 8 or 16 bytes at a time is selected
 *        only where pitches, base pointers and grid strides make every such access naturally aligned, the narrower form otherwise
 *        (smk_sim_describe / smk_sim3d_describe name the forms and the alignment facts they were chosen on);
 *      * pad columns (col >= W, or > W for v, inside a row) never influence a result; their contents after a call are unspecified;
 *      * nothing outside a field's [B][rows][pitch] extent, or outside a frame's [H][W] elements, is read into a result or written.
 */
#ifndef SMOKEHIP_H
#define SMOKEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMK_ABI_VERSION 17

typedef enum smk_status {
    SMK_OK = 0,
    SMK_ERR_INVALID = -1,      /* bad argument / shape */
    SMK_ERR_HIP = -2,          /* a HIP runtime call failed (message has hipGetErrorString) */
    SMK_ERR_UNSUPPORTED = -3,  /* valid in the reference, not built here (message says what) */
    SMK_ERR_NO_DEVICE = -4,
    SMK_ERR_TIMEOUT = -5       /* a bounded wait inside a persistent launch ran out: results were poisoned (NaN), see smk_sim_status */
} smk_status;

int smk_abi_version(void);
const char *smk_last_error(void);

/* ------------------------------------------------------------------ simulation state */
typedef struct smk_sim smk_sim; /* opaque: one BATCH of independent grids */

typedef struct smk_sim_desc {
    int32_t batch, height, width;   /* B grids of H x W (reference: grid_size=(H,W), B=1) */
    int32_t jacobi_iters;           /* reference hard-codes 20 (navier_stokes.py:139) */
    double dt, viscosity;           /* doubles: the reference multiplies python floats before casting */
    int32_t device_id;
    int32_t pitch_c, pitch_v;       /* row pitches in floats */
    float *u, *v, *p, *density;     /* caller-owned device pointers, layout above */
} smk_sim_desc;

/* NavierStokesSimulator.__init__ (navier_stokes.py:9-22): binds the caller's state tensors, allocates
 * scratch (ping-pong fields, divergence), computes the shape-only fractal constant on the device. Does NOT
 * zero the state: call smk_sim_reset. */
int smk_sim_create(const smk_sim_desc *desc, smk_sim **out);
/* Frees the handle (always).  Returns SMK_ERR_TIMEOUT if a persistent projection of this handle timed out and nobody has been told yet
 * (the frames the caller read last were NaN); SMK_OK otherwise. */
int smk_sim_destroy(smk_sim *sim);

/* Health of the handle -- no reference counterpart (the reference is synchronous: navier_stokes.py:133-149 either returns right results or
 * raises).  The persistent projection (see smk_sim_step) bounds every inter-workgroup wait; when one runs out the kernel turns the band's
 * p / u / v into NaN (so every later frame of the grid is NaN: wrong results cannot pass as data) and sets a host-visible word.  This call
 * reads and acknowledges that word: SMK_ERR_TIMEOUT exactly once per event, SMK_OK otherwise; it does not synchronise -- call it after
 * the stream the steps ran on has been synchronised to learn about THOSE steps (the Python mirror's check() does both).  Every other
 * smk_sim_* entry point performs the same check on entry, so an event is never reported later than the next call on the handle. */
int smk_sim_status(smk_sim *sim);

/* NavierStokesSimulator.setup_grid (navier_stokes.py:24-35): zero u,v,p,density of the grids whose byte in
 * grid_mask (host, B bytes) is non-zero; NULL = all grids.  If a persistent-projection time-out is pending (smk_sim_status), this call
 * returns SMK_ERR_TIMEOUT once like any other entry point -- but it has carried out the reset, so it need not be repeated. */
int smk_sim_reset(smk_sim *sim, const uint8_t *grid_mask, void *stream);

typedef struct smk_source {
    int32_t grid;       /* batch index */
    int32_t x, y;       /* (column, row), as add_smoke_source(x, y, ...) */
    int32_t radius;
    double intensity;
} smk_source;

/* NavierStokesSimulator.add_smoke_source (navier_stokes.py:37-48), n sources in one launch; sources of the
 * same grid are applied in list order (fp32 += is order-sensitive). `sources` is a HOST array. */
int smk_sim_add_sources(smk_sim *sim, const smk_source *sources, int32_t n, void *stream);

/* NavierStokesSimulator.step x n_steps (navier_stokes.py:151-173) + SmokeSimulator.simulate_step's frame emit
 * (smoke_simulator.py:31-39).  After step t (0-based) the emitted frame of grid b is written to
 *     frames + t*frame_stride_t + b*frame_stride_b   as [H][W] contiguous fp32      (frames may be NULL)
 * with frame = density + (fractal_intensity*F)*density when add_fractal != 0 (fractal_generator.py:53-62, F the
 * shape-only constant), else frame = density.  Solver state keeps the unperturbed density.
 * Launches per time step: two where the band plan allows (buoyancy + diffusion + the whole pressure projection as one persistent
 * launch whose workgroups hand halo rows to each other with bounded waits, then the three advections as one launch).  The persistent
 * launch assumes this process has the device to itself (all its workgroups resident at once): if a wait times out (0.5 s) the
 * launch still drains, the affected grids' p / u / v / density / frames become NaN, and smk_sim_status after a stream synchronise -- or
 * at the latest the NEXT call on this handle, smk_sim_destroy included -- returns SMK_ERR_TIMEOUT with a message naming the persistent
 * projection (then: smk_sim_reset; later steps use one launch per chunk of sweeps).  SMK_JACOBI_PERSIST=0 in the environment selects that
 * form from the start; stream capture always records it. */
int smk_sim_step(smk_sim *sim, int32_t n_steps, float *frames, int64_t frame_stride_b, int64_t frame_stride_t,
                 int32_t add_fractal, double fractal_intensity, void *stream);

/* Single stages of step() on the handle's state, for per-stage parity tests.  State after each call is
 * back in the caller's tensors. */
typedef enum smk_stage {
    SMK_STAGE_BUOY_DIFFUSE = 0, /* navier_stokes.py:154-160 */
    SMK_STAGE_PROJECT = 1,      /* navier_stokes.py:133-149 */
    SMK_STAGE_ADVECT_U = 2,     /* navier_stokes.py:166 */
    SMK_STAGE_ADVECT_V = 3,     /* navier_stokes.py:167 */
    SMK_STAGE_ADVECT_D = 4      /* navier_stokes.py:168-171 (advect density + 0.995 decay) */
} smk_stage;
int smk_sim_run_stage(smk_sim *sim, int32_t stage, void *stream);

/* Divergence field of the current state (navier_stokes.py:136) -> out [B][H][W] contiguous. */
int smk_sim_divergence(smk_sim *sim, float *out, void *stream);

/* Back-trace gather indices of advection_step(field; u, v) on the current state (navier_stokes.py:87-92,
 * 115-123): which = 0 (field=u), 1 (field=v), 2 (field=density). x0,y0: int32 [B][R][C] contiguous. */
int smk_sim_backtrace(smk_sim *sim, int32_t which, int32_t *x0, int32_t *y0, void *stream);

/* Diagnostic for tests and tools (it synchronises `stream` and copies; smk_sim_step never reads anything back): which of the two
 * bit-identical forms of the Jacobi cell the sweeps of the handle's LATEST projection took, per grid and band of rows -- 1: three adds and
 * one fma with -div / 4 formed once per launch, taken where every divergence value of the band is +-0 or has 2^-100 <= |div| <= 2^100;
 * 0: the reference's five operations (navier_stokes.py:141-145), which is also all that most kernels have: only the one-launch step of the
 * 256 x 256 x 64 plan (4 cells per lane, 6 rows per wave) carries both forms; every other answers 0 here.  *bands_per_grid receives the bands per grid of that projection (0: no
 * projection yet, or one on the per-sweep kernel, which has the exact form only) and out[b * bands_per_grid + band] the words; capacity
 * (in words) must be at least batch * bands_per_grid -- batch * max(64, height / 8) always suffices.  smk_sim_describe's
 * "cell_forms_of_a_step" says whether this handle's step kernel has both forms (2) or the exact one only (1). */
int smk_sim_sweep_forms(smk_sim *sim, int32_t *out, int32_t capacity, int32_t *bands_per_grid, void *stream);

/* Device pointer to the fractal constants, [W][H] fp32 each (fractal_generator.py:12-51):
 * kind 0 = perlin, 1 = mandelbrot escape counts/100, 2 = 0.7*perlin+0.3*mandelbrot. Square grids only. */
int smk_sim_fractal(smk_sim *sim, int32_t kind, const float **dev_ptr);

/* Diagnostic: a JSON object (NUL-terminated, written into buf[capacity]) describing how this handle's step is launched -- the
 * projection's kernel, bands per grid, launches and sweeps per launch.  No reference counterpart (the reference runs 20 separate
 * sweeps, navier_stokes.py:139-145); bench.py reports it beside the stencil roofline.  Members: "projection" (the plan), "buoy_diffuse"
 * (the form a step's buoyancy + diffusion takes: "vec4", "scalar" or "folded into the projection"), "buoy_diffuse_stage" (the form of
 * SMK_STAGE_BUOY_DIFFUSE run alone: "vec4" or "scalar"), "alignment" (what the gates were given: the common alignment in bytes of the
 * caller's u, v, density and of the projected u, v, the pitches and grid strides, the bytes of a band kernel's row access),
 * "advection". */
int smk_sim_describe(smk_sim *sim, char *buf, int64_t capacity);

/* ------------------------------------------------------------------ 3-D simulation state (BASELINE configs[4])
 * No reference counterpart: the reference is 2-D only (navier_stokes.py:10,21).  Semantics = SPEC_3D.md, the rule-by-rule generalisation
 * of NavierStokesSimulator (navier_stokes.py:24-173) to grids [D][H][W]; each entry point names the 2-D method it generalises.
 * Fields, batch-major with explicit row pitches (floats):
 *     u [B][D][H+1][pitch_c]   v [B][D][H][pitch_v]   w [B][D+1][H][pitch_c]   p, density [B][D][H][pitch_c]
 * Conventions as for smk_sim: caller-owned state, library-owned scratch, caller's stream, no implicit sync. */
typedef struct smk_sim3d smk_sim3d;

typedef struct smk_sim3d_desc {
    int32_t batch, depth, height, width;
    int32_t jacobi_iters;           /* SPEC_3D.md section 4: default 20, like navier_stokes.py:139 */
    double dt, viscosity;
    int32_t device_id;
    int32_t pitch_c, pitch_v;
    float *u, *v, *w, *p, *density;
} smk_sim3d_desc;

typedef struct smk_source3d {
    int32_t grid;
    int32_t x, y, z;    /* (column, row, plane): add_smoke_source(x, y, ...) of navier_stokes.py:37 with the depth index appended */
    int32_t radius;
    double intensity;
} smk_source3d;

/* __init__ (navier_stokes.py:9-22) / setup_grid (:24-35) / add_smoke_source (:37-48) in 3-D. */
int smk_sim3d_create(const smk_sim3d_desc *desc, smk_sim3d **out);
int smk_sim3d_destroy(smk_sim3d *sim);
int smk_sim3d_reset(smk_sim3d *sim, const uint8_t *grid_mask, void *stream);
int smk_sim3d_add_sources(smk_sim3d *sim, const smk_source3d *sources, int32_t n, void *stream);

/* step() x n_steps (navier_stokes.py:151-173 -> SPEC_3D.md section 6).  After step t the density of grid b (the returned frame) is
 * written to frames + t*frame_stride_t + b*frame_stride_b as [D][H][W] contiguous fp32 (frames may be NULL). */
int smk_sim3d_step(smk_sim3d *sim, int32_t n_steps, float *frames, int64_t frame_stride_b, int64_t frame_stride_t, void *stream);

/* smk_sim3d_step with SmokeSimulator.simulate_step's frame emit (smoke_simulator.py:31-45 -> SPEC_3D.md section 9): add_fractal != 0 writes
 * frame + (fractal_intensity * F) * frame to `frames`, F the [W][H] shape-only constant that apply_fractal_perturbation
 * (fractal_generator.py:53-62) builds from field.shape[-2:] and broadcasts over the planes, with the roundings of smk_apply_fractal; the
 * solver state keeps the unperturbed density (smoke_simulator.py:36-39).  Needs H == W (SMK_ERR_UNSUPPORTED otherwise, as the reference
 * raises).  add_fractal == 0 or frames == NULL: exactly smk_sim3d_step. */
int smk_sim3d_step_emit(smk_sim3d *sim, int32_t n_steps, float *frames, int64_t frame_stride_b, int64_t frame_stride_t,
                        int32_t add_fractal, double fractal_intensity, void *stream);

/* Single stages of the 3-D step on the handle's state (per-stage parity tests); state is back in the caller's tensors afterwards. */
typedef enum smk_stage3d {
    SMK_STAGE3D_BUOY_DIFFUSE = 0, /* SPEC_3D.md 6.1-6.2 */
    SMK_STAGE3D_PROJECT = 1,      /* section 4 */
    SMK_STAGE3D_ADVECT_U = 2,
    SMK_STAGE3D_ADVECT_V = 3,
    SMK_STAGE3D_ADVECT_W = 4,
    SMK_STAGE3D_ADVECT_D = 5      /* density advect + 0.995 decay */
} smk_stage3d;
int smk_sim3d_run_stage(smk_sim3d *sim, int32_t stage, void *stream);

/* Diagnostic, as smk_sim_describe: a JSON object naming the form of every stage of this handle's step that has more than one.  "jacobi":
 * "quad v4<T>" (four cells per thread, 16-byte accesses) or "xt" (one cell per thread) for the temporally blocked launches -- or, where
 * jacobi_iters has none, the form of the single sweeps; "jacobi_sweep": "quad per-sweep" / "per-sweep" for the single sweeps left over
 * (null: none); "jacobi_launches": the launches of 4, 2 and 1 sweeps; "alignment": the common alignment in bytes of p and the pressure
 * scratch, pitch_c, the grid stride and the two predicates of the gate. */
int smk_sim3d_describe(smk_sim3d *sim, char *buf, int64_t capacity);

/* ------------------------------------------------------------------ 3-D encoder pieces (BASELINE configs[4]; SPEC_3D.md section 8)
 * No reference counterpart (the reference's input_encoder is Conv2d: smokephys_net.py:24-32).  Conv3d runs as an explicit GEMM on the
 * split-bf16 MFMA linear kernel (smk_linear_forward): these two entry points are the data movement around it.
 * smk_conv3d_im2col: src [D][H][W][C] fp32 (channels-last; C = 1 is the plain volume; C = 1 or a multiple of 4), zero padding ksize/2
 *   (ksize odd), output rows for the planes z0 .. z0+nz-1: cols [nz*H*W][kpad], column tap*C + c with tap = (kz*ksize + ky)*ksize + kx,
 *   columns >= ksize^3 * C zero (kpad >= ksize^3 * C, a multiple of 4; the linear kernel wants a multiple of 64).
 * smk_pool3d_accumulate: act [nz][H][W][C] -> sums [32*32][C] += the sum over the slab's planes and over each token's (H/32) x (W/32)
 *   block (H, W multiples of 32): the two adaptive average pools of smokephys_net.py:87-91 with the depth axis pooled to 1, as sums --
 *   the caller divides by D * (H/32) * (W/32) once. */
int smk_conv3d_im2col(const float *src, int32_t C, int32_t D, int32_t H, int32_t W, int32_t ksize, int32_t z0, int32_t nz, float *cols,
                      int32_t kpad, void *stream);
int smk_pool3d_accumulate(const float *act, int32_t C, int32_t H, int32_t W, int32_t nz, float *sums, void *stream);

/* Stand-alone stateless ops (pure functions of the reference) -------------------------------------- */
/* NavierStokesSimulator.diffusion_step(field, viscosity) (navier_stokes.py:50-72) on [B][R][pitch]. */
int smk_diffuse(const float *in, float *out, int32_t B, int32_t R, int32_t C, int32_t pitch, double dt,
                double viscosity, void *stream);
/* FractalGenerator.apply_fractal_perturbation(field, intensity) (fractal_generator.py:53-62) on n_fields
 * square [N][N] contiguous fields; computes the constant itself (cached per N per device). */
int smk_apply_fractal(const float *in, float *out, int32_t n_fields, int32_t N, double intensity, void *stream);

/* NavierStokesSimulator.advection_step(field, u, v) (navier_stokes.py:74-95) as a pure function on caller buffers:
 * which = 0/1/2 selects the field's shape (u-like [H+1][pitch_c], v-like [H][pitch_v], cell [H][pitch_c]); no decay. */
int smk_advect(const float *field, float *out, int32_t which, const float *u, const float *v, int32_t B, int32_t H,
               int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, void *stream);
/* The adjoint of one step() (navier_stokes.py:151-173) with respect to its state, stage by stage -- no reference counterpart (the reference
 * is differentiated by torch autograd).  The derivative is that of the expressions as written: floor and integer casts have derivative 0,
 * a clamp of a coordinate passes its gradient where lo <= x <= hi (bounds included), dt / viscosity / jacobi_iters are constants.
 * Buffers are fp32 in the layout of smk_advect (batch-major, planes rows * pitch floats apart, pitch_c >= W, pitch_v >= W + 1), caller-owned,
 * 4-byte aligned and no better; no output may alias an input or another output; every element [row][col < columns] of every output is
 * written (the caller need not zero them; the pitch padding is left alone); fp32 sums in one fixed order, no atomics: bit-identical from
 * call to call, a grid's result independent of its batch mates.  All work is enqueued on `stream`, nothing is allocated, no
 * synchronisation.  1 <= B <= 65535, 3 <= H, W <= 32766.
 *
 * smk_advect_backward: out = advection_step(field; u, v) of smk_advect (which = 2: times 0.995, the density stage of step()), gout the
 *   gradient of out (field-shaped) -> dfield (field-shaped), du [H+1][pitch_c], dv [H][pitch_v]; field may be the same buffer as u or v (then
 *   the caller adds dfield to du or dv).  One launch.  The kernel gathers over the 3 x 3 destinations around a source cell, which holds while
 *   every back-trace moves less than one cell (|x - dt u| and |y - dt v| as the forward evaluates them); a grid that breaks this has
 *   far[b] = 1 (int32 [B]; 0 otherwise, every word written) and its three outputs are then unspecified finite-or-not values the caller
 *   must discard.  The other grids are unaffected.
 * smk_project_backward: pressure_projection (navier_stokes.py:133-149) with jacobi_iters >= 0 sweeps, (gu, gv, gp) the gradients of its
 *   results -> (du, dv, dp) those of its inputs.  ceil(jacobi_iters / 4) + 2 launches (four transposed sweeps per launch).  workspace: device memory of at
 *   least smk_project_backward_workspace(B, H, W) bytes (-1 for an unsupported shape), 4-byte aligned, contents unspecified afterwards.
 * smk_buoy_diffuse_backward: buoyancy + the three diffusion_steps (navier_stokes.py:154-160), (gu, gv, gd) the gradients of the diffused
 *   u, v, density -> (du, dv, dd) those of the step's inputs.  One launch. */
int smk_advect_backward(int32_t which, const float *field, const float *u, const float *v, const float *gout, float *dfield, float *du,
                        float *dv, int32_t *far, int32_t B, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, double dt,
                        void *stream);
int64_t smk_project_backward_workspace(int32_t B, int32_t H, int32_t W);
int smk_project_backward(const float *gu, const float *gv, const float *gp, float *du, float *dv, float *dp, int32_t B, int32_t H,
                         int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t jacobi_iters, double dt, void *workspace,
                         int64_t workspace_bytes, void *stream);
int smk_buoy_diffuse_backward(const float *gu, const float *gv, const float *gd, float *du, float *dv, float *dd, int32_t B, int32_t H,
                              int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, double viscosity, void *stream);
/* The tangent-linear (forward-mode) counterpart of the three entry points above: J t beside the step, nothing saved.  Buoyancy, the
 * diffusions and the projection are linear and homogeneous in the state, so their tangent is the stepper's own stage on the tangent state
 * (smk_sim_run_stage on a simulator of B * T grids); only the advection needs a kernel.  Same derivative conventions as the adjoint (floor
 * and integer casts have derivative 0, a clamp of a coordinate passes its tangent where lo <= x <= hi, bounds included, the weights'
 * derivatives are those of the weights as written, formed from the clamped indices, so they cancel on the upper-edge quirk; dt is a
 * constant).  Base buffers are [B] planes in the layout of smk_advect, tangent buffers [B][T] planes in the layout of their base field
 * (tangent t of grid b is plane b * T + t), fp32, caller-owned, 4-byte aligned and no better, pitch_c >= W, pitch_v >= W + 1.  fp32 sums in
 * one fixed order, no atomics, no LDS: bit-identical from call to call, a tangent's result independent of T and of its batch mates.  All
 * work is enqueued on `stream`, nothing is allocated, no synchronisation.  B, T >= 1, B * T <= 65535, 3 <= H, W <= 32766.
 *
 * smk_advect_tangent: out = advection_step(field; u, v) of smk_advect (which = 0 / 1 / 2: field shaped like u / v / a cell field; 2: times
 *   0.995, the density stage of step()); (tfield, tu, tv) the tangents of (field, u, v) -> tout, the tangent of out (field-shaped, [B][T]).
 *   Per destination cell the back-trace, the clamp decisions, the taps (y0,x0), (y0,x1), (y1,x0), (y1,x1) and their weights wa..wd are the
 *   forward's own, bit for bit, formed once; then per tangent, in this order:
 *     r = ((wa tf[y0,x0] + wb tf[y0,x1]) + wc tf[y1,x0]) + wd tf[y1,x1];   r = r + sx * dpx;   r = r + sy * dpy;   (which = 2: r = r * 0.995)
 *     sx = (fy1 - py)(f01 - f00) + (py - fy0)(f11 - f10),  sy = (fx1 - px)(f10 - f00) + (px - fx0)(f11 - f01)   (the interpolant's slopes)
 *     dpx = -(dt * ui') where 0 <= X - dt ui <= columns - 1, else 0;  dpy likewise from Y - dt vi and vi';  ui', vi': the forward's velocity
 *     samples of tu, tv at the fixed sample coordinates (same taps, weights and order as ui, vi).
 *   Every element [row][col < columns] of tout is written (the pitch padding is left alone); tout aliases no input; tfield may be the same
 *   buffer as tu or tv, as field may be u or v.  One launch.  A back-trace may move any number of cells: there is no far case, no far word.
 * smk_tangent_renorm: per grid and tangent, norms[b * T + t] (fp64, 8-byte aligned) = the Euclidean norm of the whole tangent state
 *   (tu [H+1][pitch_c], tv [H][pitch_v], tp, td [H][pitch_c]; four distinct buffers): each element converted to fp64 and squared there, the
 *   squares summed in fp64 in one fixed order (two levels: runs of consecutive rows per workgroup, then the runs in ascending order), no
 *   atomics.  The four fields are then divided in place by (float)norm with a true fp32 divide (the pitch padding is left alone); a norm
 *   that is 0 or not finite (as fp64, or once converted to fp32) leaves that tangent unscaled and is reported as it is.  Two launches.
 *   workspace: device memory of at least smk_tangent_renorm_workspace(B, T, H, W) bytes (-1 for an unsupported shape), 8-byte aligned,
 *   contents unspecified afterwards. */
int smk_advect_tangent(int32_t which, const float *field, const float *u, const float *v, const float *tfield, const float *tu,
                       const float *tv, float *tout, int32_t B, int32_t T, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v,
                       double dt, void *stream);
int64_t smk_tangent_renorm_workspace(int32_t B, int32_t T, int32_t H, int32_t W);
int smk_tangent_renorm(float *tu, float *tv, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t H, int32_t W,
                       int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes, void *stream);
/* The adjoint of one 3-D step() (SPEC_3D.md sections 3-6) with respect to its state (u, v, w, p, density), stage by stage: the 3-D
 * counterpart of the three entry points above, with the same derivative conventions (floor and integer casts have derivative 0, a clamp
 * of a coordinate passes its gradient where lo <= x <= hi, bounds included, dt / viscosity / jacobi_iters are constants; the velocity
 * sample coordinates are index grids, so a sample is linear in its component: 0.5 / 0.5 on c[z][y][x] and its +1 neighbour along the
 * acting axis where every index is <= extent - 2, exactly 0 elsewhere).  Buffers are fp32 in the 3-D stepper's layout (smk_sim3d_desc:
 * batch-major, [planes][rows][pitch], u [D][H+1][pitch_c], v [D][H][pitch_v], w [D+1][H][pitch_c], cell fields [D][H][pitch_c],
 * pitch_c >= W, pitch_v >= W + 1), caller-owned, 4-byte aligned and no better; no output may alias an input or another output; every
 * element [plane][row][col < columns] of every output is written (the caller need not zero them; the pitch padding is left alone); fp32
 * sums in one fixed order, no atomics: bit-identical from call to call, a grid's result independent of its batch mates.  All work is
 * enqueued on `stream`, nothing is allocated, no synchronisation.  Limits: smk_sim3d_create's -- B >= 1, 3 <= D, H, W <= 32766,
 * B * (D + 1) <= 65535, one grid's field below 2^31 elements.
 *
 * smk_advect3d_backward: out = advection_step(field; u, v, w) (which = 0 / 1 / 2 / 3: field shaped like u / v / w / a cell field;
 *   3: times 0.995, the density stage of step()), gout the gradient of out (field-shaped) -> dfield (field-shaped), du, dv, dw; field may
 *   be the same buffer as u, v or w (then the caller adds dfield to du, dv or dw).  One kernel launch.  The kernel gathers over the
 *   3 x 3 x 3 destinations around a source cell, which holds while every back-trace moves less than one cell on every axis (as the
 *   forward evaluates x - dt u, y - dt v, z - dt w); a grid that breaks this has far[b] = 1 (int32 [B]; 0 otherwise, every word written)
 *   and its four outputs are then unspecified finite-or-not values the caller must discard.  The other grids are unaffected.
 * smk_project3d_backward: pressure_projection with jacobi_iters >= 0 sweeps, (gu, gv, gw, gp) the gradients of its results ->
 *   (du, dv, dw, dp) those of its inputs.  ceil(jacobi_iters / 2) + 2 launches (two transposed sweeps per launch).  workspace: device
 *   memory of at least smk_project3d_backward_workspace(B, D, H, W) bytes (-1 for an unsupported shape), 4-byte aligned, contents
 *   unspecified afterwards; a smaller one is refused with SMK_ERR_INVALID and nothing is written.
 * smk_buoy_diffuse3d_backward: buoyancy + the four diffusion_steps, (gu, gv, gw, gd) the gradients of the diffused u, v, w, density ->
 *   (du, dv, dw, dd) those of the step's inputs.  One launch. */
int smk_advect3d_backward(int32_t which, const float *field, const float *u, const float *v, const float *w, const float *gout,
                          float *dfield, float *du, float *dv, float *dw, int32_t *far, int32_t B, int32_t D, int32_t H, int32_t W,
                          int32_t pitch_c, int32_t pitch_v, double dt, void *stream);
int64_t smk_project3d_backward_workspace(int32_t B, int32_t D, int32_t H, int32_t W);
int smk_project3d_backward(const float *gu, const float *gv, const float *gw, const float *gp, float *du, float *dv, float *dw, float *dp,
                           int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t jacobi_iters, double dt,
                           void *workspace, int64_t workspace_bytes, void *stream);
int smk_buoy_diffuse3d_backward(const float *gu, const float *gv, const float *gw, const float *gd, float *du, float *dv, float *dw,
                                float *dd, int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, double dt,
                                double viscosity, void *stream);
/* The tangent-linear (forward-mode) counterpart of the three entry points above: J t beside the 3-D step, nothing saved; the 3-D twin of
 * smk_advect_tangent / smk_tangent_renorm.  Buoyancy, the diffusions and the projection are linear and homogeneous in the state, so their
 * tangent is the stepper's own stage on the tangent state (smk_sim3d_run_stage on a simulator of B * T grids); only the advection needs a
 * kernel.  Same derivative conventions as the adjoint (floor and integer casts have derivative 0, a clamp of a coordinate passes its
 * tangent where lo <= x <= hi, bounds included, the weights' derivatives are those of the weights as written, formed from the clamped
 * indices, so they cancel on the upper-edge quirk; the velocity samples are linear in their component; dt is a constant).  Base buffers
 * are [B] grids in the layout of smk_advect3d_backward, tangent buffers [B][T] grids in the layout of their base field (tangent t of grid
 * b is grid b * T + t), fp32, caller-owned, 4-byte aligned and no better, pitch_c >= W, pitch_v >= W + 1.  fp32 sums in one fixed order,
 * no atomics, no LDS in the advection: bit-identical from call to call, a tangent's result independent of T and of its batch mates.  All
 * work is enqueued on `stream`, nothing is allocated, no synchronisation.  Limits: smk_sim3d_create's at B * T grids -- B, T >= 1,
 * 3 <= D, H, W <= 32766, B * T * (D + 1) <= 65535, one grid's field below 2^31 elements -- for both entry points and the query.
 *
 * smk_advect3d_tangent: out = advection_step(field; u, v, w) (which = 0 / 1 / 2 / 3: field shaped like u / v / w / a cell field; 3: times
 *   0.995, the density stage of step()); (tfield, tu, tv, tw) the tangents of (field, u, v, w) -> tout, the tangent of out (field-shaped,
 *   [B][T]).  Per destination cell (z, y, x) the velocity samples ui, vi, wi (0.5 c[o] + 0.5 c[o + step] where every index is
 *   <= extent - 2, exactly 0 elsewhere), the back-trace px, py, pz before and after its clamp, the clamped tap indices, the six per-axis
 *   weights wx0 = x1 - px, wx1 = px - x0, ... and the field's eight tap values f[zyx] are the forward's own, bit for bit, formed once;
 *   then per tangent, in this order:
 *     r = the forward's eight-term sum over tfield: weights (wx wy) wz, z-low plane first, x fastest, low before high, added left to right;
 *     r = r + sx * dpx;   r = r + sy * dpy;   r = r + sz * dpz;   (which = 3: r = r * 0.995)
 *     sx = (((wy0 wz0)(f001 - f000) + (wy1 wz0)(f011 - f010)) + (wy0 wz1)(f101 - f100)) + (wy1 wz1)(f111 - f110)
 *     sy = (((wx0 wz0)(f010 - f000) + (wx1 wz0)(f011 - f001)) + (wx0 wz1)(f110 - f100)) + (wx1 wz1)(f111 - f101)
 *     sz = (((wx0 wy0)(f100 - f000) + (wx1 wy0)(f101 - f001)) + (wx0 wy1)(f110 - f010)) + (wx1 wy1)(f111 - f011)
 *     dpx = -(dt * ui') where 0 <= x - dt ui <= columns - 1, else 0;  dpy, dpz likewise from y - dt vi, z - dt wi and vi', wi';
 *     ui', vi', wi': the forward's velocity samples of tu, tv, tw (same guard, same two elements, same 0.5 / 0.5).
 *   Every element [plane][row][col < columns] of tout is written (the pitch padding is left alone); tout aliases no input; tfield may be
 *   the same buffer as tu, tv or tw, as field may be u, v or w.  One launch.  A back-trace may move any number of cells: there is no far
 *   case, no far word.
 * smk_tangent3d_renorm: per grid and tangent, norms[b * T + t] (fp64, 8-byte aligned) = the Euclidean norm of the whole tangent state
 *   (tu [D][H+1][pitch_c], tv [D][H][pitch_v], tw [D+1][H][pitch_c], tp, td [D][H][pitch_c]; five distinct buffers): each element
 *   converted to fp64 and squared there, the squares summed in fp64 in one fixed order (two levels: the state's rows -- u's, v's, w's,
 *   p's, the density's, planes before rows -- in runs of consecutive rows per workgroup, a thread's elements in ascending order and the
 *   256 threads folded by halves; then the runs in ascending order), no atomics.  The five fields are then divided in place by
 *   (float)norm with a true fp32 divide (the pitch padding is left alone); a norm that is 0 or not finite (as fp64, or once converted to
 *   fp32) leaves that tangent unscaled and is reported as it is.  Two launches.  workspace: device memory of at least
 *   smk_tangent3d_renorm_workspace(B, T, D, H, W) bytes (-1 for an unsupported shape), 8-byte aligned, contents unspecified afterwards. */
int smk_advect3d_tangent(int32_t which, const float *field, const float *u, const float *v, const float *w, const float *tfield,
                         const float *tu, const float *tv, const float *tw, float *tout, int32_t B, int32_t T, int32_t D, int32_t H,
                         int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, void *stream);
int64_t smk_tangent3d_renorm_workspace(int32_t B, int32_t T, int32_t D, int32_t H, int32_t W);
int smk_tangent3d_renorm(float *tu, float *tv, float *tw, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t D, int32_t H,
                         int32_t W, int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes, void *stream);
/* The T tangent states of every grid orthonormalised in place by modified Gram-Schmidt: what a Lyapunov spectrum (k > 1 exponents) needs
 * where smk_tangent_renorm / smk_tangent3d_renorm serve k = 1.  Buffers are those of the renorm entry points -- [B][T] grids (vector t of
 * grid b is grid b * T + t), fp32, caller-owned, 4-byte aligned and no better, distinct buffers, pitch_c >= W, pitch_v >= W + 1 -- and the
 * state's rows are taken in the renorm entry points' order (2-D: u's, v's, p's, the density's; 3-D: u's, v's, w's, p's, the density's,
 * planes before rows).  Per grid, for j = 0 .. T-1 in turn:
 *   1. n_j = sqrt(sum (double)x (double)x) over the whole state of vector j;  norms[b * T + j] = n_j (fp64, 8-byte aligned);
 *   2. vector j is divided in place by (float)n_j with a true fp32 divide -- unless n_j is 0 or not finite (as fp64, or once converted to
 *      fp32): then it is left unscaled and n_j is reported as it is;
 *   3. for every i > j:  c = sum (double)q (double)x over (vector j after step 2, vector i), then x <- x - (float)c * q in fp32: one rounded
 *      multiply and one rounded subtract.
 * Every sum is fp64 in the renorm entry points' fixed order (two levels: runs of consecutive rows per workgroup, a thread's terms in
 * ascending order and the 256 threads folded by halves; then the runs in ascending order), no atomics: bit-identical from call to call, a
 * grid's result independent of its batch mates; with T = 1, norms and fields are bit-identical to the renorm entry point's, and for any T
 * norms[b * T] and vector 0 are those of the T = 1 call.  A zero vector stays zero, reports norm 0 and leaves the later vectors as they
 * were; a NaN makes the later vectors of its own grid NaN and touches no other grid.  The pitch padding is left alone.  2 T launches (the
 * sum of squares of vector 0; per vector one pass that reports the norm, scales and forms the dot products with the later vectors, and,
 * but for the last, one that updates the later vectors and sums the squares of the next).  All work is enqueued on `stream`, nothing is
 * allocated, no synchronisation.  Limits: the renorm entry point's and T <= 8.  workspace: device memory of at least
 * smk_tangent_orthonormalize_workspace(B, T, H, W) / smk_tangent3d_orthonormalize_workspace(B, T, D, H, W) bytes (-1 for an unsupported
 * shape), 8-byte aligned, contents unspecified afterwards; a smaller one is refused with SMK_ERR_INVALID and nothing is written. */
int64_t smk_tangent_orthonormalize_workspace(int32_t B, int32_t T, int32_t H, int32_t W);
int smk_tangent_orthonormalize(float *tu, float *tv, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t H, int32_t W,
                               int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes, void *stream);
int64_t smk_tangent3d_orthonormalize_workspace(int32_t B, int32_t T, int32_t D, int32_t H, int32_t W);
int smk_tangent3d_orthonormalize(float *tu, float *tv, float *tw, float *tp, float *td, double *norms, int32_t B, int32_t T, int32_t D,
                                 int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, void *workspace, int64_t workspace_bytes,
                                 void *stream);
/* The flow map of the 2-D stepper and its finite-time Lyapunov exponent (FTLE).  A displacement field disp [B][2][H][pitch_m] = (dx, dy) at
 * the cell centres, in cells, stands for the map x -> x + disp; u [B][H+1][pitch_c] and v [B][H][pitch_v] are the layout of smk_advect (a
 * simulator's own stores may be passed as they are).  fp32, caller-owned, 4-byte aligned and no better; 1 <= B <= 65535, 3 <= H, W <=
 * 32766, pitch_c >= W, pitch_v >= W + 1, pitch_m >= W.  fp32 with one rounding per listed operation, no atomics, every element
 * [row][col < W] of an output written, the pitch padding neither read nor written, bit-identical from call to call, a grid independent of
 * its batch mates.  All work is enqueued on `stream`, nothing is allocated, no synchronisation.
 *
 * smk_flow_map_step: one step's first-order trace composed into the map; called after every step() with that step's output velocities (the
 *   ones its density advection sampled).  One launch, one thread per cell (Y, X).  disp_out aliases no input.
 *   direction 0, backward (x + disp: where the particle now at x was when the window began):  su, sv = the density advection's velocity
 *     samples at the cell;  ax = X - dt su,  px = clamp(ax, 0, W - 1);  ix = -(dt su) where 0 <= ax <= W - 1 (bounds included), px - X
 *     otherwise;  dx' = bilinear(dx; py, px) + ix;  y likewise, dy' from bilinear(dy; py, px).  Samples, back-trace, clamp decisions, taps
 *     and weights are the density advection's, bit for bit (floor, clamped indices, weights from the clamped indices: a position on the
 *     last index reads 0).
 *   direction 1, forward (x + disp: where the particle that began at x is now):  qx = clamp(X + dx, 0, W - 1), qy likewise (sample
 *     positions only);  su = interpolate_velocity_u(u, qy, qx), sv = interpolate_velocity_v(v, qy, qx) as smk_interpolate forms them;
 *     dx' = min(max(dx + dt su, -X), W - 1 - X);  y likewise.
 * smk_ftle_field: ftle [B][H][pitch_m] of the map, and stats [B][2] = (mean, max) of each grid's field in fp64 (8-byte aligned).  With
 *   a = dx, b = dy and their differences at unit spacing (central with a factor 0.5 inside, one-sided on the first and last row and column):
 *     exx = a_x + 0.5 (a_x a_x + b_x b_x);  eyy = b_y + 0.5 (a_y a_y + b_y b_y);  exy = 0.5 (a_y + b_x) + 0.5 (a_x a_y + b_x b_y);
 *     m = 0.5 (exx + eyy);  d = 0.5 (exx - eyy);  emax = m + sqrt(d d + exy exy);
 *     ftle = log1p(max(2 emax, lo)) / (float)(2 horizon),  lo = -1 + 2^-24 (the fp32 number next above -1), a true fp32 divide.
 *   horizon > 0: the window's length in time units, n_steps * dt.  The sum is fp64 in smk_tangent_renorm's fixed order (two levels: runs
 *   of consecutive rows per workgroup, a thread's values in ascending order and the 256 threads folded by halves; then the runs in
 *   ascending order by one thread), the maximum alongside (a NaN wins).  Two launches.  workspace: device memory of at least
 *   smk_ftle_workspace(B, H, W) bytes (-1 for an unsupported shape), 8-byte aligned, contents unspecified afterwards; a smaller or
 *   misaligned one is refused with SMK_ERR_INVALID and nothing is written.  ftle does not alias disp. */
int smk_flow_map_step(int32_t direction, const float *u, const float *v, const float *disp_in, float *disp_out, int32_t B, int32_t H,
                      int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t pitch_m, double dt, void *stream);
int64_t smk_ftle_workspace(int32_t B, int32_t H, int32_t W);
int smk_ftle_field(const float *disp, float *ftle, double *stats, int32_t B, int32_t H, int32_t W, int32_t pitch_m, double horizon,
                   void *workspace, int64_t workspace_bytes, void *stream);
/* The flow map of the 3-D stepper and its FTLE: the counterparts of the three entry points above for volumes.  A displacement
 * disp [B][3][D][H][pitch_m] = (dx, dy, dz) at the cell centres, in cells, stands for the map x -> x + disp; component k acts along the
 * axis velocity component k acts along (dx along W, dy along H, dz along D).  u [B][D][H+1][pitch_c], v [B][D][H][pitch_v] and
 * w [B][D+1][H][pitch_c] are the layout of smk_advect3d_tangent (a 3-D simulator's own stores may be passed as they are).  fp32,
 * caller-owned, 4-byte aligned and no better.  Limits: those of smk_advect3d_tangent with T = 1 (B >= 1, 3 <= D, H, W <= 32766,
 * B * (D + 1) <= 65535, pitch_c >= W, pitch_v >= W + 1, (D + 1) * (H + 1) * pitch_c and ... * pitch_v < 2^31), pitch_m >= W and
 * D * H * pitch_m < 2^31.  fp32 with one rounding per listed operation, no atomics, every element [plane][row][col < W] of an output
 * written, the pitch padding neither read nor written, bit-identical from call to call, a grid independent of its batch mates; every
 * index is clamped before use, so no position -- NaN and +-inf included -- reads outside its volume.  All work is enqueued on `stream`,
 * nothing is allocated, no synchronisation.
 *
 * smk_flow_map3d_step: one step's first-order trace composed into the map; called after every step() with that step's output velocities.
 *   One launch, one thread per cell (Z, Y, X).  disp_out aliases no input.
 *   direction 0, backward:  su, sv, sw = the density advection's velocity samples at the cell;  per axis a = X - dt s,
 *     p = clamp(a, 0, n - 1), in the order px, py, pz;  the increment i = -(dt s) where 0 <= a <= n - 1 (bounds included), p - X otherwise;
 *     d' = trilinear(d; pz, py, px) + i for each of dx, dy, dz, at one set of eight taps.  Samples, back-trace, clamp decisions, taps and
 *     weights are the density advection's, bit for bit (floor, clamped indices, weights (wx wy) wz from the clamped indices: a position
 *     on the last index reads 0).
 *   direction 1, forward:  per axis q = clamp(X + d, 0, n - 1) (sample positions only);  s = the component sampled at (qz, qy, qx): +0.5
 *     along the axis it acts on, every coordinate clamped to the component's extent, then the trilinear taps;
 *     d' = min(max(d + dt s, -X), n - 1 - X).
 * smk_ftle3d_field: ftle [B][D][H][pitch_m] of the map, and stats [B][2] = (mean, max) of each grid's field in fp64 (8-byte aligned).
 *   With g[k][j] the difference of component k along axis j (x, y, z) at unit spacing (central with a factor 0.5 inside, one-sided on the
 *   first and last index of each axis):
 *     E_ii = g[i][i] + 0.5 ((g[x][i] g[x][i] + g[y][i] g[y][i]) + g[z][i] g[z][i]);
 *     E_ij = 0.5 (g[i][j] + g[j][i]) + 0.5 ((g[x][i] g[x][j] + g[y][i] g[y][j]) + g[z][i] g[z][j]);
 *     emax = the largest eigenvalue of E by cyclic Jacobi: exactly 4 sweeps of the rotations (x, y), (x, z), (y, z), no early exit; a
 *       rotation (p, q; r the third index):  theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta theta + 1)),
 *       sign(theta) = +1 for theta >= 0;  where a_pq == 0 the divide is by 1 and t = 0;  c = 1 / sqrt(t t + 1), s = t c;
 *       a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0;  a_rp' = c a_rp - s a_rq, a_rq' = s a_rp + c a_rq (correctly rounded divides and square
 *       roots);  emax = the maximum of the three diagonal entries (a NaN wins);
 *     ftle = log1p(max(2 emax, lo)) / (float)(2 horizon),  lo = -1 + 2^-24, a true fp32 divide.
 *   horizon > 0 (and finite as fp32): the window's length in time units.  The sum is fp64 in smk_tangent_renorm's fixed order (two levels:
 *   the grid's D H rows, planes before rows, in runs of at least 16 consecutive rows for at most 256 workgroups, a thread's values in
 *   ascending order and the 256 threads folded by halves; then the runs in ascending order by one thread), the maximum alongside (a NaN
 *   wins).  Two launches.  workspace: device memory of at least smk_ftle3d_workspace(B, D, H, W) bytes (-1 for an unsupported shape),
 *   8-byte aligned, contents unspecified afterwards; a smaller or misaligned one is refused with SMK_ERR_INVALID and nothing is written.
 *   ftle does not alias disp. */
int smk_flow_map3d_step(int32_t direction, const float *u, const float *v, const float *w, const float *disp_in, float *disp_out, int32_t B,
                        int32_t D, int32_t H, int32_t W, int32_t pitch_c, int32_t pitch_v, int32_t pitch_m, double dt, void *stream);
int64_t smk_ftle3d_workspace(int32_t B, int32_t D, int32_t H, int32_t W);
int smk_ftle3d_field(const float *disp, float *ftle, double *stats, int32_t B, int32_t D, int32_t H, int32_t W, int32_t pitch_m,
                     double horizon, void *workspace, int64_t workspace_bytes, void *stream);

/* NavierStokesSimulator.bilinear_interpolate(field, y, x) (navier_stokes.py:111-131; mode 0),
 * .interpolate_velocity_u(u, y, x) (:97-102; mode 1: x + 0.5 clamped to [0, w-1] first) and .interpolate_velocity_v(v, y, x)
 * (:104-109; mode 2: y + 0.5 clamped to [0, h-1] first) as pure gathers: B fields [h][pitch] (field_stride floats apart), n
 * coordinate pairs per field (coord_stride floats apart; 0 = one list shared by all fields), out [B][n].  Coordinates may be any
 * float (floor -> index clamp -> weights from the clamped indices, so a coordinate exactly on the upper edge yields 0). */
int smk_interpolate(int32_t mode, const float *field, int32_t B, int32_t h, int32_t w, int32_t pitch, int64_t field_stride,
                    const float *y, const float *x, int64_t coord_stride, int64_t n, float *out, void *stream);
/* FractalGenerator.generate_perlin_noise / generate_mandelbrot_field (fractal_generator.py:12-51) for an N x N grid:
 * writes [N][N] fp32 each (any pointer may be NULL): perlin, mandelbrot (counts/100), 0.7*perlin+0.3*mandelbrot. */
int smk_fractal_constants(int32_t N, float *perlin, float *mandel, float *field, void *stream);

/* SmokeSimulator.get_chaos_features' reductions (smoke_simulator.py:47-140) for n frames [H][W] (dense rows, frame
 * stride `frame_stride` floats): means [n] fp32 (frame.mean()), box_counts [n][5] int32 (scales 2,4,8,16,32 of
 * frame > mean), hist [n][256] int32 (torch.histogram(bins=256, range=(0,1)) counts). Needs (H/2)*(W/2) <= 65536. */
int smk_chaos_stats(const float *frames, int64_t frame_stride, int32_t n, int32_t H, int32_t W, float *means,
                    int32_t *box_counts, int32_t *hist, void *stream);
/* ||frame[i+1] - frame[i]||_2 for i < n-1 (smoke_simulator.py:73-79) -> norms [n-1] fp32 (fp64 accumulation). */
int smk_frame_diff_norms(const float *frames, int64_t frame_stride, int32_t n, int32_t H, int32_t W, float *norms,
                         void *stream);
/* SmokeSimulator.get_chaos_features' scalar formulas (smoke_simulator.py:67-87, 116-122, 136-140) on the results of the two calls
 * above over one stream of S frames: norms [S-1] (may be NULL when S == 1), box_counts [S][5], hist [S][256] (16-byte aligned).
 * Row k < F names the stream frame pos[k] and the history length hist_len[k] the reference's simulator would hold at that frame
 * (int32 device arrays, never read on the host).  features [F][3] fp64 = (lyapunov, fractal dimension, entropy):
 *   lyapunov = 0 when hist_len < 20, else max(0, mean of the 18 differences of log(norms[pos-19 .. pos-1] + 1e-8));
 *   fractal dimension = |least-squares slope| of log(count + 1) over log(2, 4, 8, 16, 32);
 *   entropy = -sum p log2(p + 1e-8), p = count / total (NaN for an empty histogram, as 0/0 in the reference).
 * All arithmetic in fp64, fixed summation order (bit-reproducible).  A row with pos outside [0, S) gets three NaNs, a row with
 * hist_len >= 20 and pos < 19 a NaN lyapunov; nothing outside the arrays is read.  n_groups > 0 (must divide F): also
 * means [n_groups][3] = the mean of each F / n_groups consecutive rows, added in ascending row order (the per-sample label of
 * data_loader.py:71-88); n_groups == 0: means is not touched and may be NULL.  One launch. */
int smk_chaos_features(const float *norms, const int32_t *box_counts, const int32_t *hist, int32_t S, const int32_t *pos,
                       const int32_t *hist_len, int32_t F, int32_t n_groups, double *features, double *means, void *stream);

/* The reductions of smk_chaos_stats and smk_frame_diff_norms (smoke_simulator.py:47-140) for n volumes [D][H][W] (dense, `vol_stride`
 * floats apart, 64-bit), SPEC_3D.md section 9: means [n] (fp64 sum over all voxels, rounded once), box_counts [n][5] (cubes of edge
 * 2,4,8,16,32 of vol > mean on the (D/s) x (H/s) x (W/s) grid, upper remainders ignored as `h // scale` does at :100-101; a scale with no
 * whole box counts 0), hist [n][256] (torch.histogram(bins=256, range=(0,1)) counts, :134-135) and, unless NULL, norms [n-1] =
 * ||vol[i+1] - vol[i]||_2 (:73-79; fp64 accumulation).  D == 1 is the 2-axis instance (s x s boxes on [H][W]: smk_chaos_stats' rule
 * without its size limit); a 3-D grid has D >= 2.  Any H, W >= 2; D*H*W <= 2^31 - 2^16.  Many workgroups per volume, two launches; all
 * outputs are bit-reproducible (integer adds, and every fp64 sum in one fixed order).  workspace: device memory of at least
 * smk_volume_stats_workspace(n, D, H, W) bytes, 8-byte aligned, passed with its size; nothing is allocated. */
int64_t smk_volume_stats_workspace(int32_t n, int32_t D, int32_t H, int32_t W);
int smk_volume_stats(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, float *means,
                     int32_t *box_counts, int32_t *hist, float *norms, void *workspace, int64_t workspace_bytes, void *stream);

/* Front-view render of n volumes rho [D][H][W] (dense, `vol_stride` floats apart, 64-bit) to images [H][W]: SPEC_3D.md section 10.  No
 * reference counterpart (the reference is 2-D).  The camera looks along +z, plane z = 0 is nearest; single scattering from one
 * directional light:
 *   tau[z,y,x] = sum_{z' < z} rho[z',y,x]
 *   A[z,y,x]   = exclusive prefix of rho along the light's direction of travel:
 *                SMK_LIGHT_POS_Y sum_{y' < y} rho[z,y',x], SMK_LIGHT_NEG_Y sum_{y' > y} rho[z,y',x], SMK_LIGHT_POS_Z tau, SMK_LIGHT_NONE 0
 *   image[y,x]         = gain * sum_z -expm1(-sigma_view rho) * (ambient + (1 - ambient) exp(-sigma_light A)) * exp(-sigma_view tau)
 *   transmittance[y,x] = exp(-sigma_view * sum_z rho[z,y,x])                                   (not written when NULL)
 * z ascending; fp32, every sum in one fixed order, no atomics: results are bit-identical from call to call and the result of a volume
 * does not depend on the others of the batch.  Negative densities follow the formula (no clamp).  The settings are doubles, cast once
 * (1 - ambient is formed in double).  image / transmittance planes are `image_stride` / `trans_stride` floats apart (>= H*W).
 * Limits: 1 <= D <= 64, any H, W >= 1, D*H*W <= 2^31 - 2^16; anything else returns SMK_ERR_UNSUPPORTED.  sigma_view, sigma_light >= 0,
 * 0 <= ambient <= 1, gain > 0 (else SMK_ERR_INVALID).  workspace: device memory of at least smk_volume_render_workspace(n, D, H, W, light)
 * bytes (0 for SMK_LIGHT_NONE / SMK_LIGHT_POS_Z and for H <= 16: NULL is accepted then; -1 for an unsupported shape or light), 4-byte
 * aligned, passed with its size.  Caller-owned memory, the caller's stream, nothing allocated, no synchronisation; SMK_LIGHT_NONE /
 * SMK_LIGHT_POS_Z read the volumes once (one launch), SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y twice (three launches). */
typedef enum smk_light { SMK_LIGHT_NONE = 0, SMK_LIGHT_POS_Y = 1, SMK_LIGHT_NEG_Y = 2, SMK_LIGHT_POS_Z = 3 } smk_light;
typedef struct smk_render_desc {
    double sigma_view, sigma_light;   /* extinction per unit density along the view ray / the light ray */
    double ambient, gain;             /* unshadowed share of the light; scale of the image */
    int32_t light;                    /* smk_light */
} smk_render_desc;
int64_t smk_volume_render_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light);
int smk_volume_render(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, const smk_render_desc *desc,
                      float *image, int64_t image_stride, float *transmittance, int64_t trans_stride, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* The gradient of smk_volume_render: given the upstream gradients G = grad_image and Gt = grad_trans of its two outputs ([H][W] planes
 * `grad_image_stride` / `grad_trans_stride` floats apart; either may be NULL, which means zero; both NULL is SMK_ERR_INVALID), writes
 * d(loss)/d(rho) for the same n volumes into grad_vols (dense [D][H][W] each, `grad_vol_stride` floats apart).  SPEC_3D.md section 10,
 * "Gradient": with T = exp(-sigma_view tau), alpha and L as above, c = alpha L T,
 *   drho[z,y,x] = gain G[y,x] sigma_view (exp(-sigma_view rho) L T - sum_{z' > z} c[z',y,x]) - sigma_view Gt[y,x] transmittance[y,x]
 *                 + the sum of S = gain G alpha T (-sigma_light (1 - ambient) exp(-sigma_light A)) over the voxels this voxel shadows
 *                   (+z: z' > z on the pixel's ray; +y: y' > y, -y: y' < y in the voxel's column of its plane, where G of other rows
 *                   enters; none: nothing).
 * A voxel with rho = 0 has a gradient (sigma_view (gain G - Gt) in an empty volume); negative densities follow the formula.  fp32, one
 * fixed order per sum, no atomics: bit-identical from call to call, independent of the other volumes of the batch, and every element of
 * grad_vols is written exactly once (no need to zero it).  Limits, the checks of desc and the status codes are smk_volume_render's; on
 * any error grad_vols is untouched.  workspace: device memory of at least smk_volume_render_backward_workspace(n, D, H, W, light) bytes
 * (0 for SMK_LIGHT_NONE / SMK_LIGHT_POS_Z: NULL is accepted then; three arrays [n][ceil(H/16)][D][W] and one [n][H][W] of floats for SMK_LIGHT_POS_Y /
 * SMK_LIGHT_NEG_Y, whatever H; -1 for an unsupported shape or light), 4-byte aligned, passed with its size.  Caller-owned memory, the
 * caller's stream, nothing allocated, no synchronisation.  The volumes are read once under SMK_LIGHT_NONE (one launch), twice under
 * SMK_LIGHT_POS_Z (one launch) and three times under SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y (five launches). */
int64_t smk_volume_render_backward_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light);
int smk_volume_render_backward(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W,
                               const smk_render_desc *desc,
                               const float *grad_image, int64_t grad_image_stride,      /* NULL: zero */
                               const float *grad_trans, int64_t grad_trans_stride,      /* NULL: zero */
                               float *grad_vols, int64_t grad_vol_stride,               /* dense [D][H][W] each */
                               void *workspace, int64_t workspace_bytes, void *stream);

/* Orbit views of the same n volumes: an orthographic camera turned about the vertical axis y (SPEC_3D.md section 10, "Orbit views").
 * azimuths: n * n_views doubles in HOST memory, degrees, volume-major (view k of volume v at [v * n_views + k]); positive turns the
 * viewing direction from +z toward +x.  (cos, sin) are formed on the host: r = remainder(azimuth, 360); a multiple of 90 gives exactly
 * (1,0), (0,1), (-1,0) or (0,-1), anything else cos / sin of r * pi / 180 in double; both cast to fp32 once.  Image row y is the volume's
 * row y and the image has the volume's W columns.  With S the smallest integer >= hypot(D, W) of D's parity, c_z = (D-1)/2,
 * c_x = (W-1)/2, a = x' - c_x and t = s - (S-1)/2 for s in [0, S):
 *   x = c_x + (a cos + t sin),  z = c_z + (t cos - a sin)                                                      (fp32, one rounding per operation)
 *   rho_s[s,y,x'] = (1-fz) ((1-fx) v00 + fx v01) + fz ((1-fx) v10 + fx v11), the bilinear interpolation of rho[.,y,.] at (z, x) with
 *                   z0 = floor(z), fz = z - z0, x0 = floor(x), fx = x - x0; a neighbour outside the volume counts as 0
 * and smk_volume_render's rule runs over rho_s with s in the role of z (sample 0 nearest the camera).  A[s,y,x'] is the same
 * interpolation of the voxel-grid prefix along y (equal to the prefix of the samples: the interpolation is linear).  Lights:
 * SMK_LIGHT_NONE, SMK_LIGHT_POS_Y, SMK_LIGHT_NEG_Y; SMK_LIGHT_POS_Z returns SMK_ERR_UNSUPPORTED.  Plane v * n_views + k of image /
 * transmittance (planes `image_stride` / `trans_stride` floats apart, >= H*W; transmittance may be NULL) is view k of volume v.  fp32,
 * every sum in one fixed order, no atomics: bit-identical from call to call, and a plane depends on its own volume and azimuth only.
 * Limits: 1 <= D <= 64, H >= 1, 1 <= W <= 1024, D*H*W <= 2^31 - 2^16 (else SMK_ERR_UNSUPPORTED); n * n_views <= 2^20, finite azimuths
 * and smk_volume_render's checks of desc (else SMK_ERR_INVALID).  workspace: device memory of at least
 * smk_volume_render_orbit_workspace(n, D, H, W, light) bytes (0 for SMK_LIGHT_NONE: NULL is accepted then; n*D*H*W floats, the prefix
 * along y, for SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y; -1 for an unsupported shape or light), 4-byte aligned, passed with its size.
 * Caller-owned memory, the caller's stream, nothing allocated on the device, no synchronisation; on any error the outputs are
 * untouched.  One launch per 16 planes, plus one for the prefix. */
int64_t smk_volume_render_orbit_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light);
int smk_volume_render_orbit(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, const smk_render_desc *desc,
                            const double *azimuths, int32_t n_views, float *image, int64_t image_stride, float *transmittance,
                            int64_t trans_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* The gradient of smk_volume_render_orbit: given the upstream gradients G = grad_image and Gt = grad_trans of its two outputs (plane
 * v * n_views + k is view k of volume v, planes `grad_image_stride` / `grad_trans_stride` floats apart, >= H*W; either may be NULL,
 * which means zero; both NULL is SMK_ERR_INVALID), writes d(loss)/d(rho) of the same n volumes, summed over each volume's n_views views,
 * into grad_vols (dense [D][H][W] each, `grad_vol_stride` floats apart).  SPEC_3D.md section 10, "Orbit views -- Gradient": with rho_s,
 * A the samples of smk_volume_render_orbit, tau their exclusive prefix over s, T = exp(-sigma_view tau), alpha = -expm1(-sigma_view rho_s),
 * X = exp(-sigma_light A), L = ambient + (1 - ambient) X (1 unlit), c = alpha L T,
 *   Q[s,y,x'] = gain G sigma_view (exp(-sigma_view rho_s) L T - sum_{s' > s} c[s',y,x']) - sigma_view Gt transmittance[y,x']
 *   R[s,y,x'] = gain G alpha T (-sigma_light (1 - ambient) X)                                               (0 under SMK_LIGHT_NONE)
 *   drho[z,y,x] = sum over the views of ( (B^T Q)[z,y,x] + the sum of (B^T R)[z,y',x] over the rows y' that y shadows )
 * (+y: y' > y, -y: y' < y), where (B^T F)[z,y,x] = sum over (s, x') of w(s,x'; z,x) F[s,y,x'] and w is the total weight with which voxel
 * (z, x) entered sample (s, x') in the forward (its four taps; a tap outside the volume drops out).  Positions and weights are the
 * forward's, formed by the same fp32 expressions, so this is the transpose of the interpolation the forward used.  A voxel with rho = 0
 * has a gradient; a voxel no ray's taps touch (possible at D > W) gets 0.  fp32, every sum in one fixed order, the views in ascending
 * order, no atomics: bit-identical from call to call, independent of the other volumes of the batch, and every element of grad_vols is
 * written (no need to zero it).  Limits, the checks of desc, the angle rule and the status codes are smk_volume_render_orbit's
 * (SMK_LIGHT_POS_Z: SMK_ERR_UNSUPPORTED); on any error grad_vols is untouched.  workspace: device memory of at least
 * smk_volume_render_orbit_backward_workspace(n, D, H, W, light) bytes, the same for any n_views (-1 for an unsupported shape or light):
 * under SMK_LIGHT_NONE min(n, 16) * H * W floats (one value per ray), under SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y two arrays of n*D*H*W
 * floats (the prefix along y; the sum of B^T R) and min(n, 16) * H rows of (2 S + 1) * W floats of per-sample scratch; either scratch is cut
 * to 256 MiB, and the call then walks the batch in smaller units.  4-byte aligned, passed with its size.  Caller-owned memory, the
 * caller's stream, nothing allocated on the device, no synchronisation.  Launches: two per view and unit (a unit: up to 16 volumes,
 * fewer where the scratch is cut), plus two under SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y. */
int64_t smk_volume_render_orbit_backward_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light);
int smk_volume_render_orbit_backward(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W,
                                     const smk_render_desc *desc, const double *azimuths, int32_t n_views,
                                     const float *grad_image, int64_t grad_image_stride,      /* planes v*n_views+k; NULL: zero */
                                     const float *grad_trans, int64_t grad_trans_stride,      /* NULL: zero; both NULL: SMK_ERR_INVALID */
                                     float *grad_vols, int64_t grad_vol_stride,               /* dense [D][H][W] each */
                                     void *workspace, int64_t workspace_bytes, void *stream);

/* Free-camera views of the same n volumes: the orthographic camera of smk_volume_render_orbit with an elevation as well (SPEC_3D.md
 * section 10, "Free camera").  azimuths, elevations: n * n_views doubles each in HOST memory, degrees, volume-major (view k of volume v
 * at [v * n_views + k]); the azimuth is the orbit's, a positive elevation in [-90, 90] raises the camera toward larger y (it looks down).
 * (c, s) = (cos, sin) of the azimuth by the orbit's rule, cast to fp32 and read back; (ce, se) of the elevation are exactly (1,0), (0,1),
 * (0,-1) at 0, 90, -90 and cos / sin of radians in double otherwise; the coefficients are formed in double and cast to fp32 once:
 *   right r = (c, 0, -s),  up e = (s se, ce, c se) (increasing image row),  view d = (s ce, -se, c ce)            in (x, y, z)
 * The image has the volume's H rows and W columns.  With S the smallest integer >= sqrt(D^2 + H^2 + W^2) of D's parity, c_z = (D-1)/2,
 * c_y = (H-1)/2, c_x = (W-1)/2, a = x' - c_x, b = y' - c_y and t = s - (S-1)/2 for s in [0, S):
 *   x = c_x + ((a r_x + b e_x) + t d_x),  y = c_y + (b e_y + t d_y),  z = c_z + ((a r_z + b e_z) + t d_z)  (fp32, one rounding per operation)
 *   rho_s[s,y',x'] = (1-fz) P(z0) + fz P(z0+1),  P(k) = (1-fy) ((1-fx) v[k,y0,x0] + fx v[k,y0,x0+1]) + fy ((1-fx) v[k,y0+1,x0] + fx v[k,y0+1,x0+1]),
 *                    i0 = floor, f = position - i0 per axis; a tap outside the volume counts as 0
 * and smk_volume_render's rule runs over rho_s with s in the role of z (sample 0 nearest the camera).  A[s,y',x'] is the same
 * interpolation of the voxel-grid exclusive prefix along y (with pitch this is the definition, not a prefix of the samples).  At
 * elevation 0 the samples are the orbit's, on a longer ray: the images agree to the fringe samples the orbit's ray drops, not bit for bit.
 * Lights: SMK_LIGHT_NONE, SMK_LIGHT_POS_Y, SMK_LIGHT_NEG_Y; SMK_LIGHT_POS_Z returns SMK_ERR_UNSUPPORTED.  Plane v * n_views + k of
 * image / transmittance (planes `image_stride` / `trans_stride` floats apart, >= H*W; transmittance may be NULL) is view k of volume v.
 * fp32, every sum in one fixed order, no atomics: bit-identical from call to call, and a plane depends on its own volume, azimuth and
 * elevation only.  Limits: 1 <= D <= 64, 1 <= H <= 65536 (the image row enters the fp32 positions), 1 <= W <= 1024,
 * D*H*W <= 2^31 - 2^16 (else SMK_ERR_UNSUPPORTED); n * n_views <= 2^20, finite angles, |elevation| <= 90 and smk_volume_render's checks
 * of desc (else SMK_ERR_INVALID).  workspace: as smk_volume_render_orbit's, sized by smk_volume_render_camera_workspace(n, D, H, W, light)
 * (0 for SMK_LIGHT_NONE; n*D*H*W floats for SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y; -1 for an unsupported shape or light).  Caller-owned
 * memory, the caller's stream, nothing allocated on the device, no synchronisation; on any error the outputs are untouched.  One launch
 * per 16 planes, plus one for the prefix. */
int64_t smk_volume_render_camera_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light);
int smk_volume_render_camera(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, const smk_render_desc *desc,
                             const double *azimuths, const double *elevations, int32_t n_views, float *image, int64_t image_stride,
                             float *transmittance, int64_t trans_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* The gradient of smk_volume_render_camera, with the promises of smk_volume_render_orbit_backward: given the upstream gradients
 * G = grad_image and Gt = grad_trans of its two outputs (plane v * n_views + k is view k of volume v, planes `grad_image_stride` /
 * `grad_trans_stride` floats apart, >= H*W; either may be NULL, which means zero; both NULL is SMK_ERR_INVALID), writes d(loss)/d(rho)
 * of the same n volumes, summed over each volume's n_views views, into grad_vols (dense [D][H][W] each, `grad_vol_stride` floats
 * apart).  SPEC_3D.md section 10, "Free camera -- Gradient": Q and R are smk_volume_render_orbit_backward's over the samples rho_s, A of
 * smk_volume_render_camera, and
 *   drho[z,y,x] = sum over the views of ( (B^T Q)[z,y,x] + the sum of (B^T R)[z,y'',x] over the voxel rows y'' that y shadows )
 * (+y: y'' > y, -y: y'' < y), where (B^T F)[z,y,x] = sum over (s, y', x') of w(s,y',x'; z,y,x) F[s,y',x'] and w is the total weight with
 * which voxel (z, y, x) entered sample (s, y', x') in the forward (its eight taps; a tap outside the volume drops out).  Positions and
 * weights are the forward's, formed by the same fp32 expressions.  A voxel with rho = 0 has a gradient; a voxel no ray's taps touch
 * gets 0.  fp32, every sum in one fixed order, the views in ascending order, no atomics: bit-identical from call to call, independent
 * of the other volumes of the batch and of how the call is cut into launches, and every element of grad_vols is written (no need to
 * zero it).  Limits: smk_volume_render_camera's and 1 <= H <= 4096 (else SMK_ERR_UNSUPPORTED); the checks of desc, the angle rule and the
 * status codes are smk_volume_render_camera's (SMK_LIGHT_POS_Z: SMK_ERR_UNSUPPORTED); on any error grad_vols is untouched.  workspace:
 * device memory of at least smk_volume_render_camera_backward_workspace(n, D, H, W, light) bytes, the same for any n_views (-1 for an
 * unsupported shape or light).  With row = W floats under SMK_LIGHT_NONE (one value per ray) and (2 S + 1) * W floats under
 * SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y (two per sample and one per ray), fit = floor(2^26 / row) (a cap of 256 MiB), band = min(32, H, fit - 3),
 * slots = min(band + 3, H) and vols = min(n, 16, floor(fit / slots)), it is vols * slots * row floats of scratch, after two arrays of
 * n*D*H*W floats (the prefix along y; the sum of B^T R) under SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y.  4-byte aligned, passed with its size.
 * Caller-owned memory, the caller's stream, nothing allocated on the device, no synchronisation.  Launches: two per view and unit (a
 * unit: up to `vols` volumes x one band of `band` image rows; none for a band that owns no voxel at that view), plus two under
 * SMK_LIGHT_POS_Y / SMK_LIGHT_NEG_Y. */
int64_t smk_volume_render_camera_backward_workspace(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light);
int smk_volume_render_camera_backward(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W,
                                      const smk_render_desc *desc, const double *azimuths, const double *elevations, int32_t n_views,
                                      const float *grad_image, int64_t grad_image_stride,     /* planes v*n_views+k; NULL: zero */
                                      const float *grad_trans, int64_t grad_trans_stride,     /* NULL: zero; both NULL: SMK_ERR_INVALID */
                                      float *grad_vols, int64_t grad_vol_stride,              /* dense [D][H][W] each */
                                      void *workspace, int64_t workspace_bytes, void *stream);

/* RobustnessEvaluator.compute_ssim's SSIM map and F.mse_loss's squared error (robustness_metrics.py:76-103) for n fp32 planes [H][W]
 * (dense rows; plane strides pred_stride / target_stride floats), summed per plane in fp64 in a fixed order (bit-reproducible):
 * ssim_sum [n], sqerr_sum [n].  avg_pool2d(window, stride 1, padding window/2, count_include_pad) with zeros outside the plane;
 * sigma^2 = E[x^2] - mu^2 and sigma_xy = E[xy] - mu_x mu_y in fp32 as the reference computes them; c1, c2 are the stabilisers
 * (0.01^2, 0.03^2 there).  Odd window 1..31, any H, W >= 1, n <= 65535.  workspace: device memory of at least
 * smk_image_quality_workspace(n, H, W) bytes, passed with its size. */
int64_t smk_image_quality_workspace(int32_t n, int32_t H, int32_t W);
int smk_image_quality(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int32_t n, int32_t H,
                      int32_t W, int32_t window, double c1, double c2, void *workspace, int64_t workspace_bytes, double *ssim_sum,
                      double *sqerr_sum, void *stream);

/* The gradient of smk_image_quality's SSIM with respect to pred (DESIGN.md 8.1 "Gradient"): with plane_grad [n] the upstream gradient
 * of each plane's MEAN SSIM (ssim_sum / (H W)), dpred [n][H][W] (dense rows, plane stride dpred_stride floats) receives
 * d(sum_i plane_grad[i] mean_ssim[i]) / d pred.  Same planes, strides, window and stabilisers as the forward; fp32 per pixel, direct
 * k-term sums in a fixed order, no atomics: every element of dpred is written exactly once (no need to zero it), results repeat bit for
 * bit and a plane's result does not depend on the others of its call.  workspace: device memory of at least
 * smk_image_quality_backward_workspace(n, H, W) bytes (3 n H W floats), passed with its size.  No gradient for target. */
int64_t smk_image_quality_backward_workspace(int32_t n, int32_t H, int32_t W);
int smk_image_quality_backward(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int32_t n, int32_t H,
                               int32_t W, int32_t window, double c1, double c2, const float *plane_grad, void *workspace,
                               int64_t workspace_bytes, float *dpred, int64_t dpred_stride, void *stream);

/* ------------------------------------------------------------------ optical-flow baselines
 * The reference's benchmark.py compares the model with cv2.calcOpticalFlowFarneback, cv2.goodFeaturesToTrack +
 * cv2.calcOpticalFlowPyrLK and cv2.remap.  These entry points implement the published algorithms with the reference's call parameters
 * (DESIGN.md "Optical-flow baselines" is the specification; equality with cv2's own output is unmeasured).  Frames are n dense uint8
 * planes [n][H][W], 32 <= H, W <= 1024, n <= 65535; flows are [n][H][W][2] fp32 (dx, dy).  Everything runs on `stream`; scratch is the
 * caller's workspace (256-byte aligned device memory of at least the matching *_workspace bytes, passed with its size); nothing is
 * allocated and the host never waits, so a sequence can be captured into a hipGraph.  Results repeat bit for bit.  A shape outside the
 * limits returns SMK_ERR_INVALID (the workspace queries return 0, the level count 0).
 *
 * Farneback (pyr_scale 0.5, 3 levels, window 15, 3 iterations, poly_n 5, poly_sigma 1.2, flags 0), also stage by stage:
 *   levels K: the largest K <= 3 with min(H, W) * 0.5^(K-1) >= 32; level k has size (round(H 0.5^k), round(W 0.5^k)), half to even
 *   level_image: frames -> out [n][h_k][w_k] fp32 (Gaussian blur of the full frame, then bilinear resize)
 *   poly_exp: img [n][h][w] -> coef [n][5][h][w] = (bx, by, axx, ayy, axy)
 *   farneback_iteration: one matrix update + 15 x 15 box mean + solve; flow [n][h][w][2] is read and overwritten
 * smk_flow_farneback_workspace(n, H, W) serves all four (for a stage call on a level, (n, h, w) of that level is enough). */
int32_t smk_flow_levels(int32_t H, int32_t W);
int64_t smk_flow_farneback_workspace(int32_t n, int32_t H, int32_t W);
int smk_flow_level_image(const uint8_t *frames, int32_t n, int32_t H, int32_t W, int32_t level, float *out, void *workspace,
                         int64_t workspace_bytes, void *stream);
int smk_flow_poly_exp(const float *img, int32_t n, int32_t h, int32_t w, float *coef, void *stream);
int smk_flow_farneback_iteration(const float *coef0, const float *coef1, float *flow, int32_t n, int32_t h, int32_t w, void *workspace,
                                 int64_t workspace_bytes, void *stream);
int smk_flow_farneback(const uint8_t *prev, const uint8_t *next, int32_t n, int32_t H, int32_t W, float *flow, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* predict_next_frame: pred(y, x) = bilinear sample of prev at (x + dx, y + dy), taps outside the image read 0, rounded half to even and
 * saturated to uint8.  With next and mse (both or neither): mse [n] = fp64 mean of (next - pred)^2 on the 0..255 scale (exact integer
 * sums); the workspace is needed only then. */
int64_t smk_warp_workspace(int32_t n, int32_t H, int32_t W);
int smk_warp_frames(const uint8_t *prev, const float *flow, const uint8_t *next, int32_t n, int32_t H, int32_t W, uint8_t *pred,
                    double *mse, void *workspace, int64_t workspace_bytes, void *stream);

/* Lucas-Kanade as the reference builds it: Shi-Tomasi corners (100 corners, quality 0.3, distance 7, block 7), pyramidal tracking
 * (window 15 x 15, maxLevel 2, 30 iterations or |delta| < 0.01), and a flow field that is zero except at the tracked corners.
 *   min_eigen: frames -> eig [n][H][W], the smaller eigenvalue of the 7 x 7 structure tensor of the Sobel derivatives
 *   good_features: eig -> pts [n][100][2] (x, y) in order of selection, counts [n]; unused slots are 0
 *   lk_track: pts, counts -> out_pts [n][100][2], status [n][100] (1 = tracked)
 *   lk_scatter: zeroes flow, then flow[int(y0), int(x0)] = out - pt for every tracked point
 * smk_flow_lk_workspace(n, H, W) serves good_features, lk_track and the whole method. */
int64_t smk_flow_lk_workspace(int32_t n, int32_t H, int32_t W);
int smk_flow_min_eigen(const uint8_t *frames, int32_t n, int32_t H, int32_t W, float *eig, void *stream);
int smk_good_features(const float *eig, int32_t n, int32_t H, int32_t W, float *pts, int32_t *counts, void *workspace,
                      int64_t workspace_bytes, void *stream);
int smk_flow_lk_track(const uint8_t *prev, const uint8_t *next, int32_t n, int32_t H, int32_t W, const float *pts, const int32_t *counts,
                      float *out_pts, uint8_t *status, void *workspace, int64_t workspace_bytes, void *stream);
int smk_flow_lk_scatter(const float *pts, const float *out_pts, const uint8_t *status, const int32_t *counts, int32_t n, int32_t H,
                        int32_t W, float *flow, void *stream);
int smk_flow_lucas_kanade(const uint8_t *prev, const uint8_t *next, int32_t n, int32_t H, int32_t W, float *flow, void *workspace,
                          int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ CNN encoder */
/* SMK_F32: fp32 MFMA; SMK_BF16X3: split-bf16 MFMA (fp32-class accuracy); SMK_BF16: single-pass bf16;
 * SMK_I8X3: 16-bit fixed point as two int8 limbs on int8 MFMA (per-tile activation scale, exact i32 accumulation). */
typedef enum smk_dtype { SMK_F32 = 0, SMK_BF16X3 = 1, SMK_BF16 = 2, SMK_I8X3 = 3 } smk_dtype;

/* Eval-mode input_encoder weights (smokephys_net.py:24-32), device pointers, PyTorch layouts:
 * conv1_w [64][1][7][7], conv2_w [128][64][3][3]; BN as (weight,bias,running_mean,running_var), eps 1e-5. */
typedef struct smk_encoder_weights {
    const float *conv1_w, *conv1_b, *bn1_w, *bn1_b, *bn1_mean, *bn1_var;
    const float *conv2_w, *conv2_b, *bn2_w, *bn2_b, *bn2_mean, *bn2_var;
} smk_encoder_weights;

typedef struct smk_encoder smk_encoder; /* opaque: folded/re-laid-out weights on the device */

int smk_encoder_create(const smk_encoder_weights *w, int32_t device_id, void *stream, smk_encoder **out);
int smk_encoder_destroy(smk_encoder *enc);

/* SmokePhysNet.input_encoder + both adaptive pools (smokephys_net.py:87-91):
 * frames [B][H][W] fp32 (row pitch W, frame stride frame_stride floats) -> features [B][128][32][32] fp32.
 * Requires H == W in {64, 128, 256, 512, 1024}, and input_dim a multiple of 32 that is a multiple/divisor of H (then the two pools
 * compose to an (H/32)^2 block mean); anything else returns SMK_ERR_UNSUPPORTED.
 * Frames of 512 and 1024 (every dtype, both layouts): a pooled cell spans 2 / 8 of the kernels' 8 x 16 tiles, so the main kernel
 * writes per-tile partial sums into a buffer the handle owns ([B][H/8][W/16][128] fp32: 1 MB per 512^2 frame, 4 MB per 1024^2 frame)
 * and one more small launch adds a cell's partials in a fixed order and stores the features.  The buffer is grown on demand and never
 * inside a stream capture: a capture that finds it missing or too small returns SMK_ERR_UNSUPPORTED with a message that says so -- run
 * one eager forward of the same shape first.  Like the tile-skip workspace below it is shared by the calls on one handle.
 * Tile skip (SMK_BF16X3, SMK_BF16, SMK_I8X3; both smk_encoder_forward and smk_encoder_forward_tokens): when a call has more 8 x 16
 * tiles than the device runs workgroups, a scan launch first finds the tiles whose 16 x 24 input window is all-zero words and leaves
 * one bit per tile; the main kernel's workgroups derive their tiles from those bits themselves and copy the features of the empty
 * tiles from the handle's zero-response table (the same kernel's output for an all-zero frame: bit-identical to computing them).
 * Two launches per call; dense input keeps the cost of the scan (about 0.5 %); SMK_ENC_SKIP=0
 * (read once per process) runs every tile.  At 256^2 under SMK_BF16X3 the decision is per pooled cell: a tile is two 8 x 8 cells with
 * a 16 x 16 window each, and a tile with one all-zero window computes the other cell only (same bits; SMK_ENC_CELLS=0, read once per
 * process, keeps whole tiles; smk_encoder_skip_stats counts tiles either way).  Table and workspace live in the handle, are built on the first eligible call outside
 * stream capture, and are reused by every later call: CALLS ON ONE HANDLE MUST BE STREAM-ORDERED (one stream, or ordered by events);
 * two forwards of one handle running concurrently on different streams would share the tile bits.  Nothing in the forward copies
 * to the host or synchronises, and every launch can be captured into a graph. */
int smk_encoder_forward(smk_encoder *enc, const float *frames, int64_t frame_stride, int32_t B, int32_t H,
                        int32_t W, int32_t input_dim, float *features, int32_t dtype, void *stream);

/* Same computation, features written token-major: [B][32*32 tokens][128 channels] fp32 -- the layout
 * `encoded.flatten(2).transpose(1, 2)` (smokephys_net.py:95) hands to feature_proj; coalesced stores. bf16 dtypes only. */
int smk_encoder_forward_tokens(smk_encoder *enc, const float *frames, int64_t frame_stride, int32_t B, int32_t H,
                               int32_t W, int32_t input_dim, float *tokens, int32_t dtype, void *stream);

/* Tile counts of the handle's LAST forward, for tests and profiles: synchronises `stream`, then tiles_total = B * (H/8) * (W/16) and
 * tiles_run = the tiles the main kernel computed (== tiles_total after a call that ran without the tile skip). */
int smk_encoder_skip_stats(smk_encoder *enc, int64_t *tiles_total, int64_t *tiles_run, void *stream);

/* conv1+BN+ReLU activations only (smokephys_net.py:25-27), [B][64][H][W] fp32 -- parity hook. */
int smk_encoder_conv1(smk_encoder *enc, const float *frames, int64_t frame_stride, int32_t B, int32_t H,
                      int32_t W, float *act, void *stream);

/* ------------------------------------------------------------------ transformer-body linear layers */
/* One nn.Linear of SmokePhysNet's token path -- feature_proj (smokephys_net.py:38,97), q/k/v/out projections
 * (chaos_attention.py:25-28,77-79,113), FFN (smokephys_net.py:153-158), output_decoder (smokephys_net.py:50-54) --
 * with its weights re-laid-out on the device for the split-bf16 MFMA kernel (fp32-class accuracy: results within
 * 1e-4 relative of the fp32 GEMM the reference runs; measured ~1e-6).
 * weight [out_features][in_features] fp32 (PyTorch layout), bias [out_features] or NULL; both are read once, on `stream`.
 * Requires in_features % 64 == 0 and out_features % 32 == 0 (else SMK_ERR_UNSUPPORTED). */
/* Activation formats between the body kernels.  SMK_FMT_SPLIT_BF16 keeps an fp32-accurate activation as two bf16 per
 * element (x = hi + lo) in the layout the MFMA kernels consume: per row, per group of 8 consecutive features, 8 hi then
 * 8 lo ([rows][features/8][2][8] bf16 -- the same 4 bytes per element as fp32, rows dense).  A producer that writes it
 * (LayerNorm, a linear layer's epilogue, the attention kernel) saves the consuming linear layer the split arithmetic in
 * its K loop.
 * SMK_FMT_SPLIT4_INPLACE (round 4) is the same pair of bf16 per element laid into the fp32 tensor's own storage: every aligned group
 * of 4 consecutive features holds {hi[0..3], lo[0..3]} in the 16 bytes of its 4 floats (any row pitch, any column range of a row).  The
 * fused q | k | v layer writes its k and v columns that way (smk_linear_forward_ln_split) and the attention kernel stages them without
 * split arithmetic (smk_attention_kv): the split is done once per element instead of once per 128-query block. */
typedef enum smk_format { SMK_FMT_F32 = 0, SMK_FMT_SPLIT_BF16 = 1, SMK_FMT_SPLIT4_INPLACE = 2 } smk_format;

typedef struct smk_linear smk_linear;
typedef enum smk_activation { SMK_ACT_NONE = 0, SMK_ACT_GELU = 1 /* erf form, nn.GELU() */, SMK_ACT_RELU = 2 } smk_activation;

int smk_linear_create(const float *weight, const float *bias, int32_t out_features, int32_t in_features,
                      int32_t device_id, void *stream, smk_linear **out);
int smk_linear_destroy(smk_linear *lin);

/* Re-split new weights into an existing handle (training: the parameters change at every optimizer step, train.py:88-93; no
 * allocation).  transposed = 0: weight is [out_features][in_features] as in smk_linear_create.  transposed = 1: weight is
 * [in_features][out_features] row-major, i.e. the handle computes x W for a PyTorch weight W whose shape is
 * [in_features][out_features] -- the input-gradient GEMM dX = dY W of nn.Linear's backward (autograd's LinearBackward0) on the
 * same kernel.  bias NULL = zeros.  Read once, on `stream`. */
int smk_linear_update(smk_linear *lin, const float *weight, int32_t transposed, const float *bias, void *stream);

/* Weight gradient of nn.Linear, dW [out_features][in_features] = dY^T X (autograd's LinearBackward0; train.py:89 `total.backward()`),
 * on the same split-bf16 kernel: dy [rows][out_features] (row pitch ld_dy floats), x [rows][in_features] (row pitch ldx), dw dense.
 * The reduction runs over the token rows, cut into segments that share one launch; the partial sums are added in segment order
 * (deterministic).  `workspace`: smk_linear_wgrad_workspace(rows, out, in) bytes of device memory, 16-byte aligned, owned by the
 * caller and free for reuse once the enqueued work has run.  Requires in_features % 32 == 0, out_features % 4 == 0,
 * (out_features + 256) * (rows + 4096) < 2^30 (longer inputs: call per row chunk and add).  db (may be NULL): the bias gradient
 * [out_features] = column sums of dy (partials per row segment, added in a fixed order).  With out_features and in_features multiples of 128
 * neither operand is copied: both are staged as they lie and read back transposed from LDS (ds_read_b64_tr_b16) -- that form also needs
 * rows >= 32, ld_dy and ldx multiples of 4 and dy and x 16-byte aligned; a call that misses one of these runs the copying form, which
 * takes any 4-byte aligned dy and x and any pitch.  Each form repeats bit for bit; the two agree to rounding (4e-6 of the largest
 * element at 512 x 128 x 128), not bit for bit, so a caller that compares runs keeps pitch and alignment fixed.  Enqueued on `stream`. */
int64_t smk_linear_wgrad_workspace(int64_t rows, int32_t out_features, int32_t in_features);
int smk_linear_wgrad(const float *dy, int64_t ld_dy, const float *x, int64_t ldx, int64_t rows, int32_t out_features,
                     int32_t in_features, float *dw, float *db, void *workspace, int64_t workspace_bytes, void *stream);

/* y = act(x W^T + b + addend) + residual over `rows` token rows:
 *   x [rows][in_features], row pitch ldx floats; y [rows][out_features], row pitch ldy (all row starts 16-byte aligned);
 *   residual (or NULL) [rows][out_features], row pitch ldr -- the `x + sublayer(x)` of the pre-LN block
 *   (smokephys_net.py:161-167); may alias y;
 *   periodic_add (or NULL) [rows / rows_per_group][period][out_features]: row i of group g receives
 *   periodic_add[g][(i % rows_per_group) % period] before the activation -- the chaos term folded into Q
 *   (the 5-step Lorenz field tiled along the sequence, chaos_attention.py:61-65,85-100); rows_per_group % 32 == 0.
 *   residual and periodic_add are mutually exclusive (no layer of the path uses both).
 *   x_format / y_format: smk_format of x and y (void pointers: fp32 or split-bf16 storage); a split tensor has dense rows
 *   (ldx == in_features, ldy == out_features); a split y excludes residual.
 * Enqueued on `stream`, no synchronisation. */
int smk_linear_forward(smk_linear *lin, const void *x, int64_t rows, int64_t ldx, void *y, int64_t ldy,
                       const float *residual, int64_t ldr, const float *periodic_add, int32_t rows_per_group,
                       int32_t period, int32_t activation, int32_t x_format, int32_t y_format, void *stream);

/* LayerNorm fused in front of the layer (nn.LayerNorm -> nn.Linear of the pre-LN block, /root/reference/src/models/smokephys_net.py:149-150,
 * 161,165): y = act(LN(x) W^T + b + periodic_add), LN over the in_features of a row with `eps`.  `lin` must have been created from the
 * FOLDED parameters W' = W diag(gamma), b' = b + W beta; wsum [out_features] = row sums of W'.  The kernel reads the raw x, gathers each
 * row's mean / variance while staging it (shifted sums about a per-thread pivot merged pairwise: no cancellation for rows whose mean
 * dwarfs their spread) and applies rstd (x W'^T - mean wsum) + b' in its epilogue: the separate LayerNorm launch and its round trip are
 * gone.  Any row count (round 3 served one tile per workgroup only; smk_linear_ln_max_rows now only reflects the 32-bit offset range).
 * fp32 in / out; no residual. */
int64_t smk_linear_ln_max_rows(smk_linear *lin);
int smk_linear_forward_ln(smk_linear *lin, const float *x, int64_t rows, int64_t ldx, float *y, int64_t ldy, const float *wsum, double eps,
                          const float *periodic_add, int32_t rows_per_group, int32_t period, int32_t activation, void *stream);
/* The same launch with the output columns >= split_from_col (a multiple of 32, below out_features; negative: none) written as
 * SMK_FMT_SPLIT4_INPLACE instead of fp32 -- the k | v columns of the fused q | k | v projection (smokephys_net.py:161,
 * chaos_attention.py:77-79), consumed by smk_attention_kv. */
int smk_linear_forward_ln_split(smk_linear *lin, const float *x, int64_t rows, int64_t ldx, float *y, int64_t ldy, const float *wsum, double eps,
                                const float *periodic_add, int32_t rows_per_group, int32_t period, int32_t activation, int32_t split_from_col,
                                void *stream);

/* Conv3d(64 -> N, kernel 3, padding 1) + bias + activation as an IMPLICIT GEMM on the split-bf16 MFMA layer kernel -- no patch matrix:
 * src [D][H][W][64] fp32 channels-last, `lin` a layer handle with in_features = 27 * 64 whose weight columns are tap * 64 + c
 * (tap = (kz*3 + ky)*3 + kx, i.e. conv.weight.permute(0, 2, 3, 4, 1).reshape(N, 1728)); output rows = the voxels of planes z0 .. z0+nz-1
 * in memory order, y [nz*H*W][ldy].  One call addresses the planes it reads with 32-bit offsets: (nz + 2) * H * W * 256 < 2^32. */
int smk_conv3d_cl_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t nz, float *y, int64_t ldy,
                          int32_t activation, void *stream);
/* Conv3d(1 -> N, kernel 7, padding 3) + bias + activation of a SCALAR volume src [D][H][W] as an implicit GEMM on the same kernel (SPEC_3D.md
 * section 8, conv1): `lin` has in_features = 448 = 56 window rows x 8 kx slots, weight column (kz*7 + ky)*8 + kx (slot kx = 7 and window rows
 * >= 49 zero); output rows = the voxels of planes z0 .. z0+nz-1, y [nz*H*W][ldy].  H, W <= 1023; (nz + 6) * H * W * 4 < 2^32. */
int smk_conv3d_s7_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t nz, float *y, int64_t ldy,
                          int32_t activation, void *stream);
/* The same Conv3d(64 -> 128, kernel 3, padding 1) + bias + activation (SMK_ACT_NONE or SMK_ACT_RELU) of a whole volume, fused with the DEPTH
 * half of the token pooling (SPEC_3D.md section 8 pools the depth axis to 1): zsum [H][W][128] = sum over z of act(conv(src)[z] + bias), planes
 * added in z order (deterministic).  A workgroup marches an 8 x 16 column of voxels along z with three planes of its halo tile in LDS, so
 * every voxel is staged once per plane instead of once per tap, and the activated convolution output is never written; follow with
 * smk_pool3d_accumulate(zsum, 128, H, W, 1, sums).  `lin` as for smk_conv3d_cl_forward with out_features = 128; H % 8 == 0, W % 16 == 0,
 * H * W * 256 < 2^31. */
int smk_conv3d_cl_zsum_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, float *zsum, int32_t activation, void *stream);
/* Conv3d(1 -> 64, kernel 7, padding 3) + bias + activation (SMK_ACT_NONE or SMK_ACT_RELU) of a whole scalar volume src [D][H][W] into the
 * channels-last activations a1 [D][H][W][64], marched along z: the weights stay in registers, each input plane of a workgroup's 14 x 22 halo
 * tile is expanded once into a table of ready MFMA fragments in LDS (no gather and no split arithmetic in the loop).  `lin`: in_features =
 * 448 = 7 kz x 8 ky slots x 8 kx slots, weight column (kz*8 + ky)*8 + kx (slot 7 of ky and of kx zero), out_features = 64.
 * H % 8 == 0, W % 16 == 0, H * W * 256 < 2^31. */
int smk_conv3d_s7_march_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, float *a1, int32_t activation, void *stream);

/* ------------------------------------------------------------------ training passes of the 3-D encoder (SPEC_3D.md section 11)
 * All activations channels-last: volume [B][D][H][W], a1 / z1 / da1 [B][D][H][W][64], z2 / dz2 [B][D][H][W][128], fp32, 16-byte aligned.
 * Weights in torch's layout: conv1 [64][1][7][7][7], conv2 [128][64][3][3][3]; they are re-laid on the device in the same call, so an
 * optimizer step needs no other notification.  H % 8 == 0 and W % 16 == 0 (a workgroup's tile is 8 x 16 voxels of one plane), B, D >= 1;
 * anything else is SMK_ERR_UNSUPPORTED.  Every pass runs on the exact fp32-input MFMA with fp32 accumulation; every reduction has a fixed
 * order and there are no atomics, so a repeated call is bit-identical.  Enqueued on `stream`.
 *   smk_conv3d_s7_train_forward  z1 = conv1(volume) + bias (bias may be NULL), raw: no activation.
 *   smk_conv3d_cl_train_forward  z2 = conv2(a1) + bias, raw.
 *   smk_conv3d_cl_dgrad          da1 = the data gradient of conv2 from dz2 (the 3 x 3 x 3 convolution 128 -> 64 with the flipped kernel).
 *   smk_conv3d_cl_wgrad          dw [128][64][3][3][3] and db [128] (may be NULL) from dz2 and a1, implicit (no patch matrix): the voxels are
 *                                the MFMA k dimension, a workgroup owns 32 output channels x one kz slice and one voxel stream, the streams'
 *                                partials are added in stream order.
 *   smk_conv3d_s7_dgrad          dvol [B][D][H][W] = the data gradient of conv1 from dz1 [B][D][H][W][64]:
 *                                dvol[z][y][x] = sum over c, kz, ky, kx of dz1[z+3-kz][y+3-ky][x+3-kx][c] w[c][0][kz][ky][kx], out-of-volume
 *                                terms zero (F.conv_transpose3d with padding 3).  A sample's result does not depend on its batch mates.
 * `workspace`: smk_conv3d_train_workspace() bytes for all but the weight gradient (their own contents: do not share one buffer between calls that may
 * overlap), smk_conv3d_cl_wgrad_workspace(B, D, H, W) bytes (negative: unsupported shape) for the weight gradient; caller-owned device memory. */
int64_t smk_conv3d_train_workspace(void);
int64_t smk_conv3d_cl_wgrad_workspace(int32_t B, int32_t D, int32_t H, int32_t W);
int smk_conv3d_s7_train_forward(const float *volume, const float *weight, const float *bias, int32_t B, int32_t D, int32_t H, int32_t W, float *z1,
                                void *workspace, void *stream);
int smk_conv3d_cl_train_forward(const float *a1, const float *weight, const float *bias, int32_t B, int32_t D, int32_t H, int32_t W, float *z2,
                                void *workspace, void *stream);
int smk_conv3d_cl_dgrad(const float *dz2, const float *weight, int32_t B, int32_t D, int32_t H, int32_t W, float *da1, void *workspace, void *stream);
int smk_conv3d_cl_wgrad(const float *dz2, const float *a1, int32_t B, int32_t D, int32_t H, int32_t W, float *dw, float *db, void *workspace,
                        void *stream);
int smk_conv3d_s7_dgrad(const float *dz1, const float *weight, int32_t B, int32_t D, int32_t H, int32_t W, float *dvol, void *workspace, void *stream);
/* Train-mode BatchNorm3d + ReLU on a channels-last matrix z [B*D*H*W][C], C = 64 or 128, in the four phases of smk_bn_relu_pool_phase
 * (enum smk_bn_phase; unused pointers may be NULL):
 *   SMK_BN_STATS     z -> mean / var (biased) / rstd [C] (the caller updates the running statistics from them);
 *   SMK_BN_APPLY     pooled = 0: out [B*D*H*W][C] = relu(bn(z)).  pooled = 1 (H, W multiples of 32): out [B][1024][C] = the token SUMS of
 *                    relu(bn(z)) over D x (H/32) x (W/32) -- the caller divides by that block size once; the activation is not written;
 *   SMK_BN_BWD_SUMS  dout, z -> dgamma = sum dy zhat, dbeta = sum dy; the ReLU mask is recomputed from z.  pooled = 0: dout [B*D*H*W][C];
 *                    pooled = 1: dout [B][1024][C] is the gradient of the token MEANS, broadcast over each block and divided by its size;
 *   SMK_BN_BWD_DZ    dz [B*D*H*W][C] from the given dgamma / dbeta and count = elements per channel.
 * Sums are fp64, two-stage, in a fixed order.  `workspace` (SMK_BN_STATS and SMK_BN_BWD_SUMS; the other phases take none): smk_bn_cl_workspace(B, D, H, W, C)
 * bytes, 8-byte aligned (it holds the fp64 partial sums; else SMK_ERR_INVALID).  z, out, dout and dz are 16-byte aligned. */
int64_t smk_bn_cl_workspace(int32_t B, int32_t D, int32_t H, int32_t W, int32_t C);
int smk_bn_cl_phase(int32_t phase, const float *z, const float *dout, int32_t B, int32_t D, int32_t H, int32_t W, int32_t C, int32_t pooled,
                    const float *gamma, const float *beta, double eps, float *mean, float *var, float *rstd, float *out, float *dz, float *dgamma,
                    float *dbeta, double count, void *workspace, void *stream);

/* smk_chaos_addend for up to 8 layers in ONE launch (a model's layers draw their noise up front; six launches of one workgroup per batch
 * element are six launch latencies at batch 1).  Each layer: its own noise [3][B], weights, output and strength; B, D and the Lorenz constants
 * are shared. */
typedef struct smk_chaos_layer {
    const float *noise, *proj_w, *proj_b, *gate_w, *gate_b;
    float *addend;
    int64_t ld_addend;
    double strength;
} smk_chaos_layer;
int smk_chaos_addend_batched(int32_t n_layers, const smk_chaos_layer *layers, int32_t B, int32_t D, double sigma, double rho, double beta,
                             double dt, void *stream);

/* SmokePhysNet's tail (smokephys_net.py:116-118): pooled [B][D] = features.mean(dim=1) of x [B][L][ldx] and out [B][H2] =
 * Linear2(ReLU(Linear1(pooled))) with w1 [H1][D], w2 [H2][H1] (row-major, nn.Linear layout), in three small launches instead of PyTorch-ROCm's
 * seven (reduce, two GEMM calls with their bias copies, ReLU, fill).  workspace: B * (32 * D + H1) floats.  fp32, fixed summation order. */
int smk_pooled_head(const float *x, int32_t B, int32_t L, int32_t D, int64_t ldx, const float *w1, const float *b1, int32_t H1,
                    const float *w2, const float *b2, int32_t H2, float *pooled, float *out, float *workspace, void *stream);

/* ChaosAttention.generate_chaos_field's five explicit-Euler Lorenz states (chaos_attention.py:39-59) for noise [3][B] (the three
 * randn(B,1) draws before the 0.1 scale): states [B][5][3].  The gradient-free part of the chaos term, for the training path. */
int smk_lorenz_states(const float *noise, int32_t B, double sigma, double rho, double beta, double dt, float *states, void *stream);

/* The element-wise chain of ChaosTransformerLayer's FFN under autograd (smokephys_net.py:153-159 Linear -> GELU -> Dropout -> Linear ->
 * Dropout, :165-167 x = x + ffn(norm2(x)); train.py:88-89) as one read + one write per tensor, n contiguous fp32 elements (n % 4 == 0):
 *   SMK_ELT_GELU_DROPOUT_FWD   out = dropout_p(gelu(a))                      a = the first Linear's output h
 *   SMK_ELT_GELU_DROPOUT_BWD   out = b * mask / (1 - p) * gelu'(a)           a = h, b = gradient of the dropout's output
 *   SMK_ELT_DROPOUT_ADD_FWD    out = b + dropout_p(a)                        a = the second Linear's output, b = the residual stream
 *   SMK_ELT_DROPOUT_BWD        out = a * mask / (1 - p)                      a = gradient of the sum (the residual's gradient is a itself)
 * GELU is the exact-erf form (nn.GELU() default).  The keep mask of element i is a pure function of (seed, i): the backward call
 * passes the forward's seed and p and no mask tensor exists (p is applied in units of 2^-16; p = 0 keeps every element). */
enum smk_elt_op { SMK_ELT_GELU_DROPOUT_FWD = 0, SMK_ELT_GELU_DROPOUT_BWD = 1, SMK_ELT_DROPOUT_ADD_FWD = 2, SMK_ELT_DROPOUT_BWD = 3 };
int smk_ffn_elementwise(int32_t op, const float *a, const float *b, float *out, int64_t n, double p, uint64_t seed, void *stream);

/* The owner's pass of the direct gradient exchange (hooks in where the reference steps the optimiser,
 * /root/reference/train.py:88-93 -- the reference itself is single-process and has no exchange): rank r holds `world` shards of n
 * gradients each (its own and the ones the all-to-all brought in, `stride` elements apart) and forms their MEAN: the sum in rank
 * order in fp32 (the same order on every rank, element and run: deterministic), a true divide by `world`, written as fp32 or bf16.
 * dtype: SMK_WIRE_F32 / SMK_WIRE_BF16 for input and output independently (world = 1 makes it the converter of the bf16 wire mode).
 * In place (out == shards) is allowed when the dtypes agree.  fp32 operands 16-byte aligned, bf16 operands 8-byte aligned, stride a
 * multiple of 4.  Enqueued on `stream`. */
enum smk_wire_dtype { SMK_WIRE_F32 = 0, SMK_WIRE_BF16 = 1 };
int smk_reduce_shards(const void *shards, int32_t in_dtype, int32_t world, int64_t n, int64_t stride, void *out, int32_t out_dtype, void *stream);

/* Training-mode BatchNorm2d (batch statistics) + ReLU + pool x pool mean pooling of an NCHW fp32 convolution output -- the
 * norm / activation / pool blocks of SmokePhysNet.input_encoder under autograd (smokephys_net.py:24-32 Conv -> BatchNorm2d -> ReLU,
 * :87-91 the two adaptive average pools as one block mean; train.py:88-89).
 *   forward:  z [B][C][H][W], gamma / beta [C], eps -> out [B][C][H/pool][W/pool] = blockmean(relu(bn(z))), and the batch
 *             statistics mean / var (biased) / rstd [C] (the caller updates running_mean / running_var from them);
 *   backward: dout [B][C][H/pool][W/pool] -> dz [B][C][H][W], dgamma / dbeta [C]; the ReLU mask is recomputed from z.
 * pool in {1, 2, 4, 8, 16, 32} (frames of 64 .. 1024 pooled to 32 x 32); H * W a whole number of chunks -- 4,096 floats at pool 1, 2 and
 * 4, 16,384 at pool 8, 8,192 at pool 16 and 32,768 at pool 32 (one row of cells) -- and pool > 1 needs W == 32 * pool; anything else is
 * SMK_ERR_UNSUPPORTED.  `workspace`: smk_bn_train_workspace(B, C, H, W, pool) bytes of device memory (one pair of partial sums per chunk
 * and channel), caller-owned.  Reductions are two-stage in a fixed order (deterministic; at pool 16 and 32 a cell's lanes are added by a
 * fixed butterfly).  Enqueued on `stream`. */
int64_t smk_bn_train_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int32_t pool);
int smk_bn_relu_pool_forward(const float *z, int32_t B, int32_t C, int32_t H, int32_t W, const float *gamma, const float *beta,
                             double eps, int32_t pool, float *out, float *mean, float *var, float *rstd, void *workspace,
                             void *stream);
int smk_bn_relu_pool_backward(const float *z, const float *dout, int32_t B, int32_t C, int32_t H, int32_t W, const float *gamma,
                              const float *beta, const float *mean, const float *rstd, int32_t pool, float *dz, float *dgamma,
                              float *dbeta, void *workspace, void *stream);

/* The encoder's first convolution for training: Conv2d(1, 64, 7, padding = 3) under autograd (smokephys_net.py:25; train.py:88-89), plain
 * fp32 on the vector ALUs (its output feeds train-mode BatchNorm + ReLU: as exact as an fp32 convolution has to be).
 *   forward: x [B][H][W] (the single input channel), weight [64][7][7], bias [64] or NULL -> z1 [B][64][H][W]; W % 4 == 0;
 *   wgrad:   dz [B][64][H][W], x -> dW [64][7][7] and db [64] (unless NULL); H % 4 == 0, W % 64 == 0; per-workgroup partial sums added
 *            in a fixed order (deterministic); `workspace`: smk_conv1_train_wgrad_workspace() bytes.
 *   dgrad:   dz [B][64][H][W], weight -> dx [B][H][W] = sum over c and taps of dz[b][c][i+3-ki][j+3-kj] * w[c][ki][kj] (zeros outside the
 *            plane), for a caller that differentiates with respect to the frames (train.py's carry no gradient; PGD and saliency do):
 *            1 <= B <= 65535, H >= 1, W % 4 == 0, dz / dx 16-byte aligned; no atomics and no workspace, every dx element is written
 *            exactly once (deterministic). */
int smk_conv1_train_forward(const float *x, const float *weight, const float *bias, int32_t B, int32_t H, int32_t W, float *z1, void *stream);
int64_t smk_conv1_train_wgrad_workspace(void);
int smk_conv1_train_wgrad(const float *dz, const float *x, int32_t B, int32_t H, int32_t W, float *dw, float *db, void *workspace, void *stream);
int smk_conv1_train_dgrad(const float *dz, const float *weight, int32_t B, int32_t H, int32_t W, float *dx, void *stream);

/* The encoder's second convolution alone, for training: z2 = Conv2d(64, 128, 3, padding = 1)(a1) + bias under autograd
 * (smokephys_net.py:28; train.py:88-89 -- train-mode BatchNorm needs the whole convolution output before it can normalise, so the
 * fused eval encoder does not apply).  a1 [B][64][H][W] and z2 [B][128][H][W] NCHW fp32, weight [128][64][3][3], bias [128] or NULL;
 * H % 8 == 0, W % 16 == 0.  Split-bf16 on the bf16 matrix cores with fp32 accumulation: three bf16 terms per operand, six products
 * (within 2e-6 of an fp64 convolution -- the output feeds BatchNorm + ReLU, whose masks amplify forward error in the gradients).  `workspace`: smk_conv2_train_workspace() bytes of device memory; the split weights are rebuilt from `weight`
 * in the same call, so an optimizer step needs no other notification.  The weight / bias gradients stay with the caller (PyTorch-ROCm's
 * convolution_backward in models/conv.py); the data gradient is smk_conv2_train_dgrad.  Enqueued on `stream`. */
int64_t smk_conv2_train_workspace(void);
int smk_conv2_train_forward(const float *a1, const float *weight, const float *bias, int32_t B, int32_t H, int32_t W, float *z2,
                            void *workspace, void *stream);
/* dX [B][64][H][W] = the data gradient of that convolution from dz [B][128][H][W] (the 3x3 convolution 128 -> 64 with the flipped
 * kernel), same arithmetic and shape rules; `workspace` as above (its own contents: do not share one buffer between a forward and a
 * data-gradient call that may overlap).  */
int smk_conv2_train_dgrad(const float *dz, const float *weight, int32_t B, int32_t H, int32_t W, float *dx, void *workspace, void *stream);
/* dW [128][64][3][3] (and db [128] = sum of dz over batch and pixels, unless NULL) of that convolution from dz [B][128][H][W] and the saved
 * input a1 [B][64][H][W]: per 8 x 16 tile a GEMM with the pixels as the MFMA k dimension, accumulated in registers per workgroup, the
 * workgroups' partial sums added in a fixed order (deterministic, no atomics).  `workspace`: smk_conv2_train_wgrad_workspace() bytes. */
int64_t smk_conv2_train_wgrad_workspace(void);
int smk_conv2_train_wgrad(const float *dz, const float *a1, int32_t B, int32_t H, int32_t W, float *dw, float *db, void *workspace, void *stream);

/* The passes of the two calls above one at a time, for BatchNorm statistics that span several processes: data-parallel training
 * (train.py under DistributedDataParallel) gives every process a shard of the batch, while the reference's BatchNorm2d layers see the
 * whole batch of ONE process (smokephys_net.py:26,29; train.py:59-93).  The host all-reduces the per-channel statistics between the
 * phases (models/sync_bn.py).  Unused pointers may be NULL.
 *   SMK_BN_STATS     z -> mean / var (biased) / rstd [C] of THIS process's batch (workspace as above);
 *   SMK_BN_APPLY     out = blockmean(relu(bn(z))) from the GIVEN mean / rstd;
 *   SMK_BN_BWD_SUMS  dout, z, given mean / rstd -> this process's dgamma = sum dy * zhat and dbeta = sum dy (workspace);
 *   SMK_BN_BWD_DZ    dz from the GIVEN (all-reduced) dgamma / dbeta and count = elements per channel of the GLOBAL batch.
 * Frozen (running) statistics under autograd are these two element-wise phases alone: SMK_BN_APPLY with mean / rstd from the running
 * statistics, and SMK_BN_BWD_DZ with zero dgamma / dbeta and count = 1, which is exactly dz = gamma * rstd * dy * [y > 0].  At pool 1 they
 * take any plane with H * W % 4 == 0 (the reductions keep whole 4,096-float chunks); every pool of the fused calls is served. */
enum smk_bn_phase { SMK_BN_STATS = 0, SMK_BN_APPLY = 1, SMK_BN_BWD_SUMS = 2, SMK_BN_BWD_DZ = 3 };
int smk_bn_relu_pool_phase(int32_t phase, const float *z, const float *dout, int32_t B, int32_t C, int32_t H, int32_t W, const float *gamma,
                           const float *beta, double eps, float *mean, float *var, float *rstd, int32_t pool, float *out, float *dz,
                           float *dgamma, float *dbeta, double count, void *workspace, void *stream);

/* The chaos term of one ChaosAttention layer folded into Q (chaos_attention.py:39-66 lorenz_system + generate_chaos_field,
 * :85-100 chaos_proj / chaos_gate / chaos_strength): noise [3][B] = the three randn(B,1) draws (before the 0.1 scale),
 * proj_w [D][3], proj_b [D], gate_w [D], gate_b [1] (PyTorch layouts) -> addend [B][5][ld_addend] (columns 0..D-1
 * written; a wider pitch lets it land in the q columns of a fused q|k|v addend), the value row l of the
 * sequence adds to its query: strength * sigmoid(gate(C_t)) * C_t, C_t = chaos_proj(Lorenz state t), t = l mod 5
 * (5 explicit-Euler steps, sigma/rho/beta/dt as given; reference: 10, 28, 8/3, 0.01).  Feed it to smk_linear_forward's
 * periodic_add of q_proj.  Replaces ~90 tiny elementwise launches per layer. */
int smk_chaos_addend(const float *noise, int32_t B, int32_t D, const float *proj_w, const float *proj_b,
                     const float *gate_w, const float *gate_b, double strength, double sigma, double rho, double beta,
                     double dt, float *addend, int64_t ld_addend, void *stream);

/* Softmax attention of ChaosAttention (chaos_attention.py:102-112) once the chaos term is folded into Q
 * (softmax(((Q + addend) K^T) * scale) V, heads merged back): q, k, v [B][L][ld*] fp32 with head h in columns
 * head_dim*h .. of a token row (the layout q_proj / k_proj / v_proj write), out [B][L][ldo] in the same convention
 * (what out_proj reads -- no transpose copy).  Flash style (no L x L tensor), split-bf16 MFMA, fp32-class accuracy.
 * Requires head_dim == 64 and L % 128 == 0 (else SMK_ERR_UNSUPPORTED); scale = 1 / (sqrt(head_dim) * temperature).
 * out_format: smk_format of out (split: dense rows, ldo == H * head_dim). */
int smk_attention(const float *q, const float *k, const float *v, void *out, int32_t B, int32_t L, int32_t H,
                  int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale, int32_t out_format,
                  void *stream);
/* The same attention with a workspace: when the grid of smk_attention would leave most CUs idle (B * H * L / 128 workgroups: 64 at batch 1 of
 * the model's shape), the keys of each query block are dealt to 2-8 workgroups whose partial (output, max, sum) states a second launch merges
 * in split order (deterministic).  smk_attention_workspace_bytes: the bytes that split needs for this problem on the current device (0: no
 * split would be made -- pass none).  A workspace that is null or too small, or a split-bf16 output, runs the unsplit kernel. */
int64_t smk_attention_workspace_bytes(int32_t B, int32_t L, int32_t H, int32_t head_dim);
int smk_attention_ws(const float *q, const float *k, const float *v, void *out, int32_t B, int32_t L, int32_t H,
                     int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale, int32_t out_format,
                     void *workspace, int64_t workspace_bytes, void *stream);
/* smk_attention_ws with k and v in kv_format = SMK_FMT_F32 or SMK_FMT_SPLIT4_INPLACE (same pointers, pitches and column convention; the
 * values the kernel multiplies are bit for bit those it would have formed from the fp32 k and v, so the output is identical). */
int smk_attention_kv(const float *q, const void *k, const void *v, void *out, int32_t B, int32_t L, int32_t H,
                     int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale, int32_t out_format, int32_t kv_format,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* Training form of smk_attention (chaos_attention.py:102-112 under autograd, train.py:88-89): the same forward with fp32 output,
 * plus lse [B][L][H] = log2 sum_j 2^(scale * log2(e) * q_i.k_j) per (token, head) -- the softmax normaliser the backward
 * recomputes P from (log2 units). */
int smk_attention_forward_lse(const float *q, const float *k, const float *v, float *out, float *lse, int32_t B, int32_t L,
                              int32_t H, int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale,
                              void *stream);

/* Backward of that attention: dq, dk, dv [B][L][ldd*] (head h = columns 64h .. 64h+63) from q, k, v, the output gradient dout
 * [B][L][ldo], the forward's lse and delta [B][L][H] = sum_d dout * out per (token, head).  Two launches of one kernel body
 * (dk/dv per 128-key block, dq per 128-query block), split-bf16 MFMA like the forward, deterministic (no atomics).
 * Same shape limits as smk_attention. */
int smk_attention_backward(const float *q, const float *k, const float *v, const float *dout, const float *lse,
                           const float *delta, float *dq, float *dk, float *dv, int32_t B, int32_t L, int32_t H,
                           int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk,
                           int64_t lddv, double scale, void *stream);
/* delta [rows][H] = sum_d dout[row][64 h + d] * out[row][64 h + d] -- the `delta` input of smk_attention_backward (rowsum(dout * out) per head)
 * as one pass over the two tensors (row pitches ld_dout / ld_out floats). */
int smk_attention_delta(const float *dout, const float *out, int64_t rows, int32_t H, int32_t head_dim, int64_t ld_dout, int64_t ld_out,
                        float *delta, void *stream);

/* The softmax weights of that attention, which the flash kernel keeps in registers only (chaos_attention.py:100-108: the `attn_weights`
 * the reference's SmokeVisualizer.plot_attention_maps takes, visualization.py:80, 102).  From q and k as smk_attention takes them (fp32,
 * the chaos term folded into q) and lse [B][L][H] as smk_attention_forward_lse writes it (log2 units):
 *     p_ij = 2^(scale * log2(e) * q_i.k_j - lse_i)          (split-bf16 MFMA, the forward's products)
 * smk_attention_received: recv [B][H][ld_recv], recv[b][h][j] = (1 / L) sum_i p_ij -- the attention key j receives (visualization.py:102,
 * `attn.mean(axis=0)`), without any L x L tensor; columns 0 .. L-1 of a row are written, each exactly once, in a summation order that
 * depends on (B, L, H) only (no atomics: a repeated call is bit-identical).
 * smk_attention_probs: the matrices themselves for batches b0 .. b0+nb-1 and heads h0 .. h0+nh-1 of the B x H the tensors hold:
 * probs [nb][nh][L][ld_probs], probs[..][i][j] = p_ij (visualization.py:80 plots [0, 0]); bit for bit the slice of the full call.
 * Limits as smk_attention: head_dim == 64 and L % 128 == 0 (else SMK_ERR_UNSUPPORTED); B * L * ld < 2^29 floats for q and k, pitches
 * multiples of 4 floats, 16-byte aligned q and k, ld_recv / ld_probs >= L (else SMK_ERR_INVALID).  Nothing is written on an error. */
int smk_attention_received(const float *q, const float *k, const float *lse, float *recv, int32_t B, int32_t L, int32_t H,
                           int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ld_recv, double scale, void *stream);
int smk_attention_probs(const float *q, const float *k, const float *lse, float *probs, int32_t B, int32_t L, int32_t H,
                        int32_t head_dim, int32_t b0, int32_t nb, int32_t h0, int32_t nh, int64_t ldq, int64_t ldk, int64_t ld_probs,
                        double scale, void *stream);

/* nn.LayerNorm over the last dimension (smokephys_net.py:149-150, applied at :161,:165; biased variance, eps as given):
 * x [rows][ldx] -> y [rows][ldy], weight / bias [D].  D % 4 == 0, D <= 2048 (else SMK_ERR_UNSUPPORTED).
 * y_format: smk_format of y (split: D % 8 == 0, dense rows, ldy == D). */
int smk_layernorm(const float *x, int64_t rows, int32_t D, int64_t ldx, const float *weight, const float *bias, double eps,
                  void *y, int64_t ldy, int32_t y_format, void *stream);

/* Backward of smk_layernorm (autograd of nn.LayerNorm, train.py:89): dx [rows][ld_dx] from x, dy and weight (the row statistics
 * are recomputed), dweight / dbias [D] as column sums over the rows added in a fixed order (deterministic).  `workspace`:
 * smk_layernorm_bwd_workspace(D) bytes of device memory, caller-owned.  Same D limits as smk_layernorm. */
int64_t smk_layernorm_bwd_workspace(int32_t D);
int smk_layernorm_backward(const float *x, const float *dy, int64_t rows, int32_t D, int64_t ldx, int64_t ld_dy,
                           const float *weight, double eps, float *dx, int64_t ld_dx, float *dweight, float *dbias,
                           void *workspace, void *stream);

/* ------------------------------------------------------------------ reconstruction head */
/* Eval-mode SmokePhysNet.reconstruction_head (smokephys_net.py:57-66): ConvTranspose2d(64,32,4,2,1) + BN + ReLU ->
 * ConvTranspose2d(32,16,4,2,1) + BN + ReLU -> Conv2d(16,1,3,padding 1) -> Sigmoid.  Device pointers, PyTorch layouts:
 * ct*_w [in][out][4][4], conv_w [1][16][3][3]; BN as (weight, bias, running_mean, running_var), eps 1e-5. */
typedef struct smk_decoder_weights {
    const float *ct1_w, *ct1_b, *bn1_w, *bn1_b, *bn1_mean, *bn1_var;
    const float *ct2_w, *ct2_b, *bn2_w, *bn2_b, *bn2_mean, *bn2_var;
    const float *conv_w, *conv_b;
} smk_decoder_weights;
typedef struct smk_decoder smk_decoder; /* opaque: BN-folded weights on the device */

int smk_decoder_create(const smk_decoder_weights *w, int32_t device_id, void *stream, smk_decoder **out);
int smk_decoder_destroy(smk_decoder *dec);

/* tokens [B][S*S][64] fp32 -- output_decoder's result, read as `transpose(1,2).view(B,64,S,S)` (smokephys_net.py:117) --
 * -> recon [B][1][4S][4S].  tmp1 [B][32][2S][2S] and tmp2 [B][16][4S][4S] are caller-owned scratch.  S % 16 == 0. */
int smk_decoder_forward(smk_decoder *dec, const float *tokens, int32_t B, int32_t S, float *tmp1, float *tmp2,
                        float *recon, void *stream);

/* The same head in TRAINING mode, under autograd: its three convolutions alone (the BatchNorms run on smk_bn_relu_pool_* with pool 1, on
 * batch statistics).  Plain fp32 FMAs; every reduction is per-workgroup partial sums in the caller's workspace added in a fixed order (no
 * atomics: repeated calls are bit-identical).  Device pointers, enqueued on `stream`.
 * ConvTranspose2d(CIN, COUT, 4, stride 2, padding 1), weight [CIN][COUT][4][4], bias [COUT] or NULL; x [B][CIN][H][W], or token-major
 * [B][H*W][CIN] when `tok` != 0 (output_decoder's result, no transpose); z / dz [B][COUT][2H][2W].  Shapes: COUT 16 or 32, CIN a multiple
 * of 16 (COUT 32) or 32 (COUT 16) up to 4096, H and W multiples of 16, 1 <= B <= 65535 (else SMK_ERR_UNSUPPORTED).
 *   forward: z = conv(x) + bias, raw (no activation);
 *   dgrad:   dx = the data gradient from dz, written in the layout `tok` names (dX[c][i][j] = sum over o, ky, kx of
 *            dz[o][2i-1+ky][2j-1+kx] W[c][o][ky][kx]);
 *   wgrad:   dw [CIN][COUT][4][4] and db [COUT] (unless NULL) from dz and the saved x; `workspace`: smk_convt4s2_train_wgrad_workspace()
 *            bytes (0 for an unsupported shape). */
int smk_convt4s2_train_forward(const float *x, const float *weight, const float *bias, int32_t B, int32_t CIN, int32_t COUT, int32_t H,
                               int32_t W, int32_t tok, float *z, void *stream);
int smk_convt4s2_train_dgrad(const float *dz, const float *weight, int32_t B, int32_t CIN, int32_t COUT, int32_t H, int32_t W, int32_t tok,
                             float *dx, void *stream);
int64_t smk_convt4s2_train_wgrad_workspace(int32_t B, int32_t CIN, int32_t COUT, int32_t H, int32_t W);
int smk_convt4s2_train_wgrad(const float *dz, const float *x, int32_t B, int32_t CIN, int32_t COUT, int32_t H, int32_t W, int32_t tok,
                             float *dw, float *db, void *workspace, void *stream);
/* Conv2d(16, 1, 3, padding 1) + Sigmoid: x [B][16][H][W] -> y [B][H][W]; H % 8 == 0, W % 32 == 0, 1 <= B <= 65535.  weight [16][3][3],
 * bias [1] or NULL.  The backward takes dy, the forward's y and x: g = dy y (1 - y), then dx [B][16][H][W], and dw [16][3][3] / db [1]
 * unless both are NULL; `workspace`: smk_conv3_sigmoid_train_workspace() bytes (g and the partial sums). */
int smk_conv3_sigmoid_train_forward(const float *x, const float *weight, const float *bias, int32_t B, int32_t H, int32_t W, float *y,
                                    void *stream);
int64_t smk_conv3_sigmoid_train_workspace(int32_t B, int32_t H, int32_t W);
int smk_conv3_sigmoid_train_backward(const float *dy, const float *y, const float *x, const float *weight, int32_t B, int32_t H, int32_t W,
                                     float *dx, float *dw, float *db, void *workspace, void *stream);

/* ------------------------------------------------------------------ train step tail: gradient clip, AdamW, loss terms */
/* One row of the HOST table the next three functions take: device pointers of one parameter's fp32 tensors of n elements each (dense;
 * 4-byte aligned, 16-byte accesses where all of a row's pointers are 16-byte aligned).  n == 0 is legal and does nothing.  The table is
 * read before the call returns: its descriptors travel in the kernel arguments, 64 rows per launch; nothing is allocated or copied. */
typedef struct smk_opt_tensor {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int64_t n;
} smk_opt_tensor;

/* The total 2-norm of every row's `grad` (the other pointers are not read) and torch's clip coefficient (clip_grads_with_norm_):
 * out[0] = norm, out[1] = clamp(max_norm / (norm + 1e-6), max = 1), both fp32; a NaN norm gives a NaN coefficient.  Work is cut into
 * chunks of 8192 elements counted from element 0 of each tensor; each chunk's sum of squares is one fp64 partial whose value depends on
 * the chunk's values only (not on the pointer's alignment), and one workgroup adds the partials in a fixed order: no atomics, repeated
 * calls are bit-identical.  workspace: device memory of at least smk_grad_norm_workspace(t, n_tensors) bytes, 8-byte aligned. */
int64_t smk_grad_norm_workspace(const smk_opt_tensor *t, int32_t n_tensors);
int smk_grad_norm(const smk_opt_tensor *t, int32_t n_tensors, double max_norm, float *out, void *workspace, int64_t workspace_bytes,
                  void *stream);
/* torch.optim.AdamW's update (decoupled weight decay, the single-tensor order) of every row, per element in fp32:
 *   g' = g * scale;  p *= 1 - lr * weight_decay;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / bias_correction1) * m / (sqrt(v) / sqrt(bias_correction2) + eps)
 * p takes one rounding per step: the two lines that touch it are evaluated as p - (lr weight_decay p + (lr / bias_correction1) m / (...)),
 * which is the same value.  The coefficients are rounded to fp32 once on the host.  scale = *grad_scale, read on the device (smk_grad_norm's out + 1: no host
 * synchronisation between the two), or 1 when grad_scale is NULL.  write_grad != 0 also stores g'.  param, exp_avg and exp_avg_sq are
 * read once and written once. */
int smk_adamw_step(const smk_opt_tensor *t, int32_t n_tensors, double lr, double beta1, double beta2, double eps, double weight_decay,
                   double bias_correction1, double bias_correction2, const float *grad_scale, int32_t write_grad, void *stream);

/* The loss of train.py's batch_losses: pred / target [planes][plane_elems], chaos_pred / chaos_target [n_chaos], and sequence
 * [seq_batch][seq_T][seq_plane] (or NULL), all dense fp32.  out [6] =
 *   total      = recon + w_chaos chaos + w_physics physics
 *   recon      = mean (pred - target)^2
 *   physics    = w_mass mass + w_continuity continuity
 *   chaos      = mean (chaos_pred - chaos_target)^2
 *   mass       = mean over planes of (sum pred - sum target)^2
 *   continuity = mean |sequence[:, t+1] - sequence[:, t]|; exactly 0 for seq_T < 2 or a NULL sequence
 * and mass_diff [planes] = sum pred - sum target, which the backward reads.  fp64 partial sums in `workspace`
 * (smk_train_loss_workspace(...) bytes, 16-byte aligned) added in a fixed order: repeated calls are bit-identical.
 * Backward, one launch, with g = grad_out [6] read on the device:
 *   d_pred  = (g[0] + g[1]) 2/N (pred - target) + (g[0] w_physics w_mass + g[2] w_mass + g[4]) 2/planes mass_diff[plane]
 *   d_chaos = (g[0] w_chaos + g[3]) 2/n_chaos (chaos_pred - chaos_target)
 * Either output may be NULL. */
int64_t smk_train_loss_workspace(int32_t planes, int32_t plane_elems, int32_t seq_batch, int32_t seq_T, int64_t seq_plane);
int smk_train_loss_forward(const float *pred, const float *target, int32_t planes, int32_t plane_elems, const float *chaos_pred,
                           const float *chaos_target, int32_t n_chaos, const float *sequence, int32_t seq_batch, int32_t seq_T,
                           int64_t seq_plane, double w_chaos, double w_physics, double w_mass, double w_continuity, float *out,
                           float *mass_diff, void *workspace, int64_t workspace_bytes, void *stream);
int smk_train_loss_backward(const float *pred, const float *target, int32_t planes, int32_t plane_elems, const float *mass_diff,
                            const float *chaos_pred, const float *chaos_target, int32_t n_chaos, const float *grad_out, double w_chaos,
                            double w_physics, double w_mass, float *d_pred, float *d_chaos, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SMOKEHIP_H */
