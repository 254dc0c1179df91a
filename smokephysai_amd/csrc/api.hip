// C ABI of libsmokehip.so (see include/smokehip.h for the contract and the reference interfaces replaced).
#include <stdlib.h>

#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "chaos.h"
#include "conv3d.h"
#include "conv3d_train.h"
#include "decoder.h"
#include "decoder_train.h"
#include "elementwise.h"
#include "encoder.h"
#include "encoder_train.h"
#include "flow.h"
#include "linear.h"
#include "loss.h"
#include "norm.h"
#include "optim.h"
#include "quality.h"
#include "stencil.h"
#include "stencil3d.h"
#include "transformer.h"

namespace smk {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int check_launch(hipError_t e, const char *what) {
    if (e != hipSuccess) {
        set_error(std::string(what) + ": " + hipGetErrorString(e));
        return SMK_ERR_HIP;
    }
    return SMK_OK;
}

namespace {
std::mutex g_dev_mu;
std::map<int, int> g_num_cu;                                  // device -> CU count
std::map<std::pair<int, const void *>, int> g_dev_int;        // (device, key) -> cached value / "seen" marker
int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}
}  // namespace

int device_num_cu() {
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = g_num_cu.find(dev);
    if (it != g_num_cu.end()) return it->second;
    hipDeviceProp_t prop;
    int n = 256;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    g_num_cu[dev] = n;
    return n;
}

bool first_use_begin(const void *key) {
    const int dev = current_device();
    g_dev_mu.lock();
    if (g_dev_int.count(std::make_pair(dev, key))) {
        g_dev_mu.unlock();
        return false;
    }
    return true;                                              // lock held until first_use_end
}
void first_use_end(const void *key) {
    g_dev_int.emplace(std::make_pair(current_device(), key), 1);
    g_dev_mu.unlock();
}

int device_cached_int(const void *key, int (*compute)()) {
    const int dev = current_device();
    {
        std::lock_guard<std::mutex> lk(g_dev_mu);
        auto it = g_dev_int.find(std::make_pair(dev, key));
        if (it != g_dev_int.end()) return it->second;
    }
    const int v = compute();                                  // (occupancy queries etc.: outside the lock)
    std::lock_guard<std::mutex> lk(g_dev_mu);
    return g_dev_int.emplace(std::make_pair(dev, key), v).first->second;
}
}  // namespace smk

using namespace smk;

struct smk_sim {
    Geom g;
    StateView s;          // caller-owned
    StateView t;          // library scratch (u2, v2, p2, d2)
    float *div = nullptr;
    float *perlin = nullptr, *mandel = nullptr, *fractal = nullptr;   // [N][N], square grids only
    uint8_t *dev_mask = nullptr;
    SrcDev *dev_src = nullptr;
    int *dev_first = nullptr;
    int src_cap = 0;
    int jacobi_iters = 20;
    int device = 0;
    ProjectSync psync;    // hand-off flags / status word of the single-launch projection
};

struct smk_sim3d {
    Geom3 g;
    State3 s;             // caller-owned
    State3 t;             // library scratch (u2, v2, w2, p2, d2)
    float *div = nullptr;
    float *p3 = nullptr;   // third pressure buffer: only when the Jacobi plan has an odd number (>= 3) of launches (launch3_jacobi)
    uint8_t *dev_mask = nullptr;
    Src3Dev *dev_src = nullptr;
    int *dev_first = nullptr;
    int src_cap = 0;
    int jacobi_iters = 20;
    int device = 0;
};

struct smk_decoder {
    DecoderDev d;
    float *blob = nullptr;
    int device = 0;
};

struct smk_linear {
    LinearDev l;
    int device = 0;
};

struct smk_encoder {
    EncoderDev e;
    float *blob = nullptr;
    unsigned short *blob16 = nullptr;
    int device = 0;
    EncoderSkip skip;     // tile-skip tables and workspace (lazy; a new handle starts without them)
    EncoderPartials partials;   // per-tile partial sums of frames beyond 256^2 (lazy; independent of the skip state)
};

namespace {

// Every entry point runs on its handle's device and leaves the CALLER's current device as it found it (PyTorch tracks its own).
struct DeviceGuard {
    int prev = -1, rc = SMK_OK;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev && hipSetDevice(dev) != hipSuccess) {
            set_error("hipSetDevice failed for the handle's device");
            rc = SMK_ERR_HIP;
        }
        if (prev == dev) prev = -1;                           // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

int report_timeout() {
    set_error("persistent projection: a band waited longer than 0.5 s for its neighbour's hand-off (its workgroups were not all "
              "resident at once -- is another kernel or process holding compute units?).  The pressure, velocity and density of the "
              "grids of that projection were set to NaN, and so is every frame emitted since: reset the simulator (smk_sim_reset).  "
              "Later projections of this handle use the multi-launch form (SMK_JACOBI_PERSIST=0 selects it from the start)");
    return SMK_ERR_TIMEOUT;
}

int project_status(hipError_t e) {
    if (e == hipErrorLaunchTimeOut) return report_timeout();
    return check_launch(e, "project");
}

// Every smk_sim_* call starts here: a time-out that a persistent projection of an EARLIER call has reported by now is returned by this
// call (once).  What the launches of the current call report is seen by smk_sim_status after the stream has been synchronised.
int sim_entry(smk_sim *sim) {
    return project_sync_take_timeout(sim->psync) ? report_timeout() : SMK_OK;
}

int run_stage(smk_sim *sim, int stage, hipStream_t st) {
    const Geom &g = sim->g;
    StateView &s = sim->s, &t = sim->t;
    switch (stage) {
        case SMK_STAGE_BUOY_DIFFUSE:   // s -> t (u2, v2, d2)
            return check_launch(launch_buoy_diffuse(g, s, t, st), "buoy_diffuse");
        case SMK_STAGE_PROJECT: {      // on t.u, t.v with s.p
            return project_status(launch_project(g, t.u, t.v, s.p, t.p, sim->div, sim->jacobi_iters, st, &sim->psync));
        }
        case SMK_STAGE_ADVECT_U:       // u <- adv(u2; u2, v2)
            return check_launch(launch_advect(g, 0, t.u, s.u, t.u, t.v, nullptr, 0, nullptr, 0.f, nullptr, nullptr, st),
                                "advect_u");
        case SMK_STAGE_ADVECT_V:       // v <- adv(v2; u, v2)
            return check_launch(launch_advect(g, 1, t.v, s.v, s.u, t.v, nullptr, 0, nullptr, 0.f, nullptr, nullptr, st),
                                "advect_v");
        case SMK_STAGE_ADVECT_D:       // density <- adv(d2; u, v) * 0.995
            return check_launch(launch_advect(g, 2, t.d, s.d, s.u, s.v, nullptr, 0, nullptr, 0.f, nullptr, nullptr, st),
                                "advect_d");
    }
    set_error("unknown stage");
    return SMK_ERR_INVALID;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int smk_abi_version(void) { return SMK_ABI_VERSION; }
const char *smk_last_error(void) { return g_err.c_str(); }

int smk_sim_create(const smk_sim_desc *d, smk_sim **out) {
    SMK_REQUIRE(d && out, "null desc/out");
    SMK_REQUIRE(d->batch >= 1 && d->height >= 3 && d->width >= 3, "batch>=1, height,width>=3");
    SMK_REQUIRE(d->pitch_c >= d->width && d->pitch_v >= d->width + 1, "pitch_c >= W and pitch_v >= W+1");
    SMK_REQUIRE(d->jacobi_iters >= 0, "jacobi_iters >= 0");
    SMK_REQUIRE(d->u && d->v && d->p && d->density, "null state pointer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible");
        return SMK_ERR_NO_DEVICE;
    }
    DeviceGuard guard(d->device_id);
    int rc = guard.rc;
    if (rc) return rc;
    smk_sim *sim = new smk_sim();
    Geom &g = sim->g;
    g.B = d->batch; g.H = d->height; g.W = d->width; g.pc = d->pitch_c; g.pv = d->pitch_v;
    g.su = (size_t)(g.H + 1) * g.pc; g.sv = (size_t)g.H * g.pv; g.sc = (size_t)g.H * g.pc;
    g.dt = (float)d->dt;
    g.coef_uv = (float)(d->dt * d->viscosity);              // navier_stokes.py:72,158-159
    g.coef_d = (float)(d->dt * (d->viscosity * 0.1));       // navier_stokes.py:160
    sim->s = {d->u, d->v, d->p, d->density};
    sim->jacobi_iters = d->jacobi_iters;
    sim->device = d->device_id;
    size_t B = g.B;
    hipError_t e = hipSuccess;
    auto alloc = [&](float **p, size_t n) { if (e == hipSuccess) e = hipMalloc((void **)p, n * sizeof(float)); };
    alloc(&sim->t.u, B * g.su); alloc(&sim->t.v, B * g.sv); alloc(&sim->t.p, B * g.sc); alloc(&sim->t.d, B * g.sc);
    alloc(&sim->div, B * g.sc);
    if (e == hipSuccess) e = project_sync_create(sim->psync, g.B);
    if (e == hipSuccess) e = hipMalloc((void **)&sim->dev_mask, B);
    if (e == hipSuccess) e = hipMalloc((void **)&sim->dev_first, (B + 1) * sizeof(int));
    if (g.H == g.W && e == hipSuccess) {
        size_t n = (size_t)g.H * g.W;
        alloc(&sim->perlin, n); alloc(&sim->mandel, n); alloc(&sim->fractal, n);
        if (e == hipSuccess) e = launch_fractal_constants(g.H, sim->perlin, sim->mandel, sim->fractal, 0);
        if (e == hipSuccess) e = hipStreamSynchronize(0);
    }
    if (e != hipSuccess) {
        set_error(std::string("smk_sim_create: ") + hipGetErrorString(e));
        smk_sim_destroy(sim);
        return SMK_ERR_HIP;
    }
    *out = sim;
    return SMK_OK;
}

int smk_sim_destroy(smk_sim *sim) {
    if (!sim) return SMK_OK;
    DeviceGuard guard(sim->device);              // frees run on the handle's device; the caller's device is restored
    float *ptrs[] = {sim->t.u, sim->t.v, sim->t.p, sim->t.d, sim->div, sim->perlin, sim->mandel, sim->fractal};
    for (float *p : ptrs) if (p) (void)hipFree(p);           // (hipFree waits for the device: every launch of this handle has finished)
    const bool timed_out = project_sync_take_timeout(sim->psync);
    project_sync_destroy(sim->psync);
    if (sim->dev_mask) (void)hipFree(sim->dev_mask);
    if (sim->dev_first) (void)hipFree(sim->dev_first);
    if (sim->dev_src) (void)hipFree(sim->dev_src);
    delete sim;
    return timed_out ? report_timeout() : SMK_OK;            // the handle is gone either way; the caller learns its last frames were NaN
}

int smk_sim_status(smk_sim *sim) {
    SMK_REQUIRE(sim, "null sim");
    return sim_entry(sim);
}

int smk_sim_reset(smk_sim *sim, const uint8_t *grid_mask, void *stream) {
    SMK_REQUIRE(sim, "null sim");
    // a pending time-out report is acknowledged here like at every entry point, but the reset -- the recovery the report asks for -- is
    // still carried out: ONE call both tells the caller and leaves the requested grids zeroed (the message stays in smk_last_error)
    const int pending = sim_entry(sim);
    if (pending && pending != SMK_ERR_TIMEOUT) return pending;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    int rc = guard.rc;
    if (rc) return rc;
    const uint8_t *dm = nullptr;
    if (grid_mask) {
        SMK_HIP_TRY(hipMemcpyAsync(sim->dev_mask, grid_mask, sim->g.B, hipMemcpyHostToDevice, st));
        dm = sim->dev_mask;
    }
    const hipError_t le = launch_zero_state(sim->g, sim->s, dm, st);
    if (le != hipSuccess) return check_launch(le, "zero_state");
    return pending;                                           // SMK_OK, or SMK_ERR_TIMEOUT once with the reset done
}

int smk_sim_add_sources(smk_sim *sim, const smk_source *src, int32_t n, void *stream) {
    SMK_REQUIRE(sim && (src || n == 0) && n >= 0, "null sim/sources");
    if (int e = sim_entry(sim)) return e;
    if (n == 0) return SMK_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    int rc = guard.rc;
    if (rc) return rc;
    const int B = sim->g.B;
    std::vector<int> first(B + 1, 0);
    for (int k = 0; k < n; ++k) {
        SMK_REQUIRE(src[k].grid >= 0 && src[k].grid < B, "source grid index out of range");
        SMK_REQUIRE(src[k].radius >= 0, "radius >= 0");
        first[src[k].grid + 1]++;
    }
    for (int b = 0; b < B; ++b) first[b + 1] += first[b];
    std::vector<SrcDev> host(n);
    std::vector<int> fill(first.begin(), first.end() - 1);
    for (int k = 0; k < n; ++k) {      // stable counting sort by grid keeps the caller's order within a grid
        const smk_source &q = src[k];
        double r3 = (double)q.radius / 3.0;
        host[fill[q.grid]++] = SrcDev{q.x, q.y, q.radius, (float)(2.0 * (r3 * r3)), (float)q.intensity};
    }
    if (n > sim->src_cap) {
        if (sim->dev_src) SMK_HIP_TRY(hipFree(sim->dev_src));
        sim->dev_src = nullptr;
        SMK_HIP_TRY(hipMalloc((void **)&sim->dev_src, (size_t)n * sizeof(SrcDev)));
        sim->src_cap = n;
    }
    SMK_HIP_TRY(hipMemcpyAsync(sim->dev_src, host.data(), (size_t)n * sizeof(SrcDev), hipMemcpyHostToDevice, st));
    SMK_HIP_TRY(hipMemcpyAsync(sim->dev_first, first.data(), (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    rc = check_launch(launch_add_sources(sim->g, sim->s.d, sim->dev_src, sim->dev_first, st), "add_sources");
    if (rc) return rc;
    SMK_HIP_TRY(hipStreamSynchronize(st));   // host staging vectors die here
    return SMK_OK;
}

int smk_sim_step(smk_sim *sim, int32_t n_steps, float *frames, int64_t fsb, int64_t fst, int32_t add_fractal,
                 double fractal_intensity, void *stream) {
    SMK_REQUIRE(sim && n_steps >= 0, "null sim / negative n_steps");
    if (int e = sim_entry(sim)) return e;
    if (add_fractal && frames && !sim->fractal) {
        // fractal_generator.py:44,49: the [w,h] mask indexes an [h,w] buffer -> the reference raises for h != w
        set_error("fractal perturbation needs a square grid (reference raises an IndexError for H != W)");
        return SMK_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    int rc = guard.rc;
    if (rc) return rc;
    const float *fr = (add_fractal && frames) ? sim->fractal : nullptr;
    for (int t = 0; t < n_steps; ++t) {
        float *ft = frames ? frames + (size_t)t * fst : nullptr;
        // buoyancy + diffusion + projection: one persistent launch where the plan allows (stencil.hip: launch_buoy_project)
        rc = project_status(launch_buoy_project(sim->g, sim->s, sim->t, sim->s.p, sim->div, sim->jacobi_iters, st, &sim->psync));
        if (rc) return rc;
        // u <- adv(u2; u2, v2), v <- adv(v2; u, v2), density <- adv(d2; u, v) * 0.995 (+ frame) in one launch
        rc = check_launch(launch_advect_fused(sim->g, sim->t, sim->s, ft, fsb, fr, (float)fractal_intensity, st), "advect_fused");
        if (rc) return rc;
    }
    return SMK_OK;
}

int smk_sim_run_stage(smk_sim *sim, int32_t stage, void *stream) {
    SMK_REQUIRE(sim, "null sim");
    if (int e = sim_entry(sim)) return e;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    int rc = guard.rc;
    if (rc) return rc;
    const Geom &g = sim->g;
    const size_t B = g.B;
    StateView &s = sim->s, &t = sim->t;
    // Stand-alone stage semantics: caller state in, caller state out.  Internally the step ping-pongs between the
    // caller's tensors (s) and scratch (t); here the stage's inputs are first mirrored into the side it reads.
    auto cp = [&](float *dst, const float *src, size_t n) {
        return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    switch (stage) {
        case SMK_STAGE_BUOY_DIFFUSE:
            rc = run_stage(sim, stage, st);
            if (rc) return rc;
            SMK_HIP_TRY(cp(s.u, t.u, B * g.su)); SMK_HIP_TRY(cp(s.v, t.v, B * g.sv)); SMK_HIP_TRY(cp(s.d, t.d, B * g.sc));
            return SMK_OK;
        case SMK_STAGE_PROJECT:
            SMK_HIP_TRY(cp(t.u, s.u, B * g.su)); SMK_HIP_TRY(cp(t.v, s.v, B * g.sv));
            rc = run_stage(sim, stage, st);
            if (rc) return rc;
            SMK_HIP_TRY(cp(s.u, t.u, B * g.su)); SMK_HIP_TRY(cp(s.v, t.v, B * g.sv));
            return SMK_OK;
        case SMK_STAGE_ADVECT_U:      // reads (u, v) -> writes u
            SMK_HIP_TRY(cp(t.u, s.u, B * g.su)); SMK_HIP_TRY(cp(t.v, s.v, B * g.sv));
            return run_stage(sim, stage, st);
        case SMK_STAGE_ADVECT_V:      // reads v (field), u (already advected), v -> writes v
            SMK_HIP_TRY(cp(t.v, s.v, B * g.sv));
            return run_stage(sim, stage, st);
        case SMK_STAGE_ADVECT_D:
            SMK_HIP_TRY(cp(t.d, s.d, B * g.sc));
            return run_stage(sim, stage, st);
    }
    set_error("unknown stage");
    return SMK_ERR_INVALID;
}

int smk_sim_divergence(smk_sim *sim, float *out, void *stream) {
    SMK_REQUIRE(sim && out, "null sim/out");
    if (int e = sim_entry(sim)) return e;
    DeviceGuard guard(sim->device);
    int rc = guard.rc;
    if (rc) return rc;
    const Geom &g = sim->g;
    return check_launch(launch_divergence(g, sim->s.u, sim->s.v, out, g.W, (size_t)g.H * g.W, (hipStream_t)stream),
                        "divergence");
}

int smk_sim_backtrace(smk_sim *sim, int32_t which, int32_t *x0, int32_t *y0, void *stream) {
    SMK_REQUIRE(sim && x0 && y0 && which >= 0 && which <= 2, "null sim/x0/y0 or which not in 0..2");
    if (int e = sim_entry(sim)) return e;
    DeviceGuard guard(sim->device);
    int rc = guard.rc;
    if (rc) return rc;
    const StateView &s = sim->s;
    const float *field = which == 0 ? s.u : (which == 1 ? s.v : s.d);
    return check_launch(launch_advect(sim->g, which, field, nullptr, s.u, s.v, nullptr, 0, nullptr, 0.f, x0, y0,
                                      (hipStream_t)stream), "backtrace");
}

int smk_sim_sweep_forms(smk_sim *sim, int32_t *out, int32_t capacity, int32_t *bands_per_grid, void *stream) {
    SMK_REQUIRE(sim && out && bands_per_grid && capacity >= 0, "null sim / out / bands_per_grid or negative capacity");
    DeviceGuard guard(sim->device);
    if (guard.rc) return guard.rc;
    const ProjectSync &ps = sim->psync;
    const int n = sim->g.B * ps.forms_nb;
    *bands_per_grid = ps.forms_nb;
    if (n > capacity) {
        set_error("smk_sim_sweep_forms: out holds fewer than batch * bands_per_grid words");
        return SMK_ERR_INVALID;
    }
    SMK_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (n > 0 && ps.forms_two) SMK_HIP_TRY(hipMemcpy(out, ps.forms, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    else if (n > 0) memset(out, 0, (size_t)n * sizeof(int32_t));      // (a kernel with the exact cell only)
    return SMK_OK;
}

int smk_sim_fractal(smk_sim *sim, int32_t kind, const float **dev_ptr) {
    SMK_REQUIRE(sim && dev_ptr && kind >= 0 && kind <= 2, "null sim/dev_ptr or kind not in 0..2");
    if (!sim->fractal) {
        set_error("fractal constants exist for square grids only");
        return SMK_ERR_UNSUPPORTED;
    }
    *dev_ptr = kind == 0 ? sim->perlin : (kind == 1 ? sim->mandel : sim->fractal);
    return SMK_OK;
}

int smk_sim_describe(smk_sim *sim, char *buf, int64_t capacity) {
    SMK_REQUIRE(sim && buf && capacity > 0, "null sim / buf or no capacity");
    DeviceGuard guard(sim->device);
    if (guard.rc) return guard.rc;
    const std::string d = "{\"projection\": " + describe_projection(sim->g, sim->jacobi_iters, &sim->psync, &sim->s, &sim->t) + ", " +
                          describe_step_forms(sim->g, sim->jacobi_iters, &sim->psync, sim->s, sim->t) + ", \"advection\": \"k_advect_rows<8,4,3> (u, v, density + frame in one launch)\", \"launches_per_step\": null}";
    if ((int64_t)d.size() + 1 > capacity) {
        set_error("smk_sim_describe: buffer too small");
        return SMK_ERR_INVALID;
    }
    memcpy(buf, d.c_str(), d.size() + 1);
    return SMK_OK;
}

// fractal constant cache for the stateless smk_apply_fractal and the 3-D stepper's emit: one per (device, N)
static std::mutex g_fr_mu;
static std::map<std::pair<int, int>, float *> g_fr_cache;

static int cached_fractal_field(int N, hipStream_t st, float **out) {
    int dev = 0;
    SMK_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_fr_mu);
    auto it = g_fr_cache.find({dev, N});
    if (it == g_fr_cache.end()) {
        float *blob = nullptr;
        size_t n = (size_t)N * N;
        SMK_HIP_TRY(hipMalloc((void **)&blob, 3 * n * sizeof(float)));
        int rc = check_launch(launch_fractal_constants(N, blob, blob + n, blob + 2 * n, st), "fractal");
        if (rc) return rc;
        it = g_fr_cache.emplace(std::make_pair(dev, N), blob + 2 * n).first;
    }
    *out = it->second;
    return SMK_OK;
}

// ------------------------------------------------------------------ 3-D stepper (SPEC_3D.md)
int smk_sim3d_create(const smk_sim3d_desc *d, smk_sim3d **out) {
    SMK_REQUIRE(d && out, "null desc/out");
    SMK_REQUIRE(d->batch >= 1 && d->depth >= 3 && d->height >= 3 && d->width >= 3, "batch>=1, depth,height,width>=3");
    SMK_REQUIRE(d->pitch_c >= d->width && d->pitch_v >= d->width + 1, "pitch_c >= W and pitch_v >= W+1");
    SMK_REQUIRE(d->jacobi_iters >= 0, "jacobi_iters >= 0");
    SMK_REQUIRE((int64_t)d->batch * (d->depth + 1) <= 65535, "batch * (depth + 1) <= 65535 (one grid z-slice per plane)");
    SMK_REQUIRE((int64_t)(d->depth + 1) * (d->height + 1) * d->pitch_v < (1LL << 31), "one grid's field must stay below 2^31 elements (32-bit in-grid offsets)");
    SMK_REQUIRE(d->u && d->v && d->w && d->p && d->density, "null state pointer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible");
        return SMK_ERR_NO_DEVICE;
    }
    DeviceGuard guard(d->device_id);
    if (guard.rc) return guard.rc;
    smk_sim3d *sim = new smk_sim3d();
    Geom3 &g = sim->g;
    g.B = d->batch; g.D = d->depth; g.H = d->height; g.W = d->width; g.pc = d->pitch_c; g.pv = d->pitch_v;
    g.su = (size_t)g.D * (g.H + 1) * g.pc; g.sv = (size_t)g.D * g.H * g.pv; g.sw = (size_t)(g.D + 1) * g.H * g.pc;
    g.sc = (size_t)g.D * g.H * g.pc;
    g.dt = (float)d->dt;
    g.coef_uv = (float)(d->dt * d->viscosity);
    g.coef_d = (float)(d->dt * (d->viscosity * 0.1));
    g.sixth = (float)(1.0 / 6.0);
    sim->s = {d->u, d->v, d->w, d->p, d->density};
    sim->t = {nullptr, nullptr, nullptr, nullptr, nullptr};
    sim->jacobi_iters = d->jacobi_iters;
    sim->device = d->device_id;
    const size_t B = g.B;
    hipError_t e = hipSuccess;
    auto alloc = [&](float **p, size_t n) { if (e == hipSuccess) e = hipMalloc((void **)p, n * sizeof(float)); };
    alloc(&sim->t.u, B * g.su); alloc(&sim->t.v, B * g.sv); alloc(&sim->t.w, B * g.sw); alloc(&sim->t.p, B * g.sc); alloc(&sim->t.d, B * g.sc);
    alloc(&sim->div, B * g.sc);
    {   // J = 4 n with n odd and >= 3 (the default J = 20): five 4-sweep launches through a third buffer instead of four + two 2-sweep ones
        const int J = sim->jacobi_iters;
        if (J % 4 == 0 && ((J / 4) & 1) && J / 4 >= 3) alloc(&sim->p3, B * g.sc);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&sim->dev_mask, B);
    if (e == hipSuccess) e = hipMalloc((void **)&sim->dev_first, (B + 1) * sizeof(int));
    if (e != hipSuccess) {
        set_error(std::string("smk_sim3d_create: ") + hipGetErrorString(e));
        smk_sim3d_destroy(sim);
        return SMK_ERR_HIP;
    }
    *out = sim;
    return SMK_OK;
}

int smk_sim3d_destroy(smk_sim3d *sim) {
    if (!sim) return SMK_OK;
    DeviceGuard guard(sim->device);
    float *ptrs[] = {sim->t.u, sim->t.v, sim->t.w, sim->t.p, sim->t.d, sim->div, sim->p3};
    for (float *p : ptrs) if (p) (void)hipFree(p);
    if (sim->dev_mask) (void)hipFree(sim->dev_mask);
    if (sim->dev_first) (void)hipFree(sim->dev_first);
    if (sim->dev_src) (void)hipFree(sim->dev_src);
    delete sim;
    return SMK_OK;
}

int smk_sim3d_reset(smk_sim3d *sim, const uint8_t *grid_mask, void *stream) {
    SMK_REQUIRE(sim, "null sim");
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    if (guard.rc) return guard.rc;
    const uint8_t *dm = nullptr;
    if (grid_mask) {
        SMK_HIP_TRY(hipMemcpyAsync(sim->dev_mask, grid_mask, sim->g.B, hipMemcpyHostToDevice, st));
        dm = sim->dev_mask;
    }
    return check_launch(launch3_zero(sim->g, sim->s, dm, st), "zero_state3d");
}

int smk_sim3d_add_sources(smk_sim3d *sim, const smk_source3d *src, int32_t n, void *stream) {
    SMK_REQUIRE(sim && (src || n == 0) && n >= 0, "null sim/sources");
    if (n == 0) return SMK_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    if (guard.rc) return guard.rc;
    const int B = sim->g.B;
    std::vector<int> first(B + 1, 0);
    for (int k = 0; k < n; ++k) {
        SMK_REQUIRE(src[k].grid >= 0 && src[k].grid < B, "source grid index out of range");
        SMK_REQUIRE(src[k].radius >= 0, "radius >= 0");
        first[src[k].grid + 1]++;
    }
    for (int b = 0; b < B; ++b) first[b + 1] += first[b];
    std::vector<Src3Dev> host(n);
    std::vector<int> fill(first.begin(), first.end() - 1);
    for (int k = 0; k < n; ++k) {      // stable counting sort by grid keeps the caller's order within a grid
        const smk_source3d &q = src[k];
        const double r3 = (double)q.radius / 3.0;
        host[fill[q.grid]++] = Src3Dev{q.x, q.y, q.z, q.radius, (float)(2.0 * (r3 * r3)), (float)q.intensity};
    }
    if (n > sim->src_cap) {
        if (sim->dev_src) SMK_HIP_TRY(hipFree(sim->dev_src));
        sim->dev_src = nullptr;
        SMK_HIP_TRY(hipMalloc((void **)&sim->dev_src, (size_t)n * sizeof(Src3Dev)));
        sim->src_cap = n;
    }
    SMK_HIP_TRY(hipMemcpyAsync(sim->dev_src, host.data(), (size_t)n * sizeof(Src3Dev), hipMemcpyHostToDevice, st));
    SMK_HIP_TRY(hipMemcpyAsync(sim->dev_first, first.data(), (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    const int rc = check_launch(launch3_add_sources(sim->g, sim->s.d, sim->dev_src, sim->dev_first, st), "add_sources3d");
    if (rc) return rc;
    SMK_HIP_TRY(hipStreamSynchronize(st));   // host staging vectors die here
    return SMK_OK;
}

namespace {
// one stage on the ping-pong pair: s = caller's tensors, t = scratch.  A step runs
//   (u, v, w, d) --buoy+diffuse--> t --project (p in place via p2)--> t --advect u--> s.u --advect v--> s.v --advect w--> s.w --advect d--> s.d
int run_stage3d(smk_sim3d *sim, int stage, hipStream_t st) {
    const Geom3 &g = sim->g;
    State3 &s = sim->s, &t = sim->t;
    switch (stage) {
        case SMK_STAGE3D_BUOY_DIFFUSE:
            return check_launch(launch3_buoy_diffuse(g, s, t, st), "buoy_diffuse3d");
        case SMK_STAGE3D_PROJECT: {
            int rc = check_launch(launch3_divergence(g, t, sim->div, st), "divergence3d");
            if (rc) return rc;
            rc = check_launch(launch3_jacobi(g, s.p, t.p, sim->p3, sim->div, sim->jacobi_iters, st), "jacobi3d");
            if (rc) return rc;
            return check_launch(launch3_grad_subtract(g, t, s.p, st), "grad_subtract3d");
        }
        case SMK_STAGE3D_ADVECT_U:
            return check_launch(launch3_advect(g, 0, t.u, s.u, t.u, t.v, t.w, nullptr, 0, st), "advect_u3d");
        case SMK_STAGE3D_ADVECT_V:
            return check_launch(launch3_advect(g, 1, t.v, s.v, s.u, t.v, t.w, nullptr, 0, st), "advect_v3d");
        case SMK_STAGE3D_ADVECT_W:
            return check_launch(launch3_advect(g, 2, t.w, s.w, s.u, s.v, t.w, nullptr, 0, st), "advect_w3d");
        case SMK_STAGE3D_ADVECT_D:
            return check_launch(launch3_advect(g, 3, t.d, s.d, s.u, s.v, s.w, nullptr, 0, st), "advect_d3d");
    }
    set_error("unknown 3-D stage");
    return SMK_ERR_INVALID;
}
}  // namespace

static int sim3d_step(smk_sim3d *sim, int32_t n_steps, float *frames, int64_t fsb, int64_t fst, const float *fractal, float fint,
                      hipStream_t st) {
    // buoyancy + diffusion + divergence (one z-marching launch), the Jacobi sweeps, then the four advections as one z-marching launch that
    // applies the projection's gradient subtraction while it stages its inputs
    const Geom3 &g = sim->g;
    for (int t = 0; t < n_steps; ++t) {
        float *ft = frames ? frames + (size_t)t * fst : nullptr;
        int rc = check_launch(launch3_diffuse_div_march(g, sim->s, sim->t, sim->div, st), "diffuse_div_march3d");
        if (rc) return rc;
        rc = check_launch(launch3_jacobi(g, sim->s.p, sim->t.p, sim->p3, sim->div, sim->jacobi_iters, st), "jacobi3d");
        if (rc) return rc;
        rc = check_launch(launch3_advect_march(g, sim->t, sim->s.p, sim->s, ft, fsb, fractal, fint, st), "advect_march3d");
        if (rc) return rc;
    }
    return SMK_OK;
}

int smk_sim3d_step(smk_sim3d *sim, int32_t n_steps, float *frames, int64_t fsb, int64_t fst, void *stream) {
    SMK_REQUIRE(sim && n_steps >= 0, "null sim / negative n_steps");
    DeviceGuard guard(sim->device);
    if (guard.rc) return guard.rc;
    return sim3d_step(sim, n_steps, frames, fsb, fst, nullptr, 0.f, (hipStream_t)stream);
}

int smk_sim3d_step_emit(smk_sim3d *sim, int32_t n_steps, float *frames, int64_t fsb, int64_t fst, int32_t add_fractal,
                        double fractal_intensity, void *stream) {
    SMK_REQUIRE(sim && n_steps >= 0, "null sim / negative n_steps");
    const bool frac = add_fractal && frames;
    if (frac && sim->g.H != sim->g.W) {
        // fractal_generator.py:44,49 builds its field from field.shape[-2:]: the [w,h] mask indexes an [h,w] buffer
        set_error("fractal perturbation needs a grid that is square in (H, W) (reference raises an IndexError for H != W)");
        return SMK_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    if (guard.rc) return guard.rc;
    float *F = nullptr;
    if (frac)
        if (int rc = cached_fractal_field(sim->g.H, st, &F)) return rc;
    return sim3d_step(sim, n_steps, frames, fsb, fst, F, (float)fractal_intensity, st);
}

int smk_sim3d_run_stage(smk_sim3d *sim, int32_t stage, void *stream) {
    SMK_REQUIRE(sim, "null sim");
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(sim->device);
    if (guard.rc) return guard.rc;
    const Geom3 &g = sim->g;
    const size_t B = g.B;
    State3 &s = sim->s, &t = sim->t;
    // stand-alone stage semantics: caller state in, caller state out -- the stage's inputs are first mirrored into the side it reads
    auto cp = [&](float *dst, const float *src, size_t n) { return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st); };
    int rc;
    switch (stage) {
        case SMK_STAGE3D_BUOY_DIFFUSE:
            rc = run_stage3d(sim, stage, st);
            if (rc) return rc;
            SMK_HIP_TRY(cp(s.u, t.u, B * g.su)); SMK_HIP_TRY(cp(s.v, t.v, B * g.sv)); SMK_HIP_TRY(cp(s.w, t.w, B * g.sw));
            SMK_HIP_TRY(cp(s.d, t.d, B * g.sc));
            return SMK_OK;
        case SMK_STAGE3D_PROJECT:
            SMK_HIP_TRY(cp(t.u, s.u, B * g.su)); SMK_HIP_TRY(cp(t.v, s.v, B * g.sv)); SMK_HIP_TRY(cp(t.w, s.w, B * g.sw));
            rc = run_stage3d(sim, stage, st);
            if (rc) return rc;
            SMK_HIP_TRY(cp(s.u, t.u, B * g.su)); SMK_HIP_TRY(cp(s.v, t.v, B * g.sv)); SMK_HIP_TRY(cp(s.w, t.w, B * g.sw));
            return SMK_OK;
        case SMK_STAGE3D_ADVECT_U:      // reads (u, v, w) -> writes u
            SMK_HIP_TRY(cp(t.u, s.u, B * g.su)); SMK_HIP_TRY(cp(t.v, s.v, B * g.sv)); SMK_HIP_TRY(cp(t.w, s.w, B * g.sw));
            return run_stage3d(sim, stage, st);
        case SMK_STAGE3D_ADVECT_V:      // reads v (field), u (already advected), v, w -> writes v
            SMK_HIP_TRY(cp(t.v, s.v, B * g.sv)); SMK_HIP_TRY(cp(t.w, s.w, B * g.sw));
            return run_stage3d(sim, stage, st);
        case SMK_STAGE3D_ADVECT_W:
            SMK_HIP_TRY(cp(t.w, s.w, B * g.sw));
            return run_stage3d(sim, stage, st);
        case SMK_STAGE3D_ADVECT_D:
            SMK_HIP_TRY(cp(t.d, s.d, B * g.sc));
            return run_stage3d(sim, stage, st);
    }
    set_error("unknown 3-D stage");
    return SMK_ERR_INVALID;
}

int smk_sim3d_describe(smk_sim3d *sim, char *buf, int64_t capacity) {
    SMK_REQUIRE(sim && buf && capacity > 0, "null sim / buf or no capacity");
    const std::string d = "{" + describe3_jacobi(sim->g, sim->s.p, sim->t.p, sim->p3, sim->div, sim->jacobi_iters) +
                          ", \"buoy_diffuse\": \"k3_diffuse_div_march (one form)\", \"advection\": \"k3_advect_march (one form)\"}";
    if ((int64_t)d.size() + 1 > capacity) {
        set_error("smk_sim3d_describe: buffer too small");
        return SMK_ERR_INVALID;
    }
    memcpy(buf, d.c_str(), d.size() + 1);
    return SMK_OK;
}

int smk_conv3d_im2col(const float *src, int32_t C, int32_t D, int32_t H, int32_t W, int32_t ksize, int32_t z0, int32_t nz, float *cols,
                      int32_t kpad, void *stream) {
    SMK_REQUIRE(src && cols, "null src/cols");
    SMK_REQUIRE(C == 1 || C % 4 == 0, "C must be 1 or a multiple of 4");
    SMK_REQUIRE(D >= 1 && H >= 1 && W >= 1 && ksize >= 1 && (ksize & 1), "D, H, W >= 1; ksize odd");
    SMK_REQUIRE(z0 >= 0 && nz >= 1 && z0 + nz <= D, "plane range outside the volume");
    SMK_REQUIRE(kpad >= ksize * ksize * ksize * C && kpad % 4 == 0, "kpad >= ksize^3 * C and a multiple of 4");
    return check_launch(launch_im2col3d(src, C, D, H, W, ksize, z0, nz, cols, kpad, (hipStream_t)stream), "im2col3d");
}

int smk_pool3d_accumulate(const float *act, int32_t C, int32_t H, int32_t W, int32_t nz, float *sums, void *stream) {
    SMK_REQUIRE(act && sums && C >= 1 && nz >= 1, "null act/sums or bad sizes");
    if (H % 32 != 0 || W % 32 != 0) {
        set_error("pool3d: H and W must be multiples of 32 (the two adaptive pools then compose to a block mean)");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(launch_pool3d_accum(act, C, H, W, nz, sums, (hipStream_t)stream), "pool3d_accum");
}

int smk_diffuse(const float *in, float *out, int32_t B, int32_t R, int32_t C, int32_t pitch, double dt, double viscosity,
                void *stream) {
    SMK_REQUIRE(in && out && in != out, "null or aliased in/out");
    SMK_REQUIRE(B >= 1 && R >= 1 && C >= 1 && pitch >= C, "B,R,C >= 1, pitch >= C");
    return check_launch(launch_diffuse(in, out, B, R, C, pitch, (float)(dt * viscosity), (hipStream_t)stream), "diffuse");
}

int smk_apply_fractal(const float *in, float *out, int32_t n_fields, int32_t N, double intensity, void *stream) {
    SMK_REQUIRE(in && out && n_fields >= 1 && N >= 2, "null in/out or bad sizes");
    float *F = nullptr;
    if (int rc = cached_fractal_field(N, (hipStream_t)stream, &F)) return rc;
    return check_launch(launch_apply_fractal(in, out, F, n_fields, N, (float)intensity, (hipStream_t)stream), "apply_fractal");
}

int smk_advect(const float *field, float *out, int32_t which, const float *u, const float *v, int32_t B, int32_t H,
               int32_t W, int32_t pitch_c, int32_t pitch_v, double dt, void *stream) {
    SMK_REQUIRE(field && out && u && v && field != out, "null or aliased pointers");
    SMK_REQUIRE(which >= 0 && which <= 2 && B >= 1 && H >= 2 && W >= 2, "which in 0..2, B>=1, H,W>=2");
    SMK_REQUIRE(pitch_c >= W && pitch_v >= W + 1, "pitch_c >= W and pitch_v >= W+1");
    Geom g{};
    g.B = B; g.H = H; g.W = W; g.pc = pitch_c; g.pv = pitch_v;
    g.su = (size_t)(H + 1) * pitch_c; g.sv = (size_t)H * pitch_v; g.sc = (size_t)H * pitch_c;
    g.dt = (float)dt;
    // which == 2 here is a plain advect (no decay / frame emit): reuse the u/v-style path via a dedicated flag
    return check_launch(launch_advect(g, which == 2 ? 3 : which, field, out, u, v, nullptr, 0, nullptr, 0.f, nullptr,
                                      nullptr, (hipStream_t)stream), "advect");
}

int smk_interpolate(int32_t mode, const float *field, int32_t B, int32_t h, int32_t w, int32_t pitch, int64_t field_stride,
                    const float *y, const float *x, int64_t coord_stride, int64_t n, float *out, void *stream) {
    SMK_REQUIRE(field && y && x && out, "null pointer");
    SMK_REQUIRE(mode >= 0 && mode <= 2, "mode: 0 bilinear_interpolate, 1 interpolate_velocity_u, 2 interpolate_velocity_v");
    SMK_REQUIRE(B >= 1 && B <= 65535 && h >= 1 && w >= 1 && pitch >= w && n >= 0 && field_stride >= 0 && coord_stride >= 0,
                "1 <= B <= 65535, h,w >= 1, pitch >= w, n >= 0");
    SMK_REQUIRE(n < ((int64_t)1 << 38), "n < 2^38 coordinates per field");
    if (n == 0) return SMK_OK;
    return check_launch(launch_interp(mode, field, B, h, w, pitch, (size_t)field_stride, y, x, (size_t)coord_stride, (size_t)n, out,
                                      (hipStream_t)stream), "interpolate");
}

int smk_fractal_constants(int32_t N, float *perlin, float *mandel, float *field, void *stream) {
    SMK_REQUIRE(N >= 2, "N >= 2");
    hipStream_t st = (hipStream_t)stream;
    size_t n = (size_t)N * N;
    float *tmp = nullptr;
    SMK_HIP_TRY(hipMalloc((void **)&tmp, 3 * n * sizeof(float)));
    int rc = check_launch(launch_fractal_constants(N, tmp, tmp + n, tmp + 2 * n, st), "fractal_constants");
    hipError_t e = hipSuccess;
    if (!rc && perlin) e = hipMemcpyAsync(perlin, tmp, n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (!rc && e == hipSuccess && mandel) e = hipMemcpyAsync(mandel, tmp + n, n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (!rc && e == hipSuccess && field) e = hipMemcpyAsync(field, tmp + 2 * n, n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(tmp);
    if (rc) return rc;
    return check_launch(e, "fractal_constants copy");
}

int smk_chaos_stats(const float *frames, int64_t frame_stride, int32_t n, int32_t H, int32_t W, float *means,
                    int32_t *box_counts, int32_t *hist, void *stream) {
    SMK_REQUIRE(frames && means && box_counts && hist, "null pointer");
    SMK_REQUIRE(n >= 1 && H >= 2 && W >= 2 && frame_stride >= (int64_t)H * W, "n>=1, H,W>=2, frame_stride >= H*W");
    if ((int64_t)(H / 2) * (W / 2) > 65536) {
        set_error("chaos_stats: frames larger than 512x512 are not built");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(launch_chaos_stats(frames, frame_stride, n, H, W, means, box_counts, hist, (hipStream_t)stream),
                        "chaos_stats");
}

int smk_frame_diff_norms(const float *frames, int64_t frame_stride, int32_t n, int32_t H, int32_t W, float *norms,
                         void *stream) {
    SMK_REQUIRE(frames && norms && n >= 2 && H >= 1 && W >= 1 && frame_stride >= (int64_t)H * W, "bad arguments");
    return check_launch(launch_diff_norms(frames, frame_stride, n - 1, H * W, norms, (hipStream_t)stream), "diff_norms");
}

int smk_chaos_features(const float *norms, const int32_t *box_counts, const int32_t *hist, int32_t S, const int32_t *pos,
                       const int32_t *hist_len, int32_t F, int32_t n_groups, double *features, double *means, void *stream) {
    SMK_REQUIRE(box_counts && hist && pos && hist_len && features, "null pointer");
    SMK_REQUIRE(S >= 1 && F >= 1 && (norms || S == 1), "S >= 1, F >= 1, norms unless S == 1");
    SMK_REQUIRE(((uintptr_t)hist & 15) == 0 && ((uintptr_t)features & 7) == 0 && ((uintptr_t)means & 7) == 0, "16-byte aligned hist, 8-byte aligned outputs");
    SMK_REQUIRE(n_groups >= 0 && (n_groups == 0 || (means && F % n_groups == 0)), "n_groups > 0 needs means and must divide F");
    return check_launch(launch_chaos_features(norms, box_counts, hist, S, pos, hist_len, F, n_groups, features, means,
                                              (hipStream_t)stream), "chaos_features");
}

static const int64_t VOLUME_STATS_MAX_CELLS = (1LL << 31) - (1LL << 16);

int64_t smk_volume_stats_workspace(int32_t n, int32_t D, int32_t H, int32_t W) {
    if (n < 1 || D < 1 || H < 2 || W < 2 || (int64_t)D * H * W > VOLUME_STATS_MAX_CELLS) return 0;
    return volume_stats_workspace(n, (int64_t)D * H * W);
}

int smk_volume_stats(const float *vols, int64_t vol_stride, int32_t n, int32_t D, int32_t H, int32_t W, float *means,
                     int32_t *box_counts, int32_t *hist, float *norms, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(vols && means && box_counts && hist && workspace, "null pointer");
    SMK_REQUIRE(n >= 1 && D >= 1 && H >= 2 && W >= 2, "n, D >= 1; H, W >= 2");
    SMK_REQUIRE((int64_t)D * H * W <= VOLUME_STATS_MAX_CELLS, "one volume must stay below 2^31 - 2^16 cells (32-bit offsets inside a volume)");
    SMK_REQUIRE(vol_stride >= (int64_t)D * H * W, "vol_stride >= D*H*W");
    SMK_REQUIRE(((uintptr_t)vols & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "4-byte aligned vols, 8-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= smk_volume_stats_workspace(n, D, H, W), "workspace smaller than smk_volume_stats_workspace(n, D, H, W)");
    return check_launch(launch_volume_stats(vols, vol_stride, n, D, H, W, means, box_counts, hist, norms, workspace, (hipStream_t)stream),
                        "volume_stats");
}

// ------------------------------------------------------------------ image quality (SSIM map + squared error)
int64_t smk_image_quality_workspace(int32_t n, int32_t H, int32_t W) {
    if (n < 1 || H < 1 || W < 1) return 0;
    return (int64_t)n * quality_tiles(H, W) * 2 * (int64_t)sizeof(double);
}

int smk_image_quality(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int32_t n, int32_t H,
                      int32_t W, int32_t window, double c1, double c2, void *workspace, int64_t workspace_bytes, double *ssim_sum,
                      double *sqerr_sum, void *stream) {
    SMK_REQUIRE(pred && target && workspace && ssim_sum && sqerr_sum, "null pointer");
    SMK_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1, "1 <= n <= 65535, H, W >= 1");
    SMK_REQUIRE(pred_stride >= (int64_t)H * W && target_stride >= (int64_t)H * W, "plane strides >= H*W");
    SMK_REQUIRE(window >= 1 && window <= QUALITY_MAX_WINDOW && window % 2 == 1, "window: odd, 1..31");
    SMK_REQUIRE(quality_tiles(H, W) <= INT32_MAX, "plane too large");
    SMK_REQUIRE(workspace_bytes >= smk_image_quality_workspace(n, H, W), "workspace smaller than smk_image_quality_workspace(n, H, W)");
    return check_launch(launch_image_quality(pred, pred_stride, target, target_stride, n, H, W, window, (float)c1, (float)c2, workspace,
                                             ssim_sum, sqerr_sum, (hipStream_t)stream),
                        "image_quality");
}

int64_t smk_image_quality_backward_workspace(int32_t n, int32_t H, int32_t W) {
    if (n < 1 || H < 1 || W < 1) return 0;
    return (int64_t)n * H * W * 3 * (int64_t)sizeof(float);
}

int smk_image_quality_backward(const float *pred, int64_t pred_stride, const float *target, int64_t target_stride, int32_t n, int32_t H,
                               int32_t W, int32_t window, double c1, double c2, const float *plane_grad, void *workspace,
                               int64_t workspace_bytes, float *dpred, int64_t dpred_stride, void *stream) {
    SMK_REQUIRE(pred && target && plane_grad && workspace && dpred, "null pointer");
    SMK_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1, "1 <= n <= 65535, H, W >= 1");
    SMK_REQUIRE(pred_stride >= (int64_t)H * W && target_stride >= (int64_t)H * W && dpred_stride >= (int64_t)H * W,
                "plane strides >= H*W");
    SMK_REQUIRE(window >= 1 && window <= QUALITY_MAX_WINDOW && window % 2 == 1, "window: odd, 1..31");
    SMK_REQUIRE(quality_tiles(H, W) <= INT32_MAX, "plane too large");
    SMK_REQUIRE(workspace_bytes >= smk_image_quality_backward_workspace(n, H, W),
                "workspace smaller than smk_image_quality_backward_workspace(n, H, W)");
    return check_launch(launch_image_quality_backward(pred, pred_stride, target, target_stride, n, H, W, window, (float)c1, (float)c2,
                                                      plane_grad, workspace, dpred, dpred_stride, (hipStream_t)stream),
                        "image_quality_backward");
}

// ------------------------------------------------------------------ optical-flow baselines (Farneback, Lucas-Kanade, warp)
namespace {
int check_flow_shape(int32_t n, int32_t H, int32_t W) {
    SMK_REQUIRE(n >= 1 && n <= 65535, "1 <= n <= 65535 frame pairs");
    SMK_REQUIRE(H >= FLOW_MIN_DIM && H <= FLOW_MAX_DIM && W >= FLOW_MIN_DIM && W <= FLOW_MAX_DIM, "32 <= H, W <= 1024");
    return SMK_OK;
}
bool flow_shape_ok(int32_t n, int32_t H, int32_t W) {
    return n >= 1 && n <= 65535 && H >= FLOW_MIN_DIM && H <= FLOW_MAX_DIM && W >= FLOW_MIN_DIM && W <= FLOW_MAX_DIM;
}
}  // namespace

int32_t smk_flow_levels(int32_t H, int32_t W) { return flow_levels(H, W); }

int64_t smk_flow_farneback_workspace(int32_t n, int32_t H, int32_t W) {
    return flow_shape_ok(n, H, W) ? (int64_t)farneback_workspace_bytes(n, H, W) : 0;
}
int64_t smk_warp_workspace(int32_t n, int32_t H, int32_t W) {
    return flow_shape_ok(n, H, W) ? (int64_t)warp_workspace_bytes(n, H, W) : 0;
}
int64_t smk_flow_lk_workspace(int32_t n, int32_t H, int32_t W) {
    return flow_shape_ok(n, H, W) ? (int64_t)lk_workspace_bytes(n, H, W) : 0;
}

int smk_flow_level_image(const uint8_t *frames, int32_t n, int32_t H, int32_t W, int32_t level, float *out, void *workspace,
                         int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(frames && out && workspace, "null pointer");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE(level >= 0 && level < flow_levels(H, W), "level: 0 .. smk_flow_levels(H, W) - 1");
    SMK_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "4-byte aligned out, 8-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= smk_flow_farneback_workspace(n, H, W), "workspace smaller than smk_flow_farneback_workspace(n, H, W)");
    return check_launch(launch_flow_level_image(frames, n, H, W, level, out, workspace, (hipStream_t)stream), "flow_level_image");
}

int smk_flow_poly_exp(const float *img, int32_t n, int32_t h, int32_t w, float *coef, void *stream) {
    SMK_REQUIRE(img && coef, "null pointer");
    if (int rc = check_flow_shape(n, h, w)) return rc;
    SMK_REQUIRE((((uintptr_t)img | (uintptr_t)coef) & 3) == 0, "4-byte aligned img, coef");
    return check_launch(launch_flow_poly_exp(img, n, h, w, coef, (hipStream_t)stream), "flow_poly_exp");
}

int smk_flow_farneback_iteration(const float *coef0, const float *coef1, float *flow, int32_t n, int32_t h, int32_t w, void *workspace,
                                 int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(coef0 && coef1 && flow && workspace, "null pointer");
    if (int rc = check_flow_shape(n, h, w)) return rc;
    SMK_REQUIRE((((uintptr_t)coef0 | (uintptr_t)coef1) & 3) == 0 && ((uintptr_t)flow & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                "4-byte aligned coefficients, 8-byte aligned flow and workspace");
    SMK_REQUIRE(workspace_bytes >= smk_flow_farneback_workspace(n, h, w), "workspace smaller than smk_flow_farneback_workspace(n, h, w)");
    return check_launch(launch_flow_iteration(coef0, coef1, flow, n, h, w, workspace, (hipStream_t)stream), "flow_farneback_iteration");
}

int smk_flow_farneback(const uint8_t *prev, const uint8_t *next, int32_t n, int32_t H, int32_t W, float *flow, void *workspace,
                       int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(prev && next && flow && workspace, "null pointer");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE(((uintptr_t)flow & 7) == 0 && ((uintptr_t)workspace & 255) == 0, "8-byte aligned flow, 256-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= smk_flow_farneback_workspace(n, H, W), "workspace smaller than smk_flow_farneback_workspace(n, H, W)");
    return check_launch(launch_flow_farneback(prev, next, n, H, W, flow, workspace, (hipStream_t)stream), "flow_farneback");
}

int smk_warp_frames(const uint8_t *prev, const float *flow, const uint8_t *next, int32_t n, int32_t H, int32_t W, uint8_t *pred,
                    double *mse, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(prev && flow && pred, "null pointer");
    SMK_REQUIRE((next == nullptr) == (mse == nullptr), "next and mse: both or neither");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE(((uintptr_t)flow & 7) == 0, "8-byte aligned flow");
    if (next) {
        SMK_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)mse & 7) == 0, "workspace and 8-byte aligned mse");
        SMK_REQUIRE(workspace_bytes >= smk_warp_workspace(n, H, W), "workspace smaller than smk_warp_workspace(n, H, W)");
    }
    return check_launch(launch_warp_frames(prev, flow, next, n, H, W, pred, mse, workspace, (hipStream_t)stream), "warp_frames");
}

int smk_flow_min_eigen(const uint8_t *frames, int32_t n, int32_t H, int32_t W, float *eig, void *stream) {
    SMK_REQUIRE(frames && eig, "null pointer");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE(((uintptr_t)eig & 3) == 0, "4-byte aligned eig");
    return check_launch(launch_flow_min_eigen(frames, n, H, W, eig, (hipStream_t)stream), "flow_min_eigen");
}

int smk_good_features(const float *eig, int32_t n, int32_t H, int32_t W, float *pts, int32_t *counts, void *workspace,
                      int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(eig && pts && counts && workspace, "null pointer");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE((((uintptr_t)eig | (uintptr_t)pts | (uintptr_t)counts) & 3) == 0 && ((uintptr_t)workspace & 255) == 0,
                "4-byte aligned eig, pts, counts; 256-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= smk_flow_lk_workspace(n, H, W), "workspace smaller than smk_flow_lk_workspace(n, H, W)");
    return check_launch(launch_good_features(eig, n, H, W, pts, counts, workspace, (hipStream_t)stream), "good_features");
}

int smk_flow_lk_track(const uint8_t *prev, const uint8_t *next, int32_t n, int32_t H, int32_t W, const float *pts, const int32_t *counts,
                      float *out_pts, uint8_t *status, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(prev && next && pts && counts && out_pts && status && workspace, "null pointer");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE((((uintptr_t)pts | (uintptr_t)counts | (uintptr_t)out_pts) & 3) == 0 && ((uintptr_t)workspace & 255) == 0,
                "4-byte aligned pts, counts, out_pts; 256-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= smk_flow_lk_workspace(n, H, W), "workspace smaller than smk_flow_lk_workspace(n, H, W)");
    return check_launch(launch_lk_track(prev, next, n, H, W, pts, counts, out_pts, status, workspace, (hipStream_t)stream), "flow_lk_track");
}

int smk_flow_lk_scatter(const float *pts, const float *out_pts, const uint8_t *status, const int32_t *counts, int32_t n, int32_t H,
                        int32_t W, float *flow, void *stream) {
    SMK_REQUIRE(pts && out_pts && status && counts && flow, "null pointer");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE((((uintptr_t)pts | (uintptr_t)counts | (uintptr_t)out_pts) & 3) == 0 && ((uintptr_t)flow & 7) == 0,
                "4-byte aligned pts, counts, out_pts; 8-byte aligned flow");
    return check_launch(launch_lk_scatter(pts, out_pts, status, counts, n, H, W, flow, (hipStream_t)stream), "flow_lk_scatter");
}

int smk_flow_lucas_kanade(const uint8_t *prev, const uint8_t *next, int32_t n, int32_t H, int32_t W, float *flow, void *workspace,
                          int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(prev && next && flow && workspace, "null pointer");
    if (int rc = check_flow_shape(n, H, W)) return rc;
    SMK_REQUIRE(((uintptr_t)flow & 7) == 0 && ((uintptr_t)workspace & 255) == 0, "8-byte aligned flow, 256-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= smk_flow_lk_workspace(n, H, W), "workspace smaller than smk_flow_lk_workspace(n, H, W)");
    return check_launch(launch_flow_lucas_kanade(prev, next, n, H, W, flow, workspace, (hipStream_t)stream), "flow_lucas_kanade");
}

// ------------------------------------------------------------------ train step tail: gradient norm, AdamW, loss terms
namespace {
int check_opt_table(const smk_opt_tensor *t, int32_t n_tensors, bool adam) {
    SMK_REQUIRE(n_tensors >= 0 && (t || n_tensors == 0), "tensor table: n_tensors >= 0 and a non-null host array");
    for (int32_t i = 0; i < n_tensors; ++i) {
        SMK_REQUIRE(t[i].n >= 0, "tensor table: n >= 0");
        if (t[i].n == 0) continue;
        SMK_REQUIRE(t[i].grad && ((uintptr_t)t[i].grad & 3) == 0, "tensor table: non-null, 4-byte aligned grad");
        if (adam)
            SMK_REQUIRE(t[i].param && t[i].exp_avg && t[i].exp_avg_sq &&
                            (((uintptr_t)t[i].param | (uintptr_t)t[i].exp_avg | (uintptr_t)t[i].exp_avg_sq) & 3) == 0,
                        "tensor table: non-null, 4-byte aligned param, exp_avg, exp_avg_sq");
    }
    const int64_t chunks = opt_chunks(t, n_tensors);
    SMK_REQUIRE(chunks >= 0 && chunks < (int64_t)1 << 30, "tensor table: fewer than 2^30 chunks of 8192 elements");
    return SMK_OK;
}
}  // namespace

int64_t smk_grad_norm_workspace(const smk_opt_tensor *t, int32_t n_tensors) {
    if (!t || n_tensors < 1) return (int64_t)sizeof(double);
    const int64_t chunks = opt_chunks(t, n_tensors);
    return (chunks < 1 ? 1 : chunks) * (int64_t)sizeof(double);
}

int smk_grad_norm(const smk_opt_tensor *t, int32_t n_tensors, double max_norm, float *out, void *workspace, int64_t workspace_bytes,
                  void *stream) {
    if (int rc = check_opt_table(t, n_tensors, false)) return rc;
    SMK_REQUIRE(out && workspace && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 3) == 0, "non-null out, 8-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= smk_grad_norm_workspace(t, n_tensors), "workspace smaller than smk_grad_norm_workspace(t, n_tensors)");
    return check_launch(launch_grad_norm(t, n_tensors, (float)max_norm, out, (double *)workspace, (hipStream_t)stream), "grad_norm");
}

int smk_adamw_step(const smk_opt_tensor *t, int32_t n_tensors, double lr, double beta1, double beta2, double eps, double weight_decay,
                   double bias_correction1, double bias_correction2, const float *grad_scale, int32_t write_grad, void *stream) {
    if (int rc = check_opt_table(t, n_tensors, true)) return rc;
    SMK_REQUIRE(bias_correction1 > 0.0 && bias_correction2 > 0.0, "bias corrections > 0 (step >= 1)");
    AdamCoef c;
    c.lr_wd = (float)(lr * weight_decay);
    c.w1 = (float)(1.0 - beta1);
    c.beta2 = (float)beta2;
    c.w2 = (float)(1.0 - beta2);
    c.step = (float)(lr / bias_correction1);
    c.rsq_bc2 = (float)sqrt(bias_correction2);
    c.eps = (float)eps;
    return check_launch(launch_adamw(t, n_tensors, c, grad_scale, write_grad, (hipStream_t)stream), "adamw_step");
}

namespace {
int loss_shape(LossShape &s, int32_t planes, int32_t plane_elems, int32_t n_chaos, int32_t seq_batch, int32_t seq_T, int64_t seq_plane) {
    SMK_REQUIRE(planes >= 1 && plane_elems >= 1 && n_chaos >= 1, "planes, plane_elems, n_chaos >= 1");
    SMK_REQUIRE(seq_batch >= 0 && seq_T >= 0 && seq_plane >= 0, "sequence dimensions >= 0");
    s.planes = planes;
    s.plane_elems = plane_elems;
    s.n_chaos = n_chaos;
    s.seq_batch = seq_batch;
    s.seq_T = seq_T;
    s.seq_plane = seq_plane;
    SMK_REQUIRE((int64_t)planes * loss_plane_chunks(plane_elems) < (int64_t)1 << 30, "pred: fewer than 2^30 chunks of 2048 elements");
    SMK_REQUIRE((int64_t)seq_batch * loss_seq_chunks(seq_plane) < (int64_t)1 << 30, "sequence: fewer than 2^30 chunks of 1024 pixels");
    return SMK_OK;
}
}  // namespace

int64_t smk_train_loss_workspace(int32_t planes, int32_t plane_elems, int32_t seq_batch, int32_t seq_T, int64_t seq_plane) {
    LossShape s;
    if (loss_shape(s, planes, plane_elems, 1, seq_batch, seq_T, seq_plane) != SMK_OK) return 0;
    return loss_workspace_doubles(s) * (int64_t)sizeof(double);
}

int smk_train_loss_forward(const float *pred, const float *target, int32_t planes, int32_t plane_elems, const float *chaos_pred,
                           const float *chaos_target, int32_t n_chaos, const float *sequence, int32_t seq_batch, int32_t seq_T,
                           int64_t seq_plane, double w_chaos, double w_physics, double w_mass, double w_continuity, float *out,
                           float *mass_diff, void *workspace, int64_t workspace_bytes, void *stream) {
    LossShape s;
    if (int rc = loss_shape(s, planes, plane_elems, n_chaos, sequence ? seq_batch : 0, seq_T, seq_plane)) return rc;
    SMK_REQUIRE(pred && target && chaos_pred && chaos_target && out && mass_diff && workspace, "null pointer");
    SMK_REQUIRE((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)chaos_pred | (uintptr_t)chaos_target | (uintptr_t)sequence |
                  (uintptr_t)out | (uintptr_t)mass_diff) & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
                "4-byte aligned tensors, 16-byte aligned workspace");
    SMK_REQUIRE(workspace_bytes >= loss_workspace_doubles(s) * (int64_t)sizeof(double), "workspace smaller than smk_train_loss_workspace(...)");
    return check_launch(launch_train_loss_forward(pred, target, chaos_pred, chaos_target, sequence, s, w_chaos, w_physics, w_mass,
                                                  w_continuity, out, mass_diff, (double *)workspace, (hipStream_t)stream),
                        "train_loss_forward");
}

int smk_train_loss_backward(const float *pred, const float *target, int32_t planes, int32_t plane_elems, const float *mass_diff,
                            const float *chaos_pred, const float *chaos_target, int32_t n_chaos, const float *grad_out, double w_chaos,
                            double w_physics, double w_mass, float *d_pred, float *d_chaos, void *stream) {
    LossShape s;
    if (int rc = loss_shape(s, planes, plane_elems, n_chaos, 0, 0, 0)) return rc;
    SMK_REQUIRE(pred && target && mass_diff && chaos_pred && chaos_target && grad_out, "null pointer");
    SMK_REQUIRE((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)chaos_pred | (uintptr_t)chaos_target | (uintptr_t)mass_diff |
                  (uintptr_t)grad_out | (uintptr_t)d_pred | (uintptr_t)d_chaos) & 3) == 0, "4-byte aligned tensors");
    return check_launch(launch_train_loss_backward(pred, target, mass_diff, chaos_pred, chaos_target, s, grad_out, w_chaos, w_physics,
                                                   w_mass, d_pred, d_chaos, (hipStream_t)stream),
                        "train_loss_backward");
}

// ------------------------------------------------------------------ encoder
int smk_encoder_create(const smk_encoder_weights *w, int32_t device_id, void *stream, smk_encoder **out) {
    SMK_REQUIRE(w && out, "null weights/out");
    const float *const *pp = (const float *const *)w;
    for (size_t k = 0; k < sizeof(*w) / sizeof(float *); ++k) SMK_REQUIRE(pp[k], "null weight pointer");
    DeviceGuard guard(device_id);
    int rc = guard.rc;
    if (rc) return rc;
    smk_encoder *enc = new smk_encoder();
    enc->device = device_id;
    const size_t n = 64 * 49 + 64 + 64 + 9 * 64 * 128 + 128 + 128 + 128 + 256;
    hipError_t e = hipMalloc((void **)&enc->blob, n * sizeof(float));
    if (e != hipSuccess) {
        delete enc;
        set_error(std::string("smk_encoder_create: ") + hipGetErrorString(e));
        return SMK_ERR_HIP;
    }
    float *p = enc->blob;
    enc->e.w2t = p; p += 9 * 64 * 128;     // 16-byte aligned first
    enc->e.w1 = p; p += 64 * 49;
    enc->e.s1 = p; p += 64;
    enc->e.t1 = p; p += 64;
    enc->e.s2 = p; p += 128;
    enc->e.t2 = p; p += 128;
    enc->e.sw2 = p; p += 128;
    enc->e.wsum = reinterpret_cast<int *>(p);
    const size_t n16 = 2 * 64 * 64 + 2 * (36 * 2 * 128 * 16) + 18 * 2 * 128 * 32 / 2;   // + int8 limbs (bytes / 2)
    e = hipMalloc((void **)&enc->blob16, n16 * sizeof(unsigned short));
    if (e != hipSuccess) {
        smk_encoder_destroy(enc);
        set_error(std::string("smk_encoder_create: ") + hipGetErrorString(e));
        return SMK_ERR_HIP;
    }
    enc->e.w2q = enc->blob16;                       // 16-byte aligned rows first
    enc->e.w2s = enc->blob16 + 36 * 2 * 128 * 16;
    enc->e.w1p = enc->blob16 + 2 * (36 * 2 * 128 * 16);
    enc->e.w2i = reinterpret_cast<signed char *>(enc->blob16 + 2 * (36 * 2 * 128 * 16) + 2 * 64 * 64);
    rc = check_launch(launch_fold_weights(*w, enc->e, (hipStream_t)stream), "fold_weights");
    if (rc) { smk_encoder_destroy(enc); return rc; }
    *out = enc;
    return SMK_OK;
}

int smk_encoder_destroy(smk_encoder *enc) {
    if (!enc) return SMK_OK;
    DeviceGuard guard(enc->device);              // frees run on the handle's device; the caller's device is restored
    if (enc->blob) (void)hipFree(enc->blob);
    if (enc->blob16) (void)hipFree(enc->blob16);
    enc->skip.release();
    enc->partials.release();
    delete enc;
    return SMK_OK;
}

static int encoder_shape_ok(int32_t B, int32_t H, int32_t W, int32_t input_dim) {
    SMK_REQUIRE(B >= 1, "B >= 1");
    if (H != W || (H != 64 && H != 128 && H != 256 && H != 512 && H != 1024)) {
        set_error("encoder: HIP path is built for square frames of 64, 128, 256, 512 or 1024");
        return SMK_ERR_UNSUPPORTED;
    }
    if (input_dim <= 0 || input_dim % 32 != 0 || (input_dim % H != 0 && H % input_dim != 0)) {
        set_error("encoder: input_dim must be a multiple of 32 and a multiple or divisor of H (pools must compose to a block mean)");
        return SMK_ERR_UNSUPPORTED;
    }
    return SMK_OK;
}

// The handle's partial buffer for this call (null in *out for H <= 256, where a pooled cell lies inside one tile).
static int encoder_partials(smk_encoder *enc, int32_t B, int32_t H, int32_t W, void *stream, float **out) {
    const hipError_t e = enc->partials.acquire(B, H, W, (hipStream_t)stream, out);
    if (e == hipErrorStreamCaptureUnsupported) {
        set_error("encoder: the stream is capturing and the handle's partial-sum buffer for frames of 512 or 1024 is missing or too small; "
                  "run one eager forward of the same shape before the capture (nothing is allocated inside a capture)");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(e, "encoder_partials");
}

int smk_encoder_forward(smk_encoder *enc, const float *frames, int64_t frame_stride, int32_t B, int32_t H, int32_t W,
                        int32_t input_dim, float *features, int32_t dtype, void *stream) {
    SMK_REQUIRE(enc && frames && features, "null enc/frames/features");
    SMK_REQUIRE(frame_stride >= (int64_t)H * W, "frame_stride >= H*W");
    int rc = encoder_shape_ok(B, H, W, input_dim);
    if (rc) return rc;
    DeviceGuard guard(enc->device);
    rc = guard.rc;
    if (rc) return rc;
    if (dtype != SMK_F32 && dtype != SMK_BF16X3 && dtype != SMK_BF16 && dtype != SMK_I8X3) {
        set_error("unknown encoder dtype");
        return SMK_ERR_INVALID;
    }
    float *part = nullptr;
    if ((rc = encoder_partials(enc, B, H, W, stream, &part))) return rc;
    if (dtype == SMK_F32)
        return check_launch(launch_encoder_f32(frames, frame_stride, B, H, W, enc->e, features, (hipStream_t)stream, part), "encoder_f32");
    if (dtype == SMK_BF16X3 || dtype == SMK_BF16)
        return check_launch(launch_encoder_bf16(frames, frame_stride, B, H, W, enc->e, features, dtype == SMK_BF16X3, false,
                                                (hipStream_t)stream, &enc->skip, part), "encoder_bf16");
    if (dtype == SMK_I8X3)
        return check_launch(launch_encoder_i8(frames, frame_stride, B, H, W, enc->e, features, false, (hipStream_t)stream, &enc->skip, part),
                            "encoder_i8");
    set_error("unknown encoder dtype");
    return SMK_ERR_INVALID;
}

int smk_encoder_forward_tokens(smk_encoder *enc, const float *frames, int64_t frame_stride, int32_t B, int32_t H,
                               int32_t W, int32_t input_dim, float *tokens, int32_t dtype, void *stream) {
    SMK_REQUIRE(enc && frames && tokens, "null enc/frames/tokens");
    SMK_REQUIRE(frame_stride >= (int64_t)H * W, "frame_stride >= H*W");
    int rc = encoder_shape_ok(B, H, W, input_dim);
    if (rc) return rc;
    DeviceGuard guard(enc->device);
    rc = guard.rc;
    if (rc) return rc;
    if (dtype != SMK_BF16X3 && dtype != SMK_BF16 && dtype != SMK_I8X3) {
        set_error("token-major output is built for the MFMA kernels SMK_BF16X3, SMK_BF16, SMK_I8X3");
        return SMK_ERR_UNSUPPORTED;
    }
    float *part = nullptr;
    if ((rc = encoder_partials(enc, B, H, W, stream, &part))) return rc;
    if (dtype == SMK_I8X3)
        return check_launch(launch_encoder_i8(frames, frame_stride, B, H, W, enc->e, tokens, true, (hipStream_t)stream, &enc->skip, part),
                            "encoder_i8_tokens");
    return check_launch(launch_encoder_bf16(frames, frame_stride, B, H, W, enc->e, tokens, dtype == SMK_BF16X3, true,
                                            (hipStream_t)stream, &enc->skip, part), "encoder_bf16_tokens");
}

int smk_encoder_skip_stats(smk_encoder *enc, int64_t *tiles_total, int64_t *tiles_run, void *stream) {
    SMK_REQUIRE(enc && tiles_total && tiles_run, "null enc/tiles_total/tiles_run");
    DeviceGuard guard(enc->device);
    if (guard.rc) return guard.rc;
    return check_launch(encoder_skip_stats(enc->skip, tiles_total, tiles_run, (hipStream_t)stream), "encoder_skip_stats");
}

int smk_encoder_conv1(smk_encoder *enc, const float *frames, int64_t frame_stride, int32_t B, int32_t H, int32_t W,
                      float *act, void *stream) {
    SMK_REQUIRE(enc && frames && act && B >= 1 && H >= 1 && W >= 1, "null enc/frames/act or bad shape");
    DeviceGuard guard(enc->device);
    int rc = guard.rc;
    if (rc) return rc;
    return check_launch(launch_conv1_only(frames, frame_stride, B, H, W, enc->e, act, (hipStream_t)stream), "conv1");
}

// ------------------------------------------------------------------ transformer-body linear layers
int smk_linear_create(const float *weight, const float *bias, int32_t out_features, int32_t in_features,
                      int32_t device_id, void *stream, smk_linear **out) {
    SMK_REQUIRE(weight && out, "null weight/out");
    SMK_REQUIRE(out_features >= 1 && in_features >= 1, "positive feature counts");
    if (in_features % 64 != 0 || out_features % 32 != 0 || (int64_t)in_features * out_features > (1 << 28)) {
        set_error("linear: HIP path is built for in_features % 64 == 0, out_features % 32 == 0, at most 2^28 weights");
        return SMK_ERR_UNSUPPORTED;
    }
    DeviceGuard guard(device_id);
    int rc = guard.rc;
    if (rc) return rc;
    smk_linear *lin = new smk_linear();
    lin->device = device_id;
    lin->l.N = out_features;
    lin->l.K = in_features;
    lin->l.wq = nullptr;
    lin->l.bias = nullptr;
    hipError_t e = hipMalloc((void **)&lin->l.wq, (size_t)in_features * out_features * 2 * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMalloc((void **)&lin->l.bias, (size_t)out_features * sizeof(float));
    if (e != hipSuccess) {
        smk_linear_destroy(lin);
        set_error(std::string("smk_linear_create: ") + hipGetErrorString(e));
        return SMK_ERR_HIP;
    }
    rc = check_launch(launch_split_linear_weights(weight, bias, lin->l, (hipStream_t)stream), "split_linear_weights");
    if (rc) { smk_linear_destroy(lin); return rc; }
    *out = lin;
    return SMK_OK;
}

int smk_linear_destroy(smk_linear *lin) {
    if (!lin) return SMK_OK;
    DeviceGuard guard(lin->device);              // frees run on the handle's device; the caller's device is restored
    if (lin->l.wq) (void)hipFree(lin->l.wq);
    if (lin->l.bias) (void)hipFree(lin->l.bias);
    delete lin;
    return SMK_OK;
}

int smk_linear_update(smk_linear *lin, const float *weight, int32_t transposed, const float *bias, void *stream) {
    SMK_REQUIRE(lin && weight, "null lin/weight");
    SMK_REQUIRE(transposed == 0 || transposed == 1, "transposed is 0 or 1");
    DeviceGuard guard(lin->device);
    int rc = guard.rc;
    if (rc) return rc;
    return check_launch(launch_split_linear_weights(weight, bias, lin->l, (hipStream_t)stream, transposed), "split_linear_weights");
}

int64_t smk_linear_wgrad_workspace(int64_t rows, int32_t out_features, int32_t in_features) {
    if (rows < 1 || out_features < 1 || in_features < 1) return 0;
    return (int64_t)plan_linear_wgrad(rows, out_features, in_features).bytes;
}

int smk_linear_wgrad(const float *dy, int64_t ld_dy, const float *x, int64_t ldx, int64_t rows, int32_t out_features,
                     int32_t in_features, float *dw, float *db, void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(dy && x && dw && workspace, "null dy/x/dw/workspace");
    SMK_REQUIRE(rows >= 1 && out_features >= 1 && in_features >= 1, "positive sizes");
    if (in_features % 32 != 0 || out_features % 4 != 0) {
        set_error("linear_wgrad: HIP path is built for in_features % 32 == 0, out_features % 4 == 0");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(ld_dy >= out_features && ldx >= in_features, "row pitches >= feature counts");
    SMK_REQUIRE((int64_t)(out_features + 256) * (rows + 4096) < (1LL << 30), "(out_features + 256) * (rows + 4096) < 2^30: chunk the rows");
    SMK_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)dw & 15) == 0, "workspace / dw 16-byte aligned");
    SMK_REQUIRE(workspace_bytes >= smk_linear_wgrad_workspace(rows, out_features, in_features), "workspace too small");
    return check_launch(launch_linear_wgrad(dy, ld_dy, x, ldx, rows, out_features, in_features, dw, db, workspace, (hipStream_t)stream),
                        "linear_wgrad");
}

int smk_linear_forward(smk_linear *lin, const void *x, int64_t rows, int64_t ldx, void *y, int64_t ldy,
                       const float *residual, int64_t ldr, const float *periodic_add, int32_t rows_per_group,
                       int32_t period, int32_t activation, int32_t x_format, int32_t y_format, void *stream) {
    SMK_REQUIRE(lin && x && y, "null lin/x/y");
    SMK_REQUIRE(rows >= 1 && rows < (1LL << 31) - 256, "1 <= rows < 2^31 - 256");
    SMK_REQUIRE(ldx >= lin->l.K && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0, "x rows: pitch >= in_features, 16-byte aligned");
    SMK_REQUIRE((rows + 256) * ldx < (1LL << 30), "x: (rows + 256) * ldx < 2^30 floats (32-bit buffer offsets)");
    SMK_REQUIRE(ldy >= lin->l.N && ldy % 4 == 0 && ((uintptr_t)y & 15) == 0, "y rows: pitch >= out_features, 16-byte aligned");
    SMK_REQUIRE(!residual || (ldr >= lin->l.N && ldr % 4 == 0 && ((uintptr_t)residual & 15) == 0),
                "residual rows: pitch >= out_features, 16-byte aligned");
    SMK_REQUIRE(!periodic_add || ((uintptr_t)periodic_add & 15) == 0, "periodic_add 16-byte aligned");
    SMK_REQUIRE(activation == SMK_ACT_NONE || activation == SMK_ACT_GELU || activation == SMK_ACT_RELU, "activation");
    SMK_REQUIRE(!(residual && periodic_add), "residual and periodic_add are exclusive (no layer of the path needs both)");
    SMK_REQUIRE((x_format == SMK_FMT_F32 || x_format == SMK_FMT_SPLIT_BF16) && (y_format == SMK_FMT_F32 || y_format == SMK_FMT_SPLIT_BF16),
                "x_format / y_format");
    SMK_REQUIRE(x_format == SMK_FMT_F32 || ldx == lin->l.K, "split x: dense rows (ldx == in_features)");
    SMK_REQUIRE(y_format == SMK_FMT_F32 || (ldy == lin->l.N && !residual), "split y: dense rows (ldy == out_features), no residual");
    if (periodic_add)
        SMK_REQUIRE(period >= 1 && rows_per_group >= 32 && rows_per_group % 32 == 0 && rows % rows_per_group == 0,
                    "periodic_add: period >= 1, rows_per_group a multiple of 32 that divides rows");
    DeviceGuard guard(lin->device);
    int rc = guard.rc;
    if (rc) return rc;
    LinearCall c;
    c.x = (const float *)x; c.ldx = ldx;
    c.y = (float *)y; c.ldy = ldy;
    c.x_split = x_format == SMK_FMT_SPLIT_BF16; c.y_split = y_format == SMK_FMT_SPLIT_BF16;
    c.res = residual; c.ldr = ldr;
    c.padd = periodic_add; c.rows_per_group = periodic_add ? rows_per_group : 1; c.period = periodic_add ? period : 1;
    c.M = (int)rows;
    c.act = activation;
    return check_launch(launch_linear_x3(lin->l, c, (hipStream_t)stream), "linear_x3");
}

int64_t smk_linear_ln_max_rows(smk_linear *lin) {
    if (!lin) return 0;
    DeviceGuard guard(lin->device);
    if (guard.rc) return 0;
    // (round 3: one tile per workgroup, i.e. 2 CUs / column tiles x 32 rows.)  The statistics now follow the chunk stream across the tiles a
    // workgroup walks, so the only bound is the 32-bit offset range of the activation buffer
    // the largest rows with (rows + 256) * K < 2^30 (smk_linear_forward_ln_split's check, strict); none for K > 2^22
    const int64_t r = ((1LL << 30) - 1) / lin->l.K - 256;
    return r > 0 ? r : 0;
}

int smk_linear_forward_ln(smk_linear *lin, const float *x, int64_t rows, int64_t ldx, float *y, int64_t ldy, const float *wsum, double eps,
                          const float *periodic_add, int32_t rows_per_group, int32_t period, int32_t activation, void *stream) {
    return smk_linear_forward_ln_split(lin, x, rows, ldx, y, ldy, wsum, eps, periodic_add, rows_per_group, period, activation, -1, stream);
}

int smk_linear_forward_ln_split(smk_linear *lin, const float *x, int64_t rows, int64_t ldx, float *y, int64_t ldy, const float *wsum, double eps,
                                const float *periodic_add, int32_t rows_per_group, int32_t period, int32_t activation, int32_t split_from_col,
                                void *stream) {
    SMK_REQUIRE(lin && x && y && wsum, "null lin/x/y/wsum");
    SMK_REQUIRE(split_from_col < 0 || (split_from_col % 32 == 0 && split_from_col < lin->l.N), "split_from_col: negative (none) or a multiple of 32 below out_features");
    SMK_REQUIRE(rows >= 1 && ldx >= lin->l.K && ldy >= lin->l.N && ldx % 4 == 0 && ldy % 4 == 0, "rows >= 1, row pitches >= features, multiples of 4");
    SMK_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)wsum) & 15) == 0, "16-byte aligned x / y / wsum");
    SMK_REQUIRE((rows + 256) * ldx < (1LL << 30), "(rows + 256) * ldx < 2^30 floats");
    SMK_REQUIRE(activation == SMK_ACT_NONE || activation == SMK_ACT_GELU || activation == SMK_ACT_RELU, "activation");
    SMK_REQUIRE(!periodic_add || (rows_per_group >= 32 && rows_per_group % 32 == 0 && period >= 1 && rows % rows_per_group == 0),
                "periodic_add: rows_per_group a multiple of 32 that divides rows, period >= 1");
    SMK_REQUIRE(eps > 0.0, "eps > 0");
    DeviceGuard guard(lin->device);
    if (guard.rc) return guard.rc;
    LinearCall c;
    c.x = x; c.ldx = ldx; c.y = y; c.ldy = ldy; c.x_split = 0; c.y_split = 0; c.res = nullptr; c.ldr = 0;
    c.padd = periodic_add; c.rows_per_group = periodic_add ? rows_per_group : 1; c.period = periodic_add ? period : 1;
    c.M = (int)rows; c.act = activation;
    c.ln_wsum = wsum; c.ln_eps = (float)eps;
    c.split_from = split_from_col < 0 ? -1 : split_from_col;
    return check_launch(launch_linear_x3(lin->l, c, (hipStream_t)stream), "linear_x3 (fused LayerNorm)");
}

int smk_conv3d_cl_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t nz, float *y, int64_t ldy,
                          int32_t activation, void *stream) {
    SMK_REQUIRE(lin && src && y, "null lin/src/y");
    SMK_REQUIRE(lin->l.K == 27 * 64, "the layer handle must have in_features = 27 * 64 (3 x 3 x 3 taps of 64 channels)");
    SMK_REQUIRE(D >= 1 && H >= 1 && W >= 1 && z0 >= 0 && nz >= 1 && z0 + nz <= D, "plane range outside the volume");
    SMK_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)y & 15) == 0 && ldy >= lin->l.N && ldy % 4 == 0, "16-byte aligned src / y, ldy >= out_features");
    SMK_REQUIRE((int64_t)(nz + 2) * H * W * 256 < (1LL << 32) - 256 && (int64_t)nz * H * W < (1LL << 31) - 256, "slab too large for 32-bit offsets: fewer planes per call");
    SMK_REQUIRE(activation == SMK_ACT_NONE || activation == SMK_ACT_GELU || activation == SMK_ACT_RELU, "activation");
    DeviceGuard guard(lin->device);
    if (guard.rc) return guard.rc;
    const int zlo = z0 > 0 ? z0 - 1 : 0, zhi = z0 + nz + 1 < D ? z0 + nz + 1 : D;
    return check_launch(launch_conv3d_cl_b16(lin->l, src + (size_t)zlo * H * W * 64, zhi - zlo, H, W, z0 - zlo, nz, y, ldy, activation,
                                             (hipStream_t)stream), "conv3d_cl_b16");
}

int smk_conv3d_cl_zsum_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, float *zsum, int32_t activation, void *stream) {
    SMK_REQUIRE(lin && src && zsum, "null lin/src/zsum");
    SMK_REQUIRE(lin->l.K == 27 * 64 && lin->l.N == 128, "the layer handle must be 27 * 64 -> 128 (3 x 3 x 3 taps of 64 channels, 128 outputs)");
    SMK_REQUIRE(D >= 1 && H >= 8 && W >= 16 && H % 8 == 0 && W % 16 == 0, "H must be a multiple of 8 and W of 16 (the 8 x 16 voxel column a workgroup marches)");
    SMK_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)zsum & 15) == 0, "16-byte aligned src / zsum");
    SMK_REQUIRE((int64_t)H * W * 256 < (1LL << 31), "a plane must stay below 2^31 bytes (32-bit offsets within a plane)");
    SMK_REQUIRE(activation == SMK_ACT_NONE || activation == SMK_ACT_RELU, "activation: none or ReLU");
    DeviceGuard guard(lin->device);
    if (guard.rc) return guard.rc;
    return check_launch(launch_conv3d_march(lin->l, src, D, H, W, zsum, activation, (hipStream_t)stream), "conv3d_march");
}

int smk_conv3d_s7_march_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, float *a1, int32_t activation, void *stream) {
    SMK_REQUIRE(lin && src && a1, "null lin/src/a1");
    SMK_REQUIRE(lin->l.K == 448 && lin->l.N == 64, "the layer handle must be 448 -> 64 (7 kz x 8 ky slots x 8 kx slots, 64 outputs)");
    SMK_REQUIRE(D >= 1 && H >= 8 && W >= 16 && H % 8 == 0 && W % 16 == 0, "H must be a multiple of 8 and W of 16 (the 8 x 16 voxel column a workgroup marches)");
    SMK_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)a1 & 15) == 0, "aligned src / a1");
    SMK_REQUIRE((int64_t)H * W * 256 < (1LL << 31), "a plane of the output must stay below 2^31 bytes");
    SMK_REQUIRE(activation == SMK_ACT_NONE || activation == SMK_ACT_RELU, "activation: none or ReLU");
    DeviceGuard guard(lin->device);
    if (guard.rc) return guard.rc;
    return check_launch(launch_conv3d_s7_march(lin->l, src, D, H, W, a1, activation, (hipStream_t)stream), "conv3d_s7_march");
}

int smk_conv3d_s7_forward(smk_linear *lin, const float *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t nz, float *y, int64_t ldy,
                          int32_t activation, void *stream) {
    SMK_REQUIRE(lin && src && y, "null lin/src/y");
    SMK_REQUIRE(lin->l.K == 448, "the layer handle must have in_features = 448 (56 window rows x 8 kx slots)");
    SMK_REQUIRE(D >= 1 && H >= 1 && W >= 1 && H <= 1023 && W <= 1023 && z0 >= 0 && nz >= 1 && z0 + nz <= D, "plane range outside the volume, or H / W > 1023");
    SMK_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)y & 15) == 0 && ldy >= lin->l.N && ldy % 4 == 0, "aligned src / y, ldy >= out_features");
    SMK_REQUIRE((int64_t)(nz + 6) * H * W * 4 < (1LL << 32) - 256 && nz + 6 <= 1022 && (int64_t)nz * H * W < (1LL << 31) - 256, "slab too large: fewer planes per call");
    SMK_REQUIRE(activation == SMK_ACT_NONE || activation == SMK_ACT_GELU || activation == SMK_ACT_RELU, "activation");
    DeviceGuard guard(lin->device);
    if (guard.rc) return guard.rc;
    const int zlo = z0 > 3 ? z0 - 3 : 0, zhi = z0 + nz + 3 < D ? z0 + nz + 3 : D;
    return check_launch(launch_conv3d_s7_b16(lin->l, src + (size_t)zlo * H * W, zhi - zlo, H, W, z0 - zlo, nz, y, ldy, activation,
                                             (hipStream_t)stream), "conv3d_s7_b16");
}

// ------------------------------------------------------------------ chaos term of ChaosAttention
int smk_chaos_addend(const float *noise, int32_t B, int32_t D, const float *proj_w, const float *proj_b,
                     const float *gate_w, const float *gate_b, double strength, double sigma, double rho, double beta,
                     double dt, float *addend, int64_t ld_addend, void *stream) {
    SMK_REQUIRE(noise && proj_w && proj_b && gate_w && gate_b && addend, "null pointer");
    SMK_REQUIRE(B >= 1 && D >= 1 && ld_addend >= D && ld_addend < (1LL << 30), "B >= 1, D >= 1, ld_addend >= D");
    ChaosAddendArgs a;
    a.noise = noise; a.proj_w = proj_w; a.proj_b = proj_b; a.gate_w = gate_w; a.gate_b = gate_b; a.addend = addend;
    a.B = B; a.D = D; a.ld = (int)ld_addend;
    a.strength = (float)strength; a.sigma = (float)sigma; a.rho = (float)rho; a.beta = (float)beta; a.dt = (float)dt;
    return check_launch(launch_chaos_addend(a, (hipStream_t)stream), "chaos_addend");
}

int smk_chaos_addend_batched(int32_t n_layers, const smk_chaos_layer *layers, int32_t B, int32_t D, double sigma, double rho, double beta,
                             double dt, void *stream) {
    SMK_REQUIRE(layers && n_layers >= 1 && n_layers <= 8, "1 .. 8 layers");
    SMK_REQUIRE(B >= 1 && D >= 1, "B >= 1, D >= 1");
    ChaosAddendBatch a;
    a.NL = n_layers;
    for (int i = 0; i < n_layers; ++i) {
        const smk_chaos_layer &l = layers[i];
        SMK_REQUIRE(l.noise && l.proj_w && l.proj_b && l.gate_w && l.gate_b && l.addend, "null pointer in a layer");
        SMK_REQUIRE(l.ld_addend >= D && l.ld_addend < (1LL << 30), "ld_addend >= D");
        ChaosAddendArgs &x = a.layer[i];
        x.noise = l.noise; x.proj_w = l.proj_w; x.proj_b = l.proj_b; x.gate_w = l.gate_w; x.gate_b = l.gate_b; x.addend = l.addend;
        x.B = B; x.D = D; x.ld = (int)l.ld_addend;
        x.strength = (float)l.strength; x.sigma = (float)sigma; x.rho = (float)rho; x.beta = (float)beta; x.dt = (float)dt;
    }
    for (int i = n_layers; i < 8; ++i) a.layer[i] = a.layer[0];
    return check_launch(launch_chaos_addend_batch(a, (hipStream_t)stream), "chaos_addend_batch");
}

int smk_pooled_head(const float *x, int32_t B, int32_t L, int32_t D, int64_t ldx, const float *w1, const float *b1, int32_t H1,
                    const float *w2, const float *b2, int32_t H2, float *pooled, float *out, float *workspace, void *stream) {
    SMK_REQUIRE(x && w1 && b1 && w2 && b2 && pooled && out && workspace, "null pointer");
    SMK_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && D >= 1 && H1 >= 1 && H2 >= 1 && ldx >= D, "B in 1 .. 65535, L, D, H1, H2 >= 1, ldx >= D");
    SMK_REQUIRE((int64_t)D * 4 <= 64 * 1024 && D % 4 == 0 && (H1 + 31) / 32 <= 65535, "D <= 16,384 (the pooled vector sits in LDS), D % 4 == 0");
    SMK_REQUIRE(((uintptr_t)w1 & 15) == 0, "16-byte aligned w1");
    PooledHeadArgs a;
    a.x = x; a.ldx = ldx; a.B = B; a.L = L; a.D = D; a.w1 = w1; a.b1 = b1; a.H1 = H1; a.w2 = w2; a.b2 = b2; a.H2 = H2;
    a.pooled = pooled; a.out = out; a.ws = workspace;
    return check_launch(launch_pooled_head(a, (hipStream_t)stream), "pooled_head");
}

int smk_lorenz_states(const float *noise, int32_t B, double sigma, double rho, double beta, double dt, float *states, void *stream) {
    SMK_REQUIRE(noise && states && B >= 1, "null noise / states or B < 1");
    return check_launch(launch_lorenz_states(noise, B, (float)sigma, (float)rho, (float)beta, (float)dt, states, (hipStream_t)stream), "lorenz_states");
}

// ------------------------------------------------------------------ element-wise chain of the FFN block in training
int smk_ffn_elementwise(int32_t op, const float *a, const float *b, float *out, int64_t n, double p, uint64_t seed, void *stream) {
    SMK_REQUIRE(a && out && n >= 0, "null a / out or negative n");
    SMK_REQUIRE(op >= SMK_ELT_GELU_DROPOUT_FWD && op <= SMK_ELT_DROPOUT_BWD, "op: smk_elt_op");
    SMK_REQUIRE((op != SMK_ELT_GELU_DROPOUT_BWD && op != SMK_ELT_DROPOUT_ADD_FWD) || b, "this op needs the second operand");
    SMK_REQUIRE(p >= 0.0 && p < 1.0, "0 <= p < 1");
    if (n % 4 != 0) {
        set_error("ffn_elementwise: HIP path is built for element counts that are multiples of 4");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0, "16-byte aligned tensors");
    if (n == 0) return SMK_OK;
    EltArgs e{a, b, out, (long long)n, (float)p, (unsigned long long)seed};
    hipStream_t st = (hipStream_t)stream;
    switch (op) {
        case SMK_ELT_GELU_DROPOUT_FWD: return check_launch(launch_gelu_dropout_fwd(e, st), "gelu_dropout_fwd");
        case SMK_ELT_GELU_DROPOUT_BWD: return check_launch(launch_gelu_dropout_bwd(e, st), "gelu_dropout_bwd");
        case SMK_ELT_DROPOUT_ADD_FWD: return check_launch(launch_dropout_add_fwd(e, st), "dropout_add_fwd");
        default: return check_launch(launch_dropout_bwd(e, st), "dropout_bwd");
    }
}

int smk_reduce_shards(const void *shards, int32_t in_dtype, int32_t world, int64_t n, int64_t stride, void *out, int32_t out_dtype, void *stream) {
    SMK_REQUIRE(shards && out && n >= 0 && world >= 1, "null shards / out, negative n or world < 1");
    SMK_REQUIRE((in_dtype == SMK_WIRE_F32 || in_dtype == SMK_WIRE_BF16) && (out_dtype == SMK_WIRE_F32 || out_dtype == SMK_WIRE_BF16), "dtype: smk_wire_dtype");
    SMK_REQUIRE(world == 1 || (stride >= n && stride % 4 == 0), "stride >= n and a multiple of 4");
    SMK_REQUIRE(((uintptr_t)shards & (in_dtype == SMK_WIRE_F32 ? 15 : 7)) == 0 && ((uintptr_t)out & (out_dtype == SMK_WIRE_F32 ? 15 : 7)) == 0,
                "fp32 operands 16-byte aligned, bf16 operands 8-byte aligned");
    SMK_REQUIRE(shards != out || in_dtype == out_dtype, "in place needs equal dtypes");
    return check_launch(launch_reduce_shards(shards, in_dtype == SMK_WIRE_BF16, world, n, stride, out, out_dtype == SMK_WIRE_BF16, (hipStream_t)stream), "reduce_shards");
}

// ------------------------------------------------------------------ softmax attention (chaos term folded into Q)
int smk_attention(const float *q, const float *k, const float *v, void *out, int32_t B, int32_t L, int32_t H,
                  int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale, int32_t out_format,
                  void *stream) {
    return smk_attention_ws(q, k, v, out, B, L, H, head_dim, ldq, ldk, ldv, ldo, scale, out_format, nullptr, 0, stream);
}

int64_t smk_attention_workspace_bytes(int32_t B, int32_t L, int32_t H, int32_t head_dim) {
    if (B < 1 || H < 1 || L < 128 || head_dim != 64 || L % 128 != 0) return 0;
    return (int64_t)attention_workspace_bytes(B, L, H);
}

int smk_attention_ws(const float *q, const float *k, const float *v, void *out, int32_t B, int32_t L, int32_t H,
                     int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale, int32_t out_format,
                     void *workspace, int64_t workspace_bytes, void *stream) {
    return smk_attention_kv(q, k, v, out, B, L, H, head_dim, ldq, ldk, ldv, ldo, scale, out_format, SMK_FMT_F32, workspace, workspace_bytes, stream);
}

int smk_attention_kv(const float *q, const void *k, const void *v, void *out, int32_t B, int32_t L, int32_t H,
                     int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale, int32_t out_format, int32_t kv_format,
                     void *workspace, int64_t workspace_bytes, void *stream) {
    SMK_REQUIRE(q && k && v && out, "null q/k/v/out");
    SMK_REQUIRE(kv_format == SMK_FMT_F32 || kv_format == SMK_FMT_SPLIT4_INPLACE, "kv_format: SMK_FMT_F32 or SMK_FMT_SPLIT4_INPLACE");
    SMK_REQUIRE(B >= 1 && H >= 1 && L >= 128, "B >= 1, H >= 1, L >= 128");
    if (head_dim != 64 || L % 128 != 0) {
        set_error("attention: HIP path is built for head_dim 64 and L a multiple of 128");
        return SMK_ERR_UNSUPPORTED;
    }
    const int64_t cols = (int64_t)H * 64;
    SMK_REQUIRE(ldq >= cols && ldk >= cols && ldv >= cols && ldo >= cols, "row pitches >= H * head_dim");
    SMK_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0, "row pitches multiples of 4 floats");
    SMK_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "16-byte aligned tensors");
    SMK_REQUIRE((int64_t)B * L * ldk < (1LL << 29) && (int64_t)B * L * ldv < (1LL << 29) && (int64_t)B * H * (L / 128) < (1LL << 31),
                "B * L * ld < 2^29 floats (32-bit buffer offsets)");
    AttnArgs a;
    SMK_REQUIRE(out_format == SMK_FMT_F32 || (out_format == SMK_FMT_SPLIT_BF16 && ldo == cols), "out_format (split: ldo == H * head_dim)");
    a.q = q; a.k = (const float *)k; a.v = (const float *)v; a.o = (float *)out; a.o_split = out_format == SMK_FMT_SPLIT_BF16;
    a.kv_split = kv_format == SMK_FMT_SPLIT4_INPLACE;
    a.ldq = (int)ldq; a.ldk = (int)ldk; a.ldv = (int)ldv; a.ldo = (int)ldo;
    a.B = B; a.L = L; a.H = H;
    a.scale_log2e = (float)(scale * 1.4426950408889634074);
    if (workspace && out_format == SMK_FMT_F32) {            // enough for the split the launcher would choose, or none at all
        const int64_t need = (int64_t)attention_workspace_bytes(B, L, H);
        SMK_REQUIRE(((uintptr_t)workspace & 15) == 0, "16-byte aligned workspace");
        if (need > 0 && workspace_bytes >= need) a.ws = (float *)workspace;
    }
    return check_launch(launch_attention_x3(a, (hipStream_t)stream), "attention_x3");
}

int smk_attention_forward_lse(const float *q, const float *k, const float *v, float *out, float *lse, int32_t B, int32_t L,
                              int32_t H, int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, double scale,
                              void *stream) {
    SMK_REQUIRE(q && k && v && out && lse, "null q/k/v/out/lse");
    SMK_REQUIRE(B >= 1 && H >= 1 && L >= 128, "B >= 1, H >= 1, L >= 128");
    if (head_dim != 64 || L % 128 != 0) {
        set_error("attention: HIP path is built for head_dim 64 and L a multiple of 128");
        return SMK_ERR_UNSUPPORTED;
    }
    const int64_t cols = (int64_t)H * 64;
    SMK_REQUIRE(ldq >= cols && ldk >= cols && ldv >= cols && ldo >= cols, "row pitches >= H * head_dim");
    SMK_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0, "row pitches multiples of 4 floats");
    SMK_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "16-byte aligned tensors");
    SMK_REQUIRE((int64_t)B * L * ldk < (1LL << 29) && (int64_t)B * L * ldv < (1LL << 29) && (int64_t)B * H * (L / 128) < (1LL << 31),
                "B * L * ld < 2^29 floats (32-bit buffer offsets)");
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.o = out; a.o_split = 0; a.lse = lse;
    a.ldq = (int)ldq; a.ldk = (int)ldk; a.ldv = (int)ldv; a.ldo = (int)ldo;
    a.B = B; a.L = L; a.H = H;
    a.scale_log2e = (float)(scale * 1.4426950408889634074);
    return check_launch(launch_attention_x3(a, (hipStream_t)stream), "attention_x3");
}

// the softmax weights from q, k and the forward's lse (AttnMapArgs)
static int attention_maps(const float *q, const float *k, const float *lse, float *out, int32_t B, int32_t L, int32_t H, int32_t head_dim,
                          int32_t b0, int32_t nb, int32_t h0, int32_t nh, int64_t ldq, int64_t ldk, int64_t ldo, double scale, bool probs,
                          void *stream) {
    SMK_REQUIRE(q && k && lse && out, "null q/k/lse/out");
    SMK_REQUIRE(B >= 1 && H >= 1 && L >= 128, "B >= 1, H >= 1, L >= 128");
    if (head_dim != 64 || L % 128 != 0) {
        set_error("attention maps: HIP path is built for head_dim 64 and L a multiple of 128");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(b0 >= 0 && nb >= 1 && b0 <= B - nb && h0 >= 0 && nh >= 1 && h0 <= H - nh, "batch / head range inside B x H");
    const int64_t cols = (int64_t)H * 64;
    SMK_REQUIRE(ldq >= cols && ldk >= cols && ldo >= L, "row pitches >= H * head_dim (q, k) and >= L (output)");
    SMK_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0, "q / k row pitches multiples of 4 floats");
    SMK_REQUIRE((((uintptr_t)q | (uintptr_t)k) & 15) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)lse & 3) == 0, "16-byte aligned q and k");
    SMK_REQUIRE((int64_t)B * L * ldq < (1LL << 29) && (int64_t)B * L * ldk < (1LL << 29) && (int64_t)nb * nh * (L / 128) < (1LL << 31),
                "B * L * ld < 2^29 floats (32-bit buffer offsets)");
    AttnMapArgs a;
    a.q = q; a.k = k; a.lse = lse; a.out = out;
    a.ldq = (int)ldq; a.ldk = (int)ldk; a.ldo = ldo;
    a.B = B; a.L = L; a.H = H;
    a.b0 = b0; a.nb = nb; a.h0 = h0; a.nh = nh;
    a.scale_log2e = (float)(scale * 1.4426950408889634074);
    return check_launch(launch_attention_maps(a, probs, (hipStream_t)stream), probs ? "attention_probs" : "attention_received");
}

int smk_attention_received(const float *q, const float *k, const float *lse, float *recv, int32_t B, int32_t L, int32_t H,
                           int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ld_recv, double scale, void *stream) {
    return attention_maps(q, k, lse, recv, B, L, H, head_dim, 0, B, 0, H, ldq, ldk, ld_recv, scale, false, stream);
}

int smk_attention_probs(const float *q, const float *k, const float *lse, float *probs, int32_t B, int32_t L, int32_t H,
                        int32_t head_dim, int32_t b0, int32_t nb, int32_t h0, int32_t nh, int64_t ldq, int64_t ldk, int64_t ld_probs,
                        double scale, void *stream) {
    return attention_maps(q, k, lse, probs, B, L, H, head_dim, b0, nb, h0, nh, ldq, ldk, ld_probs, scale, true, stream);
}

int smk_attention_delta(const float *dout, const float *out, int64_t rows, int32_t H, int32_t head_dim, int64_t ld_dout, int64_t ld_out,
                        float *delta, void *stream) {
    SMK_REQUIRE(dout && out && delta && rows >= 0 && H >= 1, "null pointer / rows < 0 / H < 1");
    if (head_dim != 64) {
        set_error("attention_delta: HIP path is built for head_dim 64");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(ld_dout >= (int64_t)H * 64 && ld_out >= (int64_t)H * 64 && ld_dout % 4 == 0 && ld_out % 4 == 0, "row pitches >= H * 64, multiples of 4");
    SMK_REQUIRE((((uintptr_t)dout | (uintptr_t)out) & 15) == 0, "16-byte aligned tensors");
    if (rows == 0) return SMK_OK;
    return check_launch(launch_attn_delta(dout, out, rows, H, ld_dout, ld_out, delta, (hipStream_t)stream), "attn_delta");
}

int smk_attention_backward(const float *q, const float *k, const float *v, const float *dout, const float *lse,
                           const float *delta, float *dq, float *dk, float *dv, int32_t B, int32_t L, int32_t H,
                           int32_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddq, int64_t lddk,
                           int64_t lddv, double scale, void *stream) {
    SMK_REQUIRE(q && k && v && dout && lse && delta && dq && dk && dv, "null pointer");
    SMK_REQUIRE(B >= 1 && H >= 1 && L >= 128, "B >= 1, H >= 1, L >= 128");
    if (head_dim != 64 || L % 128 != 0) {
        set_error("attention: HIP path is built for head_dim 64 and L a multiple of 128");
        return SMK_ERR_UNSUPPORTED;
    }
    const int64_t cols = (int64_t)H * 64;
    SMK_REQUIRE(ldq >= cols && ldk >= cols && ldv >= cols && ldo >= cols && lddq >= cols && lddk >= cols && lddv >= cols,
                "row pitches >= H * head_dim");
    SMK_REQUIRE((ldq | ldk | ldv | ldo | lddq | lddk | lddv) % 4 == 0, "row pitches multiples of 4 floats");
    SMK_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15) == 0,
                "16-byte aligned tensors");
    SMK_REQUIRE((int64_t)B * H * (L / 128) < (1LL << 31), "B * H * L / 128 < 2^31");
    AttnBwdArgs a;
    a.q = q; a.k = k; a.v = v; a.dout = dout; a.lse = lse; a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv;
    a.ldq = (int)ldq; a.ldk = (int)ldk; a.ldv = (int)ldv; a.ldo = (int)ldo; a.lddq = (int)lddq; a.lddk = (int)lddk; a.lddv = (int)lddv;
    a.B = B; a.L = L; a.H = H;
    a.scale = (float)scale;
    a.scale_log2e = (float)(scale * 1.4426950408889634074);
    return check_launch(launch_attention_bwd_x3(a, (hipStream_t)stream), "attention_bwd_x3");
}

// ------------------------------------------------------------------ training-mode BatchNorm + ReLU + pool
static int bn_check(int32_t B, int32_t C, int32_t H, int32_t W, int32_t pool) {
    SMK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "positive sizes");
    // the rule and the chunk are norm.h's (bn_pool_built / bn_chunk_floats): the grids and the workspace size derive from the same two
    const int64_t chunk = bn_pool_built(pool) ? bn_chunk_floats(pool) : 1;
    if (!bn_pool_built(pool) || ((int64_t)H * W) % chunk != 0 || (pool > 1 && (W != 32 * pool || H % pool != 0)) ||
        (int64_t)B * (H * (int64_t)W / chunk) >= (1LL << 31) || C > 65535) {
        set_error("bn_relu_pool: HIP path is built for pool in {1, 2, 4, 8, 16, 32}, H * W a multiple of 4096 (pool 8: 16384, pool 16: 8192, "
                  "pool 32: 32768), W == 32 * pool when pooling");
        return SMK_ERR_UNSUPPORTED;
    }
    return SMK_OK;
}

int smk_conv1_train_forward(const float *x, const float *weight, const float *bias, int32_t B, int32_t H, int32_t W, float *z1, void *stream) {
    SMK_REQUIRE(x && weight && z1, "null x/weight/z1");
    if (B < 1 || H < 1 || W < 4 || W % 4 != 0 || B > 65535) {
        set_error("conv1_train_forward: 1 <= B <= 65535, W a multiple of 4");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(launch_conv1_train_forward(x, weight, bias, B, H, W, z1, (hipStream_t)stream), "conv1_train_forward");
}

int64_t smk_conv1_train_wgrad_workspace(void) { return (int64_t)conv1_wgrad_workspace_bytes(); }

int smk_conv1_train_wgrad(const float *dz, const float *x, int32_t B, int32_t H, int32_t W, float *dw, float *db, void *workspace, void *stream) {
    SMK_REQUIRE(dz && x && dw && workspace, "null dz/x/dw/workspace");
    if (B < 1 || H < 4 || W < 64 || H % 4 != 0 || W % 64 != 0) {
        set_error("conv1_train_wgrad: B >= 1, H a multiple of 4, W a multiple of 64");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(launch_conv1_train_wgrad(dz, x, B, H, W, dw, db, workspace, (hipStream_t)stream), "conv1_train_wgrad");
}

int smk_conv1_train_dgrad(const float *dz, const float *weight, int32_t B, int32_t H, int32_t W, float *dx, void *stream) {
    SMK_REQUIRE(dz && weight && dx, "null dz/weight/dx");
    if (B < 1 || B > 65535 || H < 1 || H > 65535 * 32 || W < 4 || W % 4 != 0) {
        set_error("conv1_train_dgrad: 1 <= B <= 65535, H >= 1, W a multiple of 4");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE((((uintptr_t)dz | (uintptr_t)dx) & 15) == 0, "16-byte aligned dz / dx");
    return check_launch(launch_conv1_train_dgrad(dz, weight, B, H, W, dx, (hipStream_t)stream), "conv1_train_dgrad");
}

int64_t smk_conv2_train_workspace(void) { return (int64_t)conv2_train_workspace_bytes(); }

int smk_conv2_train_forward(const float *a1, const float *weight, const float *bias, int32_t B, int32_t H, int32_t W, float *z2,
                            void *workspace, void *stream) {
    SMK_REQUIRE(a1 && weight && z2 && workspace, "null a1/weight/z2/workspace");
    if (B < 1 || H < 8 || W < 16 || H % 8 != 0 || W % 16 != 0 || (int64_t)B * 128 * H * W >= (1ll << 40)) {
        set_error("conv2_train_forward: B >= 1, H a multiple of 8, W a multiple of 16");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(launch_conv2_train_forward(a1, weight, bias, B, H, W, z2, workspace, (hipStream_t)stream), "conv2_train_forward");
}

int smk_conv2_train_dgrad(const float *dz, const float *weight, int32_t B, int32_t H, int32_t W, float *dx, void *workspace, void *stream) {
    SMK_REQUIRE(dz && weight && dx && workspace, "null dz/weight/dx/workspace");
    if (B < 1 || H < 8 || W < 16 || H % 8 != 0 || W % 16 != 0 || (int64_t)B * 128 * H * W >= (1ll << 40)) {
        set_error("conv2_train_dgrad: B >= 1, H a multiple of 8, W a multiple of 16");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(launch_conv2_train_dgrad(dz, weight, B, H, W, dx, workspace, (hipStream_t)stream), "conv2_train_dgrad");
}

int64_t smk_conv2_train_wgrad_workspace(void) { return (int64_t)conv2_wgrad_workspace_bytes(conv2_wgrad_streams()); }

int smk_conv2_train_wgrad(const float *dz, const float *a1, int32_t B, int32_t H, int32_t W, float *dw, float *db, void *workspace, void *stream) {
    SMK_REQUIRE(dz && a1 && dw && workspace, "null dz/a1/dw/workspace");
    if (B < 1 || H < 8 || W < 16 || H % 8 != 0 || W % 16 != 0 || (int64_t)B * 128 * H * W >= (1ll << 40)) {
        set_error("conv2_train_wgrad: B >= 1, H a multiple of 8, W a multiple of 16");
        return SMK_ERR_UNSUPPORTED;
    }
    return check_launch(launch_conv2_train_wgrad(dz, a1, B, H, W, dw, db, workspace, (hipStream_t)stream), "conv2_train_wgrad");
}

// ------------------------------------------------------------------ 3-D encoder, training (csrc/conv3d_train.hip)
static int conv3d_train_check(int32_t B, int32_t D, int32_t H, int32_t W, const char *what) {
    if (!conv3d_train_shape_ok(B, D, H, W)) {
        set_error(std::string(what) + ": B, D >= 1, H a multiple of 8, W a multiple of 16");
        return SMK_ERR_UNSUPPORTED;
    }
    return SMK_OK;
}
#define SMK_ALIGNED16(p) (((uintptr_t)(p) & 15) == 0)

int64_t smk_conv3d_train_workspace(void) { return (int64_t)C3T_W2_BYTES; }
int64_t smk_conv3d_cl_wgrad_workspace(int32_t B, int32_t D, int32_t H, int32_t W) {
    return conv3d_train_shape_ok(B, D, H, W) ? (int64_t)conv3d_wgrad_workspace_bytes(B, D, H, W) : -1;
}

int smk_conv3d_s7_train_forward(const float *volume, const float *weight, const float *bias, int32_t B, int32_t D, int32_t H, int32_t W, float *z1,
                                void *workspace, void *stream) {
    SMK_REQUIRE(volume && weight && z1 && workspace, "null volume/weight/z1/workspace");
    if (int rc = conv3d_train_check(B, D, H, W, "conv3d_s7_train_forward")) return rc;
    SMK_REQUIRE(SMK_ALIGNED16(z1) && SMK_ALIGNED16(workspace), "16-byte aligned z1 / workspace");
    return check_launch(launch_conv3d_s7_train_forward(volume, weight, bias, B, D, H, W, z1, workspace, (hipStream_t)stream), "conv3d_s7_train_forward");
}

int smk_conv3d_s7_dgrad(const float *dz1, const float *weight, int32_t B, int32_t D, int32_t H, int32_t W, float *dvol, void *workspace, void *stream) {
    SMK_REQUIRE(dz1 && weight && dvol && workspace, "null dz1/weight/dvol/workspace");
    if (int rc = conv3d_train_check(B, D, H, W, "conv3d_s7_dgrad")) return rc;
    SMK_REQUIRE(SMK_ALIGNED16(dz1) && SMK_ALIGNED16(dvol) && SMK_ALIGNED16(workspace), "16-byte aligned dz1 / dvol / workspace");
    return check_launch(launch_conv3d_s7_dgrad(dz1, weight, B, D, H, W, dvol, workspace, (hipStream_t)stream), "conv3d_s7_dgrad");
}

int smk_conv3d_cl_train_forward(const float *a1, const float *weight, const float *bias, int32_t B, int32_t D, int32_t H, int32_t W, float *z2,
                                void *workspace, void *stream) {
    SMK_REQUIRE(a1 && weight && z2 && workspace, "null a1/weight/z2/workspace");
    if (int rc = conv3d_train_check(B, D, H, W, "conv3d_cl_train_forward")) return rc;
    SMK_REQUIRE(SMK_ALIGNED16(a1) && SMK_ALIGNED16(z2) && SMK_ALIGNED16(workspace), "16-byte aligned a1 / z2 / workspace");
    return check_launch(launch_conv3d_cl_train_forward(a1, weight, bias, B, D, H, W, z2, workspace, (hipStream_t)stream), "conv3d_cl_train_forward");
}

int smk_conv3d_cl_dgrad(const float *dz2, const float *weight, int32_t B, int32_t D, int32_t H, int32_t W, float *da1, void *workspace, void *stream) {
    SMK_REQUIRE(dz2 && weight && da1 && workspace, "null dz2/weight/da1/workspace");
    if (int rc = conv3d_train_check(B, D, H, W, "conv3d_cl_dgrad")) return rc;
    SMK_REQUIRE(SMK_ALIGNED16(dz2) && SMK_ALIGNED16(da1) && SMK_ALIGNED16(workspace), "16-byte aligned dz2 / da1 / workspace");
    return check_launch(launch_conv3d_cl_dgrad(dz2, weight, B, D, H, W, da1, workspace, (hipStream_t)stream), "conv3d_cl_dgrad");
}

int smk_conv3d_cl_wgrad(const float *dz2, const float *a1, int32_t B, int32_t D, int32_t H, int32_t W, float *dw, float *db, void *workspace,
                        void *stream) {
    SMK_REQUIRE(dz2 && a1 && dw && workspace, "null dz2/a1/dw/workspace");
    if (int rc = conv3d_train_check(B, D, H, W, "conv3d_cl_wgrad")) return rc;
    SMK_REQUIRE(SMK_ALIGNED16(dz2) && SMK_ALIGNED16(a1) && SMK_ALIGNED16(workspace), "16-byte aligned dz2 / a1 / workspace");
    return check_launch(launch_conv3d_cl_wgrad(dz2, a1, B, D, H, W, dw, db, workspace, (hipStream_t)stream), "conv3d_cl_wgrad");
}

static bool bn_cl_shape_ok(int32_t B, int32_t D, int32_t H, int32_t W, int32_t C, int32_t pooled) {
    if (B < 1 || D < 1 || H < 1 || W < 1 || (C != 64 && C != 128) || (int64_t)B * D * H * W >= (1ll << 40)) return false;
    return !pooled || (H % 32 == 0 && W % 32 == 0);
}
int64_t smk_bn_cl_workspace(int32_t B, int32_t D, int32_t H, int32_t W, int32_t C) {
    return bn_cl_shape_ok(B, D, H, W, C, 0) ? (int64_t)bn_cl_workspace_bytes((long long)B * D * H * W, C) : -1;
}

int smk_bn_cl_phase(int32_t phase, const float *z, const float *dout, int32_t B, int32_t D, int32_t H, int32_t W, int32_t C, int32_t pooled,
                    const float *gamma, const float *beta, double eps, float *mean, float *var, float *rstd, float *out, float *dz, float *dgamma,
                    float *dbeta, double count, void *workspace, void *stream) {
    if (!bn_cl_shape_ok(B, D, H, W, C, pooled)) {
        set_error("bn_cl_phase: C 64 or 128, B, D, H, W >= 1, and H, W multiples of 32 when pooled");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(z && mean && rstd && SMK_ALIGNED16(z), "null or unaligned z / mean / rstd");
    switch (phase) {
    case SMK_BN_STATS: SMK_REQUIRE(var && workspace && ((uintptr_t)workspace & 7) == 0, "STATS: null var/workspace, or a workspace that is not 8-byte aligned (fp64 partial sums)"); break;
    case SMK_BN_APPLY: SMK_REQUIRE(gamma && beta && out && SMK_ALIGNED16(out), "APPLY: null gamma/beta/out"); break;
    case SMK_BN_BWD_SUMS: SMK_REQUIRE(gamma && beta && dout && dgamma && dbeta && workspace && SMK_ALIGNED16(dout) && ((uintptr_t)workspace & 7) == 0, "BWD_SUMS: null gamma/beta/dout/dgamma/dbeta/workspace, or a workspace that is not 8-byte aligned (fp64 partial sums)"); break;
    case SMK_BN_BWD_DZ: SMK_REQUIRE(gamma && beta && dout && dgamma && dbeta && dz && count > 0 && SMK_ALIGNED16(dout) && SMK_ALIGNED16(dz), "BWD_DZ: null gamma/beta/dout/dgamma/dbeta/dz, or count <= 0"); break;
    default: SMK_REQUIRE(false, "unknown phase");
    }
    return check_launch(launch_bn_cl_phase(phase, z, dout, B, D, H, W, C, pooled, gamma, beta, eps, mean, var, rstd, out, dz, dgamma, dbeta, count,
                                           workspace, (hipStream_t)stream), "bn_cl_phase");
}

// ------------------------------------------------------------------ reconstruction head, training (csrc/decoder_train.hip)
static int convt_train_check(int32_t B, int32_t CIN, int32_t COUT, int32_t H, int32_t W, const char *what) {
    if (!convt_train_shape_ok(B, CIN, COUT, H, W)) {
        set_error(std::string(what) + ": COUT 16 or 32, CIN a multiple of 16 (COUT 32) or 32 (COUT 16) up to 4096, H and W multiples of 16, "
                  "1 <= B <= 65535");
        return SMK_ERR_UNSUPPORTED;
    }
    return SMK_OK;
}

int smk_convt4s2_train_forward(const float *x, const float *weight, const float *bias, int32_t B, int32_t CIN, int32_t COUT, int32_t H,
                               int32_t W, int32_t tok, float *z, void *stream) {
    SMK_REQUIRE(x && weight && z, "null x/weight/z");
    SMK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)z & 7) == 0, "alignment");
    if (int rc = convt_train_check(B, CIN, COUT, H, W, "convt4s2_train_forward")) return rc;
    return check_launch(launch_convt_train_forward(x, weight, bias, B, CIN, COUT, H, W, tok != 0, z, (hipStream_t)stream), "convt4s2_train_forward");
}

int smk_convt4s2_train_dgrad(const float *dz, const float *weight, int32_t B, int32_t CIN, int32_t COUT, int32_t H, int32_t W, int32_t tok,
                             float *dx, void *stream) {
    SMK_REQUIRE(dz && weight && dx, "null dz/weight/dx");
    SMK_REQUIRE(((uintptr_t)dx & 15) == 0, "alignment");
    if (int rc = convt_train_check(B, CIN, COUT, H, W, "convt4s2_train_dgrad")) return rc;
    return check_launch(launch_convt_train_dgrad(dz, weight, B, CIN, COUT, H, W, tok != 0, dx, (hipStream_t)stream), "convt4s2_train_dgrad");
}

int64_t smk_convt4s2_train_wgrad_workspace(int32_t B, int32_t CIN, int32_t COUT, int32_t H, int32_t W) {
    return (int64_t)convt_train_wgrad_workspace_bytes(B, CIN, COUT, H, W);
}

int smk_convt4s2_train_wgrad(const float *dz, const float *x, int32_t B, int32_t CIN, int32_t COUT, int32_t H, int32_t W, int32_t tok,
                             float *dw, float *db, void *workspace, void *stream) {
    SMK_REQUIRE(dz && x && dw && workspace, "null dz/x/dw/workspace");
    SMK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "alignment");
    if (int rc = convt_train_check(B, CIN, COUT, H, W, "convt4s2_train_wgrad")) return rc;
    return check_launch(launch_convt_train_wgrad(dz, x, B, CIN, COUT, H, W, tok != 0, dw, db, workspace, (hipStream_t)stream),
                        "convt4s2_train_wgrad");
}

static int conv3_train_check(int32_t B, int32_t H, int32_t W, const char *what) {
    if (!conv3_train_shape_ok(B, H, W)) {
        set_error(std::string(what) + ": H a multiple of 8, W a multiple of 32, 1 <= B <= 65535");
        return SMK_ERR_UNSUPPORTED;
    }
    return SMK_OK;
}

int smk_conv3_sigmoid_train_forward(const float *x, const float *weight, const float *bias, int32_t B, int32_t H, int32_t W, float *y,
                                    void *stream) {
    SMK_REQUIRE(x && weight && y, "null x/weight/y");
    if (int rc = conv3_train_check(B, H, W, "conv3_sigmoid_train_forward")) return rc;
    return check_launch(launch_conv3_sigmoid_train_forward(x, weight, bias, B, H, W, y, (hipStream_t)stream), "conv3_sigmoid_train_forward");
}

int64_t smk_conv3_sigmoid_train_workspace(int32_t B, int32_t H, int32_t W) { return (int64_t)conv3_sigmoid_train_workspace_bytes(B, H, W); }

int smk_conv3_sigmoid_train_backward(const float *dy, const float *y, const float *x, const float *weight, int32_t B, int32_t H, int32_t W,
                                     float *dx, float *dw, float *db, void *workspace, void *stream) {
    SMK_REQUIRE(dy && y && x && weight && dx && workspace, "null dy/y/x/weight/dx/workspace");
    SMK_REQUIRE(((uintptr_t)workspace & 15) == 0, "alignment");
    if (int rc = conv3_train_check(B, H, W, "conv3_sigmoid_train_backward")) return rc;
    return check_launch(launch_conv3_sigmoid_train_backward(dy, y, x, weight, B, H, W, dx, dw, db, workspace, (hipStream_t)stream),
                        "conv3_sigmoid_train_backward");
}

int64_t smk_bn_train_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int32_t pool) {
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    return bn_train_workspace_floats(B, C, H, W, pool) * (int64_t)sizeof(float);
}

int smk_bn_relu_pool_forward(const float *z, int32_t B, int32_t C, int32_t H, int32_t W, const float *gamma, const float *beta,
                             double eps, int32_t pool, float *out, float *mean, float *var, float *rstd, void *workspace,
                             void *stream) {
    SMK_REQUIRE(z && gamma && beta && out && mean && var && rstd && workspace, "null pointer");
    int rc = bn_check(B, C, H, W, pool);
    if (rc) return rc;
    SMK_REQUIRE((((uintptr_t)z | (uintptr_t)out | (uintptr_t)workspace) & 15) == 0, "16-byte aligned tensors");
    BnTrainArgs a = {};
    a.z = z; a.gamma = gamma; a.beta = beta; a.B = B; a.C = C; a.H = H; a.W = W; a.pool = pool; a.eps = (float)eps;
    a.part = (float *)workspace; a.out = out; a.mean = mean; a.var = var; a.rstd = rstd;
    return check_launch(launch_bn_relu_pool_forward(a, (hipStream_t)stream), "bn_relu_pool_forward");
}

int smk_bn_relu_pool_backward(const float *z, const float *dout, int32_t B, int32_t C, int32_t H, int32_t W, const float *gamma,
                              const float *beta, const float *mean, const float *rstd, int32_t pool, float *dz, float *dgamma,
                              float *dbeta, void *workspace, void *stream) {
    SMK_REQUIRE(z && dout && gamma && beta && mean && rstd && dz && dgamma && dbeta && workspace, "null pointer");
    int rc = bn_check(B, C, H, W, pool);
    if (rc) return rc;
    SMK_REQUIRE((((uintptr_t)z | (uintptr_t)dz | (uintptr_t)dout | (uintptr_t)workspace) & 15) == 0, "16-byte aligned tensors");
    BnTrainArgs a = {};
    a.z = z; a.gamma = gamma; a.beta = beta; a.B = B; a.C = C; a.H = H; a.W = W; a.pool = pool;
    a.part = (float *)workspace; a.mean = const_cast<float *>(mean); a.rstd = const_cast<float *>(rstd);
    a.dout = dout; a.dz = dz; a.dgamma = dgamma; a.dbeta = dbeta;
    return check_launch(launch_bn_relu_pool_backward(a, (hipStream_t)stream), "bn_relu_pool_backward");
}

// The passes of smk_bn_relu_pool_forward / _backward one at a time, for BatchNorm statistics that span several processes
// (models/sync_bn.py all-reduces the per-channel statistics between them).  phase:
//   SMK_BN_STATS        z -> mean / var (biased) / rstd of THIS process's batch                      (needs workspace)
//   SMK_BN_APPLY        out = blockmean(relu(bn(z))) from the GIVEN mean / rstd
//   SMK_BN_BWD_SUMS     dout, z, given mean / rstd -> this process's dgamma = sum dy * zhat, dbeta = sum dy   (needs workspace)
//   SMK_BN_BWD_DZ       dz from the GIVEN (all-reduced) dgamma / dbeta and `count` = elements per channel of the global batch
int smk_bn_relu_pool_phase(int32_t phase, const float *z, const float *dout, int32_t B, int32_t C, int32_t H, int32_t W, const float *gamma,
                           const float *beta, double eps, float *mean, float *var, float *rstd, int32_t pool, float *out, float *dz,
                           float *dgamma, float *dbeta, double count, void *workspace, void *stream) {
    SMK_REQUIRE(z && gamma && beta && mean && rstd, "null pointer");
    // the two element-wise passes at pool 1 take any plane of whole float4s (frozen statistics on the 32 x 32 token grid); the reductions keep whole chunks
    const bool elementwise = (phase == SMK_BN_APPLY || phase == SMK_BN_BWD_DZ) && pool == 1 && B >= 1 && C >= 1 && C <= 65535 && H >= 1 && W >= 1 &&
                             ((int64_t)H * W) % 4 == 0 && (int64_t)H * W < (1LL << 31) - 4096 && (int64_t)B * (((int64_t)H * W + 4095) / 4096) < (1LL << 31);
    int rc = elementwise ? SMK_OK : bn_check(B, C, H, W, pool);
    if (rc) return rc;
    SMK_REQUIRE(((uintptr_t)z & 15) == 0, "16-byte aligned z");
    BnTrainArgs a = {};
    a.z = z; a.gamma = gamma; a.beta = beta; a.B = B; a.C = C; a.H = H; a.W = W; a.pool = pool; a.eps = (float)eps;
    a.part = (float *)workspace; a.mean = mean; a.var = var; a.rstd = rstd;
    a.out = out; a.dout = dout; a.dz = dz; a.dgamma = dgamma; a.dbeta = dbeta; a.count = (float)count;
    hipStream_t st = (hipStream_t)stream;
    switch (phase) {
        case SMK_BN_STATS:
            SMK_REQUIRE(var && workspace && ((uintptr_t)workspace & 15) == 0, "stats: var and an aligned workspace");
            return check_launch(launch_bn_stats(a, st), "bn_stats");
        case SMK_BN_APPLY:
            SMK_REQUIRE(out && ((uintptr_t)out & 15) == 0, "apply: aligned out");
            return check_launch(launch_bn_relu_pool_apply(a, st), "bn_relu_pool_apply");
        case SMK_BN_BWD_SUMS:
            SMK_REQUIRE(dout && dgamma && dbeta && workspace && (((uintptr_t)dout | (uintptr_t)workspace) & 15) == 0, "sums: dout, dgamma, dbeta, workspace");
            return check_launch(launch_bn_relu_pool_backward_sums(a, st), "bn_relu_pool_backward_sums");
        case SMK_BN_BWD_DZ:
            SMK_REQUIRE(dout && dz && dgamma && dbeta && count > 0 && (((uintptr_t)dout | (uintptr_t)dz) & 15) == 0, "dz: dout, dz, dgamma, dbeta, count > 0");
            return check_launch(launch_bn_relu_pool_backward_dz(a, st), "bn_relu_pool_backward_dz");
    }
    set_error("bn_relu_pool_phase: unknown phase");
    return SMK_ERR_INVALID;
}

// ------------------------------------------------------------------ LayerNorm
int smk_layernorm(const float *x, int64_t rows, int32_t D, int64_t ldx, const float *weight, const float *bias, double eps,
                  void *y, int64_t ldy, int32_t y_format, void *stream) {
    SMK_REQUIRE(x && y && weight && bias, "null x/y/weight/bias");
    SMK_REQUIRE(rows >= 1 && rows < (1LL << 31) - 4, "1 <= rows < 2^31");
    if (D < 4 || D % 4 != 0 || D > 2048) {
        set_error("layernorm: HIP path is built for D a multiple of 4, at most 2048");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(ldx >= D && ldy >= D && ldx % 4 == 0 && ldy % 4 == 0, "row pitches >= D, multiples of 4 floats");
    SMK_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)weight | (uintptr_t)bias) & 15) == 0, "16-byte aligned tensors");
    LayerNormArgs a;
    SMK_REQUIRE(y_format == SMK_FMT_F32 || (y_format == SMK_FMT_SPLIT_BF16 && D % 8 == 0 && ldy == D), "y_format (split: D % 8 == 0, ldy == D)");
    a.x = x; a.y = (float *)y; a.w = weight; a.b = bias; a.ldx = ldx; a.ldy = ldy; a.rows = (int)rows; a.D = D; a.eps = (float)eps;
    a.y_split = y_format == SMK_FMT_SPLIT_BF16;
    return check_launch(launch_layernorm(a, (hipStream_t)stream), "layernorm");
}

int64_t smk_layernorm_bwd_workspace(int32_t D) { return D >= 1 ? (int64_t)LN_BWD_WGS * 2 * D * (int64_t)sizeof(float) : 0; }

int smk_layernorm_backward(const float *x, const float *dy, int64_t rows, int32_t D, int64_t ldx, int64_t ld_dy,
                           const float *weight, double eps, float *dx, int64_t ld_dx, float *dweight, float *dbias,
                           void *workspace, void *stream) {
    SMK_REQUIRE(x && dy && weight && dx && dweight && dbias && workspace, "null pointer");
    SMK_REQUIRE(rows >= 1 && rows < (1LL << 31) - 4, "1 <= rows < 2^31");
    if (D < 4 || D % 4 != 0 || D > 2048) {
        set_error("layernorm: HIP path is built for D a multiple of 4, at most 2048");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(ldx >= D && ld_dy >= D && ld_dx >= D && ldx % 4 == 0 && ld_dy % 4 == 0 && ld_dx % 4 == 0, "row pitches >= D, multiples of 4 floats");
    SMK_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)weight | (uintptr_t)workspace) & 15) == 0, "16-byte aligned tensors");
    LayerNormBwdArgs a;
    a.x = x; a.dy = dy; a.w = weight; a.dx = dx; a.dw = dweight; a.db = dbias; a.part = (float *)workspace;
    a.ldx = ldx; a.lddy = ld_dy; a.lddx = ld_dx; a.rows = (int)rows; a.D = D; a.eps = (float)eps;
    return check_launch(launch_layernorm_bwd(a, (hipStream_t)stream), "layernorm_bwd");
}

// ------------------------------------------------------------------ reconstruction head
int smk_decoder_create(const smk_decoder_weights *w, int32_t device_id, void *stream, smk_decoder **out) {
    SMK_REQUIRE(w && out, "null weights/out");
    const float *const *pp = (const float *const *)w;
    for (size_t k = 0; k < sizeof(*w) / sizeof(float *); ++k) SMK_REQUIRE(pp[k], "null weight pointer");
    DeviceGuard guard(device_id);
    int rc = guard.rc;
    if (rc) return rc;
    smk_decoder *dec = new smk_decoder();
    dec->device = device_id;
    const size_t n = 64 * 32 * 16 + 32 * 16 * 16 + 16 * 9 + 32 + 16 + 16;
    hipError_t e = hipMalloc((void **)&dec->blob, n * sizeof(float));
    if (e != hipSuccess) {
        delete dec;
        set_error(std::string("smk_decoder_create: ") + hipGetErrorString(e));
        return SMK_ERR_HIP;
    }
    float *p = dec->blob;
    dec->d.w1 = p; p += 64 * 32 * 16;
    dec->d.w2 = p; p += 32 * 16 * 16;
    dec->d.w3 = p; p += 16 * 9;
    dec->d.t1 = p; p += 32;
    dec->d.t2 = p; p += 16;
    dec->d.b3 = p;
    rc = check_launch(launch_fold_decoder(*w, dec->d, (hipStream_t)stream), "fold_decoder");
    if (rc) { smk_decoder_destroy(dec); return rc; }
    *out = dec;
    return SMK_OK;
}

int smk_decoder_destroy(smk_decoder *dec) {
    if (!dec) return SMK_OK;
    DeviceGuard guard(dec->device);              // frees run on the handle's device; the caller's device is restored
    if (dec->blob) (void)hipFree(dec->blob);
    delete dec;
    return SMK_OK;
}

int smk_decoder_forward(smk_decoder *dec, const float *tokens, int32_t B, int32_t S, float *tmp1, float *tmp2,
                        float *recon, void *stream) {
    SMK_REQUIRE(dec && tokens && tmp1 && tmp2 && recon, "null dec/tokens/tmp/recon");
    SMK_REQUIRE(B >= 1 && B <= 65535, "1 <= B <= 65535");
    if (S < 16 || S % 16 != 0) {
        set_error("decoder: HIP path is built for token grids whose side is a multiple of 16");
        return SMK_ERR_UNSUPPORTED;
    }
    SMK_REQUIRE(((uintptr_t)tokens & 15) == 0 && ((uintptr_t)tmp1 & 7) == 0 && ((uintptr_t)tmp2 & 7) == 0, "alignment");
    DeviceGuard guard(dec->device);
    int rc = guard.rc;
    if (rc) return rc;
    return check_launch(launch_decoder(dec->d, tokens, B, S, tmp1, tmp2, recon, (hipStream_t)stream), "decoder");
}

}  // extern "C"
#pragma GCC visibility pop
