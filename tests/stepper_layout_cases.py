"""The state layouts the C ABI accepts for the 2-D and 3-D steppers (include/smokehip.h, "state layouts"), as one table, and the runner
that steps a layout through ctypes with every field and frame carved from one guarded arena (tests/guarded_arena.py).  A plain helper
module; tests/test_hip_stepper_layouts.py runs the table on the device (the 2-D cases in child processes, tests/_stepper_layout_child.py,
one per SMK_JACOBI_PERSIST setting: the switch is read once per process), tests/test_stepper_layout_table_host.py holds the table's
form strings to the CPU plan code.

A layout names the two pitches and, per field, the byte offset of its base pointer from 16-byte alignment.  Each case lists the kernel
forms smk_sim_describe / smk_sim3d_describe must report for it: the GPU tests compare the strings and never re-derive the gates."""
import ctypes as C
import hashlib
import json
from dataclasses import dataclass

import numpy as np

B2, CALLS, STEPS_PER_CALL = 3, 2, 3          # 2-D: grids, smk_sim_step calls, steps per call
B3 = 2
VELS = (0.5, 300.0)                          # dense signed states: every back-trace near (0.5) / several cells away and clamped (300)
FILLS = (-1, 0)                              # pad columns, guards and frame gaps: 0xFFFFFFFF (a NaN) and 0

# (H, W, J): the smallest shapes at which each 2-D kernel family is selected
SHAPES_2D = [(64, 64, 20), (96, 128, 8), (256, 256, 20), (64, 512, 6), (33, 50, 6), (70, 131, 6)]
# (D, H, W, J)
SHAPES_3D = [(4, 16, 64, 4), (9, 20, 28, 7), (13, 22, 19, 6)]


def up32(x):
    return (x + 31) // 32 * 32


@dataclass(frozen=True)
class Layout:
    name: str
    pc: object                    # W -> pitch of the cell fields and u (and w)
    pv: object                    # W -> pitch of v
    off: tuple = (0, 0, 0, 0)     # byte offsets from 16-byte alignment of u, v, p, density (w: u's)
    frames_off: int = 4


LAYOUTS = [
    Layout("wrapper", up32, lambda W: up32(W + 1), frames_off=0),                  # the simulator classes' own
    Layout("dense", lambda W: W, lambda W: W + 1),                                  # the reference's shapes
    Layout("pitch4", lambda W: W + 4, lambda W: W + 4),                             # both multiples of 4, not of 32
    Layout("vodd", lambda W: W + 8, lambda W: W + 3),                               # cell pitch a multiple of 4, v's odd
    Layout("odd", lambda W: W + 1, lambda W: W + 2),                                # both odd
    Layout("offset", up32, lambda W: up32(W + 1), off=(4, 8, 4, 12)),               # the wrapper's pitches, every base off 16 bytes
    Layout("strides", lambda W: W + 12, lambda W: W + 4),                           # grid strides (H + 1) pc: multiples of 4, not of 8
    Layout("poffset", up32, lambda W: up32(W + 1), off=(0, 0, 4, 0)),               # only the pressure off 16 bytes (3-D: vec && !quad)
]
LAYOUT = {l.name: l for l in LAYOUTS}

# What smk_sim_describe must report: (projection kernel with SMK_JACOBI_PERSIST=1, =0, "buoy_diffuse" with =1, =0).  "F": folded into the
# projection.  From the plan code (tests/test_stepper_layout_table_host.py recomputes every entry on the CPU).
_F, _V, _S = "folded into the projection", "vec4", "scalar"
FORMS_2D = {
    (64, 64): {
        "wrapper": ("k_jacobi_band<1,4>", "k_jacobi_band<1,2>", _F, _V),
        "dense": ("k_jacobi_band<1,4>", "k_jacobi_band<1,2>", _S, _S),
        "pitch4": ("k_jacobi_band<1,4>", "k_jacobi_band<1,2>", _F, _V),
        "vodd": ("k_jacobi_band<1,4>", "k_jacobi_band<1,2>", _S, _S),
        "odd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "offset": ("k_jacobi_band<1,4>", "k_jacobi_band<1,2>", _F, _S),
        "strides": ("k_jacobi_band<1,4>", "k_jacobi_band<1,2>", _F, _V),
        "poffset": ("k_jacobi_band<1,4>", "k_jacobi_band<1,2>", _F, _V),
    },
    (96, 128): {
        "wrapper": ("k_jacobi_band<2,2>", "k_jacobi_band<2,2>", _F, _V),
        "dense": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "pitch4": ("k_jacobi_band<2,2>", "k_jacobi_band<2,2>", _F, _V),
        "vodd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "odd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "offset": ("k_jacobi_band<2,2>", "k_jacobi_band<2,2>", _S, _S),
        "strides": ("k_jacobi_band<2,2>", "k_jacobi_band<2,2>", _F, _V),
        "poffset": ("k_jacobi_band<2,2>", "k_jacobi_band<2,2>", _F, _V),
    },
    (256, 256): {
        "wrapper": ("k_jacobi_band<4,2>", "k_jacobi_band<4,2>", _F, _V),
        "dense": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "pitch4": ("k_jacobi_band<4,2>", "k_jacobi_band<4,2>", _F, _V),
        "vodd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "odd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "offset": ("k_jacobi_band<4,2>", "k_jacobi_band<4,2>", _S, _S),
        "strides": ("k_jacobi_band<4,2>", "k_jacobi_band<4,2>", _F, _V),
        "poffset": ("k_jacobi_band<4,2>", "k_jacobi_band<4,2>", _F, _V),
    },
    (64, 512): {
        "wrapper": ("k_jacobi_band<8,2>", "k_jacobi_band<8,2>", _V, _V),
        "dense": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "pitch4": ("k_jacobi_band<8,2>", "k_jacobi_band<8,2>", _V, _V),
        "vodd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "odd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "offset": ("k_jacobi_band<8,2>", "k_jacobi_band<8,2>", _S, _S),
        "strides": ("k_jacobi_band<8,2>", "k_jacobi_band<8,2>", _V, _V),
        "poffset": ("k_jacobi_band<8,2>", "k_jacobi_band<8,2>", _V, _V),
    },
    (33, 50): {
        "wrapper": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "dense": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "pitch4": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "vodd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "odd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "offset": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "strides": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "poffset": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
    },
    (70, 131): {
        "wrapper": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "dense": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "pitch4": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "vodd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "odd": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "offset": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "strides": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
        "poffset": ("k_jacobi_sweep", "k_jacobi_sweep", _S, _S),
    },
}

# What smk_sim3d_describe must report: ("jacobi", "jacobi_sweep", alignment.vec, alignment.quad).  Between them the cases reach the three
# branches of the gate: quad, vec && !quad (aligned pitches, p off 16 bytes) and !vec at W % 4 == 0 (an odd pitch).
_Q, _X = "quad v4<T>", "xt"
FORMS_3D = {
    (4, 16, 64): {
        "wrapper": (_Q, None, True, True),
        "dense": (_Q, None, True, True),
        "pitch4": (_Q, None, True, True),
        "vodd": (_Q, None, True, True),
        "odd": (_X, None, False, False),
        "offset": (_X, None, True, False),
        "strides": (_Q, None, True, True),
        "poffset": (_X, None, True, False),
    },
    (9, 20, 28): {
        "wrapper": (_Q, "quad per-sweep", True, True),
        "dense": (_Q, "quad per-sweep", True, True),
        "pitch4": (_Q, "quad per-sweep", True, True),
        "vodd": (_Q, "quad per-sweep", True, True),
        "odd": (_X, "per-sweep", False, False),
        "offset": (_X, "per-sweep", True, False),
        "strides": (_Q, "quad per-sweep", True, True),
        "poffset": (_X, "per-sweep", True, False),
    },
    (13, 22, 19): {
        "wrapper": (_X, None, False, False),
        "dense": (_X, None, False, False),
        "pitch4": (_X, None, False, False),
        "vodd": (_X, None, False, False),
        "odd": (_X, None, False, False),
        "offset": (_X, None, False, False),
        "strides": (_X, None, False, False),
        "poffset": (_X, None, False, False),
    },
}


def forms_2d(H, W, layout, persist):
    row = FORMS_2D[(H, W)][layout]
    return {"kernel": row[0 if persist else 1], "buoy_diffuse": row[2 if persist else 3]}


def forms_3d(D, H, W, layout):
    row = FORMS_3D[(D, H, W)][layout]
    return {"jacobi": row[0], "jacobi_sweep": row[1], "vec": row[2], "quad": row[3]}


def case_ids_2d():
    return [f"{H}x{W}-J{J}-{l.name}" for H, W, J in SHAPES_2D for l in LAYOUTS]


def case_ids_3d():
    return [f"{D}x{H}x{W}-J{J}-{l.name}" for D, H, W, J in SHAPES_3D for l in LAYOUTS]


# ------------------------------------------------------------------------------------------------ reference states and trajectories
def dense_state_2d(H, W, vel, b):
    """The dense signed states of test_whole_steps_from_dense_random_states_bit_exact_vs_oracle (tests/test_hip_physics.py)."""
    rng = np.random.RandomState(1000 * H + W + b)
    return {"u": (rng.standard_normal((H + 1, W)) * vel).astype(np.float32), "v": (rng.standard_normal((H, W + 1)) * vel).astype(np.float32),
            "p": (rng.standard_normal((H, W)) * 0.1).astype(np.float32), "density": rng.uniform(0.0, 1.8, (H, W)).astype(np.float32)}


KEYS2 = ("u", "v", "p", "density")
KEYS3 = ("u", "v", "w", "p", "density")
_ref_cache = {}


def reference_2d(H, W, J, vel):
    """Per grid: the state after each single stage (with the divergence and the back-trace indices) from the initial state, and the
    trajectory of CALLS * STEPS_PER_CALL whole steps from the same initial state.  Computed once per (shape, scale), never changed."""
    key = (2, H, W, J, vel)
    if key in _ref_cache:
        return _ref_cache[key]
    import oracle
    grids = []
    for b in range(B2):
        s0 = dense_state_2d(H, W, vel, b)
        o = oracle.OracleNS((H, W), jacobi_iters=J)
        for k in KEYS2:
            setattr(o, k, s0[k].copy())
        snap = lambda: {k: getattr(o, k).copy() for k in KEYS2}                      # noqa: E731
        stages = {}
        o.buoyancy()
        o.u, o.v, o.density = o.diffusion_step(o.u, o.viscosity), o.diffusion_step(o.v, o.viscosity), o.diffusion_step(o.density, o.viscosity * 0.1)
        stages["buoy_diffuse"] = snap()
        stages["div"] = o.divergence()
        o.pressure_projection()
        stages["project"] = snap()
        for name, tag in (("u", "advect_u"), ("v", "advect_v"), ("density", "advect_d")):
            out, x0, y0 = o.advection_step(getattr(o, name), o.u, o.v, want_indices=True)
            if name == "density":
                out = (out * np.float32(0.995)).astype(np.float32)
            setattr(o, name, out)
            stages[tag] = snap()
            stages[tag + "_x0"], stages[tag + "_y0"] = x0.astype(np.int32), y0.astype(np.int32)
        o2 = oracle.OracleNS((H, W), jacobi_iters=J)
        for k in KEYS2:
            setattr(o2, k, s0[k].copy())
        frames = [o2.step() for _ in range(CALLS * STEPS_PER_CALL)]
        # the state at the end of every call
        o3 = oracle.OracleNS((H, W), jacobi_iters=J)
        for k in KEYS2:
            setattr(o3, k, s0[k].copy())
        ends = []
        for _ in range(CALLS):
            for _ in range(STEPS_PER_CALL):
                o3.step()
            ends.append({k: getattr(o3, k).copy() for k in KEYS2})
        grids.append({"init": s0, "stages": stages, "frames": frames, "ends": ends})
        assert all(np.isfinite(f).all() for f in frames)
    _ref_cache[key] = grids
    return grids


def dense_state_3d(shape, vel, b):
    """The dense random states of tests/test_hip_physics3d.py."""
    from oracle.ns_nd import OracleNSnd
    rng = np.random.default_rng(sum(shape) + 17 * b)
    o = OracleNSnd(shape)
    for k in ("u", "v", "w"):
        setattr(o, k, (rng.standard_normal(getattr(o, k).shape) * vel).astype(np.float32))
    o.p = (rng.standard_normal(o.p.shape) * 0.1).astype(np.float32)
    o.density = rng.random(o.density.shape).astype(np.float32) * 2.0
    return {k: getattr(o, k) for k in KEYS3}


STEPS_3D = 2


def reference_3d(D, H, W, J, vel):
    key = (3, D, H, W, J, vel)
    if key in _ref_cache:
        return _ref_cache[key]
    from oracle.ns_nd import OracleNSnd
    grids = []
    for b in range(B3):
        s0 = dense_state_3d((D, H, W), vel, b)

        def fresh():
            o = OracleNSnd((D, H, W), jacobi_iters=J)
            for k in KEYS3:
                setattr(o, k, s0[k].copy())
            return o
        o = fresh()
        snap = lambda: {k: getattr(o, k).copy() for k in KEYS3}                      # noqa: E731
        stages = {}
        o.buoyancy(); o.diffuse_all()
        stages["buoy_diffuse"] = snap()
        o.pressure_projection()
        stages["project"] = snap()
        for name in ("u", "v", "w"):
            setattr(o, name, o.advection_step(getattr(o, name), o.velocity()))
            stages["advect_" + name] = snap()
        o.density = (o.advection_step(o.density, o.velocity()) * np.float32(0.995)).astype(np.float32)
        stages["advect_d"] = snap()
        o2 = fresh()
        frames = [o2.step().copy() for _ in range(2 * STEPS_3D)]
        o3 = fresh()
        ends = []
        for _ in range(2):
            for _ in range(STEPS_3D):
                o3.step()
            ends.append({k: getattr(o3, k).copy() for k in KEYS3})
        grids.append({"init": s0, "stages": stages, "frames": frames, "ends": ends})
    _ref_cache[key] = grids
    return grids


# ------------------------------------------------------------------------------------------------ the arena of one run
class LayoutRun:
    """One simulator on one arena: the fields [B][rows][pitch] as owned buffers (pad columns hold the fill when the state is written),
    the frame buffers as owned spans whose gaps are checked like guards, and dense outputs for the divergence and the back-trace."""

    def __init__(self, dims, J, layout, fill, frame_specs, three_d=False):
        import torch
        from guarded_arena import Arena, Buf
        from smokephysai_amd import _lib
        self.torch, self.lib, self._lib = torch, _lib.load(), _lib
        self.three_d, self.fill = three_d, fill
        if three_d:
            self.B, (self.D, self.H, self.W) = B3, dims
        else:
            self.B, self.D, (self.H, self.W) = B2, 1, dims
        B, D, H, W = self.B, self.D, self.H, self.W
        self.pc, self.pv = layout.pc(W), layout.pv(W)
        offs = dict(zip(KEYS2, layout.off))
        offs["w"] = offs["u"]
        # name -> (rows of one grid, pitch, live columns)
        self.fields = {"u": (D * (H + 1), self.pc, W), "v": (D * H, self.pv, W + 1), "p": (D * H, self.pc, W), "density": (D * H, self.pc, W)}
        if three_d:
            self.fields["w"] = ((D + 1) * H, self.pc, W)

        def buf(name, elems, off, dtype=torch.float32):
            return Buf(name, dtype, elems, align=16 if off == 0 else 4, phase=None if off == 0 else off, role="inout")
        bufs = [buf(k, B * r * p, offs[k]) for k, (r, p, _) in self.fields.items()]
        # frame buffers: name -> (fsb, fst, T); element (t, b) at t * fst + b * fsb, D * H * W dense floats each
        self.frame_specs, self.n = frame_specs, D * H * W
        for name, (fsb, fst, T) in frame_specs.items():
            span = (T - 1) * fst + (B - 1) * fsb + self.n
            bufs.append(buf(name, span, layout.frames_off))
        bufs.append(buf("div", B * H * W, 0))
        bufs += [buf("x0", B * (H + 1) * (W + 1), 4, torch.int32), buf("y0", B * (H + 1) * (W + 1), 8, torch.int32)]
        self.arena = Arena(bufs)
        self.arena.fill(fill)
        self.dev = self.arena.buf.device
        self.handle = C.c_void_p()
        self.J = J

    def create(self):
        L, _lib, a = self.lib, self._lib, self.arena
        if self.three_d:
            desc = _lib.SmkSim3dDesc(self.B, self.D, self.H, self.W, self.J, 0.01, 0.001, self.dev.index or 0, self.pc, self.pv,
                                     a.ptr("u"), a.ptr("v"), a.ptr("w"), a.ptr("p"), a.ptr("density"))
            _lib.check(L.smk_sim3d_create(C.byref(desc), C.byref(self.handle)))
        else:
            desc = _lib.SmkSimDesc(self.B, self.H, self.W, self.J, 0.01, 0.001, self.dev.index or 0, self.pc, self.pv,
                                   a.ptr("u"), a.ptr("v"), a.ptr("p"), a.ptr("density"))
            _lib.check(L.smk_sim_create(C.byref(desc), C.byref(self.handle)))
        return self

    def destroy(self):
        self.torch.cuda.synchronize()
        if self.handle:
            self._lib.check((self.lib.smk_sim3d_destroy if self.three_d else self.lib.smk_sim_destroy)(self.handle))
            self.handle = C.c_void_p()

    def st(self):
        return self._lib.stream_ptr(self.dev)

    def describe(self):
        buf = C.create_string_buffer(8192)
        self._lib.check((self.lib.smk_sim3d_describe if self.three_d else self.lib.smk_sim_describe)(self.handle, buf, 8192))
        return json.loads(buf.value.decode())

    # ---- fields
    def _field(self, name):
        rows, pitch, cols = self.fields[name]
        return self.arena.view(name).view(self.B, rows, pitch), cols

    def set_state(self, grids_state):
        """grids_state[b][name]: dense numpy arrays.  Pad columns are (re)filled with the fill word."""
        t = self.torch
        for name in self.fields:
            v, cols = self._field(name)
            v.view(t.int32).fill_(self.fill)
            dense = np.stack([g[name].reshape(-1, g[name].shape[-1]) for g in grids_state])
            v[:, :, :cols] = t.from_numpy(dense).to(self.dev)

    def live(self, name):
        v, cols = self._field(name)
        return v[:, :, :cols].clone().contiguous()              # (a copy even where pitch == columns: the state moves on)

    def frames(self, name):
        """[T][B][n] of the frame buffer `name`."""
        fsb, fst, T = self.frame_specs[name]
        return self.arena.view(name).as_strided((T, self.B, self.n), (fst, fsb, 1)).clone().contiguous()

    def frame_gap_damage(self):
        """Words of the frame buffers' spans that belong to no frame and no longer hold the fill."""
        t, bad = self.torch, 0
        for name, (fsb, fst, T) in self.frame_specs.items():
            words = self.arena.view(name).view(t.int32)
            gap = t.ones(words.numel(), dtype=t.bool, device=self.dev)
            gap.as_strided((T, self.B, self.n), (fst, fsb, 1)).fill_(False)
            bad += int(((words != self.fill) & gap).sum())
        return bad

    def guard_damage(self):
        return self.arena.guard_damage(self.fill)


def same(got, want_np):
    """Equality with the oracle as the stepper tests define it (numpy's array_equal: values, NaN equal to NaN); got: a device tensor."""
    g = got.detach().cpu().numpy().reshape(-1)
    w = np.ascontiguousarray(want_np).reshape(-1)
    if g.shape != w.shape:
        return False
    return bool(np.array_equal(g, w, equal_nan=g.dtype.kind == "f"))


def digest(tensors):
    h = hashlib.sha1()
    for x in tensors:
        h.update(x.detach().cpu().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ one 2-D case
def frame_specs_2d(H, W):
    n, T = H * W, STEPS_PER_CALL
    fsb = n + 3
    fst = B2 * fsb + 5
    tst = n + 3                                  # transposed ([B][T] order): frame_stride_t < frame_stride_b
    return {"frames_tb": (fsb, fst, T), "frames_bt": (T * tst + 5, tst, T)}


def run_case_2d(H, W, J, layout, vel, fill):
    """Everything one 2-D case asserts, for one velocity scale and one fill: returns {"bad": [what differs from the oracle], "guards":
    damaged words, "describe": ..., "digest": of every live result}."""
    t = None
    ref = reference_2d(H, W, J, vel)
    run = LayoutRun((H, W), J, layout, fill, frame_specs_2d(H, W)).create()
    t, L, _lib, a = run.torch, run.lib, run._lib, run.arena
    bad, digs = [], []
    try:
        desc = run.describe()

        def check(tag, names=KEYS2):
            t.cuda.synchronize()
            for k in names:
                got = run.live(k)
                digs.append(got)
                if not same(got, np.stack([g["stages"][tag][k] if tag in g["stages"] else g["ends"][int(tag[3:])][k] for g in ref])):
                    bad.append(f"{tag}: {k}")
        # ---- single stages
        run.set_state([g["init"] for g in ref])
        _lib.check(L.smk_sim_run_stage(run.handle, _lib.STAGE_BUOY_DIFFUSE, run.st())); check("buoy_diffuse")
        _lib.check(L.smk_sim_divergence(run.handle, a.ptr("div"), run.st()))
        t.cuda.synchronize()
        digs.append(a.view("div").clone())
        if not same(a.view("div"), np.stack([g["stages"]["div"] for g in ref])):
            bad.append("divergence")
        _lib.check(L.smk_sim_run_stage(run.handle, _lib.STAGE_PROJECT, run.st())); check("project")
        for which, (stage, tag, R, Cc) in enumerate(((_lib.STAGE_ADVECT_U, "advect_u", H + 1, W), (_lib.STAGE_ADVECT_V, "advect_v", H, W + 1),
                                                     (_lib.STAGE_ADVECT_D, "advect_d", H, W))):
            _lib.check(L.smk_sim_backtrace(run.handle, which, a.ptr("x0"), a.ptr("y0"), run.st()))
            t.cuda.synchronize()
            for nm in ("x0", "y0"):
                got = a.view(nm)[:B2 * R * Cc]
                digs.append(got.clone())
                if not same(got, np.stack([g["stages"][f"{tag}_{nm}"] for g in ref])):
                    bad.append(f"backtrace {which}: {nm}")
            _lib.check(L.smk_sim_run_stage(run.handle, stage, run.st())); check(tag)
        # ---- whole steps: two calls of STEPS_PER_CALL; scale 0.5: [T][B] frames with gaps (+ the fractal multiplier on square grids),
        # then the transposed order; scale 300: [T][B] frames, then no frames at all
        run.set_state([g["init"] for g in ref])
        fractal = None
        if H == W:                                   # the library's own [W][H] constant (its sin / cos sums are held to the oracle's elsewhere)
            fractal = t.empty(H * W, dtype=t.float32, device=run.dev)
            _lib.check(L.smk_fractal_constants(H, None, None, fractal.data_ptr(), run.st()))
        plans = [("frames_tb", 1 if (fractal is not None and vel == VELS[0]) else 0), ("frames_bt" if vel == VELS[0] else None, 0)]
        for call, (fname, add_fractal) in enumerate(plans):
            if fname is None:
                _lib.check(L.smk_sim_step(run.handle, STEPS_PER_CALL, None, 0, 0, 0, 0.05, run.st()))
            else:
                fsb, fst, T = run.frame_specs[fname]
                _lib.check(L.smk_sim_step(run.handle, STEPS_PER_CALL, a.ptr(fname), fsb, fst, add_fractal, 0.05, run.st()))
            check(f"end{call}")
            if fname is not None:
                got = run.frames(fname)
                digs.append(got)
                want = np.stack([np.stack([g["frames"][call * STEPS_PER_CALL + s].reshape(-1) for g in ref]) for s in range(STEPS_PER_CALL)])
                if add_fractal:
                    import oracle
                    Fh = fractal.cpu().numpy().reshape(W, H)
                    want = np.stack([np.stack([oracle.apply_fractal_perturbation(f.reshape(H, W), 0.05, Fh).reshape(-1) for f in step]) for step in want])
                if not same(got, want):
                    bad.append(f"frames of call {call} ({fname}, add_fractal {add_fractal})")
        t.cuda.synchronize()
        guards = int(run.guard_damage()) + run.frame_gap_damage()
    finally:
        run.destroy()
    return {"bad": bad, "guards": guards, "describe": desc, "digest": digest(digs)}


# ------------------------------------------------------------------------------------------------ one 3-D case
def frame_specs_3d(D, H, W):
    n, T = D * H * W, STEPS_3D
    fsb = n + 3
    fst = B3 * fsb + 5
    tst = n + 3
    return {"frames_tb": (fsb, fst, T), "frames_bt": (T * tst + 5, tst, T)}


def run_case_3d(D, H, W, J, layout, vel, fill):
    """As run_case_2d, on smk_sim3d_run_stage, smk_sim3d_step and smk_sim3d_step_emit."""
    ref = reference_3d(D, H, W, J, vel)
    run = LayoutRun((D, H, W), J, layout, fill, frame_specs_3d(D, H, W), three_d=True).create()
    t, L, _lib, a = run.torch, run.lib, run._lib, run.arena
    bad, digs = [], []
    try:
        desc = run.describe()

        def check(tag):
            t.cuda.synchronize()
            for k in KEYS3:
                got = run.live(k)
                digs.append(got)
                if not same(got, np.stack([g["stages"][tag][k] if tag in g["stages"] else g["ends"][int(tag[3:])][k] for g in ref])):
                    bad.append(f"{tag}: {k}")
        run.set_state([g["init"] for g in ref])
        for stage, tag in enumerate(("buoy_diffuse", "project", "advect_u", "advect_v", "advect_w", "advect_d")):      # smk_stage3d
            _lib.check(L.smk_sim3d_run_stage(run.handle, stage, run.st())); check(tag)
        run.set_state([g["init"] for g in ref])
        for call, fname in enumerate(("frames_tb", "frames_bt" if vel == VELS[0] else None)):
            fsb, fst, T = run.frame_specs[fname] if fname else (0, 0, 0)
            ptr = a.ptr(fname) if fname else None
            if call == 0:
                _lib.check(L.smk_sim3d_step(run.handle, STEPS_3D, ptr, fsb, fst, run.st()))
            else:
                _lib.check(L.smk_sim3d_step_emit(run.handle, STEPS_3D, ptr, fsb, fst, 0, 0.05, run.st()))
            check(f"end{call}")
            if fname:
                got = run.frames(fname)
                digs.append(got)
                want = np.stack([np.stack([g["frames"][call * STEPS_3D + s].reshape(-1) for g in ref]) for s in range(STEPS_3D)])
                if not same(got, want):
                    bad.append(f"frames of call {call} ({fname})")
        t.cuda.synchronize()
        guards = int(run.guard_damage()) + run.frame_gap_damage()
    finally:
        run.destroy()
    return {"bad": bad, "guards": guards, "describe": desc, "digest": digest(digs)}


def run_wrapper_class_2d(H, W, J, vel):
    """The digest run_case_2d forms, from the Python class (its own tensors, dense [B][T] frame buffers) through the same sequence on the
    same states."""
    import torch
    from smokephysai_amd import _lib
    from smokephysai_amd.physics import NavierStokesSimulator
    ref = reference_2d(H, W, J, vel)
    ns = NavierStokesSimulator((H, W), batch_size=B2, jacobi_iters=J)
    digs = []

    def load():
        for k in KEYS2:
            setattr(ns, k, torch.from_numpy(np.stack([g["init"][k] for g in ref])))

    def state():
        torch.cuda.synchronize()
        digs.extend(getattr(ns, k).contiguous().clone() for k in KEYS2)
    load()
    ns.run_stage(_lib.STAGE_BUOY_DIFFUSE); state()
    digs.append(ns.divergence().reshape(-1))
    ns.run_stage(_lib.STAGE_PROJECT); state()
    for which, stage in enumerate((_lib.STAGE_ADVECT_U, _lib.STAGE_ADVECT_V, _lib.STAGE_ADVECT_D)):
        x0, y0 = ns.backtrace_indices(which)
        digs += [x0.reshape(-1), y0.reshape(-1)]
        ns.run_stage(stage); state()
    load()
    for call, (frames, add_fractal) in enumerate(((True, H == W and vel == VELS[0]), (vel == VELS[0], False))):
        fr = torch.empty(B2, STEPS_PER_CALL, H, W, device=ns.u.device) if frames else None
        ns.step_into(fr, STEPS_PER_CALL, add_fractal=add_fractal, fractal_intensity=0.05)
        state()
        if frames:
            digs.append(fr.permute(1, 0, 2, 3).contiguous())
    return digest(digs)


def run_wrapper_class_3d(D, H, W, J, vel):
    """The digest run_case_3d forms, from NavierStokesSimulator3D (its own tensors, dense [B][T] frame buffers) through the same stages
    and the same two calls of STEPS_3D steps on the same states (the class makes both through step_into, which calls smk_sim3d_step where
    no fractal is asked for: what smk_sim3d_step_emit with add_fractal 0 is specified to equal)."""
    import torch
    from smokephysai_amd.physics import NavierStokesSimulator3D
    ref = reference_3d(D, H, W, J, vel)
    ns = NavierStokesSimulator3D((D, H, W), batch_size=B3, jacobi_iters=J)
    digs = []

    def load():
        for k in KEYS3:
            setattr(ns, k, torch.from_numpy(np.stack([g["init"][k] for g in ref])))

    def state():
        torch.cuda.synchronize()
        digs.extend(getattr(ns, k).contiguous().clone().reshape(B3, -1, getattr(ns, k).shape[-1]) for k in KEYS3)
    load()
    for stage in range(6):
        ns.run_stage(stage); state()
    load()
    for frames in (True, vel == VELS[0]):
        fr = torch.empty(B3, STEPS_3D, D, H, W, device=ns.u.device) if frames else None
        ns.step_into(fr, STEPS_3D)
        state()
        if frames:
            digs.append(fr.permute(1, 0, 2, 3, 4).contiguous())
    return digest(digs)
