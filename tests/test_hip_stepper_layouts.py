"""The steppers at every state layout the C ABI accepts (include/smokehip.h "state layouts"; DESIGN "Stepper state layouts"): the table
of tests/stepper_layout_cases.py through smk_sim_create / smk_sim3d_create by ctypes, every field and frame carved from one guarded arena.

Every case -- a shape x a layout (pitches, base-pointer offsets; frames with gaps, off 16 bytes, transposed, absent) -- runs at velocity
scales 0.5 and 300 (the near and the far branch of the advection) and with pad columns, guards and frame gaps filled with 0xFFFFFFFF and
with 0, and asserts:
  (a) u, v, p, density (and w), the divergence, the back-trace indices and all frames equal the oracle's after every single stage and
      after two calls of whole steps (equality as the existing stepper tests define it: numpy's array_equal);
  (b) the two fills give identical bits; (c) no guard word and no word between frames changed;
  (d) smk_sim_describe / smk_sim3d_describe report the form the case is listed for (the table's strings: the gates are not re-derived);
  (e) all layouts of a shape give the bits of the classes' own layout, and those of the Python class on the same states.
2-D cases run in one child process per SMK_JACOBI_PERSIST setting (the switch is read once per process)."""
import json
import os
import subprocess
import sys

import pytest

import stepper_layout_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_results = {}


def _child(persist):
    """The child's results; it runs once per setting whatever its outcome, and not at all after another child ended abnormally."""
    if persist not in _results:
        assert not any(isinstance(v, str) for v in _results.values()), "an earlier child process ended abnormally: " + str(_results)
        env = dict(os.environ)
        env["SMK_JACOBI_PERSIST"] = persist
        env.pop("SMK_JACOBI_FAULT", None)
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_stepper_layout_child.py")], env=env, capture_output=True, text=True,
                               timeout=900)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            _results[persist] = json.loads(lines[-1][len("RESULT "):]) if r.returncode == 0 and lines else \
                f"exit status {r.returncode}: {r.stdout[-1500:]} {r.stderr[-3000:]}"
        except subprocess.TimeoutExpired as e:
            _results[persist] = f"timed out: {e}"
    assert not isinstance(_results[persist], str), _results[persist]
    return _results[persist]


def _check_runs(runs, want_describe):
    for key, r in runs.items():
        assert r["bad"] == [], (key, r["bad"])                         # (a)
        assert r["guards"] == 0, (key, r["guards"])                    # (c)
        want_describe(key, r["describe"])                              # (d)
    for vel in S.VELS:                                                 # (b)
        assert runs[f"{vel}/{S.FILLS[0]}"]["digest"] == runs[f"{vel}/{S.FILLS[1]}"]["digest"], vel


@pytest.mark.parametrize("persist", ["1", "0"], ids=["persist", "launches"])
@pytest.mark.parametrize("case", S.case_ids_2d())
def test_2d_layout(case, persist):
    res = _child(persist)
    runs = res["cases"][case]
    shape, j, layout = case.split("-")
    H, W = map(int, shape.split("x"))
    want = S.forms_2d(H, W, layout, persist == "1")

    def describe(key, d):
        assert d["projection"]["kernel"] == want["kernel"], (key, d)
        if want["kernel"] != "k_jacobi_sweep":
            assert d["projection"]["persistent"] == (persist == "1"), (key, d)
        assert d["buoy_diffuse"] == want["buoy_diffuse"], (key, d)
        assert d["buoy_diffuse_stage"] == S.forms_2d(H, W, layout, False)["buoy_diffuse"], (key, d)      # (run alone, the stage never folds)
        lay = S.LAYOUT[layout]
        assert (d["alignment"]["pitch_c"], d["alignment"]["pitch_v"]) == (lay.pc(W), lay.pv(W)), (key, d)
    _check_runs(runs, describe)
    for vel in S.VELS:                                                 # (e)
        mine = runs[f"{vel}/0"]["digest"]
        assert mine == res["cases"][f"{shape}-{j}-wrapper"][f"{vel}/0"]["digest"], vel
        assert mine == res["class"][f"{shape}-{j}-{vel}"], vel


_fixed_3d = {}


def _fixed_digests_3d(D, H, W, J):
    """Per shape, once: the digests of the classes' own layout (fill 0) and of NavierStokesSimulator3D, per velocity scale -- what every
    case of the shape is compared with, whichever cases run and in whatever order."""
    if (D, H, W) not in _fixed_3d:
        _fixed_3d[(D, H, W)] = {vel: (S.run_case_3d(D, H, W, J, S.LAYOUT["wrapper"], vel, 0)["digest"], S.run_wrapper_class_3d(D, H, W, J, vel))
                                for vel in S.VELS}
    return _fixed_3d[(D, H, W)]


@pytest.mark.parametrize("case", S.case_ids_3d())
def test_3d_layout(case):
    shape, j, layout = case.split("-")
    D, H, W = map(int, shape.split("x"))
    J = int(j[1:])
    want = S.forms_3d(D, H, W, layout)
    runs = {f"{vel}/{fill}": S.run_case_3d(D, H, W, J, S.LAYOUT[layout], vel, fill) for vel in S.VELS for fill in S.FILLS}

    def describe(key, d):
        assert (d["jacobi"], d["jacobi_sweep"], d["alignment"]["vec"], d["alignment"]["quad"]) == \
            (want["jacobi"], want["jacobi_sweep"], want["vec"], want["quad"]), (key, d)
    _check_runs(runs, describe)
    fixed = _fixed_digests_3d(D, H, W, J)
    for vel in S.VELS:                                                 # (e)
        assert runs[f"{vel}/0"]["digest"] == fixed[vel][0], vel
        assert runs[f"{vel}/0"]["digest"] == fixed[vel][1], vel


# ------------------------------------------------------------------------------------------------ the stateless field helpers
def _helper_call(bufs, inputs, call, outs):
    """One stateless call on a guarded arena, once per fill: bufs name -> (elements, byte offset from 16-byte alignment, dtype); inputs
    name -> (numpy [planes][rows][cols], pitch, plane stride) written into a fill-initialised buffer; returns the outputs of the fill-0 run
    after holding the two fills' to each other and the guards to their fill."""
    import numpy as np
    import torch
    from guarded_arena import Arena, Buf
    from smokephysai_amd import _lib
    results = []
    for fill in S.FILLS:
        arena = Arena([Buf(n, dt, e, align=16 if off == 0 else 4, phase=None if off == 0 else off, role="inout") for n, (e, off, dt) in bufs.items()])
        arena.fill(fill)
        for name, (arr, pitch, stride) in inputs.items():
            P, R, Cc = arr.shape
            arena.view(name).as_strided((P, R, Cc), (stride, pitch, 1)).copy_(torch.from_numpy(arr).to(arena.buf.device))
        _lib.check(call(_lib.load(), arena, _lib.stream_ptr(arena.buf.device)))
        torch.cuda.synchronize()
        got = {}
        for name, (shape, strides) in outs.items():
            live = arena.view(name).as_strided(shape, strides).clone()
            got[name] = live.cpu().numpy()
            mask = torch.ones(arena.view(name).numel(), dtype=torch.bool, device=arena.buf.device)      # the output's pad words hold the fill
            mask.as_strided(shape, strides).fill_(False)
            assert int(((arena.view(name).view(torch.int32) != fill) & mask).sum()) == 0, (name, fill)
        for name, (arr, pitch, stride) in inputs.items():                                                # inputs come back unchanged
            P, R, Cc = arr.shape
            back = arena.view(name).as_strided((P, R, Cc), (stride, pitch, 1)).cpu().numpy()
            assert np.array_equal(back.view(np.int32), arr.view(np.int32)), name
        assert arena.guard_damage(fill) == 0, str(arena.guard_damage(fill))
        results.append(got)
    for name in outs:
        assert np.array_equal(results[0][name].view(np.int32), results[1][name].view(np.int32)), name
    return results[1]


_PITCHES = [("dense", lambda C: C, 0, 0), ("plus4-off", lambda C: C + 4, 4, 8), ("plus3", lambda C: C + 3, 0, 12), ("pad32-off", S.up32, 12, 4)]


@pytest.mark.parametrize("pitch_id", [p[0] for p in _PITCHES])
@pytest.mark.parametrize("R,C", [(33, 50), (65, 64)])
def test_smk_diffuse_at_every_pitch(R, C, pitch_id):
    import numpy as np
    import torch
    import oracle
    _, pf, off_in, off_out = next(p for p in _PITCHES if p[0] == pitch_id)
    pitch, B = pf(C), 3
    rng = np.random.RandomState(R * C)
    f = (rng.standard_normal((B, R, C)) * 3).astype(np.float32)
    n = B * R * pitch
    got = _helper_call({"in": (n, off_in, torch.float32), "out": (n, off_out, torch.float32)}, {"in": (f, pitch, R * pitch)},
                       lambda L, a, st: L.smk_diffuse(a.ptr("in"), a.ptr("out"), B, R, C, pitch, 0.01, 0.001, st),
                       {"out": ((B, R, C), (R * pitch, pitch, 1))})["out"]
    o = oracle.OracleNS((R, C))
    np.testing.assert_array_equal(got, np.stack([o.diffusion_step(f[b], 0.001) for b in range(B)]))


@pytest.mark.parametrize("layout", ["dense", "vodd", "odd", "offset", "wrapper"])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("vel", S.VELS)
def test_smk_advect_at_every_pitch_gives_the_stage_s_bits(vel, which, layout):
    """smk_advect on the projected state of the layout table's 70 x 131 case: the field smk_sim_run_stage's advection of the same inputs
    leaves (test_2d_layout holds that stage to the same oracle values); which = 2 is the plain advection, without the decay."""
    import numpy as np
    import torch
    import oracle
    from smokephysai_amd import _lib
    H, W, J = 70, 131, 6
    ref = S.reference_2d(H, W, J, vel)
    lay, B = S.LAYOUT[layout], S.B2
    pc, pv = lay.pc(W), lay.pv(W)
    proj = [g["stages"]["project"] for g in ref]
    u_in = np.stack([(g["stages"]["advect_u"] if which >= 1 else g["stages"]["project"])["u"] for g in ref])
    v_in = np.stack([(g["stages"]["advect_v"] if which == 2 else g["stages"]["project"])["v"] for g in ref])
    field = [u_in, v_in, np.stack([p["density"] for p in proj])][which]
    R, Cc, pitch = [(H + 1, W, pc), (H, W + 1, pv), (H, W, pc)][which]
    if which == 0:
        want = np.stack([g["stages"]["advect_u"]["u"] for g in ref])
    elif which == 1:
        want = np.stack([g["stages"]["advect_v"]["v"] for g in ref])
    else:
        o = oracle.OracleNS((H, W))
        want = np.stack([o.advection_step(field[b], u_in[b], v_in[b]) for b in range(B)])
    offs = lay.off
    bufs = {"field": (B * R * pitch, offs[3], torch.float32), "out": (B * R * pitch, offs[2], torch.float32),
            "u": (B * (H + 1) * pc, offs[0], torch.float32), "v": (B * H * pv, offs[1], torch.float32)}
    got = _helper_call(bufs, {"field": (field, pitch, R * pitch), "u": (u_in, pc, (H + 1) * pc), "v": (v_in, pv, H * pv)},
                       lambda L, a, st: L.smk_advect(a.ptr("field"), a.ptr("out"), which, a.ptr("u"), a.ptr("v"), B, H, W, pc, pv, 0.01, st),
                       {"out": ((B, R, Cc), (R * pitch, pitch, 1))})["out"]
    np.testing.assert_array_equal(got, want)
    # ... and, to the bit, what the matching smk_sim_run_stage leaves in the same layout from the same inputs (the density stage decays
    # its result: one float32 multiply by 0.995 on top of the plain advection)
    run = S.LayoutRun((H, W), J, lay, 0, {}).create()
    try:
        run.set_state([{"u": u_in[b], "v": v_in[b], "p": proj[b]["p"], "density": proj[b]["density"]} for b in range(B)])
        _lib.check(run.lib.smk_sim_run_stage(run.handle, [_lib.STAGE_ADVECT_U, _lib.STAGE_ADVECT_V, _lib.STAGE_ADVECT_D][which], run.st()))
        torch.cuda.synchronize()
        stage = run.live(["u", "v", "density"][which]).cpu().numpy()
    finally:
        run.destroy()
    mine = got if which < 2 else (got * np.float32(0.995)).astype(np.float32)
    assert np.array_equal(mine.view(np.int32), stage.view(np.int32))


@pytest.mark.parametrize("coords", ["shared", "dense", "strided"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_smk_interpolate_with_pitches_strides_and_far_coordinates(mode, coords):
    """pitch > w, field_stride > h * pitch, coord_stride 0 / n / n + 7, n no multiple of the 256-thread block, every mode; coordinates
    from well inside the field to far outside it (the reference floors and clamps: any float is legal)."""
    import numpy as np
    import torch
    import oracle
    B, h, w, n = 3, 37, 53, 777
    pitch, fstride = w + 5, h * (w + 5) + 11
    cstride = {"shared": 0, "dense": n, "strided": n + 7}[coords]
    rng = np.random.RandomState(100 * mode + cstride)
    f = rng.standard_normal((B, h, w)).astype(np.float32)
    nc = 1 if cstride == 0 else B
    ys = (rng.uniform(-3, h + 3, (nc, 1, n))).astype(np.float32)
    xs = (rng.uniform(-3, w + 3, (nc, 1, n))).astype(np.float32)
    for arr, far in ((ys, 1e9), (xs, -3e7)):                          # far outside, both signs, and the exact edges
        arr[:, 0, :8] = [far, -far, 0.0, -0.0, 2e18, -2e18, 0.5, -0.5]      # (within int64, which the reference floors to)
    ys[:, 0, 8:10], xs[:, 0, 8:10] = [h - 1, h], [w - 1, w]
    bufs = {"field": ((B - 1) * fstride + h * pitch, 4, torch.float32), "y": ((nc - 1) * max(cstride, 1) + n, 8, torch.float32),
            "x": ((nc - 1) * max(cstride, 1) + n, 12, torch.float32), "out": (B * n, 4, torch.float32)}
    got = _helper_call(bufs, {"field": (f, pitch, fstride), "y": (ys, n, max(cstride, 1)), "x": (xs, n, max(cstride, 1))},
                       lambda L, a, st: L.smk_interpolate(mode, a.ptr("field"), B, h, w, pitch, fstride, a.ptr("y"), a.ptr("x"), cstride, n, a.ptr("out"), st),
                       {"out": ((B, n), (n, 1))})["out"]
    fn = [oracle.bilinear_interpolate, oracle.interpolate_velocity_u, oracle.interpolate_velocity_v][mode]
    want = np.stack([fn(f[b], ys[b % nc, 0], xs[b % nc, 0]) for b in range(B)])
    np.testing.assert_array_equal(got, want)


def test_the_3d_class_reports_its_jacobi_form():
    """NavierStokesSimulator3D.jacobi_plan(): the table's row of the class's own layout."""
    from smokephysai_amd.physics import NavierStokesSimulator3D
    D, H, W, J = S.SHAPES_3D[0]
    d = NavierStokesSimulator3D((D, H, W), batch_size=S.B3, jacobi_iters=J).jacobi_plan()
    want = S.forms_3d(D, H, W, "wrapper")
    assert (d["jacobi"], d["jacobi_sweep"], d["alignment"]["vec"], d["alignment"]["quad"]) == (want["jacobi"], want["jacobi_sweep"], want["vec"], want["quad"])
    assert d["alignment"]["pitch_c"] == S.up32(W) and d["alignment"]["pressure_bytes"] == 16
