"""The 3-D flow map and its FTLE on the device (physics.flow_map_step3d, ftle_field3d, flow_ftle3d; csrc/flow_map3d.hip) against the oracle
of DESIGN.md 3.14 / 3.15: the rule in fp64 along the Branches recorded by the fp32 CPU run of the rule (tests/flow_map3d_oracle.py).  The
replay is that fp32 CPU run.  Metric per field max|x - ref| / max|ref| (exactly 0 where max|ref| is 0); bound: 10 x the replay's worst
over the same cases, per quantity.  Cases: grids (3,3,3), (4,5,7), (9,19,37), (12,33,40) with B = 1 and 3 at amplitude 5, the state at
rest, an amplitude-300 state on (6,12,16) whose traces leave through all six faces, the last-index quirk; chained runs of 1 and 4 steps in
both directions; smk_ftle3d_field alone also on (16,272,8), whose runs of rows exceed 16.  The single kernels run on odd pitches whose NaN
padding must stay NaN.

Figures measured on MI355X, worst over the cases (device / replay; profiles/r33/test_figures.txt has every case, DESIGN.md 3.15 the table).
The displacements' figures are the replay's to four digits in every case; the FTLE's differ from it in single cases (the device's log1p):
  smk_flow_map3d_step ...... backward 1.531e-06 / 1.531e-06     forward 4.956e-07 / 4.956e-07
  smk_ftle3d_field ......... drawn displacement 1.508e-07 / 1.508e-07 (at 16x272x8)     1e-4 of it 1.977e-07 / 1.909e-07
  flow_ftle3d, 1 step ...... backward ftle 1.743e-06 / 1.817e-06, displacement 2.803e-06 / 2.803e-06
                             forward  ftle 1.843e-06 / 1.843e-06, displacement 2.518e-06 / 2.518e-06
  flow_ftle3d, 4 steps ..... backward ftle 3.065e-06 / 3.065e-06, displacement 4.809e-06 / 4.809e-06
                             forward  ftle 2.584e-06 / 2.584e-06, displacement 4.157e-06 / 4.157e-06"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import flow_map3d_oracle as F                                                                     # noqa: E402
import step3d_grad_oracle as O                                                                    # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import (NavierStokesSimulator3D, SmokeSimulator3D, flow_ftle3d, flow_map_step3d,        # noqa: E402
                                     flow_map_step3d_rule, ftle_field3d)

DEV = "cuda"
CASES = F.cases()
case_param = pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
PAD = -7.0
LONG = "x".join(str(n) for n in F.LONG_ROWS) + "-B2-field"


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _stream():
    return _lib.stream_ptr(torch.device(DEV, 0))


def _pitched(t, pitch):
    """[..., R, C] CPU tensor -> a device buffer [..., R, pitch] full of NaN with t in its first C columns."""
    buf = torch.full(tuple(t.shape[:-1]) + (pitch,), float("nan"), device=DEV)
    buf[..., :t.shape[-1]] = t.to(DEV)
    return buf


def _padding_is_nan(buf, cols):
    return bool(torch.isnan(buf[..., cols:]).all())


def _map_step_pitched(direction, disp, u, v, w, dt=F.DT):
    """One smk_flow_map3d_step on buffers with odd pitches whose padding is NaN (the output's too) -> (disp' [B, 3, D, H, W], whether
    every padding is still NaN)."""
    B, _, D, H, W = disp.shape
    pc, pv, pm = (W + 2) | 1, (W + 3) | 1, (W + 4) | 1
    u_b, v_b, w_b, d_b = _pitched(u, pc), _pitched(v, pv), _pitched(w, pc), _pitched(disp, pm)
    out = torch.full((B, 3, D, H, pm), float("nan"), device=DEV)
    _lib.check(_lib.load().smk_flow_map3d_step(F.DIRECTIONS.index(direction), u_b.data_ptr(), v_b.data_ptr(), w_b.data_ptr(), d_b.data_ptr(),
                                               out.data_ptr(), B, D, H, W, pc, pv, pm, dt, _stream()))
    pads = (_padding_is_nan(out, W) and _padding_is_nan(u_b, W) and _padding_is_nan(v_b, W + 1) and _padding_is_nan(w_b, W) and
            _padding_is_nan(d_b, W))
    return out[..., :W].contiguous(), pads


def _ftle_pitched(disp, horizon):
    """smk_ftle3d_field on an odd pitch with NaN padding -> (ftle [B, D, H, W], stats [B, 2], whether the paddings are still NaN)."""
    B, _, D, H, W = disp.shape
    L = _lib.load()
    pm = (W + 4) | 1
    d_b = _pitched(disp, pm)
    out = torch.full((B, D, H, pm), float("nan"), device=DEV)
    stats = torch.full((B, 2), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = int(L.smk_ftle3d_workspace(B, D, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    _lib.check(L.smk_ftle3d_field(d_b.data_ptr(), out.data_ptr(), stats.data_ptr(), B, D, H, W, pm, horizon, ws.data_ptr(), nbytes, _stream()))
    return out[..., :W].contiguous(), stats, _padding_is_nan(out, W) and _padding_is_nan(d_b, W)


def _check_stats(ftle, stats, what):
    """stats against torch's fp64 mean and max of the device's own field: relative 1e-12 for the mean, exact for the max."""
    flat = ftle.double().flatten(1)
    mean, top = flat.mean(dim=1), flat.max(dim=1).values
    assert torch.equal(stats[:, 1], top), f"{what}: max {stats[:, 1].tolist()} against {top.tolist()}"
    assert bool(((stats[:, 0] - mean).abs() <= 1e-12 * mean.abs()).all()), f"{what}: mean {stats[:, 0].tolist()} against {mean.tolist()}"


def _field_figures(cid, disp0, refs):
    """smk_ftle3d_field on the drawn displacement and on 1e-4 of it: pitched against dense, the statistics, the two figures."""
    figs = {}
    for name, disp, horizon in F.field_inputs(disp0):
        oracle, replay = refs["ftle_field", name]
        got, stats, pads = _ftle_pitched(disp, horizon)
        assert pads, f"{cid}: a pitch padding was written by smk_ftle3d_field"
        dense, mean, top = ftle_field3d(disp.to(DEV), horizon)
        assert _bits_equal(got, dense) and torch.equal(stats[:, 0], mean) and torch.equal(stats[:, 1], top), cid
        _check_stats(got, stats, cid)
        figs[f"ftle_field {name}"] = (O.metric(got, oracle), O.metric(replay, oracle))
    return figs


@functools.lru_cache(maxsize=None)
def _long_rows_disp():
    return F.draw_disp3d(F.LONG_ROWS, 2, 1.5)


@functools.lru_cache(maxsize=None)
def _case_figures(cid):
    """Everything one case measures, once: {quantity: (device figure, replay figure)}, with the checks that are not figures made on the
    way (paddings, the dense call, the statistics)."""
    if cid == LONG:
        disp0 = _long_rows_disp()
        return _field_figures(cid, disp0, {("ftle_field", name): F.ftle3d_oracle(d, h) for name, d, h in F.field_inputs(disp0)})
    _, state, disp0 = next(c for c in CASES if c[0] == cid)
    refs = F.references(cid)
    dstate = [s.to(DEV) for s in state]
    figs = {}
    for direction in F.DIRECTIONS:
        oracle, replay = refs["map_step", direction]
        got, pads = _map_step_pitched(direction, disp0, *state[:3])
        assert pads, f"{cid} {direction}: a pitch padding was written"
        dense = flow_map_step3d(disp0.to(DEV), *dstate[:3], dt=F.DT, direction=direction)
        assert _bits_equal(got, dense), f"{cid} {direction}: the pitched call differs from physics.flow_map_step3d"
        figs[f"map_step {direction}"] = (O.metric(got, oracle), O.metric(replay, oracle))
    figs.update(_field_figures(cid, disp0, refs))
    for n_steps in F.CHAIN_STEPS:
        for direction in F.DIRECTIONS:
            oracle, replay = refs["flow_ftle", direction, n_steps]
            got = flow_ftle3d(*dstate, n_steps, dt=F.DT, viscosity=F.NU, jacobi_iters=F.J, direction=direction)
            _check_stats(got.ftle, torch.stack([got.mean, got.max], dim=1), cid)
            key = f"flow_ftle {direction} x{n_steps}"
            figs[key + " ftle"] = (O.metric(got.ftle, oracle.ftle), O.metric(replay.ftle, oracle.ftle))
            figs[key + " displacement"] = (O.metric(got.displacement, oracle.displacement), O.metric(replay.displacement, oracle.displacement))
    return figs


ALL_IDS = [c[0] for c in CASES] + [LONG]


# ------------------------------------------------------------------------------------------------ 1. the cases, one by one
@pytest.mark.parametrize("cid", ALL_IDS)
def test_case_runs_clean(cid):
    """Per case: paddings untouched, the pitched calls equal the dense ones, the statistics are the field's; every figure is finite, and
    exactly 0 where the oracle is 0."""
    for key, (dev, rep) in _case_figures(cid).items():
        print(f"FIG {cid:20s} {key:36s} device {dev:.3e}  replay {rep:.3e}")
        assert dev == dev and dev != float("inf"), f"{cid} {key}: {dev}"
    if cid.endswith("rest"):
        assert all(dev == 0.0 and rep == 0.0 for dev, rep in _case_figures(cid).values())


def test_the_far_state_leaves_through_all_six_faces():
    state = next(s for cid, s, _ in CASES if cid.endswith("a300"))
    assert F.leaves_through_all_six_faces(state)


# ------------------------------------------------------------------------------------------------ 2. the bounds, per quantity over all cases
def test_every_quantity_stays_within_ten_times_the_replay():
    worst = {}
    for cid in ALL_IDS:
        for key, (dev, rep) in _case_figures(cid).items():
            w = worst.setdefault(key, [0.0, 0.0, None])
            if dev > w[0]:
                w[0], w[2] = dev, cid
            w[1] = max(w[1], rep)
    failed = []
    for key, (dev, rep, where) in worst.items():
        print(f"FIG worst                {key:36s} device {dev:.3e} (at {where})  replay {rep:.3e}  bound {F.REPLAY_MARGIN * rep:.3e}")
        if not dev <= F.REPLAY_MARGIN * rep:
            failed.append(key)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 3. the density advection's own trace, exactly
@pytest.mark.parametrize("batch", [1, 3])
def test_one_backward_step_from_zero_equals_the_fp32_rule_exactly(batch):
    """With a zero displacement the gathers add exact zeros, so the result is the increment alone: the density advection's samples,
    clamps and decisions, which the kernel forms with the forward's own expressions -- bit for bit the CPU rule's."""
    shape = (9, 19, 37)
    u, v, w, _, _ = O.draw_state3d(shape, 60.0, seed=5, batch=batch)
    zero = torch.zeros(batch, 3, *shape)
    want = flow_map_step3d_rule(zero, u, v, w, dt=F.DT, direction="backward")
    got = flow_map_step3d(zero.to(DEV), u.to(DEV), v.to(DEV), w.to(DEV), dt=F.DT, direction="backward")
    assert torch.equal(got.cpu(), want)
    assert bool((want.abs() > 0.5).any())                     # (the traces did move)


def test_the_returned_state_is_the_steppers_own():
    shape, n_steps = (9, 19, 37), 4
    state = [s.to(DEV) for s in O.draw_state3d(shape, 5.0, seed=6, batch=3)]
    sim = NavierStokesSimulator3D(shape, dt=F.DT, viscosity=F.NU, device=DEV, batch_size=3, jacobi_iters=F.J)
    sim.u, sim.v, sim.w, sim.p, sim.density = state
    sim.step_into(None, n_steps)
    want = sim.state()
    for direction in F.DIRECTIONS:
        got = flow_ftle3d(*state, n_steps, dt=F.DT, viscosity=F.NU, jacobi_iters=F.J, direction=direction)
        assert len(got.state) == 5
        for name, a, b in zip(("u", "v", "w", "p", "density"), got.state, want):
            assert _bits_equal(a, b), f"{direction}: the returned {name} is not the stepper's after {n_steps} steps"


# ------------------------------------------------------------------------------------------------ 4. determinism and batch independence
def test_two_calls_are_bit_equal_and_a_grid_does_not_depend_on_its_batch_mates():
    shape = (9, 19, 37)
    state = [s.to(DEV) for s in O.draw_state3d(shape, 5.0, seed=6, batch=3)]
    disp0 = F.draw_disp3d(shape, 3, 1.5).to(DEV)
    vel = state[:3]
    for direction in F.DIRECTIONS:
        a = flow_map_step3d(disp0, *vel, direction=direction)
        assert _bits_equal(a, flow_map_step3d(disp0, *vel, direction=direction))
        alone = flow_map_step3d(disp0[1:2], *[c[1:2] for c in vel], direction=direction)
        assert _bits_equal(alone[0], a[1]) and _bits_equal(flow_map_step3d(disp0[2], *[c[2] for c in vel], direction=direction), a[2])
        res = flow_ftle3d(*state, 4, direction=direction)
        again = flow_ftle3d(*state, 4, direction=direction)
        one = flow_ftle3d(*[s[1:2] for s in state], 4, direction=direction)
        single = flow_ftle3d(*[s[2] for s in state], 4, direction=direction)
        for name in ("ftle", "displacement", "mean", "max"):
            x = getattr(res, name)
            assert torch.equal(x, getattr(again, name)), (direction, name)
            assert torch.equal(x[1], getattr(one, name)[0]) and torch.equal(x[2], getattr(single, name)), (direction, name)
    f, mean, top = ftle_field3d(disp0, 0.08)
    f2, mean2, top2 = ftle_field3d(disp0, 0.08)
    assert _bits_equal(f, f2) and torch.equal(mean, mean2) and torch.equal(top, top2)
    f1, mean1, top1 = ftle_field3d(disp0[1], 0.08)
    assert _bits_equal(f1, f[1]) and float(mean1) == float(mean[1]) and float(top1) == float(top[1])


def test_a_nan_reaches_the_maximum_of_its_own_grid_only():
    disp0 = F.draw_disp3d((4, 5, 7), 2, 1.0)
    disp0[1, 2, 1, 2, 3] = float("nan")
    f, mean, top = ftle_field3d(disp0.to(DEV), 0.1)
    assert bool(torch.isfinite(f[0]).all()) and bool(torch.isfinite(top[0])) and bool(torch.isfinite(mean[0]))
    assert bool(torch.isnan(top[1])) and bool(torch.isnan(mean[1])) and bool(torch.isnan(f[1, 1, 1, 3]))


def test_refusals_of_the_entry_points():
    L = _lib.load()
    D, H, W = 4, 5, 7
    st = _stream()
    u, v, w = torch.zeros(1, D, H + 1, W, device=DEV), torch.zeros(1, D, H, W + 1, device=DEV), torch.zeros(1, D + 1, H, W, device=DEV)
    disp, out = torch.zeros(1, 3, D, H, W, device=DEV), torch.full((1, 3, D, H, W), PAD, device=DEV)
    ftle, stats = torch.full((1, D, H, W), PAD, device=DEV), torch.full((1, 2), PAD, dtype=torch.float64, device=DEV)
    ws = torch.empty(8, dtype=torch.float64, device=DEV)
    need = int(L.smk_ftle3d_workspace(1, D, H, W))
    assert need == 2 * 16

    def refused(rc, word):
        assert rc == _lib.SMK_ERR_INVALID and word in L.smk_last_error().decode(), (rc, L.smk_last_error().decode())
    step = lambda direction, u_, v_, w_, d_, o_, pm=W, dims=(1, D, H, W): L.smk_flow_map3d_step(                  # noqa: E731
        direction, u_, v_, w_, d_, o_, *dims, W, W + 1, pm, 0.01, st)
    ptr = lambda t: t.data_ptr()                                                                                  # noqa: E731
    refused(step(0, None, ptr(v), ptr(w), ptr(disp), ptr(out)), "null pointer")
    refused(step(0, ptr(u), ptr(v), None, ptr(disp), ptr(out)), "null pointer")
    refused(step(0, ptr(u), ptr(v), ptr(w), ptr(disp), None), "null pointer")
    refused(step(2, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(out)), "direction")
    refused(step(-1, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(out)), "direction")
    refused(step(0, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(disp)), "aliases")
    refused(step(1, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(w)), "aliases")
    refused(step(0, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(out), W - 1), "pitch_m >= W")
    refused(step(0, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(out), dims=(1, 2, H, W)), "3 <= D, H, W")
    refused(step(0, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(out), dims=(16384, D, H, W)), "B * (D + 1) <= 65535")
    refused(step(0, ptr(u), ptr(v), ptr(w), ptr(disp), ptr(out), pm=1 << 27), "D * H * pitch_m < 2^31")
    field = lambda d_, f_, s_, w_, n_, horizon=0.1, pm=W: L.smk_ftle3d_field(d_, f_, s_, 1, D, H, W, pm, horizon, w_, n_, st)       # noqa: E731
    refused(field(None, ptr(ftle), ptr(stats), ptr(ws), need), "null pointer")
    refused(field(ptr(disp), ptr(ftle), None, ptr(ws), need), "null pointer")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws), need - 1), "workspace")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), None, need), "workspace")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws) + 4, need), "8-byte")
    refused(field(ptr(disp), ptr(ftle), ptr(stats) + 4, ptr(ws), need), "8-byte")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws), need, horizon=bad), "horizon")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws), need, pm=W - 1), "pitch_m >= W")
    refused(field(ptr(disp), ptr(disp), ptr(stats), ptr(ws), need), "aliases")
    torch.cuda.synchronize()
    assert bool((out == PAD).all()) and bool((ftle == PAD).all()) and bool((stats == PAD).all())     # a refused call writes nothing


# ------------------------------------------------------------------------------------------------ 5. SmokeSimulator3D.flow_ftle
@pytest.mark.parametrize("batch", [None, 2], ids=["single", "batched"])
def test_flow_ftle_leaves_the_simulator_alone(batch):
    shape = (8, 16, 16)
    sim = SmokeSimulator3D(shape, device=DEV, batch_size=batch)
    sim.add_incense_source([(8, 10, 4)], [1.0])
    for _ in range(10):
        sim.simulate_step(add_fractal=False)
    ns = sim.ns_solver
    before = [t.clone() for t in ns.state()]
    feats = sim.get_chaos_features()
    ring, hist_len, pair = sim._ring.clone(), sim.history_len, sim._pair.clone()
    res = sim.flow_ftle(n_steps=8)
    want = flow_ftle3d(*before, 8, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters)
    if batch is None:
        assert tuple(res.ftle.shape) == shape and tuple(res.displacement.shape) == (3,) + shape
        assert isinstance(res.mean, float) and isinstance(res.max, float) and res.max >= res.mean and res.max > 0
        assert torch.equal(res.ftle, want.ftle[0]) and res.mean == float(want.mean[0]) and res.max == float(want.max[0])
    else:
        assert tuple(res.ftle.shape) == (2,) + shape and res.mean.dtype == torch.float64 and bool(torch.isfinite(res.ftle).all())
        assert torch.equal(res.ftle, want.ftle) and torch.equal(res.mean, want.mean) and torch.equal(res.max, want.max)
    for a, b in zip(ns.state(), before):
        assert _bits_equal(a, b)
    assert sim.history_len == hist_len and torch.equal(sim._ring, ring) and _bits_equal(sim._pair, pair)
    assert sim.get_chaos_features() == feats
    forward = sim.flow_ftle(n_steps=8, direction="forward")
    assert bool(torch.isfinite(forward.ftle).all()) and not torch.equal(forward.ftle, res.ftle)
