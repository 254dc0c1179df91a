"""The flow map and its FTLE on the device (physics.flow_map_step, ftle_field, flow_ftle; csrc/flow_map.hip) against the oracle of DESIGN.md
3.14: the rule in fp64 along the Branches recorded by the fp32 CPU run of the rule (tests/flow_map_oracle.py).  The replay is that fp32 CPU
run.  Metric per field max|x - ref| / max|ref| (exactly 0 where max|ref| is 0); bound: 10 x the replay's worst over the same cases, per
quantity.  Cases: grids 3 x 3, 4 x 5, 12 x 33, 9 x 37 and 64 x 64 with B = 1 and 3 at amplitude 5, the state at rest, an amplitude-300
state whose traces leave the domain on all four sides, the last-index quirk; the single kernels run on odd pitches whose NaN padding must
stay NaN.

Figures measured on MI355X, worst over the cases (device / replay; profiles/r32/test_figures.txt has every case, DESIGN.md 3.14 the table).
The displacements' figures are the replay's to four digits in every case; the FTLE's differ from it in single cases (the device's log1p),
not in the worst:
  smk_flow_map_step ........ backward 1.654e-06 / 1.654e-06     forward 9.632e-07 / 9.632e-07
  smk_ftle_field ........... drawn displacement 1.830e-07 / 1.830e-07     1e-4 of it 1.606e-07 / 1.606e-07
  flow_ftle, 1 step ........ backward ftle 2.299e-06 / 2.299e-06, displacement 3.673e-06 / 3.673e-06
                             forward  ftle 2.906e-06 / 2.906e-06, displacement 3.673e-06 / 3.673e-06
  flow_ftle, 8 steps ....... backward ftle 7.253e-05 / 7.253e-05, displacement 7.329e-06 / 7.329e-06
                             forward  ftle 1.096e-02 / 1.096e-02, displacement 5.926e-06 / 5.926e-06
(the last two FTLE figures are the amplitude-300 state's: after 8 steps of 3-cell moves most of its particles sit on the domain's rim,
the map is nearly singular there, 2 emax is close to -1 and log1p magnifies an fp32 rounding; the other cases' are at most 4.6e-06)"""
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

import flow_map_oracle as F                                                                       # noqa: E402
import step_grad_oracle as O                                                                      # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import NavierStokesSimulator, SmokeSimulator, flow_ftle, flow_map_step, ftle_field       # noqa: E402

DEV = "cuda"
CASES = F.cases()
case_param = pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
PAD = -7.0


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _pitched(t, pitch):
    """[..., R, C] CPU tensor -> a device buffer [..., R, pitch] full of NaN with t in its first C columns."""
    buf = torch.full(tuple(t.shape[:-1]) + (pitch,), float("nan"), device=DEV)
    buf[..., :t.shape[-1]] = t.to(DEV)
    return buf


def _padding_is_nan(buf, cols):
    return bool(torch.isnan(buf[..., cols:]).all())


def _map_step_pitched(direction, disp, u, v, dt=F.DT):
    """One smk_flow_map_step on buffers with odd pitches whose padding is NaN (the output's too) -> (disp' [B, 2, H, W], whether every
    padding is still NaN)."""
    B, _, H, W = disp.shape
    pc, pv, pm = (W + 2) | 1, (W + 3) | 1, (W + 4) | 1
    u_b, v_b, d_b = _pitched(u, pc), _pitched(v, pv), _pitched(disp, pm)
    out = torch.full((B, 2, H, pm), float("nan"), device=DEV)
    _lib.check(_lib.load().smk_flow_map_step(F.DIRECTIONS.index(direction), u_b.data_ptr(), v_b.data_ptr(), d_b.data_ptr(), out.data_ptr(),
                                             B, H, W, pc, pv, pm, dt, _lib.stream_ptr(torch.device(DEV, 0))))
    pads = _padding_is_nan(out, W) and _padding_is_nan(u_b, W) and _padding_is_nan(v_b, W + 1) and _padding_is_nan(d_b, W)
    return out[..., :W].contiguous(), pads


def _ftle_pitched(disp, horizon):
    """smk_ftle_field on an odd pitch with NaN padding -> (ftle [B, H, W], stats [B, 2], whether the paddings are still NaN)."""
    B, _, H, W = disp.shape
    L = _lib.load()
    pm = (W + 4) | 1
    d_b = _pitched(disp, pm)
    out = torch.full((B, H, pm), float("nan"), device=DEV)
    stats = torch.full((B, 2), float("nan"), dtype=torch.float64, device=DEV)
    nbytes = int(L.smk_ftle_workspace(B, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    _lib.check(L.smk_ftle_field(d_b.data_ptr(), out.data_ptr(), stats.data_ptr(), B, H, W, pm, horizon, ws.data_ptr(), nbytes,
                                _lib.stream_ptr(torch.device(DEV, 0))))
    return out[..., :W].contiguous(), stats, _padding_is_nan(out, W) and _padding_is_nan(d_b, W)


@functools.lru_cache(maxsize=None)
def _case_figures(cid):
    """Everything one case measures, once: {quantity: (device figure, replay figure)}, with the checks that are not figures made on the
    way (paddings, the dense call, the stepper's state, the statistics)."""
    _, state, disp0 = next(c for c in CASES if c[0] == cid)
    u, v = state[0], state[1]
    dstate = [s.to(DEV) for s in state]
    figs = {}
    for direction in F.DIRECTIONS:
        oracle, replay = F.map_step_oracle(disp0, u, v, direction)
        got, pads = _map_step_pitched(direction, disp0, u, v)
        assert pads, f"{cid} {direction}: a pitch padding was written"
        dense = flow_map_step(disp0.to(DEV), dstate[0], dstate[1], dt=F.DT, direction=direction)
        assert _bits_equal(got, dense), f"{cid} {direction}: the pitched call differs from physics.flow_map_step"
        figs[f"map_step {direction}"] = (O.metric(got, oracle), O.metric(replay, oracle))
    for name, disp, horizon in (("drawn", disp0, 0.08), ("small", 1e-4 * disp0, 0.2)):
        oracle, replay = F.ftle_oracle(disp, horizon)
        got, stats, pads = _ftle_pitched(disp, horizon)
        assert pads, f"{cid}: a pitch padding was written by smk_ftle_field"
        dense, mean, top = ftle_field(disp.to(DEV), horizon)
        assert _bits_equal(got, dense) and torch.equal(stats[:, 0], mean) and torch.equal(stats[:, 1], top), cid
        _check_stats(got, stats, cid)
        figs[f"ftle_field {name}"] = (O.metric(got, oracle), O.metric(replay, oracle))
    for n_steps in (1, 8):
        for direction in F.DIRECTIONS:
            oracle, replay = F.flow_ftle_oracle(state, n_steps, direction)
            got = flow_ftle(*dstate, n_steps, dt=F.DT, viscosity=F.NU, jacobi_iters=F.J, direction=direction)
            for name, a, b in zip("uvpd", got.state, replay.state):
                assert torch.equal(a.cpu(), b), f"{cid} {direction} x{n_steps}: the returned {name} differs from the fp32 rule's"
            _check_stats(got.ftle, torch.stack([got.mean, got.max], dim=1), cid)
            key = f"flow_ftle {direction} x{n_steps}"
            figs[key + " ftle"] = (O.metric(got.ftle, oracle.ftle), O.metric(replay.ftle, oracle.ftle))
            figs[key + " displacement"] = (O.metric(got.displacement, oracle.displacement), O.metric(replay.displacement, oracle.displacement))
    return figs


def _check_stats(ftle, stats, what):
    """stats against torch's fp64 mean and max of the device's own field: relative 1e-12 for the mean, exact for the max."""
    flat = ftle.double().flatten(1)
    mean, top = flat.mean(dim=1), flat.max(dim=1).values
    assert torch.equal(stats[:, 1], top), f"{what}: max {stats[:, 1].tolist()} against {top.tolist()}"
    assert bool(((stats[:, 0] - mean).abs() <= 1e-12 * mean.abs()).all()), f"{what}: mean {stats[:, 0].tolist()} against {mean.tolist()}"


# ------------------------------------------------------------------------------------------------ 1. the cases, one by one
@case_param
def test_case_runs_clean(case):
    """Per case: paddings untouched, the pitched calls equal the dense ones, the stepper's state is the fp32 rule's, the statistics are
    the field's; every figure is finite, and exactly 0 where the oracle is 0."""
    cid = case[0]
    for key, (dev, rep) in _case_figures(cid).items():
        print(f"FIG {cid:16s} {key:36s} device {dev:.3e}  replay {rep:.3e}")
        assert dev == dev and dev != float("inf"), f"{cid} {key}: {dev}"
    if cid.endswith("rest"):
        assert all(dev == 0.0 and rep == 0.0 for dev, rep in _case_figures(cid).values())


def test_the_far_state_leaves_on_all_four_sides():
    state = next(s for cid, s, _ in CASES if cid.endswith("a300"))
    assert F.leaves_on_all_sides(state)


# ------------------------------------------------------------------------------------------------ 2. the bounds, per quantity over all cases
def test_every_quantity_stays_within_ten_times_the_replay():
    worst = {}
    for cid, _, _ in CASES:
        for key, (dev, rep) in _case_figures(cid).items():
            w = worst.setdefault(key, [0.0, 0.0, None])
            if dev > w[0]:
                w[0], w[2] = dev, cid
            w[1] = max(w[1], rep)
    failed = []
    for key, (dev, rep, where) in worst.items():
        print(f"FIG worst            {key:36s} device {dev:.3e} (at {where})  replay {rep:.3e}  bound {F.REPLAY_MARGIN * rep:.3e}")
        if not dev <= F.REPLAY_MARGIN * rep:
            failed.append(key)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 3. the live simulator's own trace
@pytest.mark.parametrize("batch", [1, 3])
def test_one_backward_step_on_a_live_simulator_lands_in_backtrace_indices(batch):
    H, W = 33, 40
    u, v, p, d = O.draw_state((H, W), 60.0, seed=5, batch=batch)
    sim = NavierStokesSimulator((H, W), device=DEV, batch_size=batch)
    sim.u, sim.v, sim.p, sim.density = u, v, p, d
    sim.step()
    x0, y0 = sim.backtrace_indices(2)                         # of a density advection with the velocities the simulator now holds
    disp = torch.zeros(batch, 2, H, W, device=DEV)
    out = torch.empty_like(disp)
    _lib.check(_lib.load().smk_flow_map_step(0, sim._u.data_ptr(), sim._v.data_ptr(), disp.data_ptr(), out.data_ptr(), batch, H, W, sim._pc,
                                             sim._pv, W, sim.dt, _lib.stream_ptr(torch.device(DEV, 0))))
    sim.check()
    Y, X = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=DEV), torch.arange(W, dtype=torch.float32, device=DEV), indexing="ij")
    assert torch.equal(torch.floor(X + out[:, 0]).int(), x0) and torch.equal(torch.floor(Y + out[:, 1]).int(), y0)
    assert bool((x0 != X.int()).any()) and bool((y0 != Y.int()).any())          # (the traces did move)
    sim.close()


# ------------------------------------------------------------------------------------------------ 4. determinism and batch independence
def test_two_calls_are_bit_equal_and_a_grid_does_not_depend_on_its_batch_mates():
    state = [s.to(DEV) for s in O.draw_state((33, 40), 5.0, seed=6, batch=3)]
    disp0 = F.draw_disp((33, 40), 3, 1.5).to(DEV)
    for direction in F.DIRECTIONS:
        a = flow_map_step(disp0, state[0], state[1], direction=direction)
        assert _bits_equal(a, flow_map_step(disp0, state[0], state[1], direction=direction))
        alone = flow_map_step(disp0[1:2], state[0][1:2], state[1][1:2], direction=direction)
        assert _bits_equal(alone[0], a[1]) and _bits_equal(flow_map_step(disp0[2], state[0][2], state[1][2], direction=direction), a[2])
        res = flow_ftle(*state, 4, direction=direction)
        again = flow_ftle(*state, 4, direction=direction)
        one = flow_ftle(*[s[1:2] for s in state], 4, direction=direction)
        single = flow_ftle(*[s[2] for s in state], 4, direction=direction)
        for name in ("ftle", "displacement", "mean", "max"):
            x = getattr(res, name)
            assert torch.equal(x, getattr(again, name)), (direction, name)
            assert torch.equal(x[1], getattr(one, name)[0]) and torch.equal(x[2], getattr(single, name)), (direction, name)
    f, mean, top = ftle_field(disp0, 0.08)
    f2, mean2, top2 = ftle_field(disp0, 0.08)
    assert _bits_equal(f, f2) and torch.equal(mean, mean2) and torch.equal(top, top2)
    f1, mean1, top1 = ftle_field(disp0[1], 0.08)
    assert _bits_equal(f1, f[1]) and float(mean1) == float(mean[1]) and float(top1) == float(top[1])


def test_refusals_of_the_entry_points():
    L = _lib.load()
    H, W = 5, 7
    st = _lib.stream_ptr(torch.device(DEV, 0))
    u, v = torch.zeros(1, H + 1, W, device=DEV), torch.zeros(1, H, W + 1, device=DEV)
    disp, out = torch.zeros(1, 2, H, W, device=DEV), torch.full((1, 2, H, W), PAD, device=DEV)
    ftle, stats = torch.full((1, H, W), PAD, device=DEV), torch.full((1, 2), PAD, dtype=torch.float64, device=DEV)
    ws = torch.empty(4, dtype=torch.float64, device=DEV)

    def refused(rc, word):
        assert rc == _lib.SMK_ERR_INVALID and word in L.smk_last_error().decode(), (rc, L.smk_last_error().decode())
    step = lambda direction, u_, v_, d_, o_, pm=W: L.smk_flow_map_step(direction, u_, v_, d_, o_, 1, H, W, W, W + 1, pm, 0.01, st)   # noqa: E731
    ptr = lambda t: t.data_ptr()                                                                                                      # noqa: E731
    refused(step(0, None, ptr(v), ptr(disp), ptr(out)), "null pointer")
    refused(step(0, ptr(u), ptr(v), ptr(disp), None), "null pointer")
    refused(step(2, ptr(u), ptr(v), ptr(disp), ptr(out)), "direction")
    refused(step(0, ptr(u), ptr(v), ptr(disp), ptr(disp)), "aliases")
    refused(step(1, ptr(u), ptr(v), ptr(disp), ptr(u)), "aliases")
    refused(step(0, ptr(u), ptr(v), ptr(disp), ptr(out), W - 1), "pitch_m >= W")
    field = lambda d_, f_, s_, w_, n_, horizon=0.1, pm=W: L.smk_ftle_field(d_, f_, s_, 1, H, W, pm, horizon, w_, n_, st)              # noqa: E731
    refused(field(None, ptr(ftle), ptr(stats), ptr(ws), 16), "null pointer")
    refused(field(ptr(disp), ptr(ftle), None, ptr(ws), 16), "null pointer")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws), 15), "workspace")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), None, 16), "workspace")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws) + 4, 16), "8-byte")
    refused(field(ptr(disp), ptr(ftle), ptr(stats) + 4, ptr(ws), 16), "8-byte")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws), 16, horizon=0.0), "horizon")
    refused(field(ptr(disp), ptr(ftle), ptr(stats), ptr(ws), 16, pm=W - 1), "pitch_m >= W")
    refused(field(ptr(disp), ptr(disp), ptr(stats), ptr(ws), 16), "aliases")
    torch.cuda.synchronize()
    assert bool((out == PAD).all()) and bool((ftle == PAD).all()) and bool((stats == PAD).all())     # a refused call writes nothing


# ------------------------------------------------------------------------------------------------ 5. SmokeSimulator.flow_ftle
@pytest.mark.parametrize("batch", [None, 2], ids=["single", "batched"])
def test_flow_ftle_leaves_the_simulator_alone(batch):
    sim = SmokeSimulator((32, 32), device=DEV, batch_size=batch)
    sim.add_incense_source([(16, 20)], [1.0])
    for _ in range(10):
        sim.simulate_step(add_fractal=False)
    before = [t.clone() for t in sim.ns_solver.state()]
    history = [h.clone() for h in sim.history]
    feats = sim.get_chaos_features()
    res = sim.flow_ftle(n_steps=8)
    ns = sim.ns_solver
    want = flow_ftle(*before, 8, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters)
    if batch is None:
        assert tuple(res.ftle.shape) == (32, 32) and tuple(res.displacement.shape) == (2, 32, 32)
        assert isinstance(res.mean, float) and isinstance(res.max, float) and res.max >= res.mean and res.max > 0
        assert torch.equal(res.ftle, want.ftle[0]) and res.mean == float(want.mean[0]) and res.max == float(want.max[0])
    else:
        assert tuple(res.ftle.shape) == (2, 32, 32) and res.mean.dtype == torch.float64 and bool(torch.isfinite(res.ftle).all())
        assert torch.equal(res.ftle, want.ftle) and torch.equal(res.mean, want.mean) and torch.equal(res.max, want.max)
    for a, b in zip(sim.ns_solver.state(), before):
        assert _bits_equal(a, b)
    assert len(sim.history) == len(history) and all(_bits_equal(a, b) for a, b in zip(sim.history, history))
    assert sim.get_chaos_features() == feats
    forward = sim.flow_ftle(n_steps=8, direction="forward")
    assert bool(torch.isfinite(forward.ftle).all()) and not torch.equal(forward.ftle, res.ftle)
