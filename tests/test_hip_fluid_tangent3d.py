"""The tangent-linear 3-D fluid step on the device (physics.fluid_step3d_jvp, lyapunov_exponents3d; csrc/fluid_tangent3d.hip) against the
oracle of DESIGN.md 3.12: fluid_step3d_jvp_rule (torch.autograd.forward_ad over the rule) in fp64 along the Branches recorded by the fp32
CPU run of the rule -- that run is the device's forward bit for bit.  The replay is the same rule's JVP in fp32 on the CPU.  Metric per
tensor max|d - ref| / max|ref| (step_grad_oracle.metric); bounds: step_grad_oracle.device_bounds(replay worst), i.e. the project's 1e-4 and
10 x the replay's worst over the same cases, the replay computed here.  Every draw has a fixed seed (tests/step3d_tangent_oracle.py),
B = 2, grids of at most 16 x 32 x 32.

Figures measured on MI355X (device worst / replay worst; DESIGN.md 3.12 has them all):
  smk_advect3d_tangent alone .......... 2.546e-06 / 2.546e-06
  fluid_step3d_jvp, one step .......... 2.804e-06 / 2.770e-06     four chained steps 6.810e-06 / 6.573e-06
  dot-product identity ................ 7.261e-09 / 2.641e-09
  amplitude-300 state (no far limit) .. 6.557e-06 / 6.557e-06
  lyapunov_exponents3d, per log_growth  drawn 5.364e-07 / 5.868e-07, noise 3.979e-07 / 3.397e-07"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step_grad_oracle as O2                                                                     # noqa: E402
import step3d_grad_oracle as O3                                                                   # noqa: E402
import step3d_tangent_oracle as OT                                                                # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import (Branches, NavierStokesSimulator3D, SmokeSimulator3D, fluid_step3d, fluid_step3d_jvp,   # noqa: E402
                                     fluid_tangent_rollout3d, lyapunov_exponents3d)

DEV = "cuda"


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _hold(device_worst, replay_worst, what):
    project, margin = O2.device_bounds(replay_worst)
    print(f"{what}: device worst {device_worst:.3e}; replay worst {replay_worst:.3e} (10 x = {margin:.3e}); project bound {project:g}")
    assert device_worst <= project, f"{what}: {device_worst:.3e} exceeds the project's {project:g}"
    assert device_worst <= margin, f"{what}: {device_worst:.3e} exceeds 10 x the replay's {replay_worst:.3e}"


# ------------------------------------------------------------------------------------------------ 1. smk_advect3d_tangent alone
PAD_FILL = -7.0


def _pitched(t, pitch, fill=float("nan")):
    """[n, P, R, C] CPU tensor -> a device buffer [n, P, R, pitch] full of `fill` with t in its first C columns."""
    buf = torch.full((*t.shape[:-1], pitch), fill, device=DEV)
    buf[..., :t.shape[-1]] = t.to(DEV)
    return buf


def _advect_tangent(which, field, u, v, w, tfield, tu, tv, tw, dt, T):
    """One smk_advect3d_tangent call on pitched buffers with odd pitches and NaN-filled padding; base [B, ...], tangents [B * T, ...] CPU
    tensors -> (tout [B * T, Df, Hf, Wf] as the kernel left it, whether the padding of tout still holds its fill)."""
    L = _lib.load()
    Bn, D, H, W = u.shape[0], u.shape[1], v.shape[2], u.shape[3]
    pc, pv = (W + 2) | 1, (W + 3) | 1
    pitch = pv if which == 1 else pc

    def put(t, is_v):
        return _pitched(t, pv if is_v else pc)
    f_b, tf_b = put(field, which == 1), put(tfield, which == 1)
    u_b, v_b, w_b, tu_b, tv_b, tw_b = put(u, False), put(v, True), put(w, False), put(tu, False), put(tv, True), put(tw, False)
    out = torch.full((Bn * T, *field.shape[1:3], pitch), PAD_FILL, device=DEV)
    _lib.check(L.smk_advect3d_tangent(which, *[t.data_ptr() for t in (f_b, u_b, v_b, w_b, tf_b, tu_b, tv_b, tw_b, out)],
                                      Bn, T, D, H, W, pc, pv, dt, _lib.stream_ptr(torch.device(DEV, 0))))
    C = field.shape[3]
    return out[..., :C].contiguous(), bool((out[..., C:] == PAD_FILL).all())


def test_advect3d_tangent_against_the_stage_oracle():
    device_worst, replay_worst, where = 0.0, 0.0, None
    T = 3
    for cid, (u, v, w, d), dt in OT.stage_states():
        for which in (0, 1, 2, 3):
            field = (u, v, w, d)[which].clone()
            tans = OT.tangents((field, u, v, w), 40 + which, T)                        # (tfield, tu, tv, tw), each [B, T, ...]
            flat = [t.flatten(0, 1) for t in tans]
            got3, pad3 = _advect_tangent(which, field, u, v, w, *flat, dt, T)
            again, _ = _advect_tangent(which, field, u, v, w, *flat, dt, T)
            assert _bits_equal(got3, again), f"{cid} which={which}: two calls differ"
            assert pad3, f"{cid} which={which}: the pitch padding of tout was written"
            assert bool(torch.isfinite(got3).all()), f"{cid} which={which}: the NaN padding of an input was read"
            got3 = got3.view(OT.B, T, *field.shape[1:])
            for k in range(T):
                got1, pad1 = _advect_tangent(which, field, u, v, w, *[t[:, k] for t in tans], dt, 1)
                assert pad1 and _bits_equal(got1, got3[:, k]), f"{cid} which={which}: tangent {k} of the T = 3 call differs from its T = 1 call"
            oracle, replay = OT.stage_reference(field, u, v, w, tans, which, dt)
            dev, rep = O2.metric(got3, oracle), O2.metric(replay, oracle)
            if dev > device_worst:
                device_worst, where = dev, (cid, which)
            replay_worst = max(replay_worst, rep)
            print(f"{cid:28s} which={which}: device {dev:.2e} replay {rep:.2e}")
    _hold(device_worst, replay_worst, f"smk_advect3d_tangent, worst at {where}")


# ------------------------------------------------------------------------------------------------ 2. fluid_step3d_jvp
def _device_jvp(state, tangents, settings, n_steps=1):
    dt, nu, J = settings
    s, t = [x.to(DEV) for x in state], [x.to(DEV) for x in tangents]
    if n_steps == 1:
        return fluid_step3d_jvp(s, t, dt=dt, viscosity=nu, jacobi_iters=J)
    return fluid_tangent_rollout3d(s, t, n_steps, dt=dt, viscosity=nu, jacobi_iters=J)


def test_whole_step_tangents_stay_within_both_bounds_and_the_state_is_the_steppers():
    device_worst, replay_worst, where = 0.0, 0.0, None
    refs = OT.whole_step_references()
    for cid, state, settings in O3.whole_step_cases():
        dt, nu, J = settings
        sim = NavierStokesSimulator3D(tuple(state[4].shape[1:]), dt=dt, viscosity=nu, device=DEV, batch_size=OT.B, jacobi_iters=J)
        sim.u, sim.v, sim.w, sim.p, sim.density = state
        sim.step()
        want = sim.state()
        tans, oracle, replay, outs = refs[cid]                        # T = 2 tangents per grid
        new, got = _device_jvp(state, tans, settings)
        for name, a, b, c in zip("uvwpd", new, want, outs):
            assert _bits_equal(a, b), f"{cid}: the returned {name} differs from step()"
            assert torch.equal(a.cpu(), c), f"{cid}: the device forward's {name} differs from the fp32 rule"
        assert all(g.shape == t.shape for g, t in zip(got, tans))
        dev, rep = OT.figures(got, oracle, replay)
        print(f"{cid:28s} device {['%.2e' % m for m in dev]} replay {['%.2e' % m for m in rep]}")
        if max(dev) > device_worst:
            device_worst, where = max(dev), (cid, OT.NAMES[dev.index(max(dev))])
        replay_worst = max(replay_worst, max(rep))
    _hold(device_worst, replay_worst, f"one tangent step, worst at {where}")


def test_state_shaped_and_unbatched_tangents_are_the_T1_call():
    cid, state, settings = O3.whole_step_cases()[2]                   # (4, 5, 7)
    tans = OT.tangents(state, 53)
    _, flat = _device_jvp(state, tans, settings)
    _, t1 = _device_jvp(state, [t[:, None] for t in tans], settings)
    new0, one = _device_jvp([s[0] for s in state], [t[0] for t in tans], settings)
    for a, b, c, n, s in zip(flat, t1, one, new0, state):
        assert _bits_equal(a, b[:, 0]) and _bits_equal(c, a[0]) and n.shape == s.shape[1:]


def test_four_chained_tangent_steps_stay_within_the_bounds():
    state, settings, tans, oracle, replay, outs = OT.four_step_reference()
    assert tuple(state[4].shape[1:]) == (9, 19, 37)
    new, got = _device_jvp(state, tans, settings, n_steps=4)
    for a, b in zip(new, outs):
        assert torch.equal(a.cpu(), b)
    dev, rep = OT.figures(got, oracle, replay)
    print("four steps: device", ["%.2e" % m for m in dev], "replay", ["%.2e" % m for m in rep])
    _hold(max(dev), max(rep), "four chained tangent steps")


def test_a_tangent_is_independent_of_T_and_of_its_batch_mates_and_two_calls_are_bit_equal():
    state, settings = O3.draw_state3d((9, 19, 37), 50.0), (0.01, 0.001, 20)
    tans = OT.tangents(state, 52, 3)
    _, both = _device_jvp(state, tans, settings)
    _, again = _device_jvp(state, tans, settings)
    for a, b in zip(both, again):
        assert _bits_equal(a, b)
    for k in range(3):
        _, alone = _device_jvp(state, [t[:, k] for t in tans], settings)
        for name, a, c in zip("uvwpd", alone, both):
            assert _bits_equal(a, c[:, k]), (k, name)
    _, grid1 = _device_jvp([s[1:] for s in state], [t[1:] for t in tans], settings)
    for name, a, c in zip("uvwpd", grid1, both):
        assert _bits_equal(a[0], c[1]), name


# ------------------------------------------------------------------------------------------------ 3. the dot-product identity on the device
def test_device_jvp_and_device_vjp_are_transposes():
    """<J t, g> (fluid_step3d_jvp) against <t, J^T g> (fluid_step3d's backward), both on route="hip", summed in fp64, as
    |<Jt, g> - <t, JTg>| / (|Jt| |g|); the bound is 10 x the same mismatch of the CPU fp32 replay (forward-mode against reverse-mode of the
    rule), the worst over the same cases."""
    device_worst, replay_worst = 0.0, 0.0
    for cid, state, settings in O3.whole_step_cases():
        assert O3.max_move(state, *settings) < 1.0, cid               # the adjoint kernels' one-cell limit
        dt, nu, J = settings
        t, g = OT.tangents(state, 60), OT.tangents(state, 61)
        rep = OT.replay_dot_mismatch(state, settings, t, g)
        _, djt = _device_jvp(state, t, settings)
        xs = [s.to(DEV).requires_grad_(True) for s in state]
        djtg = torch.autograd.grad(fluid_step3d(*xs, dt=dt, viscosity=nu, jacobi_iters=J), xs, [x.to(DEV) for x in g])
        assert all(bool(torch.isfinite(x).all()) for x in djtg)
        dev = abs(OT.dot(djt, g) - OT.dot(t, djtg)) / (OT.norm(djt) * OT.norm(g))
        print(f"{cid:28s} device mismatch {dev:.2e}  replay mismatch {rep:.2e}")
        device_worst, replay_worst = max(device_worst, dev), max(replay_worst, rep)
    print(f"dot-product identity: device worst {device_worst:.3e}, replay worst {replay_worst:.3e} (10 x = {10 * replay_worst:.3e})")
    assert device_worst <= O2.REPLAY_MARGIN * replay_worst


# ------------------------------------------------------------------------------------------------ 4. no far limit
def test_no_far_limit():
    state, settings, tans, oracle, replay, outs = OT.far_reference()
    dt, nu, J = settings
    assert O3.max_move(state, *settings) > 2.0
    xs = [s.to(DEV).requires_grad_(True) for s in state]
    grads = torch.autograd.grad(fluid_step3d(*xs, dt=dt, viscosity=nu, jacobi_iters=J), xs, [x.to(DEV) for x in OT.tangents(state, 70)])
    assert all(bool(torch.isnan(x).all()) for x in grads)            # the adjoint's documented answer to a far grid
    new, got = _device_jvp(state, tans, settings)
    for a, b in zip(new, outs):
        assert torch.equal(a.cpu(), b)
    assert all(bool(torch.isfinite(x).all()) for x in got)
    dev, rep = OT.figures(got, oracle, replay)
    print("far state: device", ["%.2e" % m for m in dev], "replay", ["%.2e" % m for m in rep])
    _hold(max(dev), max(rep), "amplitude-300 state")


# ------------------------------------------------------------------------------------------------ 5. smk_tangent3d_renorm
def _renorm(fields, Bn, T):
    """smk_tangent3d_renorm on copies of dense [Bn * T, ...] device tensors -> (scaled fields, norms [Bn * T] fp64)."""
    L = _lib.load()
    D, H, W = fields[4].shape[1:]
    fields = [f.clone() for f in fields]
    norms = torch.full((Bn * T,), -1.0, dtype=torch.float64, device=DEV)
    nbytes = int(L.smk_tangent3d_renorm_workspace(Bn, T, D, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    _lib.check(L.smk_tangent3d_renorm(*[f.data_ptr() for f in fields], norms.data_ptr(), Bn, T, D, H, W, W, W + 1, ws.data_ptr(), nbytes,
                                      _lib.stream_ptr(torch.device(DEV, 0))))
    return fields, norms


@pytest.mark.parametrize("shape", [(3, 3, 3), (4, 5, 7), (9, 19, 37)], ids=lambda s: "x".join(str(n) for n in s))
def test_tangent3d_renorm(shape):
    T = 3
    state = O3.draw_state3d(shape, 50.0)
    fields = [t.flatten(0, 1) for t in OT.tangents(state, 80, T)]    # [B * T, ...]
    fields[0] = 1e3 * fields[0]
    for f in fields:
        f[4] = 0.0                                                   # tangent 1 of grid 1 is all zero
    fields = [f.to(DEV) for f in fields]
    got, norms = _renorm(fields, OT.B, T)
    want = torch.stack([sum((f[i].double() ** 2).sum() for f in fields).sqrt() for i in range(OT.B * T)])
    rel = ((norms - want).abs() / want.clamp_min(1e-300)).max()
    print(f"{shape}: norms against torch's fp64 norm: worst relative difference {float(rel):.2e}")
    assert float(rel) <= 1e-12 and float(norms[4]) == 0.0
    for name, f, g in zip("uvwpd", fields, got):
        for i in range(OT.B * T):
            expect = f[i].cpu() if i == 4 else f[i].cpu() / norms[i].float().cpu()           # (the host's divide: IEEE, rounded once)
            assert _bits_equal(g[i].cpu(), expect), f"{name}[{i}] is not x / (float)norm"
    again, norms2 = _renorm(fields, OT.B, T)
    assert torch.equal(norms, norms2) and all(_bits_equal(a, b) for a, b in zip(got, again))
    for i in (0, 5):                                                 # a tangent alone: its batch mates do not matter
        alone, n1 = _renorm([f[i:i + 1] for f in fields], 1, 1)
        assert float(n1[0]) == float(norms[i]) and all(_bits_equal(a[0], g[i]) for a, g in zip(alone, got))
    unit, _ = _renorm(got, OT.B, T)                                  # already unit: the norms of the result are 1 to rounding
    _, n3 = _renorm(unit, OT.B, T)
    assert float((n3[[0, 1, 2, 3, 5]] - 1).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ 6. lyapunov_exponents3d
@pytest.mark.parametrize("noise", [False, True], ids=["drawn", "noise20"])
def test_lyapunov_exponents3d_against_the_benettin_run_along_the_branches(noise):
    _, steps, J = OT.LYAPUNOV
    state = OT.lyapunov_state(noise)
    rec = Branches()
    replay = lyapunov_exponents3d(*state, steps, jacobi_iters=J, route="torch", branches=rec)
    oracle = lyapunov_exponents3d(*[s.double() for s in state], steps, jacobi_iters=J, route="torch", branches=rec.replayer())
    got = lyapunov_exponents3d(*[s.to(DEV) for s in state], steps, jacobi_iters=J)
    assert tuple(got.log_growth.shape) == (OT.B, steps, 1) and got.log_growth.dtype == torch.float64
    for a, b in zip(got.state, replay.state):
        assert torch.equal(a.cpu(), b)
    assert float(oracle.log_growth.abs().min()) >= 8e-3              # no growth factor so near 1 that its log is all rounding
    rep = float((replay.log_growth - oracle.log_growth).abs().max())
    dev = float((got.log_growth.cpu() - oracle.log_growth).abs().max())
    print(f"lyapunov3d ({'noise' if noise else 'drawn'}): exponents {oracle.exponents[:, 0].tolist()}")
    _hold(dev, rep, f"lyapunov_exponents3d ({'noise' if noise else 'drawn'}), per log_growth entry")
    assert torch.allclose(got.exponents.cpu(), got.log_growth.cpu().sum(dim=1) / (steps * 0.01), rtol=0, atol=1e-12)
    again = lyapunov_exponents3d(*[s.to(DEV) for s in state], steps, jacobi_iters=J)
    assert torch.equal(again.log_growth, got.log_growth)             # the default tangent0 comes from the CPU generator


def test_lyapunov_exponents3d_with_gram_schmidt_on_the_device():
    state = [s.to(DEV) for s in OT.lyapunov_state(True)]
    res = lyapunov_exponents3d(*state, 4, k=2, renorm_every=2)
    assert tuple(res.exponents.shape) == (OT.B, 2) and bool(torch.isfinite(res.log_growth).all())
    assert bool((res.exponents[:, 0] >= res.exponents[:, 1]).all())   # largest first
    for b in range(OT.B):
        q = [[t[b, j] for t in res.tangents] for j in range(2)]
        assert abs(OT.dot(q[0], q[1])) <= 1e-5 and abs(OT.dot(q[0], q[0]) - 1) <= 1e-5 and abs(OT.dot(q[1], q[1]) - 1) <= 1e-5


@pytest.mark.parametrize("batch", [None, 2], ids=["single", "batched"])
def test_flow_lyapunov_leaves_the_simulator_alone(batch):
    sim = SmokeSimulator3D((8, 16, 16), device=DEV, batch_size=batch)
    sim.add_incense_source([(8, 10, 4)], [1.0])
    for _ in range(10):
        sim.simulate_step(add_fractal=False)
    ns = sim.ns_solver
    before = [t.clone() for t in ns.state()]
    feats = sim.get_chaos_features()
    ring, hist_len = sim._ring.clone(), sim.history_len
    lam = sim.flow_lyapunov(n_steps=8)
    if batch is None:
        assert isinstance(lam, float) and lam == lam
    else:
        assert tuple(lam.shape) == (2,) and lam.dtype == torch.float64 and bool(torch.isfinite(lam).all())
    for a, b in zip(ns.state(), before):
        assert _bits_equal(a, b)
    assert sim.history_len == hist_len and torch.equal(sim._ring, ring)
    assert sim.get_chaos_features() == feats
    want = lyapunov_exponents3d(*before, 8, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters)
    assert (lam == float(want.exponents[0, 0])) if batch is None else torch.equal(lam, want.exponents[:, 0])
