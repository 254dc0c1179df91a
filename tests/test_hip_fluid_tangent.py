"""The tangent-linear 2-D fluid step on the device (physics.fluid_step_jvp, lyapunov_exponents; csrc/fluid_tangent.hip) against the oracle
of DESIGN.md 3.11: fluid_step_jvp_rule (torch.autograd.forward_ad over the rule) in fp64 along the Branches recorded by the fp32 CPU run
of the rule -- that run is the device's forward bit for bit.  The replay is the same rule's JVP in fp32 on the CPU.  Metric per tensor
max|d - ref| / max|ref| (step_grad_oracle.metric); bounds: the project's 1e-4 and 10 x the replay's worst over the same cases, whichever
is smaller.  Every draw has a fixed seed, B = 2, grids of at most 64 x 64.

Figures measured on MI355X (device worst / replay worst; DESIGN.md 3.11 has them all):
  smk_advect_tangent alone ............ 2.455e-06 / 2.420e-06
  fluid_step_jvp, one step ............ 4.025e-06 / 3.931e-06     four chained steps 1.186e-05 / 1.202e-05
  dot-product identity ................ 2.129e-08 / 2.057e-08
  amplitude-300 state (no far limit) .. 2.520e-06 / 2.520e-06
  lyapunov_exponents, per log_growth .. rest 1.937e-06 / 1.303e-06, noise 1.011e-06 / 9.973e-07"""
import os
import sys

import pytest
import torch
import torch.autograd.forward_ad as fwad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step_grad_oracle as O                                                                      # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import (Branches, NavierStokesSimulator, SmokeSimulator, advect_rule, fluid_step,       # noqa: E402
                                     fluid_step_jvp, fluid_step_jvp_rule, fluid_step_rule, fluid_tangent_rollout, lyapunov_exponents)

DEV = "cuda"
FAR = ((24, 24), 0.01, 300.0)            # white-noise velocities whose back-traces move up to 3 cells


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _hold(device_worst, replay_worst, what):
    project, margin = O.device_bounds(replay_worst)
    print(f"{what}: device worst {device_worst:.3e}; replay worst {replay_worst:.3e} (10 x = {margin:.3e}); project bound {project:g}")
    assert device_worst <= project, f"{what}: {device_worst:.3e} exceeds the project's {project:g}"
    assert device_worst <= margin, f"{what}: {device_worst:.3e} exceeds 10 x the replay's {replay_worst:.3e}"


def _tangents(state, seed, T=None):
    g = O._gen(seed, *state[-1].shape)
    return [torch.randn(s.shape if T is None else (s.shape[0], T) + tuple(s.shape[1:]), generator=g) for s in state]


def _dot(a, b):
    return sum(float((x.double().cpu() * y.double().cpu()).sum()) for x, y in zip(a, b))


def _norm(a):
    return _dot(a, a) ** 0.5


# ------------------------------------------------------------------------------------------------ 1. smk_advect_tangent alone
def _jvp_of(fn, inputs, tangents, dtype, branches):
    """forward_ad of fn(*inputs, branches=) in `dtype` on the CPU -> the output's tangent."""
    with fwad.dual_level():
        duals = [fwad.make_dual(x.to(dtype), t.to(dtype)) for x, t in zip(inputs, tangents)]
        return fwad.unpack_dual(fn(*duals, branches=branches)).tangent.detach()


def _pitched(t, rows_pitch, fill=float("nan")):
    """[n, R, C] CPU tensor -> a device buffer [n, R, pitch] full of `fill` with t in its first C columns; returns (buffer, view)."""
    n, R, C = t.shape
    buf = torch.full((n, R, rows_pitch), fill, device=DEV)
    buf[:, :, :C] = t.to(DEV)
    return buf, buf[:, :, :C]


def _advect_tangent(which, field, u, v, tfield, tu, tv, dt, T):
    """One smk_advect_tangent call on pitched buffers with odd pitches; base [B, ...], tangents [B * T, ...] CPU tensors -> (tout
    [B * T, R, C] as the kernel left it, whether the padding of tout still holds its fill)."""
    L = _lib.load()
    Bn, H, W = u.shape[0], u.shape[1] - 1, u.shape[2]
    pc, pv = (W + 2) | 1, (W + 3) | 1
    pitch = pv if which == 1 else pc

    def put(t, is_v):
        return _pitched(t, pv if is_v else pc)[0]
    f_b, tf_b = put(field, which == 1), put(tfield, which == 1)
    u_b, v_b, tu_b, tv_b = put(u, False), put(v, True), put(tu, False), put(tv, True)
    out = torch.full((Bn * T, field.shape[1], pitch), -7.0, device=DEV)
    _lib.check(L.smk_advect_tangent(which, f_b.data_ptr(), u_b.data_ptr(), v_b.data_ptr(), tf_b.data_ptr(), tu_b.data_ptr(), tv_b.data_ptr(),
                                    out.data_ptr(), Bn, T, H, W, pc, pv, dt, _lib.stream_ptr(torch.device(DEV, 0))))
    C = field.shape[2]
    return out[:, :, :C].contiguous(), bool((out[:, :, C:] == -7.0).all())


def _stage_states():
    """(id, (u, v, density), dt) of the stage test: two shapes in both regimes, the far state, the state at rest."""
    cases = []
    for shape in ((5, 7), (33, 40)):
        for dt, amp, _ in O.REGIMES:
            u, v, _, d = O.draw_state(shape, amp, seed=3)
            cases.append((f"{shape[0]}x{shape[1]}-dt{dt}-a{amp:g}", (u, v, d), dt))
    shape, dt, amp = FAR
    u, v, _, d = O.draw_state(shape, amp, seed=3)
    assert dt * float(u.abs().max()) > 2.5                          # back-traces well beyond one cell
    cases.append(("far-24x24-a300", (u, v, d), dt))
    u, v, _, d = O.rest_state()
    cases.append(("rest-16x24", (u, v, d), 0.01))
    return cases


def test_advect_tangent_against_the_stage_oracle():
    device_worst, replay_worst, where = 0.0, 0.0, None
    T = 3
    for cid, (u, v, d), dt in _stage_states():
        for which in (0, 1, 2):
            field = (u, v, d)[which].clone()
            decay = 0.995 if which == 2 else 1.0
            fn = lambda f, uu, vv, branches=None: advect_rule(f, uu, vv, dt=dt, branches=branches) * decay      # noqa: E731
            tans = [_tangents((field, u, v), 40 + 10 * k + which) for k in range(T)]          # T tangent triples (tfield, tu, tv)
            stack = [torch.stack([tans[k][i] for k in range(T)], dim=1).flatten(0, 1) for i in range(3)]     # [B * T, ...]
            got3, pad3 = _advect_tangent(which, field, u, v, *stack, dt, T)
            again, _ = _advect_tangent(which, field, u, v, *stack, dt, T)
            assert _bits_equal(got3, again), f"{cid} which={which}: two calls differ"
            assert pad3, f"{cid} which={which}: the pitch padding of tout was written"
            got3 = got3.view(O.B, T, *field.shape[1:])
            for k in range(T):
                rec = Branches()
                replay = _jvp_of(fn, (field, u, v), tans[k], torch.float32, rec)
                oracle = _jvp_of(fn, (field, u, v), tans[k], torch.float64, rec.replayer())
                got1, pad1 = _advect_tangent(which, field, u, v, *tans[k], dt, 1)
                assert pad1 and _bits_equal(got1, got3[:, k]), f"{cid} which={which}: tangent {k} of the T = 3 call differs from its T = 1 call"
                dev, rep = O.metric(got1, oracle), O.metric(replay, oracle)
                if dev > device_worst:
                    device_worst, where = dev, (cid, which, k)
                replay_worst = max(replay_worst, rep)
            print(f"{cid:24s} which={which}: device {dev:.2e} replay {rep:.2e}")
    _hold(device_worst, replay_worst, f"smk_advect_tangent, worst at {where}")


# ------------------------------------------------------------------------------------------------ 2. fluid_step_jvp
def _rule_jvps(state, tangents, settings, n_steps=1):
    """-> (oracle tangents fp64, replay tangents fp32, fp32 states): the rule's JVP in fp32 recording its branches, then in fp64 along
    them."""
    dt, nu, J = settings
    rec = Branches()

    def run(dtype, br):
        s, t = [x.to(dtype) for x in state], [x.to(dtype) for x in tangents]
        for _ in range(n_steps):
            s, t = fluid_step_jvp_rule(s, t, dt=dt, viscosity=nu, jacobi_iters=J, branches=br)
        return s, t
    outs, replay = run(torch.float32, rec)
    _, oracle = run(torch.float64, rec.replayer())
    return oracle, replay, outs


def _device_jvp(state, tangents, settings, n_steps=1):
    dt, nu, J = settings
    s, t = [x.to(DEV) for x in state], [x.to(DEV) for x in tangents]
    if n_steps == 1:
        return fluid_step_jvp(s, t, dt=dt, viscosity=nu, jacobi_iters=J)
    return fluid_tangent_rollout(s, t, n_steps, dt=dt, viscosity=nu, jacobi_iters=J)


def _figures(device, oracle, replay):
    return [O.metric(d, r) for d, r in zip(device, oracle)], [O.metric(p, r) for p, r in zip(replay, oracle)]


def test_whole_step_tangents_stay_within_both_bounds_and_the_state_is_the_steppers():
    device_worst, replay_worst, where = 0.0, 0.0, None
    for cid, state, settings in O.whole_step_cases():
        dt, nu, J = settings
        H, W = state[3].shape[1:]
        sim = NavierStokesSimulator((H, W), dt=dt, viscosity=nu, device=DEV, batch_size=O.B, jacobi_iters=J)
        sim.u, sim.v, sim.p, sim.density = state
        sim.step()
        want = sim.state()
        sim.check()
        sim.close()
        for T in (None, 2):                                          # state-shaped tangents, and two per grid
            tans = _tangents(state, 50, T)
            oracle, replay, outs = _rule_jvps(state, tans, settings)
            new, got = _device_jvp(state, tans, settings)
            for name, a, b, c in zip("uvpd", new, want, outs):
                assert _bits_equal(a, b), f"{cid}: the returned {name} differs from step()"
                assert torch.equal(a.cpu(), c), f"{cid}: the device forward's {name} differs from the fp32 rule"
            assert all(g.shape == t.shape for g, t in zip(got, tans))
            dev, rep = _figures(got, oracle, replay)
            print(f"{cid:28s} T={T} device {['%.2e' % m for m in dev]} replay {['%.2e' % m for m in rep]}")
            if max(dev) > device_worst:
                device_worst, where = max(dev), (cid, T, "uvpd"[dev.index(max(dev))])
            replay_worst = max(replay_worst, max(rep))
    _hold(device_worst, replay_worst, f"one tangent step, worst at {where}")


def test_four_chained_tangent_steps_stay_within_the_bounds():
    state, settings = O.simulated_state(), (0.01, 0.001, 20)
    tans = _tangents(state, 51, 2)
    oracle, replay, outs = _rule_jvps(state, tans, settings, n_steps=4)
    new, got = _device_jvp(state, tans, settings, n_steps=4)
    for a, b in zip(new, outs):
        assert torch.equal(a.cpu(), b)
    dev, rep = _figures(got, oracle, replay)
    print("four steps: device", ["%.2e" % m for m in dev], "replay", ["%.2e" % m for m in rep])
    _hold(max(dev), max(rep), "four chained tangent steps")


def test_a_tangent_is_independent_of_T_and_of_its_batch_mates_and_two_calls_are_bit_equal():
    state, settings = O.draw_state((33, 40), 60.0), (0.01, 0.001, 20)
    tans = _tangents(state, 52, 3)
    _, both = _device_jvp(state, tans, settings)
    _, again = _device_jvp(state, tans, settings)
    for a, b in zip(both, again):
        assert _bits_equal(a, b)
    for k in range(3):
        _, alone = _device_jvp(state, [t[:, k] for t in tans], settings)
        for name, a, c in zip("uvpd", alone, both):
            assert _bits_equal(a, c[:, k]), (k, name)
    _, grid1 = _device_jvp([s[1:] for s in state], [t[1:] for t in tans], settings)
    for name, a, c in zip("uvpd", grid1, both):
        assert _bits_equal(a[0], c[1]), name


# ------------------------------------------------------------------------------------------------ 3. the dot-product identity on the device
def test_device_jvp_and_device_vjp_are_transposes():
    """<J t, g> (fluid_step_jvp) against <t, J^T g> (fluid_step's backward), both on route="hip", summed in fp64; the bound is 10 x the
    same mismatch of the CPU fp32 replay (forward-mode against reverse-mode of the rule), the worst over the same cases."""
    device_worst, replay_worst = 0.0, 0.0
    for cid, state, settings in O.whole_step_cases():
        assert O.max_move(state, *settings) < 1.0, cid               # the adjoint kernels' one-cell limit
        dt, nu, J = settings
        t, g = _tangents(state, 60), _tangents(state, 61)
        # the replay, on the CPU in fp32
        _, jt = fluid_step_jvp_rule(state, t, dt=dt, viscosity=nu, jacobi_iters=J)
        xs = [s.clone().requires_grad_(True) for s in state]
        jtg = torch.autograd.grad(fluid_step_rule(*xs, dt=dt, viscosity=nu, jacobi_iters=J), xs, g)
        rep = abs(_dot(jt, g) - _dot(t, jtg)) / (_norm(jt) * _norm(g))
        # the device
        _, djt = _device_jvp(state, t, settings)
        xs = [s.to(DEV).requires_grad_(True) for s in state]
        djtg = torch.autograd.grad(fluid_step(*xs, dt=dt, viscosity=nu, jacobi_iters=J), xs, [x.to(DEV) for x in g])
        assert all(bool(torch.isfinite(x).all()) for x in djtg)
        dev = abs(_dot(djt, g) - _dot(t, djtg)) / (_norm(djt) * _norm(g))
        print(f"{cid:28s} device mismatch {dev:.2e}  replay mismatch {rep:.2e}")
        device_worst, replay_worst = max(device_worst, dev), max(replay_worst, rep)
    print(f"dot-product identity: device worst {device_worst:.3e}, replay worst {replay_worst:.3e} (10 x = {10 * replay_worst:.3e})")
    assert device_worst <= O.REPLAY_MARGIN * replay_worst


# ------------------------------------------------------------------------------------------------ 4. no far limit
def test_no_far_limit():
    shape, dt, amp = FAR
    state, settings = O.draw_state(shape, amp, seed=3), (dt, 0.001, 20)
    assert O.max_move(state, *settings) > 2.0
    xs = [s.to(DEV).requires_grad_(True) for s in state]
    grads = torch.autograd.grad(fluid_step(*xs, dt=dt, viscosity=0.001, jacobi_iters=20), xs, [x.to(DEV) for x in _tangents(state, 70)])
    assert all(bool(torch.isnan(x).all()) for x in grads)            # the adjoint's documented answer to a far grid
    tans = _tangents(state, 71, 2)
    oracle, replay, outs = _rule_jvps(state, tans, settings)
    new, got = _device_jvp(state, tans, settings)
    for a, b in zip(new, outs):
        assert torch.equal(a.cpu(), b)
    assert all(bool(torch.isfinite(x).all()) for x in got)
    dev, rep = _figures(got, oracle, replay)
    print("far state: device", ["%.2e" % m for m in dev], "replay", ["%.2e" % m for m in rep])
    _hold(max(dev), max(rep), "amplitude-300 state")


# ------------------------------------------------------------------------------------------------ 5. smk_tangent_renorm
def _renorm(fields, Bn, T):
    """smk_tangent_renorm on copies of dense [Bn * T, ...] device tensors -> (scaled fields, norms [Bn * T] fp64)."""
    L = _lib.load()
    H, W = fields[3].shape[1:]
    fields = [f.clone() for f in fields]
    norms = torch.full((Bn * T,), -1.0, dtype=torch.float64, device=DEV)
    nbytes = int(L.smk_tangent_renorm_workspace(Bn, T, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    _lib.check(L.smk_tangent_renorm(*[f.data_ptr() for f in fields], norms.data_ptr(), Bn, T, H, W, W, W + 1, ws.data_ptr(), nbytes,
                                    _lib.stream_ptr(torch.device(DEV, 0))))
    return fields, norms


@pytest.mark.parametrize("shape", [(5, 7), (33, 40), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tangent_renorm(shape):
    T = 3
    state = O.draw_state(shape, 60.0)
    fields = [t.flatten(0, 1) for t in _tangents(state, 80, T)]      # [B * T, ...]
    fields[0] = 1e3 * fields[0]
    for f in fields:
        f[4] = 0.0                                                   # tangent 1 of grid 1 is all zero
    fields = [f.to(DEV) for f in fields]
    got, norms = _renorm(fields, O.B, T)
    want = torch.stack([sum((f[i].double() ** 2).sum() for f in fields).sqrt() for i in range(O.B * T)])
    rel = ((norms - want).abs() / want.clamp_min(1e-300)).max()
    print(f"{shape}: norms against torch's fp64 norm: worst relative difference {float(rel):.2e}")
    assert float(rel) <= 1e-12 and float(norms[4]) == 0.0
    for name, f, g in zip("uvpd", fields, got):
        for i in range(O.B * T):
            expect = f[i].cpu() if i == 4 else f[i].cpu() / norms[i].float().cpu()           # (the host's divide: IEEE, rounded once)
            assert _bits_equal(g[i].cpu(), expect), f"{name}[{i}] is not x / (float)norm"
    again, norms2 = _renorm(fields, O.B, T)
    assert torch.equal(norms, norms2) and all(_bits_equal(a, b) for a, b in zip(got, again))
    for i in (0, 5):                                                 # a tangent alone: its batch mates do not matter
        alone, n1 = _renorm([f[i:i + 1] for f in fields], 1, 1)
        assert float(n1[0]) == float(norms[i]) and all(_bits_equal(a[0], g[i]) for a, g in zip(alone, got))
    unit, _ = _renorm(got, O.B, T)                                   # already unit: the norms of the result are 1 to rounding
    _, n3 = _renorm(unit, O.B, T)
    assert float((n3[[0, 1, 2, 3, 5]] - 1).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ 6. lyapunov_exponents
def _lyapunov_state(noise):
    """32 x 32, B = 2: one Gaussian source per grid (with white-noise velocities of amplitude 20 added first if `noise`), 10 steps of
    the fp32 rule, J = 20."""
    H = W = 32
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    d = torch.stack([torch.exp(-((xx - x0) ** 2 + (yy - y0) ** 2).float() / (2 * s * s)) for x0, y0, s in ((16, 20, 3.0), (12, 14, 4.0))])
    u, v = torch.zeros(O.B, H + 1, W), torch.zeros(O.B, H, W + 1)
    if noise:
        g = O._gen(90)
        u, v = 20.0 * (2 * torch.rand(u.shape, generator=g) - 1), 20.0 * (2 * torch.rand(v.shape, generator=g) - 1)
    state = (u, v, torch.zeros(O.B, H, W), d)
    for _ in range(10):
        state = fluid_step_rule(*state, jacobi_iters=20)
    return state


@pytest.mark.parametrize("noise", [False, True], ids=["rest", "noise20"])
def test_lyapunov_exponents_against_the_benettin_run_along_the_branches(noise):
    state = _lyapunov_state(noise)
    rec = Branches()
    replay = lyapunov_exponents(*state, 16, route="torch", branches=rec)
    oracle = lyapunov_exponents(*[s.double() for s in state], 16, route="torch", branches=rec.replayer())
    got = lyapunov_exponents(*[s.to(DEV) for s in state], 16)
    assert tuple(got.log_growth.shape) == (O.B, 16, 1) and got.log_growth.dtype == torch.float64
    for a, b in zip(got.state, replay.state):
        assert torch.equal(a.cpu(), b)
    rep = float((replay.log_growth - oracle.log_growth).abs().max())
    dev = float((got.log_growth.cpu() - oracle.log_growth).abs().max())
    bound = min(O.PROJECT_BOUND, O.REPLAY_MARGIN * rep)
    print(f"lyapunov ({'noise' if noise else 'rest'}): exponents {oracle.exponents[:, 0].tolist()}; per log_growth entry: device {dev:.3e}, "
          f"replay {rep:.3e}, bound {bound:.3e}")
    assert dev <= bound
    assert torch.allclose(got.exponents.cpu(), got.log_growth.cpu().sum(dim=1) / (16 * 0.01), rtol=0, atol=1e-12)
    again = lyapunov_exponents(*[s.to(DEV) for s in state], 16)
    assert torch.equal(again.log_growth, got.log_growth)             # the default tangent0 comes from the CPU generator


def test_lyapunov_exponents_with_gram_schmidt_on_the_device():
    state = [s.to(DEV) for s in _lyapunov_state(True)]
    res = lyapunov_exponents(*state, 4, k=2, renorm_every=2)
    assert tuple(res.exponents.shape) == (O.B, 2) and bool(torch.isfinite(res.log_growth).all())
    for b in range(O.B):
        q = [[t[b, j] for t in res.tangents] for j in range(2)]
        assert abs(_dot(q[0], q[1])) <= 1e-5 and abs(_dot(q[0], q[0]) - 1) <= 1e-5 and abs(_dot(q[1], q[1]) - 1) <= 1e-5


@pytest.mark.parametrize("batch", [None, 2], ids=["single", "batched"])
def test_flow_lyapunov_leaves_the_simulator_alone(batch):
    sim = SmokeSimulator((32, 32), device=DEV, batch_size=batch)
    sim.add_incense_source([(16, 20)], [1.0])
    for _ in range(10):
        sim.simulate_step(add_fractal=False)
    before = [t.clone() for t in sim.ns_solver.state()]
    history = [h.clone() for h in sim.history]
    feats = sim.get_chaos_features()
    lam = sim.flow_lyapunov(n_steps=8)
    if batch is None:
        assert isinstance(lam, float) and lam == lam
    else:
        assert tuple(lam.shape) == (2,) and lam.dtype == torch.float64 and bool(torch.isfinite(lam).all())
    for a, b in zip(sim.ns_solver.state(), before):
        assert _bits_equal(a, b)
    assert len(sim.history) == len(history) and all(_bits_equal(a, b) for a, b in zip(sim.history, history))
    assert sim.get_chaos_features() == feats
    want = lyapunov_exponents(*before, 8, dt=sim.ns_solver.dt, viscosity=sim.ns_solver.viscosity, jacobi_iters=sim.ns_solver.jacobi_iters)
    assert (lam == float(want.exponents[0, 0])) if batch is None else torch.equal(lam, want.exponents[:, 0])
