"""The differentiable 3-D fluid step on the device (physics.fluid_step3d / fluid_rollout3d, csrc/fluid_grad3d.hip) against the oracle of
tests/step3d_grad_oracle.py: the fp64 rule along the fp32 run's integer decisions.  Metric per gradient tensor max|d - ref| / max|ref|
(exactly 0 where the reference is); bounds: the project's 1e-4 and 10 x the replay's worst over the same cases (torch's fp32 autograd of the
rule on the CPU), both of them.  Every draw has a fixed seed, B = 2, densities rand^4 * 2.  The twin of tests/test_hip_fluid_grad.py."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step3d_grad_oracle as O                                                                    # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import (FluidRollout, FluidRollout3D, NavierStokesSimulator3D, advect3d_rule,   # noqa: E402
                                     buoy_diffuse3d_rule, fluid_rollout3d, fluid_step3d, project3d_rule)
from smokephysai_amd.physics.fluid_grad import Branches                                            # noqa: E402

DEV = "cuda"
PB_T = 2                          # csrc/fluid_grad3d.h FG3_PB_T: transposed Jacobi sweeps per launch


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _hip_grads(state, upstream, settings, n_steps=1, route="hip"):
    """Gradients of sum(out * g) through fluid_step3d / fluid_rollout3d on the device -> (gradients, outputs)."""
    dt, nu, J = settings
    xs = [t.to(DEV).requires_grad_(True) for t in state]
    if n_steps == 1:
        outs = fluid_step3d(*xs, dt=dt, viscosity=nu, jacobi_iters=J, route=route)
    else:
        outs, _ = fluid_rollout3d(*xs, n_steps, dt=dt, viscosity=nu, jacobi_iters=J, route=route)
    pairs = [(o, g.to(DEV)) for o, g in zip(outs, upstream) if g is not None]
    grads = torch.autograd.grad([o for o, _ in pairs], xs, [g for _, g in pairs])
    return grads, [o.detach() for o in outs]


def _figures(device, oracle, replay):
    return [O.metric(d, r) for d, r in zip(device, oracle)], [O.metric(p, r) for p, r in zip(replay, oracle)]


def _hold(device_worst, replay_worst, what):
    project, margin = O.device_bounds(replay_worst)
    print(f"{what}: device worst {device_worst:.3e}; replay worst {replay_worst:.3e} (10 x = {margin:.3e}); project bound {project:g}")
    assert device_worst <= project, f"{what}: {device_worst:.3e} exceeds the project's {project:g}"
    assert device_worst <= margin, f"{what}: {device_worst:.3e} exceeds 10 x the replay's {replay_worst:.3e}"


def test_whole_step_gradients_stay_within_both_bounds():
    device_worst, replay_worst, where = 0.0, 0.0, None
    refs = O.whole_step_references()
    for cid, state, settings in O.whole_step_cases():
        for only in (False, True):
            ups, oracle, replay, outs = refs[(cid, only)]
            grads, dev_outs = _hip_grads(state, ups, settings)
            for name, a, b in zip("uvwpd", dev_outs, outs):          # the premise of the replay: the device takes the CPU rule's branches
                assert torch.equal(a.cpu(), b), f"{cid}: the device forward's {name} differs from the fp32 rule"
            dev, rep = _figures(grads, oracle, replay)
            print(f"{cid:28s} {'density' if only else 'all    '} device {['%.2e' % m for m in dev]} replay {['%.2e' % m for m in rep]}")
            if max(dev) > device_worst:
                device_worst, where = max(dev), (cid, only, O.NAMES[dev.index(max(dev))])
            replay_worst = max(replay_worst, max(rep))
    _hold(device_worst, replay_worst, f"one step, worst at {where}")


def test_dp_is_exactly_zero_where_the_reference_is():
    state, settings = O.draw_state3d((3, 3, 3), 50.0), (0.01, 0.001, 20)
    grads, _ = _hip_grads(state, O.draw_upstream3d(state), settings)
    assert not bool((grads[3] != 0).any())


@pytest.mark.parametrize("shape", [(9, 19, 37), (12, 33, 40)], ids=lambda s: "x".join(map(str, s)))
def test_forward_is_bit_identical_to_the_rule_and_to_the_simulators_step(shape):
    cpu = O.draw_state3d(shape, 50.0)
    rule = O.step3d_fn(0.01, 0.001, 20)(*cpu)
    state = [t.to(DEV) for t in cpu]
    sim = NavierStokesSimulator3D(shape, dt=0.01, viscosity=0.001, device=DEV, batch_size=O.B, jacobi_iters=20)
    sim.u, sim.v, sim.w, sim.p, sim.density = state
    frame = sim.step()
    want = sim.state()
    for grad in (False, True):                                       # the saving path runs the stage kernels, the other the fused step
        xs = [t.clone().requires_grad_(grad) for t in state]
        got = fluid_step3d(*xs, dt=0.01, viscosity=0.001, jacobi_iters=20)
        for name, a, b, c in zip("uvwpd", got, want, rule):
            assert _bits_equal(a.detach(), b), f"{name} differs from step() (requires_grad={grad})"
            assert _bits_equal(a.detach().cpu(), c), f"{name} differs from the CPU rule (requires_grad={grad})"
        assert _bits_equal(got[4].detach(), frame)


def _advect_backward(which, field, u, v, w, gout, dt):
    L = _lib.load()
    B, D, H, W = u.shape[0], u.shape[1], v.shape[2], w.shape[3]
    field, u, v, w, gout = (t.to(DEV).contiguous() for t in (field, u, v, w, gout))
    df, du, dv, dw = torch.empty_like(field), torch.empty_like(u), torch.empty_like(v), torch.empty_like(w)
    far = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    _lib.check(L.smk_advect3d_backward(which, field.data_ptr(), u.data_ptr(), v.data_ptr(), w.data_ptr(), gout.data_ptr(), df.data_ptr(),
                                       du.data_ptr(), dv.data_ptr(), dw.data_ptr(), far.data_ptr(), B, D, H, W, W, W + 1, dt,
                                       _lib.stream_ptr(torch.device(DEV, 0))))
    return df, du, dv, dw, far


@pytest.mark.parametrize("shape", [(4, 5, 7), (9, 19, 37)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_advect_backward_against_the_stage_oracle(which, shape):
    dt = 0.1
    u, v, w, _, d = O.draw_state3d(shape, 5.0, seed=which + 1)
    field = (u, v, w, d)[which].clone()
    decay = 0.995 if which == 3 else 1.0
    gout = torch.randn(field.shape, generator=O._gen(21, which, *shape))
    fn = lambda f, uu, vv, ww, branches=None: advect3d_rule(f, uu, vv, ww, dt=dt, branches=branches) * decay          # noqa: E731
    oracle, replay, _ = O.oracle_and_replay(fn, (field, u, v, w), [gout])
    df, du, dv, dw, far = _advect_backward(which, field, u, v, w, gout, dt)
    assert far.tolist() == [0, 0]
    dev, rep = _figures((df, du, dv, dw), oracle, replay)
    _hold(max(dev), max(rep), f"smk_advect3d_backward which={which} {shape}")


def _state_shapes(shape):
    D, H, W = shape
    return (D, H + 1, W), (D, H, W + 1), (D + 1, H, W), (D, H, W)


@pytest.mark.parametrize("shape", [(4, 5, 7), (9, 19, 37)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("J", sorted({0, 1, PB_T - 1, PB_T, PB_T + 1, 20, 100}))
def test_project_backward_against_the_stage_oracle(J, shape):
    D, H, W = shape
    dt = 0.01
    L = _lib.load()
    g = O._gen(31, J, D, H, W)
    ups = [torch.randn(O.B, *s, generator=g) for s in _state_shapes(shape)]
    xs = [torch.randn(O.B, *s, generator=g) for s in _state_shapes(shape)]                       # (the stage is linear: any point will do)
    fn = lambda a, b, c, d, branches=None: project3d_rule(a, b, c, d, dt=dt, jacobi_iters=J)     # noqa: E731
    oracle, replay, _ = O.oracle_and_replay(fn, xs, ups)
    gs = [t.to(DEV) for t in ups]
    outs = [torch.empty_like(t) for t in gs]
    nbytes = L.smk_project3d_backward_workspace(O.B, D, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(L.smk_project3d_backward(*[t.data_ptr() for t in gs], *[t.data_ptr() for t in outs], O.B, D, H, W, W, W + 1, J, dt,
                                        ws.data_ptr(), nbytes, _lib.stream_ptr(torch.device(DEV, 0))))
    dev, rep = _figures(outs, oracle, replay)
    _hold(max(dev), max(rep), f"smk_project3d_backward J={J} {shape}")


@pytest.mark.parametrize("shape", [(4, 5, 7), (9, 19, 37)], ids=lambda s: "x".join(map(str, s)))
def test_buoy_diffuse_backward_against_the_stage_oracle(shape):
    D, H, W = shape
    dt, nu = 0.1, 0.05                                               # (a coefficient large enough for the Laplacian to show)
    L = _lib.load()
    g = O._gen(37, D, H, W)
    ups = [torch.randn(O.B, *s, generator=g) for s in _state_shapes(shape)]
    xs = [torch.randn(O.B, *s, generator=g) for s in _state_shapes(shape)]
    fn = lambda a, b, c, d, branches=None: buoy_diffuse3d_rule(a, b, c, d, dt=dt, viscosity=nu)  # noqa: E731
    oracle, replay, _ = O.oracle_and_replay(fn, xs, ups)
    gs = [t.to(DEV) for t in ups]
    outs = [torch.empty_like(t) for t in gs]
    _lib.check(L.smk_buoy_diffuse3d_backward(*[t.data_ptr() for t in gs], *[t.data_ptr() for t in outs], O.B, D, H, W, W, W + 1, dt, nu,
                                             _lib.stream_ptr(torch.device(DEV, 0))))
    dev, rep = _figures(outs, oracle, replay)
    _hold(max(dev), max(rep), f"smk_buoy_diffuse3d_backward {shape}")


def test_one_hot_upstream_reaches_only_the_backtrace_taps():
    shape, dt = (8, 16, 24), 0.1
    D, H, W = shape
    u, v, w, _, d = O.draw_state3d(shape, 5.0, seed=5)
    rec = Branches()
    advect3d_rule(d, u, v, w, dt=dt, branches=rec)                   # the fp32 CPU rule: the device's branches
    x0, y0, z0 = rec.log[-3:]                                        # the floors of the field's interpolation, recorded in the order x, y, z
    hit_neighbour, reached = False, 0
    pairs = (((0, 0, 0), (D - 2, H - 2, W - 2)), ((3, 7, 11), (0, 0, W - 2)), ((D - 2, H - 2, 0), (4, 8, 22)), ((0, 3, 1), (D - 1, H - 1, W - 1)),
             ((D - 1, 5, 9), (2, H - 2, 13)))
    for a, b in pairs:
        gout = torch.zeros(O.B, D, H, W)
        gout[(0,) + a], gout[(1,) + b] = 1.0, 1.0
        df, _, _, _, far = _advect_backward(3, d, u, v, w, gout, dt)
        assert far.tolist() == [0, 0]
        for g, c in enumerate((a, b)):
            tz, ty, tx = (int(t[(g,) + c]) for t in (z0, y0, x0))
            allowed = {(min(max(tz + k, 0), D - 1), min(max(ty + j, 0), H - 1), min(max(tx + i, 0), W - 1))
                       for k in (0, 1) for j in (0, 1) for i in (0, 1)}
            touched = {tuple(t) for t in torch.nonzero(df[g].cpu()).tolist()}
            assert touched <= allowed, (g, c, touched, allowed)
            hit_neighbour |= any(t != c for t in touched)
            reached += bool(touched)          # (a back-trace on an upper edge has eight zero weights: the quirk; nothing to reach)
    # all but the corner (D-1, H-1, W-1): its y and x back-traces are the quirk's (the last row and column sample no velocity)
    assert hit_neighbour and reached == 2 * len(pairs) - 1, reached


def test_four_chained_steps_stay_within_the_bounds():
    state, settings = O.simulated_state3d(), (0.01, 0.001, 20)
    ups, oracle, replay, outs = O.four_step_reference()
    grads, dev_outs = _hip_grads(state, ups, settings, n_steps=4)
    for a, b in zip(dev_outs, outs):
        assert torch.equal(a.cpu(), b)
    dev, rep = _figures(grads, oracle, replay)
    print("four steps: device", ["%.2e" % m for m in dev], "replay", ["%.2e" % m for m in rep])
    _hold(max(dev), max(rep), "four chained steps")
    _, frames = fluid_rollout3d(*[t.to(DEV) for t in state], 4, jacobi_iters=20)
    rule, want = state, []
    for _ in range(4):
        rule = O.step3d_fn(*settings)(*rule)
        want.append(rule[4])
    assert tuple(frames.shape) == (O.B, 4, 12, 32, 32) and _bits_equal(frames.cpu(), torch.stack(want, dim=1))


def test_two_calls_are_bit_equal():
    state, settings = O.draw_state3d((12, 33, 40), 50.0), (0.01, 0.001, 20)
    ups = O.draw_upstream3d(state)
    first, _ = _hip_grads(state, ups, settings)
    second, _ = _hip_grads(state, ups, settings)
    for name, a, b in zip(O.NAMES, first, second):
        assert _bits_equal(a, b), name


def test_a_grid_is_independent_of_its_batch_mates():
    state, settings = O.draw_state3d((12, 33, 40), 50.0), (0.01, 0.001, 20)
    ups = O.draw_upstream3d(state)
    both, _ = _hip_grads(state, ups, settings)
    for b in range(O.B):
        alone, _ = _hip_grads([t[b:b + 1] for t in state], [g[b:b + 1] for g in ups], settings)
        for name, a, c in zip(O.NAMES, alone, both):
            assert _bits_equal(a[0], c[b]), (b, name)


def test_a_far_grid_gets_nan_and_its_batch_mate_is_untouched():
    shape, settings = (8, 16, 24), (0.01, 0.001, 20)
    u, v, w, p, d = O.draw_state3d(shape, 50.0, smooth=1)
    u, v, w = u.clone(), v.clone(), w.clone()
    u[1], v[1], w[1] = 150.0, 150.0, 150.0                          # 1.5 cells per step
    state = (u, v, w, p, d)
    ups = O.draw_upstream3d(state)
    grads, outs = _hip_grads(state, ups, settings)
    assert all(bool(torch.isfinite(o).all()) for o in outs)          # the forward is unaffected
    alone, _ = _hip_grads([t[:1] for t in state], [g[:1] for g in ups], settings)
    for name, g, a in zip(O.NAMES, grads, alone):
        assert bool(torch.isnan(g[1]).all()), f"{name} of the far grid is not NaN"
        assert bool(torch.isfinite(g[0]).all()) and _bits_equal(g[0], a[0]), f"{name} of the near grid changed beside a far grid"
    via_torch, _ = _hip_grads(state, ups, settings, route="torch")
    assert all(bool(torch.isfinite(g).all()) for g in via_torch)


def test_adversarial_test_through_the_stepper_and_the_renders():
    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    from smokephysai_amd.physics import RenderSettings
    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()
    volumes = (torch.rand(2, 1, 8, 128, 128, generator=O._gen(41)) ** 4).to(DEV)
    for views in ({}, {"azimuth": [0, 30]}):
        res = PerturbationTester().adversarial_test(model, volumes, epsilon=0.1, num_steps=2, simulate=FluidRollout3D(steps=2),
                                                    render=RenderSettings(), **views)
        assert res["adversarial_perturbation_norm"] > 0, views
        assert all(torch.isfinite(torch.tensor(v)) for v in res.values()), views
        assert all(p.grad is None and p.requires_grad for p in model.parameters())
    with pytest.raises(ValueError, match="simulate"):
        PerturbationTester().adversarial_test(model, volumes[:, :, 0], simulate=FluidRollout(steps=2), render=RenderSettings())


def test_adversarial_test_through_the_stepper_alone_shows_a_volume_model_the_evolved_volume():
    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet3D
    torch.manual_seed(0)
    model = SmokePhysNet3D(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()
    wanted = [p.requires_grad for p in model.parameters()]
    volumes = (torch.rand(2, 1, 4, 32, 32, generator=O._gen(43)) ** 4).to(DEV)
    res = PerturbationTester().adversarial_test(model, volumes, epsilon=0.1, num_steps=2, simulate=FluidRollout3D(steps=2))
    assert res["adversarial_perturbation_norm"] > 0
    assert all(torch.isfinite(torch.tensor(v)) for v in res.values())
    assert all(p.grad is None for p in model.parameters()) and [p.requires_grad for p in model.parameters()] == wanted
    with pytest.raises(ValueError, match="initial volumes"):
        PerturbationTester().adversarial_test(model, volumes[:, :, 0], simulate=FluidRollout3D(steps=2))
