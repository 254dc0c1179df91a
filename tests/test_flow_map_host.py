"""The flow-map rule on the CPU (smokephysai_amd/physics/flow_map.py): closed forms, the tie to the density advection's
own trace, the refusals and signatures, and the property that decides how the backward increment is formed."""
import inspect
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import flow_map_oracle as F                                                                       # noqa: E402
import step_grad_oracle as O                                                                      # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd import physics                                                               # noqa: E402
from smokephysai_amd.physics import fluid_rule                                                    # noqa: E402
from smokephysai_amd.physics.flow_map import (LO, FtleResult, _clamp_decided, flow_ftle, flow_ftle_rule, flow_map_step,      # noqa: E402
                                              flow_map_step_rule, ftle_field, ftle_rule)


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("direction", F.DIRECTIONS)
def test_pure_strain_gives_log1p_a_dt_over_dt(direction):
    """u = a (x - c), v = -a (y - c) as the cells sample them (the staggered stores hold the value half a cell earlier).  A linear
    velocity keeps the map linear: its gradient is diag((1 -+ a dt)^n, (1 +- a dt)^n), so the larger stretch is (1 + a dt)^n and the
    FTLE log1p(a dt) / dt, on the cells that no clamped trace and no last-index sample has reached.  Those spread by at most one cell
    per step from the rim, and the difference stencil reaches one cell further: n + 2 cells are left out.  In fp64 a displacement of
    at most a few cells carries ~n * 10 roundings of 2.2e-16 cells; the differences and 1 / (2 horizon) = 12.5 leave it below 1e-12."""
    a, dt, n, H, W = 5.0, 0.01, 4, 24, 26
    cy, cx = 11.0, 12.0
    u = (a * (torch.arange(W, dtype=torch.float64) - 0.5 - cx)).expand(H + 1, W).contiguous()
    v = (-a * (torch.arange(H, dtype=torch.float64) - 0.5 - cy))[:, None].expand(H, W + 1).contiguous()
    disp = torch.zeros(2, H, W, dtype=torch.float64)
    for _ in range(n):
        disp = flow_map_step_rule(disp, u, v, dt=dt, direction=direction)
    ftle = ftle_rule(disp, n * dt)
    m = n + 2
    want = math.log1p(a * dt) / dt
    err = float((ftle[m:-m, m:-m] - want).abs().max())
    print(f"pure strain, {direction}: ftle {want:.12f}, worst difference {err:.2e}")
    assert ftle[m:-m, m:-m].numel() > 50 and err <= 1e-12
    shrink = (1 - a * dt) ** n - 1 if direction == "backward" else (1 + a * dt) ** n - 1      # the x-gradient of dx
    assert float(((disp[0, m:-m, m + 1:-m] - disp[0, m:-m, m:-m - 1]) - shrink).abs().max()) <= 1e-12


@pytest.mark.parametrize("direction", F.DIRECTIONS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_state_at_rest_gives_exactly_zero(direction, dtype):
    H, W = 9, 37
    u, v = torch.zeros(2, H + 1, W, dtype=dtype), torch.zeros(2, H, W + 1, dtype=dtype)
    disp = torch.zeros(2, 2, H, W, dtype=dtype)
    for _ in range(3):
        disp = flow_map_step_rule(disp, u, v, direction=direction)
    assert not bool((disp != 0).any()) and not bool((ftle_rule(disp, 0.03) != 0).any())
    res = flow_ftle_rule(u, v, torch.zeros(2, H, W, dtype=dtype), torch.zeros(2, H, W, dtype=dtype), 3, direction=direction)
    assert not bool((res.ftle != 0).any()) and not bool((res.displacement != 0).any())
    assert res.mean.tolist() == [0.0, 0.0] and res.max.tolist() == [0.0, 0.0]


def test_one_backward_step_from_zero_lands_in_the_density_advections_cells():
    """floor(X + dx) and floor(Y + dy) are the floors the density advection recorded for its final gather, exactly: where the clamp passes
    X + (-(dt su)) is X - dt su bit for bit, elsewhere X + (px - X) is px, an integer."""
    for cid, state, _ in F.cases():
        u, v, _, d = state
        rec = fluid_rule.Branches()
        fluid_rule.advect(d, (u, v), F.DT, rec)
        x0, y0 = rec.log[-2], rec.log[-1]                     # the field interpolation's floors, x then y
        disp = flow_map_step_rule(torch.zeros(d.shape[0], 2, *d.shape[1:]), u, v, dt=F.DT, direction="backward")
        Y, X = torch.meshgrid(torch.arange(d.shape[1], dtype=torch.float32), torch.arange(d.shape[2], dtype=torch.float32), indexing="ij")
        assert torch.equal(torch.floor(X + disp[:, 0]).long(), x0.expand_as(disp[:, 0])), cid
        assert torch.equal(torch.floor(Y + disp[:, 1]).long(), y0.expand_as(disp[:, 1])), cid


def test_the_far_case_leaves_on_all_four_sides_and_the_quirk_case_reads_zero():
    state = dict((cid, s) for cid, s, _ in F.cases())
    assert F.leaves_on_all_sides(state["12x33-B3-a300"])
    (u, v, _, _), disp0 = state["4x5-B3-quirk"], dict((cid, d) for cid, _, d in F.cases())["4x5-B3-quirk"]
    out = flow_map_step_rule(disp0, u, v, dt=F.DT, direction="backward")
    assert not bool((out[:, :, -1, -1] != 0).any())          # the corner's samples and its interpolation all sit on the last index
    assert torch.equal(out[:, 0, :-1, -1], torch.zeros(3, 3))          # last column: su reads 0, the trace stays, the interpolation reads 0
    assert bool((out[:, 0, :-1, :-1] != 0).all())


# ------------------------------------------------------------------------------------------------ the increment's form
def _px_minus_x_step(disp, u, v, *, dt, direction, branches):
    """The backward map step with the increment formed as px - X everywhere: the variant the rule rejects."""
    assert direction == "backward"
    H, W = disp.shape[-2:]
    Y, X = torch.meshgrid(*[torch.arange(n, dtype=disp.dtype) for n in (H, W)], indexing="ij")
    su = fluid_rule._sample(u, -1, (Y, X), branches)
    sv = fluid_rule._sample(v, -2, (Y, X), branches)
    px, _ = _clamp_decided(branches, X - dt * su, 0.0, float(W - 1))
    py, _ = _clamp_decided(branches, Y - dt * sv, 0.0, float(H - 1))
    moved = fluid_rule._interpolate(disp, (py.unsqueeze(-3), px.unsqueeze(-3)), branches)
    return moved + torch.stack([px - X, py - Y], dim=-3)


def _chain(step_fn):
    def rule(u, v, p, density, n_steps, *, dt, viscosity, jacobi_iters, direction, branches):
        state = (u, v, p, density)
        disp = density.new_zeros(density.shape[0], 2, *density.shape[1:])
        for _ in range(n_steps):
            state = fluid_rule.step(state, dt, viscosity, jacobi_iters, branches)
            disp = step_fn(disp, state[0], state[1], dt=dt, direction=direction, branches=branches)
        return ftle_rule(disp, n_steps * dt)
    return rule


def test_the_increment_form_keeps_small_displacements():
    """On dataset-like 64 x 64 states (from rest, 20 steps, J = 20) a particle moves ~3e-5 cells per step while ulp(64) = 7.6e-6: the
    px - X form rounds every increment to that grid and its fp32 FTLE is useless (measured: 3-7e-2 of the field's maximum off the fp64
    run along the same branches), the rule's form keeps the increment's own 24 bits (measured: 2-5e-6).  Held here: the rule within the
    project's 1e-4 of fp64, and the variant at least 100 x worse."""
    state = F.dataset_like_state()
    oracle, replay = F.flow_ftle_oracle(state, 20, "backward", rule=_chain(flow_map_step_rule))
    again = flow_ftle_rule(*state, 20, dt=F.DT, viscosity=F.NU, jacobi_iters=F.J, direction="backward")
    assert torch.equal(again.ftle, replay)                    # (the chain written here is flow_ftle_rule's)
    _, variant = F.flow_ftle_oracle(state, 20, "backward", rule=_chain(_px_minus_x_step))
    for b in range(2):
        good, bad = O.metric(replay[b], oracle[b]), O.metric(variant[b], oracle[b])
        print(f"grid {b}: max ftle {float(oracle[b].max()):.3e} mean {float(oracle[b].mean()):.3e}; rule {good:.2e}, px - X variant {bad:.2e}")
        assert good <= O.PROJECT_BOUND and bad >= 100 * good


# ------------------------------------------------------------------------------------------------ refusals, signatures, the result's fields
def test_refusals():
    H, W = 5, 7
    disp, u, v = torch.zeros(2, 2, H, W), torch.zeros(2, H + 1, W), torch.zeros(2, H, W + 1)
    p = d = torch.zeros(2, H, W)
    for fn in (flow_map_step_rule, lambda *a, **k: flow_map_step(*a, route="torch", **k)):
        with pytest.raises(ValueError, match="direction is 'backward' or 'forward'"):
            fn(disp, u, v, direction="sideways")
        with pytest.raises(ValueError, match=r"u must be \(2, 6, 7\)"):
            fn(disp, v, v)
        with pytest.raises(ValueError, match=r"disp must be \[2, H, W\] or \[B, 2, H, W\]"):
            fn(disp[:, :1], u, v)
        with pytest.raises(ValueError, match="H, W >= 3"):
            fn(torch.zeros(2, 2, 6), torch.zeros(3, 6), torch.zeros(2, 7))
    with pytest.raises(ValueError, match="route is 'hip' or 'torch'"):
        flow_map_step(disp, u, v, route="cuda")
    with pytest.raises(ValueError, match="route is 'hip' or 'torch'"):
        ftle_field(disp, 0.1, route="cuda")
    with pytest.raises(ValueError, match="route is 'hip' or 'torch'"):
        flow_ftle(u, v, p, d, 2, route="cuda")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="horizon > 0"):
            ftle_rule(disp, bad)
        with pytest.raises(ValueError, match="horizon > 0"):
            ftle_field(disp, bad, route="torch")
    with pytest.raises(ValueError, match="disp must be"):
        ftle_field(torch.zeros(2, 3, H, W), 0.1, route="torch")
    with pytest.raises(ValueError, match="n_steps >= 1"):
        flow_ftle(u, v, p, d, 0, route="torch")
    with pytest.raises(ValueError, match="dt > 0"):
        flow_ftle(u, v, p, d, 2, dt=0.0, route="torch")
    with pytest.raises(ValueError, match="direction"):
        flow_ftle(u, v, p, d, 2, direction="up", route="torch")
    with pytest.raises(ValueError, match="fluid_step: u must be"):
        flow_ftle(v, v, p, d, 2, route="torch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # the hip route has none
        flow_map_step(disp, u, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ftle_field(disp, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_ftle(u, v, p, d, 2)


def test_signatures_and_exports():
    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults(flow_map_step) == dict(dt=0.01, direction="backward", route="hip")
    assert defaults(flow_map_step_rule) == dict(dt=0.01, direction="backward", branches=None)
    assert defaults(ftle_field) == dict(route="hip")
    assert defaults(flow_ftle) == dict(dt=0.01, viscosity=0.001, jacobi_iters=20, direction="backward", route="hip")
    assert defaults(flow_ftle_rule) == dict(dt=0.01, viscosity=0.001, jacobi_iters=20, direction="backward", branches=None)
    assert defaults(physics.SmokeSimulator.flow_ftle) == dict(n_steps=20)
    for name in ("FtleResult", "flow_ftle", "flow_ftle_rule", "flow_map_step", "flow_map_step_rule", "ftle_field", "ftle_rule"):
        assert name in physics.__all__ and getattr(physics, name) is globals().get(name, getattr(physics, name))
    assert [f for f in FtleResult.__dataclass_fields__] == ["ftle", "displacement", "mean", "max", "state"]
    assert LO == -1.0 + 2.0 ** -24


def test_the_binding_and_the_header_agree():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION          # additive exports
    for name, nargs in (("smk_flow_map_step", 13), ("smk_ftle_field", 11)):
        proto = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert proto and len(proto.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name]), name
    assert re.search(r"int64_t smk_ftle_workspace\(int32_t B, int32_t H, int32_t W\);", hdr)
    L = _lib.load()
    for name in ("smk_flow_map_step", "smk_ftle_field", "smk_ftle_workspace"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.smk_ftle_workspace(2, 64, 64) == 2 * 4 * 2 * 8 and L.smk_ftle_workspace(1, 3, 3) == 16             # runs of 16 rows
    assert L.smk_ftle_workspace(1, 32766, 3) == 256 * 2 * 8                                                     # at most 256 runs
    for bad in ((0, 8, 8), (65536, 8, 8), (1, 2, 8), (1, 8, 2), (1, 32767, 8)):
        assert L.smk_ftle_workspace(*bad) == -1, bad


def test_flow_ftle_rule_result_shapes_batched_and_not():
    state = O.draw_state((5, 7), 5.0, batch=2)
    res = flow_ftle_rule(*state, 2, direction="forward")
    assert tuple(res.ftle.shape) == (2, 5, 7) and tuple(res.displacement.shape) == (2, 2, 5, 7)
    assert res.mean.dtype == res.max.dtype == torch.float64 and tuple(res.mean.shape) == tuple(res.max.shape) == (2,)
    assert [tuple(s.shape) for s in res.state] == [(2, 6, 7), (2, 5, 8), (2, 5, 7), (2, 5, 7)]
    one = flow_ftle_rule(*[s[1] for s in state], 2, direction="forward")
    assert torch.equal(one.ftle, res.ftle[1]) and torch.equal(one.displacement, res.displacement[1])
    assert one.mean.dim() == 0 and float(one.max) == float(res.max[1]) and all(torch.equal(a, b[1]) for a, b in zip(one.state, res.state))
    f, mean, top = ftle_field(res.displacement, 0.02, route="torch")
    assert torch.equal(f, res.ftle) and torch.equal(mean, res.mean) and torch.equal(top, res.max)
    assert torch.equal(flow_map_step(res.displacement[0], state[0][0], state[1][0], route="torch"),
                       flow_map_step_rule(res.displacement, state[0], state[1])[0])


# ------------------------------------------------------------------------------------------------ the figure
def test_visualizer_plot_ftle(tmp_path):
    import matplotlib.pyplot as plt
    from smokephysai_amd.utils import SmokeVisualizer
    viz = SmokeVisualizer()
    g = torch.Generator().manual_seed(0)
    frame, field = torch.rand(1, 1, 16, 16, generator=g), torch.rand(16, 16, generator=g)
    path = str(tmp_path / "ftle.png")
    fig = viz.plot_ftle(frame, field, path)
    with open(path, "rb") as f:
        assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    panels = [ax for ax in fig.axes if ax.get_title()]
    assert [ax.get_title() for ax in panels] == ["Input Smoke", "FTLE", "FTLE Upper Decile"]
    assert len(panels[2].collections) >= 1                     # the contour
    flat = viz.plot_ftle(frame, torch.zeros(16, 16))           # a constant field: no contour, no error
    assert len([ax for ax in flat.axes if ax.get_title()][2].collections) == 0
    with pytest.raises(ValueError):
        viz.plot_ftle(frame, torch.zeros(8, 8))
    plt.close("all")
