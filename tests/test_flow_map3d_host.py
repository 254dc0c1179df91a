"""The 3-D flow-map rule on the CPU (smokephysai_amd/physics/flow_map3d.py): the three exact properties, the eigenvalue
step against torch.linalg.eigvalsh, the property that decides how the backward increment is formed, the refusals, signatures and exports,
the header and the binding, the result's shapes, and the figure.

fp32 bounds of the exact properties: 10 x what the fp32 rule shows on this file's inputs (CPU, measured once and written here) --
  z-invariant displacement against the 2-D rule ... 4.8e-07 absolute on a field of maximum 7.07  -> 4.8e-06
  pure strain, forward ............................ 1.2e-07 absolute on 1.98 (half an ulp)       -> 1.2e-06
  pure strain, backward ........................... 0 on 2.96: the fp32 number nearest to the closed form; the bound is the forward's,
                                                    10 x half an ulp of the result               -> 1.2e-06
In fp64 all three are held to 1e-12 (measured: 8.9e-16, 4.4e-16, 8.9e-16), and a state at rest gives exactly 0 in both dtypes."""
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

import flow_map3d_oracle as F3                                                                    # noqa: E402
import step3d_grad_oracle as O3                                                                   # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd import physics                                                               # noqa: E402
from smokephysai_amd.physics import fluid_rule                                                    # noqa: E402
from smokephysai_amd.physics.flow_map import FtleResult, _clamp_decided, ftle_rule                # noqa: E402
from smokephysai_amd.physics.flow_map3d import (flow_ftle3d, flow_ftle3d_rule, flow_map_step3d, flow_map_step3d_rule,      # noqa: E402
                                                ftle3d_rule, ftle_field3d, strain_emax3d)

FP64_BOUND = 1e-12
FP32_Z_INVARIANT, FP32_STRAIN = 4.8e-6, 1.2e-6              # module docstring
DTYPES = [torch.float32, torch.float64]


# ------------------------------------------------------------------------------------------------ the three exact properties
@pytest.mark.parametrize("direction", F3.DIRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_state_at_rest_gives_exactly_zero(direction, dtype):
    D, H, W = 5, 9, 11
    z = lambda *s: torch.zeros(2, *s, dtype=dtype)                                                                  # noqa: E731
    u, v, w = z(D, H + 1, W), z(D, H, W + 1), z(D + 1, H, W)
    disp = z(3, D, H, W)
    for _ in range(3):
        disp = flow_map_step3d_rule(disp, u, v, w, direction=direction)
    assert not bool((disp != 0).any()) and not bool((ftle3d_rule(disp, 0.03) != 0).any())
    res = flow_ftle3d_rule(u, v, w, z(D, H, W), z(D, H, W), 3, direction=direction)
    assert not bool((res.ftle != 0).any()) and not bool((res.displacement != 0).any())
    assert res.mean.tolist() == [0.0, 0.0] and res.max.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_z_invariant_displacement_gives_the_2d_field_or_zero(dtype):
    """disp independent of z with dz = 0: the strain's z row and column are exact zeros, the z direction has stretch exactly 1, and the
    largest eigenvalue is max(the 2-D one, 0)."""
    D, H, W = 6, 7, 9
    g = torch.Generator().manual_seed(1)
    d2 = (torch.rand(2, 2, H, W, generator=g, dtype=torch.float64) - 0.5).to(dtype)
    d3 = torch.cat([d2[:, :, None].expand(2, 2, D, H, W), torch.zeros(2, 1, D, H, W, dtype=dtype)], dim=1)
    got = ftle3d_rule(d3, 0.1)
    want = ftle_rule(d2, 0.1).clamp_min(0)[:, None].expand(2, D, H, W)
    err = float((got - want).abs().max())
    print(f"z-invariant, {dtype}: field maximum {float(want.max()):.3f}, worst difference {err:.2e}")
    assert bool((want > 0).any()) and bool((want == 0).any())
    assert err <= (FP64_BOUND if dtype == torch.float64 else FP32_Z_INVARIANT)


@pytest.mark.parametrize("direction", F3.DIRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pure_strain_gives_the_closed_form(direction, dtype):
    """u = a (x - c), v = b (y - c), w = -(a + b) (z - c) as the cells sample them (the staggered stores hold the value half a cell
    earlier), one map step from zero.  Forward the particle moves by dt * velocity: stretches 1 + a dt, 1 + b dt, 1 - (a + b) dt, the
    largest log1p(a dt).  Backward the map is x - dt * velocity: stretches 1 - a dt, 1 - b dt, 1 + (a + b) dt: it stretches along z,
    log1p((a + b) dt).  Away from the rim: two cells are left out (a clamped trace or a last-index sample, and the difference stencil)."""
    a, b, dt, n = 2.0, 1.0, 0.01, 12
    c = (n - 1) / 2
    face = torch.arange(n + 1, dtype=dtype) - 0.5 - c
    u = (a * face[:n]).expand(1, n, n + 1, n).clone()
    v = (b * face[:n])[:, None].expand(1, n, n, n + 1).clone()
    w = (-(a + b) * face)[:, None, None].expand(1, n + 1, n, n).clone()
    disp = flow_map_step3d_rule(torch.zeros(1, 3, n, n, n, dtype=dtype), u, v, w, dt=dt, direction=direction)
    inner = ftle3d_rule(disp, dt)[0, 2:-2, 2:-2, 2:-2]
    want = math.log1p((a if direction == "forward" else a + b) * dt) / dt
    err = float((inner - want).abs().max())
    print(f"pure strain, {direction}, {dtype}: ftle {want:.12f}, worst difference {err:.2e}")
    assert inner.numel() == 8 ** 3 and err <= (FP64_BOUND if dtype == torch.float64 else FP32_STRAIN)


# ------------------------------------------------------------------------------------------------ the eigenvalue step alone
N_MATRICES = 4000


def _sym(g, scale):
    """The Green-Lagrange strains (G + G^T + G^T G) / 2 of Gaussian gradients G of the given scale, fp64 [N, 3, 3]."""
    G = scale * torch.randn(N_MATRICES, 3, 3, generator=g, dtype=torch.float64)
    return 0.5 * (G + G.transpose(1, 2) + G.transpose(1, 2) @ G)


def _rotated(g, eig):
    """Q diag(eig) Q^T under random rotations Q, fp64 [N, 3, 3]."""
    Q = torch.linalg.qr(torch.randn(N_MATRICES, 3, 3, generator=g, dtype=torch.float64)).Q
    return Q @ torch.diag_embed(eig) @ Q.transpose(1, 2)


def _families():
    g = torch.Generator().manual_seed(33)
    fam = {f"gaussian gradients, scale {s:g}": _sym(g, s) for s in (1e-5, 1e-2, 1.0, 30.0)}
    top, low = torch.randn(N_MATRICES, generator=g, dtype=torch.float64), torch.rand(N_MATRICES, generator=g, dtype=torch.float64)
    fam["two equal largest eigenvalues"] = _rotated(g, torch.stack([top, top, top - low], dim=1))
    fam["two largest equal to 1e-6 relative"] = _rotated(g, torch.stack([top, top * (1 + 1e-6 * torch.sign(top) * -1), top - 1 - low], dim=1))
    fam["diagonal"] = torch.diag_embed(torch.randn(N_MATRICES, 3, generator=g, dtype=torch.float64))
    return fam


def _emax(E):
    return strain_emax3d(E[:, 0, 0], E[:, 1, 1], E[:, 2, 2], E[:, 0, 1], E[:, 0, 2], E[:, 1, 2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_four_jacobi_sweeps_against_eigvalsh(dtype):
    """strain_emax3d against torch.linalg.eigvalsh in fp64 of the same rounded matrix: fp32 <= 1e-6 ||E||_F, fp64 <= 1e-13 ||E||_F (4 x
    and 50 x the worst measured over 200,000 matrices per family: 2.5e-7 and 2.0e-15)."""
    bound = 1e-6 if dtype == torch.float32 else 1e-13
    for name, E in _families().items():
        E = E.to(dtype)
        E = 0.5 * (E + E.transpose(1, 2))                     # (exactly symmetric once rounded)
        want = torch.linalg.eigvalsh(E.double())[:, -1]
        err = ((_emax(E).double() - want).abs() / torch.linalg.matrix_norm(E.double())).max()
        print(f"{name:40s} {dtype}: worst error {float(err):.2e} ||E||_F")
        assert float(err) <= bound, name


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_zero_matrix_gives_zero_and_a_nan_gives_nan(dtype):
    z = torch.zeros(4, dtype=dtype)
    assert not bool((strain_emax3d(z, z, z, z, z, z) != 0).any())
    for slot in range(6):
        entries = [torch.tensor([0.3, -0.2, 0.0, 1.0], dtype=dtype) * (k + 1) for k in range(6)]
        entries[slot] = entries[slot].clone()
        entries[slot][2] = float("nan")
        got = strain_emax3d(*entries)
        assert bool(torch.isnan(got[2])) and bool(torch.isfinite(got[[0, 1, 3]]).all()), slot
    diag = [torch.tensor([1.0], dtype=dtype), torch.tensor([float("nan")], dtype=dtype), torch.tensor([2.0], dtype=dtype)]
    assert bool(torch.isnan(strain_emax3d(*diag, *[torch.zeros(1, dtype=dtype)] * 3)).all())      # nothing to rotate: the maximum carries it
    disp = torch.zeros(3, 4, 4, 4, dtype=dtype)
    disp[1, 2, 2, 2] = float("nan")
    f = ftle3d_rule(disp, 0.1)
    assert all(bool(torch.isnan(f[at])) for at in ((2, 1, 2), (2, 3, 2), (1, 2, 2), (2, 2, 1)))      # the cells whose differences read it
    assert float(f[2, 2, 2]) == 0.0 and float(f[0, 0, 0]) == 0.0                                      # (a central difference skips its own cell)


# ------------------------------------------------------------------------------------------------ the tie to the density advection
def test_one_backward_step_from_zero_lands_in_the_density_advections_cells():
    """floor(X + d) per axis are the floors the density advection recorded for its final gather, exactly."""
    for cid, state, _ in F3.cases():
        u, v, w, _, d = state
        rec = fluid_rule.Branches()
        fluid_rule.advect(d, (u, v, w), F3.DT, rec)
        floors = rec.log[-3:]                                  # the field interpolation's floors: x, y, z
        disp = flow_map_step3d_rule(torch.zeros(d.shape[0], 3, *d.shape[1:]), u, v, w, dt=F3.DT, direction="backward")
        index = torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in d.shape[1:]], indexing="ij")
        for k, act in enumerate((-1, -2, -3)):
            assert torch.equal(torch.floor(index[act] + disp[:, k]).long(), floors[k].expand_as(disp[:, k])), (cid, k)


def test_the_far_case_leaves_through_all_six_faces_and_the_quirk_case_reads_zero():
    state = dict((cid, s) for cid, s, _ in F3.cases())
    assert F3.leaves_through_all_six_faces(state["6x12x16-B2-a300"])
    assert not F3.leaves_through_all_six_faces(state["4x5x7-B3-a5"])
    (u, v, w, _, _), disp0 = state["4x5x7-B3-quirk"], dict((cid, d) for cid, _, d in F3.cases())["4x5x7-B3-quirk"]
    out = flow_map_step3d_rule(disp0, u, v, w, dt=F3.DT, direction="backward")
    assert not bool((out[:, :, -1, -1, -1] != 0).any())      # the corner's samples and its interpolation all sit on the last index
    assert not bool((out[:, 0, :-1, :-1, -1] != 0).any())    # last column: su reads 0, the trace stays, the interpolation reads 0
    assert bool((out[:, 0, :-1, :-1, :-1] != 0).all())


# ------------------------------------------------------------------------------------------------ the increment's form
def _p_minus_x_step(disp, u, v, w, *, dt, direction, branches):
    """The backward map step with the increment formed as p - X everywhere: the variant the rule rejects."""
    assert direction == "backward"
    grid = disp.shape[-3:]
    index = torch.meshgrid(*[torch.arange(n, dtype=disp.dtype) for n in grid], indexing="ij")
    s = [fluid_rule._sample(c, act, index, branches) for c, act in zip((u, v, w), (-1, -2, -3))]
    p = [_clamp_decided(branches, index[act] - dt * s[k], 0.0, float(grid[act] - 1))[0] for k, act in enumerate((-1, -2, -3))]
    moved = fluid_rule._interpolate(disp, tuple(p[k].unsqueeze(-4) for k in (2, 1, 0)), branches)
    return moved + torch.stack([p[k] - index[act] for k, act in enumerate((-1, -2, -3))], dim=-4)


def _chain(step_fn):
    def rule(u, v, w, p, density, n_steps, *, dt, viscosity, jacobi_iters, direction, branches):
        state = (u, v, w, p, density)
        disp = density.new_zeros(density.shape[0], 3, *density.shape[1:])
        for _ in range(n_steps):
            state = fluid_rule.step(state, dt, viscosity, jacobi_iters, branches)
            disp = step_fn(disp, *state[:3], dt=dt, direction=direction, branches=branches)
        return ftle3d_rule(disp, n_steps * dt)
    return rule


def test_the_increment_form_keeps_small_displacements():
    """On dataset-like (16, 32, 32) states (from rest, 20 steps, J = 20) a particle moves far less per step than ulp(X): the p - X form
    rounds every increment to that grid.  Measured here, as a share of the field's maximum off the fp64 rule along the same branches:
    the rule 3.8e-6 / 1.2e-6, the variant 3.3e-2 / 8.3e-3 (grid 0 / grid 1, with the sources flow_map3d_oracle.dataset_like_state3d
    places).  Held: the rule within 1e-4, and the variant at least 100 x worse."""
    state = F3.dataset_like_state3d()
    assert [tuple(s.shape) for s in state][4] == (2, 16, 32, 32) and not any(bool((s != 0).any()) for s in state[:4])
    oracle, replay = F3.flow_ftle3d_oracle(state, 20, "backward", rule=_chain(flow_map_step3d_rule))
    again = flow_ftle3d_rule(*state, 20, dt=F3.DT, viscosity=F3.NU, jacobi_iters=F3.J, direction="backward")
    assert torch.equal(again.ftle, replay)                    # (the chain written here is flow_ftle3d_rule's)
    _, variant = F3.flow_ftle3d_oracle(state, 20, "backward", rule=_chain(_p_minus_x_step))
    for b in range(2):
        good, bad = O3.metric(replay[b], oracle[b]), O3.metric(variant[b], oracle[b])
        print(f"grid {b}: max ftle {float(oracle[b].max()):.3e} mean {float(oracle[b].mean()):.3e}; rule {good:.2e}, p - X variant {bad:.2e}")
        assert good <= 1e-4 and bad >= 100 * good


# ------------------------------------------------------------------------------------------------ refusals, signatures, the result's fields
def test_refusals():
    D, H, W = 4, 5, 7
    disp = torch.zeros(2, 3, D, H, W)
    u, v, w = torch.zeros(2, D, H + 1, W), torch.zeros(2, D, H, W + 1), torch.zeros(2, D + 1, H, W)
    p = d = torch.zeros(2, D, H, W)
    for fn in (flow_map_step3d_rule, lambda *a, **k: flow_map_step3d(*a, route="torch", **k)):
        with pytest.raises(ValueError, match="direction is 'backward' or 'forward'"):
            fn(disp, u, v, w, direction="sideways")
        with pytest.raises(ValueError, match=r"u must be \(2, 4, 6, 7\)"):
            fn(disp, v, v, w)
        with pytest.raises(ValueError, match=r"w must be \(2, 5, 5, 7\)"):
            fn(disp, u, v, u)
        with pytest.raises(ValueError, match=r"disp must be \[3, D, H, W\] or \[B, 3, D, H, W\]"):
            fn(disp[:, :2], u, v, w)
        with pytest.raises(ValueError, match="D, H, W >= 3"):
            fn(torch.zeros(3, 2, 5, 6), torch.zeros(2, 6, 6), torch.zeros(2, 5, 7), torch.zeros(3, 5, 6))
    for fn, args in ((flow_map_step3d, (disp, u, v, w)), (ftle_field3d, (disp, 0.1)), (flow_ftle3d, (u, v, w, p, d, 2))):
        with pytest.raises(ValueError, match="route is 'hip' or 'torch'"):
            fn(*args, route="cuda")
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # the hip route has none
            fn(*args)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="horizon > 0"):
            ftle3d_rule(disp, bad)
        with pytest.raises(ValueError, match="horizon > 0"):
            ftle_field3d(disp, bad, route="torch")
    with pytest.raises(ValueError, match="disp must be"):
        ftle_field3d(torch.zeros(2, 2, D, H, W), 0.1, route="torch")
    with pytest.raises(ValueError, match="disp must be"):
        ftle3d_rule(torch.zeros(3, 2, H, W), 0.1)
    with pytest.raises(ValueError, match="flow_ftle3d: n_steps >= 1"):
        flow_ftle3d(u, v, w, p, d, 0, route="torch")
    with pytest.raises(ValueError, match="flow_ftle3d: dt > 0"):
        flow_ftle3d(u, v, w, p, d, 2, dt=0.0, route="torch")
    with pytest.raises(ValueError, match="flow_ftle3d: direction"):
        flow_ftle3d(u, v, w, p, d, 2, direction="up", route="torch")
    with pytest.raises(ValueError, match="fluid_step3d: u must be"):
        flow_ftle3d(v, v, w, p, d, 2, route="torch")


def test_signatures_and_exports():
    def defaults(fn):
        return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}
    assert list(inspect.signature(flow_map_step3d).parameters)[:4] == ["disp", "u", "v", "w"]
    assert list(inspect.signature(flow_ftle3d).parameters)[:6] == ["u", "v", "w", "p", "density", "n_steps"]
    assert defaults(flow_map_step3d) == dict(dt=0.01, direction="backward", route="hip")
    assert defaults(flow_map_step3d_rule) == dict(dt=0.01, direction="backward", branches=None)
    assert defaults(ftle_field3d) == dict(route="hip")
    assert defaults(flow_ftle3d) == dict(dt=0.01, viscosity=0.001, jacobi_iters=20, direction="backward", route="hip")
    assert defaults(flow_ftle3d_rule) == dict(dt=0.01, viscosity=0.001, jacobi_iters=20, direction="backward", branches=None)
    assert defaults(physics.SmokeSimulator3D.flow_ftle) == dict(n_steps=20)
    for name in ("flow_ftle3d", "flow_ftle3d_rule", "flow_map_step3d", "flow_map_step3d_rule", "ftle_field3d", "ftle3d_rule"):
        assert name in physics.__all__ and getattr(physics, name) is globals()[name]
    assert physics.FtleResult is FtleResult and "FtleResult" in physics.__all__


def test_the_binding_and_the_header_agree():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION          # additive exports
    for name, nargs in (("smk_flow_map3d_step", 15), ("smk_ftle3d_field", 12)):
        proto = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert proto and len(proto.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name]), name
    assert re.search(r"int64_t smk_ftle3d_workspace\(int32_t B, int32_t D, int32_t H, int32_t W\);", hdr)
    L = _lib.load()
    for name in ("smk_flow_map3d_step", "smk_ftle3d_field", "smk_ftle3d_workspace"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.smk_ftle3d_workspace(2, 4, 16, 8) == 2 * 4 * 2 * 8 and L.smk_ftle3d_workspace(1, 3, 3, 3) == 16      # runs of 16 rows
    assert L.smk_ftle3d_workspace(1, 16, 272, 8) == 256 * 2 * 8                                                   # 4352 rows: runs of 17
    assert L.smk_ftle3d_workspace(1, 3000, 3000, 3) == 256 * 2 * 8                                                # at most 256 runs
    for bad in ((0, 8, 8, 8), (1, 2, 8, 8), (1, 8, 2, 8), (1, 8, 8, 2), (1, 32767, 8, 8), (8192, 7, 8, 8), (1, 8, 32766, 32766)):
        assert L.smk_ftle3d_workspace(*bad) == -1, bad


def test_flow_ftle3d_rule_result_shapes_batched_and_not():
    state = O3.draw_state3d((4, 5, 7), 5.0, batch=2)
    res = flow_ftle3d_rule(*state, 2, direction="forward")
    assert tuple(res.ftle.shape) == (2, 4, 5, 7) and tuple(res.displacement.shape) == (2, 3, 4, 5, 7)
    assert res.mean.dtype == res.max.dtype == torch.float64 and tuple(res.mean.shape) == tuple(res.max.shape) == (2,)
    assert [tuple(s.shape) for s in res.state] == [(2, 4, 6, 7), (2, 4, 5, 8), (2, 5, 5, 7), (2, 4, 5, 7), (2, 4, 5, 7)]
    one = flow_ftle3d_rule(*[s[1] for s in state], 2, direction="forward")
    assert torch.equal(one.ftle, res.ftle[1]) and torch.equal(one.displacement, res.displacement[1])
    assert one.mean.dim() == 0 and float(one.max) == float(res.max[1]) and all(torch.equal(a, b[1]) for a, b in zip(one.state, res.state))
    f, mean, top = ftle_field3d(res.displacement, 0.02, route="torch")
    assert torch.equal(f, res.ftle) and torch.equal(mean, res.mean) and torch.equal(top, res.max)
    f1, mean1, _ = ftle_field3d(res.displacement[0], 0.02, route="torch")
    assert torch.equal(f1, f[0]) and mean1.dim() == 0
    assert torch.equal(flow_map_step3d(res.displacement[0], *[s[0] for s in state[:3]], route="torch"),
                       flow_map_step3d_rule(res.displacement, *state[:3])[0])
    via_route = flow_ftle3d(*state, 2, direction="forward", route="torch")
    assert torch.equal(via_route.ftle, res.ftle)


# ------------------------------------------------------------------------------------------------ the figure
def test_visualizer_plot_ftle3d(tmp_path):
    import matplotlib.pyplot as plt
    from smokephysai_amd.utils import SmokeVisualizer
    viz = SmokeVisualizer()
    g = torch.Generator().manual_seed(0)
    frame, vol = torch.rand(1, 16, 16, generator=g), torch.rand(1, 6, 16, 16, generator=g)
    path = str(tmp_path / "ftle3d.png")
    fig = viz.plot_ftle3d(frame, vol, path)
    with open(path, "rb") as f:
        assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    panels = [ax for ax in fig.axes if ax.get_title()]
    assert [ax.get_title() for ax in panels] == ["Input Smoke", "FTLE (max over depth)", "FTLE Upper Decile"]
    assert len(panels[2].collections) >= 1                     # the contour
    shown = panels[1].images[0].get_array()
    assert float(abs(shown - vol[0].max(dim=0).values.numpy()).max()) == 0.0
    flat = viz.plot_ftle3d(frame.numpy(), torch.zeros(6, 16, 16).numpy())     # a constant volume: no contour, no error
    assert len([ax for ax in flat.axes if ax.get_title()][2].collections) == 0
    with pytest.raises(ValueError):
        viz.plot_ftle3d(frame, torch.zeros(6, 8, 8))
    with pytest.raises(ValueError):
        viz.plot_ftle3d(frame, torch.zeros(16, 16))
    plt.close("all")
