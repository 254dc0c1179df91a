"""smk_tangent_orthonormalize / smk_tangent3d_orthonormalize (csrc/tangent_qr.hip) and what is built on them -- lyapunov_exponents(...,
gram_schmidt="hip"), flow_chaos, SmokeSimulator.flow_chaos and their 3-D twins -- against the oracle of DESIGN.md 3.13: physics'
_gram_schmidt (the torch form the kernel restates) on .double() copies on the CPU.  The replay is _gram_schmidt in fp32 on the CPU.

Metrics.  norms: max |n - n_ref| / n_ref.  Tangents, per field: max |q - q_ref| / max |q_ref| (step_grad_oracle.metric).
Bound.    REPLAY_MARGIN (10) x the replay's worst over the same cases, taken per input kind; for the norms at least 1e-12: at T = 1 and for
          vector 0 the replay's error is exactly 0 and only the fp64 summation order differs, and with fewer than 8,192 elements per state
          N 2^-53 < 1e-12.
Cases.    B = 2; grids (3,3), (5,7), (33,40) -- three runs of rows per grid, the last one partial -- and (3,4,5), (6,9,12); T in
          {1, 2, 3, 8}; kinds normal, nearly dependent (v_j = v_0 + 1e-3 noise), scaled (vector j times 10^(3j-6)); dense and pitched
          (pitch_c = W + 3, pitch_v = W + 5, the padding pre-filled with a sentinel that must survive).

Figures measured on MI355X (device worst / replay worst; the bound is 10 x the replay's; DESIGN.md 3.13 has them all):
  normal ............ norms 2.292e-08 / 2.292e-08, tangents 1.626e-07 / 1.626e-07, |<q_i, q_j> - delta_ij| 1.019e-07
  nearly dependent .. norms 1.261e-05 / 1.261e-05, tangents 1.640e-04 / 1.640e-04
  scaled ............ norms 2.622e-08 / 2.622e-08, tangents 1.764e-07 / 1.764e-07, |<q_i, q_j> - delta_ij| 1.078e-07
  spectrum, k = 3, 16 steps, per log_growth entry: 32 x 32 noise20 4.474e-06 / 4.698e-06, 8 x 12 x 12 6.986e-07 / 7.414e-07"""
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

import step_grad_oracle as O2                                                                     # noqa: E402
import step3d_grad_oracle as O3                                                                   # noqa: E402
from smokephysai_amd import _lib                                                                  # noqa: E402
from smokephysai_amd.physics import (Branches, FlowChaos, SmokeSimulator, SmokeSimulator3D, flow_chaos, flow_chaos3d,        # noqa: E402
                                     fluid_step_rule, kaplan_yorke_dimension, ks_entropy, lyapunov_exponents, lyapunov_exponents3d)
from smokephysai_amd.physics.fluid_tangent import _gram_schmidt                                   # noqa: E402

DEV = "cuda"
B = 2
GRIDS = [(3, 3), (5, 7), (33, 40), (3, 4, 5), (6, 9, 12)]
TS = (1, 2, 3, 8)
KINDS = ("normal", "dependent", "scaled")
NORM_FLOOR = 1e-12
ORTHONORMAL = 1e-5                       # |<q_i, q_j> - delta_ij| in fp64: tests/test_hip_fluid_tangent.py's figure for k = 2
SENTINEL = -7.0
grid_param = pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(str(n) for n in g))


def _bits_equal(a, b):
    if a.dtype == torch.float64:
        return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _field_shapes(grid):
    """The shapes of a state's fields, in the entry points' order: (u, v, p, density) or (u, v, w, p, density)."""
    if len(grid) == 2:
        H, W = grid
        return [(H + 1, W), (H, W + 1), (H, W), (H, W)]
    D, H, W = grid
    return [(D, H + 1, W), (D, H, W + 1), (D + 1, H, W), (D, H, W), (D, H, W)]


@functools.lru_cache(maxsize=None)
def _draw(grid, T, kind, batch=B):
    """T vectors per grid, each a whole state: a tuple of CPU fp32 fields [batch, T, ...] from a seeded generator."""
    g = O2._gen(700 + KINDS.index(kind), T, *grid)
    fields = [torch.randn(batch, T, *s, generator=g) for s in _field_shapes(grid)]
    if kind == "dependent":
        fields = [torch.cat([f[:, :1], f[:, :1] + 1e-3 * f[:, 1:]], dim=1) for f in fields]
    elif kind == "scaled":
        scale = torch.tensor([10.0 ** (3 * j - 6) for j in range(T)])
        fields = [f * scale.view(1, T, *[1] * (f.dim() - 2)) for f in fields]
    return tuple(fields)


@functools.lru_cache(maxsize=None)
def _references(grid, T, kind):
    """-> ((oracle tangents fp64, oracle norms), (replay tangents fp32, replay norms)): computed once, shared, left unchanged."""
    fields = _draw(grid, T, kind)
    return _gram_schmidt(tuple(f.double() for f in fields)), _gram_schmidt(fields)


def _call(fields, pitched=False, entry="orthonormalize"):
    """One call of smk_tangent[3d]_orthonormalize (entry="renorm": smk_tangent[3d]_renorm) on device copies of CPU fields [Bn, T, ...]
    -> (fields as the kernel left them (CPU), norms [Bn, T] fp64 (CPU), whether the pitch padding still holds its sentinel)."""
    L = _lib.load()
    Bn, T = fields[0].shape[:2]
    grid = tuple(fields[-1].shape[2:])
    W = grid[-1]
    pc, pv = (W + 3, W + 5) if pitched else (W, W + 1)
    name = "smk_tangent" + ("3d" if len(grid) == 3 else "") + "_" + entry
    bufs = []
    for i, f in enumerate(fields):
        buf = torch.full((*f.shape[:-1], pv if i == 1 else pc), SENTINEL, device=DEV)
        buf[..., :f.shape[-1]] = f.to(DEV)
        bufs.append(buf)
    norms = torch.full((Bn, T), -1.0, dtype=torch.float64, device=DEV)
    nbytes = int(getattr(L, name + "_workspace")(Bn, T, *grid))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    _lib.check(getattr(L, name)(*[b.data_ptr() for b in bufs], norms.data_ptr(), Bn, T, *grid, pc, pv, ws.data_ptr(), nbytes,
                                _lib.stream_ptr(torch.device(DEV, 0))))
    padding = all(bool((b[..., f.shape[-1]:] == SENTINEL).all()) for b, f in zip(bufs, fields))
    return [b[..., :f.shape[-1]].contiguous().cpu() for b, f in zip(bufs, fields)], norms.cpu(), padding


def _gram(fields, b):
    """<q_i, q_j> over whole states of grid b in fp64 -> [T, T]."""
    T = fields[0].shape[1]
    flat = torch.cat([f[b].double().reshape(T, -1) for f in fields], dim=1)
    return flat @ flat.t()


def _rel(n, ref):
    return float(((n - ref).abs() / ref).max())


# ------------------------------------------------------------------------------------------------ 1. the bounds
@pytest.mark.parametrize("kind", KINDS)
def test_orthonormalize_stays_within_ten_times_the_replay(kind):
    dev_n = rep_n = dev_t = rep_t = ortho = 0.0
    for grid in GRIDS:
        for T in TS:
            (oracle, oracle_n), (replay, replay_n) = _references(grid, T, kind)
            rep_n = max(rep_n, _rel(replay_n, oracle_n))
            rep_t = max(rep_t, max(O2.metric(q, r) for q, r in zip(replay, oracle)))
            dense = None
            for pitched in (False, True):
                got, norms, padding = _call(_draw(grid, T, kind), pitched)
                assert padding, f"{grid}, T={T}, {kind}: the pitch padding was written to"
                assert bool(torch.isfinite(norms).all()) and all(bool(torch.isfinite(q).all()) for q in got)
                dn, dt_ = _rel(norms, oracle_n), max(O2.metric(q, r) for q, r in zip(got, oracle))
                dev_n, dev_t = max(dev_n, dn), max(dev_t, dt_)
                if dense is None:
                    dense = (got, norms)
                else:                                                # the pitch changes addresses only
                    assert _bits_equal(norms, dense[1]) and all(_bits_equal(a, b) for a, b in zip(got, dense[0])), (grid, T)
                if kind != "dependent":
                    for b in range(B):
                        ortho = max(ortho, float((_gram(got, b) - torch.eye(T, dtype=torch.float64)).abs().max()))
    bound_n, bound_t = max(O2.REPLAY_MARGIN * rep_n, NORM_FLOOR), O2.REPLAY_MARGIN * rep_t
    print(f"{kind}: norms device {dev_n:.3e}, replay {rep_n:.3e}, bound {bound_n:.3e}; tangents device {dev_t:.3e}, replay {rep_t:.3e}, "
          f"bound {bound_t:.3e}; |<q_i, q_j> - delta_ij| {ortho:.3e}")
    assert dev_n <= bound_n, f"{kind}: norms {dev_n:.3e} exceed {bound_n:.3e}"
    assert dev_t <= bound_t, f"{kind}: tangents {dev_t:.3e} exceed {bound_t:.3e}"
    if kind != "dependent":
        assert ortho <= ORTHONORMAL, f"{kind}: {ortho:.3e}"


# ------------------------------------------------------------------------------------------------ 2. the bits
@grid_param
def test_two_calls_and_a_grid_alone_give_the_same_bits(grid):
    fields = _draw(grid, 3, "normal")
    got, norms, _ = _call(fields)
    again, norms2, _ = _call(fields)
    assert _bits_equal(norms, norms2) and all(_bits_equal(a, b) for a, b in zip(got, again))
    for b in range(B):                                               # a grid alone: its batch mates do not matter
        alone, n1, _ = _call([f[b:b + 1] for f in fields])
        assert _bits_equal(n1[0], norms[b]) and all(_bits_equal(a[0], g[b]) for a, g in zip(alone, got)), b


@grid_param
def test_one_vector_is_the_renorm_entry_point_and_vector_zero_never_sees_the_others(grid):
    fields = _draw(grid, 3, "scaled")
    first = [f[:, :1].contiguous() for f in fields]
    one, n1, _ = _call(first)
    renorm, nr, _ = _call(first, entry="renorm")
    assert _bits_equal(n1, nr) and all(_bits_equal(a, b) for a, b in zip(one, renorm))
    for pitched in (False, True):
        three, n3, _ = _call(fields, pitched)
        assert _bits_equal(n3[:, 0], n1[:, 0]) and all(_bits_equal(a[:, 0], b[:, 0]) for a, b in zip(three, one))
    whole, nw, _ = _call(fields, entry="renorm")                     # (the renorm entry point at T = 3 agrees on vector 0 as well)
    assert _bits_equal(nw[:, 0], n1[:, 0])


@pytest.mark.parametrize("grid", [(33, 40), (6, 9, 12)], ids=["33x40", "6x9x12"])
def test_a_zero_vector_stays_zero_and_is_invisible_to_the_others(grid):
    fields = [f.clone() for f in _draw(grid, 3, "normal")]
    for f in fields:
        f[1, 1] = 0.0                                                # vector 1 of grid 1 is all zero
    got, norms, _ = _call(fields)
    clean, clean_n, _ = _call(_draw(grid, 3, "normal"))
    assert float(norms[1, 1]) == 0.0 and all(not bool((q[1, 1] != 0).any()) for q in got)
    two, n2, _ = _call([f[1:2, [0, 2]].contiguous() for f in fields])            # vectors 0 and 2 of grid 1, as if T were 2
    assert _bits_equal(norms[1, [0, 2]], n2[0]) and all(_bits_equal(q[1, [0, 2]], t[0]) for q, t in zip(got, two))
    assert _bits_equal(norms[0], clean_n[0]) and all(_bits_equal(q[0], c[0]) for q, c in zip(got, clean))            # the batch mate


@pytest.mark.parametrize("grid", [(33, 40), (6, 9, 12)], ids=["33x40", "6x9x12"])
def test_a_nan_stays_in_its_own_grid(grid):
    fields = [f.clone() for f in _draw(grid, 3, "normal")]
    fields[1][0, 0].view(-1)[5] = float("nan")                       # one element of v in vector 0 of grid 0
    got, norms, padding = _call(fields, pitched=True)
    clean, clean_n, _ = _call(_draw(grid, 3, "normal"), pitched=True)
    assert padding and bool(torch.isnan(norms[0]).all())
    for q, f in zip(got, fields):
        assert _bits_equal(q[0, 0], f[0, 0])                         # vector 0: the norm is not finite, so it is left unscaled
        assert bool(torch.isnan(q[0, 1:]).all())                     # the later vectors of that grid: NaN, as in torch
    want, want_n = _gram_schmidt(tuple(fields))
    assert bool(torch.isnan(want_n[0]).all()) and all(bool(torch.isnan(q[0, 1:]).all()) for q in want)
    assert _bits_equal(norms[1], clean_n[1]) and all(_bits_equal(q[1], c[1]) for q, c in zip(got, clean))


# ------------------------------------------------------------------------------------------------ 3. the spectrum, end to end
def _noise20_state():
    """tests/test_hip_fluid_tangent.py's `noise20` state: 32 x 32, B = 2, one Gaussian source per grid over white-noise velocities of
    amplitude 20, 10 steps of the fp32 rule, J = 20."""
    H = W = 32
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    d = torch.stack([torch.exp(-((xx - x0) ** 2 + (yy - y0) ** 2).float() / (2 * s * s)) for x0, y0, s in ((16, 20, 3.0), (12, 14, 4.0))])
    g = O2._gen(90)
    u, v = 20.0 * (2 * torch.rand(B, H + 1, W, generator=g) - 1), 20.0 * (2 * torch.rand(B, H, W + 1, generator=g) - 1)
    state = (u, v, torch.zeros(B, H, W), d)
    for _ in range(10):
        state = fluid_step_rule(*state, jacobi_iters=20)
    return state


def _volume_state():
    """8 x 12 x 12, B = 2: draw_state3d at amplitude 5 with white-noise velocities of amplitude 20 added."""
    u, v, w, p, d = O3.draw_state3d((8, 12, 12), 5.0)
    g = O2._gen(91)
    u, v, w = [c + 20.0 * (2 * torch.rand(c.shape, generator=g) - 1) for c in (u, v, w)]
    return u, v, w, p, d


@pytest.mark.parametrize("nd", [2, 3], ids=["32x32-noise20", "8x12x12"])
def test_the_spectrum_against_the_benettin_run_along_the_branches(nd):
    state, spectrum = (_noise20_state(), lyapunov_exponents) if nd == 2 else (_volume_state(), lyapunov_exponents3d)
    rec = Branches()
    replay = spectrum(*state, 16, k=3, route="torch", branches=rec)
    oracle = spectrum(*[s.double() for s in state], 16, k=3, route="torch", branches=rec.replayer())
    got = spectrum(*[s.to(DEV) for s in state], 16, k=3, gram_schmidt="hip")
    assert tuple(got.log_growth.shape) == (B, 16, 3) and got.log_growth.dtype == torch.float64
    for a, b in zip(got.state, replay.state):
        assert torch.equal(a.cpu(), b)
    rep = float((replay.log_growth - oracle.log_growth).abs().max())
    dev = float((got.log_growth.cpu() - oracle.log_growth).abs().max())
    bound = min(O2.PROJECT_BOUND, O2.REPLAY_MARGIN * rep)
    print(f"spectrum {nd}-D: exponents {oracle.exponents.tolist()}; per log_growth entry: device {dev:.3e}, replay {rep:.3e}, bound {bound:.3e}")
    assert dev <= bound
    for b in range(B):
        assert float((_gram([t.cpu() for t in got.tangents], b) - torch.eye(3, dtype=torch.float64)).abs().max()) <= ORTHONORMAL
    again = spectrum(*[s.to(DEV) for s in state], 16, k=3, gram_schmidt="hip")
    assert torch.equal(again.log_growth, got.log_growth) and all(_bits_equal(a, b) for a, b in zip(again.tangents, got.tangents))


@pytest.mark.parametrize("batch", [None, 2], ids=["single", "batched"])
@pytest.mark.parametrize("nd", [2, 3], ids=["2d", "3d"])
def test_flow_chaos_leaves_the_simulator_alone(nd, batch):
    if nd == 2:
        sim, chaos = SmokeSimulator((32, 32), device=DEV, batch_size=batch), flow_chaos
        sim.add_incense_source([(16, 20)], [1.0])
    else:
        sim, chaos = SmokeSimulator3D((8, 16, 16), device=DEV, batch_size=batch), flow_chaos3d
        sim.add_incense_source([(8, 10, 4)], [1.0])
    for _ in range(10):
        sim.simulate_step(add_fractal=False)
    ns = sim.ns_solver
    before = [t.clone() for t in ns.state()]
    feats = sim.get_chaos_features()
    if nd == 2:
        kept = [h.clone() for h in sim.history]
    else:
        kept, hist_len = sim._ring.clone(), sim.history_len
    got = sim.flow_chaos(n_steps=8, k=3)
    for a, b in zip(ns.state(), before):
        assert _bits_equal(a, b)
    if nd == 2:
        assert len(sim.history) == len(kept) and all(_bits_equal(a, b) for a, b in zip(sim.history, kept))
    else:
        assert sim.history_len == hist_len and torch.equal(sim._ring, kept)
    assert sim.get_chaos_features() == feats
    want = chaos(*before, 8, k=3, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters)
    assert isinstance(want, FlowChaos) and tuple(want.exponents.shape) == (batch or 1, 3) and want.exponents.dtype == torch.float64
    assert bool((want.exponents[:, :-1] >= want.exponents[:, 1:]).all())         # sorted descending
    assert torch.equal(want.lyapunov, want.exponents[:, 0])
    ky, truncated = kaplan_yorke_dimension(want.exponents)
    assert torch.equal(want.kaplan_yorke, ky) and torch.equal(want.truncated, truncated) and want.truncated.dtype == torch.bool
    assert torch.equal(want.ks_entropy, ks_entropy(want.exponents))
    assert bool(torch.isfinite(want.exponents).all())
    if batch is None:
        assert set(got) == {"lyapunov", "kaplan_yorke", "ks_entropy", "truncated", "exponents"}
        assert all(isinstance(got[key], float) for key in ("lyapunov", "kaplan_yorke", "ks_entropy")) and isinstance(got["truncated"], bool)
        assert got["exponents"] == want.exponents[0].tolist() and got["lyapunov"] == got["exponents"][0]
        assert got["kaplan_yorke"] == float(want.kaplan_yorke[0]) and got["ks_entropy"] == float(want.ks_entropy[0])
        assert got["truncated"] == bool(want.truncated[0])
    else:
        assert isinstance(got, FlowChaos)
        for name in ("exponents", "lyapunov", "kaplan_yorke", "ks_entropy", "truncated", "log_growth"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
