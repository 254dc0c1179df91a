"""Oracle, replay, draws and closed forms for the differentiable 2-D fluid step (smokephysai_amd/physics/fluid_grad.py).
A plain helper module, imported by tests/test_fluid_grad_host.py (CPU) and tests/test_hip_fluid_grad.py (device).

Oracle.   fluid_step_rule in fp32 on the CPU with a Branches recorder, then the same rule in fp64 replaying those branches, and torch
          autograd of sum(out * g): the fp64 derivative along the fp32 run's integer decisions.  A free-running fp64 rule is the wrong
          yardstick: fp32 and fp64 take different floor branches on real states (a displacement of 1e-8 cell vanishes in fp32), and the
          interpolant's slope jumps there.
Replay.   torch's fp32 autograd of the rule on the CPU: the arithmetic error of an fp32 backward in another summation order.  It takes the
          device's branches, because the device forward is bit-identical to the CPU rule.
Metric.   per gradient tensor: max|d - ref| / max|ref|; where max|ref| == 0 the tensor must be exactly 0.
Bounds.   the project's 1e-4, and 10 x the replay's worst over the same cases (the renderers' margin for summation order)."""
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from smokephysai_amd.physics.fluid_grad import Branches, advect_rule, buoy_diffuse_rule, fluid_step_rule, project_rule   # noqa: E402

PROJECT_BOUND = 1e-4
REPLAY_MARGIN = 10.0
B = 2
NAMES = ("du", "dv", "dp", "ddensity")

# (shape, (dt, velocity amplitude, jacobi_iters)) of the drawn whole-step cases
SHAPES = [(3, 3), (5, 7), (16, 24), (33, 40), (64, 64)]
REGIMES = [(0.01, 60.0, 20), (0.1, 6.0, 3)]
BIG = ((64, 64), (0.01, 90.0, 100))


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


def _smooth(t):
    """One pass of the 3 x 3 binomial filter with replicate padding (keeps the amplitude bound: a convex combination)."""
    def blur(x, dim):
        n = x.shape[dim]
        lo = torch.cat([x.narrow(dim, 0, 1), x.narrow(dim, 0, n - 1)], dim=dim)
        hi = torch.cat([x.narrow(dim, 1, n - 1), x.narrow(dim, n - 1, 1)], dim=dim)
        return 0.25 * lo + 0.5 * x + 0.25 * hi
    return blur(blur(t, -1), -2)


def draw_state(shape, amplitude, seed=0, batch=B, smooth=0):
    """A drawn state (CPU fp32): velocities amplitude * (2 rand - 1), a carried-over p of unit normal noise, densities rand^4 * 2.
    smooth: passes of the 3 x 3 binomial filter over the velocities.  White noise has a divergence of the order of 4 * amplitude per cell,
    which the projection answers with velocities of up to about 1.5 times the amplitude: at amplitude * dt = 0.6 the back-traces still
    move less than a cell (at most 0.94 over the shapes here, max_move), at 0.9 they would not (1.29 at 64 x 64), so that case is drawn
    with one pass (0.66)."""
    H, W = shape
    g = _gen(seed, H, W, int(amplitude))
    u = amplitude * (2 * torch.rand(batch, H + 1, W, generator=g) - 1)
    v = amplitude * (2 * torch.rand(batch, H, W + 1, generator=g) - 1)
    for _ in range(smooth):
        u, v = _smooth(u), _smooth(v)
    p = torch.randn(batch, H, W, generator=g)
    d = torch.rand(batch, H, W, generator=g) ** 4 * 2
    return u, v, p, d


def draw_upstream(state, seed=0, only_density=False):
    g = _gen(seed + 101, *state[3].shape)
    gs = [torch.randn(t.shape, generator=g) for t in state]
    return [None, None, None, gs[3]] if only_density else gs


@functools.lru_cache(maxsize=None)
def simulated_state(steps=30, J=20):
    """The 48 x 48 state after `steps` steps of the fp32 rule from rest with two sources per grid (B grids, different sources)."""
    H = W = 48
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")

    def source(x, y, radius, intensity):
        dist = torch.sqrt(((xx - x) ** 2 + (yy - y) ** 2).float())
        return torch.where(dist <= radius, intensity * torch.exp(-(dist * dist) / (2 * (radius / 3) ** 2)), torch.zeros(()))
    d = torch.stack([source(16, 30, 6, 1.0) + source(33, 20, 8, 1.5), source(24, 24, 10, 1.0) + source(10, 12, 5, 2.0)])
    state = (torch.zeros(B, H + 1, W), torch.zeros(B, H, W + 1), torch.zeros(B, H, W), d)
    for _ in range(steps):
        state = fluid_step_rule(*state, jacobi_iters=J)
    return tuple(t.clone() for t in state)


def rest_state(shape=(16, 24)):
    """At rest with a source: every back-trace coordinate is a tie (X - dt * 0 is an integer and sits on the clamp bounds at the rim)."""
    H, W = shape
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    dist = torch.sqrt(((xx - W // 2) ** 2 + (yy - H // 2) ** 2).float())
    d = torch.where(dist <= 5, torch.exp(-(dist * dist) / (2 * (5 / 3) ** 2)), torch.zeros(()))
    d = torch.stack([d, 0.5 * d.flip(-1)])
    return torch.zeros(B, H + 1, W), torch.zeros(B, H, W + 1), torch.zeros(B, H, W), d


def grads_of(fn, inputs, upstream, dtype, branches):
    """torch autograd of sum(out * g) for out = fn(*inputs, branches=...) in `dtype` on the CPU -> (gradients, outputs)."""
    xs = [t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    outs = fn(*xs, branches=branches)
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, upstream) if g is not None)
    grads = torch.autograd.grad(loss, xs, allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for g, x in zip(grads, xs)], [o.detach() for o in outs]


def oracle_and_replay(fn, inputs, upstream):
    """-> (oracle gradients fp64, replay gradients fp32, fp32 outputs): fn(*inputs, branches=) is run in fp32 recording its branches (the
    replay), then in fp64 along them (the oracle)."""
    rec = Branches()
    replay, outs = grads_of(fn, inputs, upstream, torch.float32, rec)
    oracle, _ = grads_of(fn, inputs, upstream, torch.float64, rec.replayer())
    return oracle, replay, outs


def step_fn(dt, viscosity, J, n_steps=1):
    def fn(u, v, p, d, branches=None):
        state = (u, v, p, d)
        for _ in range(n_steps):
            state = fluid_step_rule(*state, dt=dt, viscosity=viscosity, jacobi_iters=J, branches=branches)
        return state
    return fn


def metric(d, ref):
    """max|d - ref| / max|ref|; with max|ref| == 0: 0.0 if d is exactly 0, inf otherwise."""
    d, ref = d.detach().double().cpu(), ref.detach().double().cpu()
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if not bool((d != 0).any()) else float("inf")
    return float((d - ref).abs().max()) / top


def device_bounds(replay_worst):
    """The two bounds a device figure must stay within, given the replay's worst over the same cases."""
    return PROJECT_BOUND, REPLAY_MARGIN * replay_worst


def max_move(state, dt, viscosity, J):
    """An upper bound of the largest back-trace displacement (cells) of the step's three advections: dt * max|velocity| over the
    velocities they sample (a sample is a convex combination of two cells, or 0)."""
    u, v, _ = buoy_diffuse_rule(state[0], state[1], state[3], dt=dt, viscosity=viscosity)
    u, v, _ = project_rule(u, v, state[2], dt=dt, jacobi_iters=J)
    ua = advect_rule(u, u, v, dt=dt)
    va = advect_rule(v, ua, v, dt=dt)
    return dt * max(float(t.abs().max()) for t in (u, v, ua, va))


def whole_step_cases():
    """[(id, state, (dt, viscosity, J))] of the bounds test: the drawn shapes x regimes, the big one, the simulated state, the state at
    rest.  Each is run with g on all four outputs and with g on the density alone."""
    cases = []
    for shape in SHAPES:
        for dt, amp, J in REGIMES:
            cases.append((f"{shape[0]}x{shape[1]}-dt{dt}-a{amp:g}-J{J}", draw_state(shape, amp), (dt, 0.001, J)))
    shape, (dt, amp, J) = BIG
    cases.append((f"{shape[0]}x{shape[1]}-dt{dt}-a{amp:g}-J{J}", draw_state(shape, amp, smooth=1), (dt, 0.001, J)))
    cases.append(("simulated-48x48", simulated_state(), (0.01, 0.001, 20)))
    cases.append(("rest-16x24", rest_state(), (0.01, 0.001, 20)))
    return cases


# ------------------------------------------------------------------------------------------------ closed forms of the device backward
def project_backward_form(gu, gv, gp, dt, J):
    """The transposed projection as csrc/fluid_grad.hip computes it: lambda = gp plus the gradient subtraction's
    transpose; J times: m = interior-masked lambda, ddiv -= 0.25 m, lambda = 0.25 * (neighbour sum of m, zero outside the grid); then
    dp = lambda, g = ddiv / dt, du = gu with +g on [1:] and -g on [:-1], dv likewise along x."""
    lam = gp.clone()
    lam[..., 1:, :] -= dt * gu[..., 1:-1, :]
    lam[..., :-1, :] += dt * gu[..., 1:-1, :]
    lam[..., :, 1:] -= dt * gv[..., :, 1:-1]
    lam[..., :, :-1] += dt * gv[..., :, 1:-1]
    ddiv = torch.zeros_like(lam)
    mask = torch.zeros_like(lam)
    mask[..., 1:-1, 1:-1] = 1
    for _ in range(J):
        m = lam * mask
        ddiv = ddiv - 0.25 * m
        mp = torch.nn.functional.pad(m, (1, 1, 1, 1))
        lam = 0.25 * (mp[..., :-2, 1:-1] + mp[..., 2:, 1:-1] + mp[..., 1:-1, :-2] + mp[..., 1:-1, 2:])
    g = ddiv / dt
    du, dv = gu.clone(), gv.clone()
    du[..., 1:, :] += g
    du[..., :-1, :] -= g
    dv[..., :, 1:] += g
    dv[..., :, :-1] -= g
    return du, dv, lam


def _taps(h, w, y, x):
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = (x0 + 1).clamp(0, w - 1), (y0 + 1).clamp(0, h - 1)
    x0, y0 = x0.clamp(0, w - 1), y0.clamp(0, h - 1)
    fx0, fx1, fy0, fy1 = (t.to(x.dtype) for t in (x0, x1, y0, y1))
    return (y0, y1, x0, x1), ((fx1 - x) * (fy1 - y), (x - fx0) * (fy1 - y), (fx1 - x) * (y - fy0), (x - fx0) * (y - fy0)), (fx0, fx1, fy0, fy1)


def advect_backward_form(field, u, v, gout, dt, decay=1.0):
    """The 3 x 3 gather of csrc/fluid_grad.hip for one un-batched advection out = adv(field; u, v) * decay, in the inputs' dtype:
    -> (dfield, du, dv, far).  Per destination the forward's own taps and weights; dfield[j] sums, over the 3 x 3 destinations around j in
    row-major order, g times the weights of the taps that are j; du[j] sums (-dt gpx) times the weight with which the destinations
    (y, x-1), (y, x) sample u[j]; dv[j] likewise from (y-1, x), (y, x)."""
    R, C = field.shape
    H, W = u.shape[0] - 1, u.shape[1]
    dtype = field.dtype
    Y, X = torch.meshgrid(torch.arange(R, dtype=dtype), torch.arange(C, dtype=dtype), indexing="ij")
    ut, uw, _ = _taps(H + 1, W, Y, (X + 0.5).clamp(0, W - 1))
    vt, vw, _ = _taps(H, W + 1, (Y + 0.5).clamp(0, H - 1), X)
    ui = sum(wk * u[ty, tx] for wk, (ty, tx) in zip(uw, ((ut[0], ut[2]), (ut[0], ut[3]), (ut[1], ut[2]), (ut[1], ut[3]))))
    vi = sum(wk * v[ty, tx] for wk, (ty, tx) in zip(vw, ((vt[0], vt[2]), (vt[0], vt[3]), (vt[1], vt[2]), (vt[1], vt[3]))))
    pxu, pyu = X - dt * ui, Y - dt * vi
    far = bool(((pxu - X).abs() >= 1).any() or ((pyu - Y).abs() >= 1).any())
    px, py = pxu.clamp(0, C - 1), pyu.clamp(0, R - 1)
    (y0, y1, x0, x1), ws, (fx0, fx1, fy0, fy1) = _taps(R, C, py, px)
    g = gout * decay
    f00, f01, f10, f11 = field[y0, x0], field[y0, x1], field[y1, x0], field[y1, x1]
    gpx = g * ((fy1 - py) * (f01 - f00) + (py - fy0) * (f11 - f10)) * ((pxu >= 0) & (pxu <= C - 1))
    gpy = g * ((fx1 - px) * (f10 - f00) + (px - fx0) * (f11 - f01)) * ((pyu >= 0) & (pyu <= R - 1))

    def padded(t, fill):
        return torch.nn.functional.pad(t, (1, 1, 1, 1), value=fill)
    jy, jx = torch.meshgrid(torch.arange(R), torch.arange(C), indexing="ij")
    dfield = torch.zeros(R, C, dtype=dtype)
    taps = ((y0, x0), (y0, x1), (y1, x0), (y1, x1))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sl = (slice(1 + dy, 1 + dy + R), slice(1 + dx, 1 + dx + C))
            for (ty, tx), wk in zip(taps, ws):
                hit = (padded(ty, -1)[sl] == jy) & (padded(tx, -1)[sl] == jx)
                dfield = dfield + torch.where(hit, padded(g * wk, 0.0)[sl], torch.zeros((), dtype=dtype))
    # velocity stencils: scatter the per-destination terms to the taps (<= 2 destinations per cell, so the order is immaterial in exact
    # arithmetic; the kernel gathers them)
    du, dv = torch.zeros_like(u), torch.zeros_like(v)
    tpx, tpy = -dt * gpx, -dt * gpy
    du.index_put_((ut[0], ut[2]), tpx * uw[0], accumulate=True)
    du.index_put_((ut[0], ut[3]), tpx * uw[1], accumulate=True)
    dv.index_put_((vt[0], vt[2]), tpy * vw[0], accumulate=True)
    dv.index_put_((vt[1], vt[2]), tpy * vw[2], accumulate=True)
    return dfield, du, dv, far
