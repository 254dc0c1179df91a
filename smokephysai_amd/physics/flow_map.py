"""The flow map of the 2-D stepper and its finite-time Lyapunov exponent (FTLE) field, on libsmokehip (csrc/flow_map.hip).  DESIGN.md section
3.14.

A displacement field disp [B, 2, H, W] = (dx, dy) at the cell centres, in cells, stands for the map x -> x + disp.  After every step() the
step's own first-order trace -- with its output velocities, the ones its density advection sampled -- is composed into it:
  direction="backward"   x + disp is where the particle now at x was when the window began (semi-Lagrangian composition in time order).
                         Ridges of its FTLE are where smoke filaments collect.
  direction="forward"    x + disp is where the particle that began at x is now.
The FTLE of the map over a window of n_steps * dt is log(largest singular value of its gradient) / horizon, per cell: the local, Lagrangian
counterpart of fluid_tangent.py's global exponents, and unlike them it tells one sample of the dataset from another (section 3.14).

  flow_map_step_rule(disp, u, v, ...)   the rule of one map step in torch ops over fluid_rule's _sample / _interpolate / Branches: any dtype
                                        and device, fp32 decisions replayable in fp64.
  ftle_rule(disp, horizon)              the FTLE field of a displacement field, likewise.
  flow_ftle_rule(u, v, p, density, n)   fluid_rule.step and the map step chained: route="torch", and the tests' oracle.
  flow_map_step / ftle_field / flow_ftle   the public functions; route="hip": smk_flow_map_step and smk_ftle_field.

The rule, one rounding per listed op.  Backward, at cell (Y, X): su, sv = the density advection's velocity samples; ax = X - dt su,
px = clamp(ax, 0, W - 1); the increment ix = -(dt su) where 0 <= ax <= W - 1 (bounds included), px - X otherwise; y likewise;
dx' = interp(dx; py, px) + ix, dy' = interp(dy; py, px) + iy (interp: floor, clamped indices, weights from the clamped indices -- a position
on the last index reads 0, the reference's quirk).  Forward: qx = clamp(X + dx, 0, W - 1), qy likewise, sample positions only; su = u
sampled at (qy, qx) by the interpolate_velocity_u rule, sv likewise; dx' = min(max(dx + dt su, -X), W - 1 - X), dy' likewise (the bounds
are exact integers in fp32).

The increment is never formed as px - X where the clamp passes.  X - dt su is rounded to a multiple of ulp(X), 7.6e-6 at X = 64, while the
dataset's flows displace a particle by about 3e-5 cells per step: on such 64 x 64 states the fp32 FTLE of the px - X form differed from the
fp64 one by 3-7 % of the field's maximum, that of the form above by 2-5e-6 of it (measured on the CPU; tests/test_flow_map_host.py holds
the property).

FTLE: with a = dx, b = dy and their differences at unit spacing (central with a factor 0.5 inside, one-sided on the first and last row and
column), the Green-Lagrange strain formed so that the identity never enters --
  exx = a_x + 0.5 (a_x^2 + b_x^2),  eyy = b_y + 0.5 (a_y^2 + b_y^2),  exy = 0.5 (a_y + b_x) + 0.5 (a_x a_y + b_x b_y),
  m = 0.5 (exx + eyy),  d = 0.5 (exx - eyy),  emax = m + sqrt(d^2 + exy^2),
  ftle = log1p(max(2 emax, lo)) / (2 horizon),  lo = the fp32 number next above -1 (so the result is finite).
Values may be negative where the map contracts in every direction: the projected velocities are only approximately divergence-free.

Where things live: what the flow map of a 2-D and of a 3-D stepper share -- the direction, route and window checks, the shape checks, the
result packing, the single calls and the chained loop -- is written once here over a MapRoute record (fluid_grad's HipRoute, the two rules
and the entry points' names): the route_* functions.  The public functions below bind them to MAP2, those of flow_map3d.py (DESIGN.md
section 3.15, which also has the 3-D rule) to MAP3.

Out of scope: a dataset label built from the statistics, derivatives of the map, higher-order particle integration (the stepper's own
first-order trace is the flow being described)."""
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from . import fluid_rule
from .fluid_grad import HIP2, Branches, HipRoute, check_state, simulator

__all__ = ["FtleResult", "flow_ftle", "flow_ftle_rule", "flow_map_step", "flow_map_step_rule", "ftle_field", "ftle_rule"]

DIRECTIONS = {"backward": 0, "forward": 1}                  # smk_flow_map_step's constants
LO = float(np.nextafter(np.float32(-1.0), np.float32(0.0)))  # -1 + 2^-24, in every dtype


# ------------------------------------------------------------------------------------------------ the rule in torch ops
def _clamp_decided(br, x, lo, hi):
    """br.clamp(x, lo, hi) for scalar or tensor bounds, and where it passed (lo <= x <= hi, bounds included): the recorded decision on a
    replay, so an fp64 run takes the fp32 run's."""
    lt, gt = br._next(lambda: (x.detach() < lo, x.detach() > hi))
    lo, hi = (torch.as_tensor(b, dtype=x.dtype, device=x.device) for b in (lo, hi))
    return torch.where(lt, lo, torch.where(gt, hi, x)), ~(lt | gt)


def _direction(direction, what):
    if direction not in DIRECTIONS:
        raise ValueError(f"{what}: direction is 'backward' or 'forward', got {direction!r}")
    return DIRECTIONS[direction]


def _check_disp(dim, disp, vel, what):
    """Shapes of one map step's operands (leading dimensions: [B] or none) over the dimension record -> the grid (H, W) or (D, H, W)."""
    nd = dim.nd
    if disp.dim() not in (nd + 1, nd + 2) or disp.shape[-nd - 1] != nd:
        raise ValueError(f"{what}: disp must be [{nd}, {dim.axes}] or [B, {nd}, {dim.axes}], got {tuple(disp.shape)}")
    lead, grid = tuple(disp.shape[:-nd - 1]), tuple(disp.shape[-nd:])
    for name, t, want in zip(dim.fields, vel, dim.shapes(lead, grid)):
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: {name} must be {want} beside disp {tuple(disp.shape)}, got {tuple(t.shape)}")
    if min(grid) < 3:
        raise ValueError(f"{what}: {dim.axes} >= 3")
    return grid


def flow_map_step_rule(disp, u, v, *, dt: float = 0.01, direction: str = "backward", branches: Optional[Branches] = None):
    """One map step in torch ops (module docstring): disp [..., 2, H, W], u [..., H+1, W], v [..., H, W+1] of any floating dtype on any
    device -> disp'.  branches: a Branches recorder (filled) or replayer (followed); None: decisions are made and not kept."""
    forward = _direction(direction, "flow_map_step_rule")
    H, W = _check_disp(HIP2, disp, (u, v), "flow_map_step_rule")
    br = Branches() if branches is None else branches
    Y, X = torch.meshgrid(*[torch.arange(n, dtype=disp.dtype, device=disp.device) for n in (H, W)], indexing="ij")
    dx, dy = disp[..., 0, :, :], disp[..., 1, :, :]
    if forward:
        qx = br.clamp(X + dx, 0.0, float(W - 1))
        qy = br.clamp(Y + dy, 0.0, float(H - 1))
        su = fluid_rule._sample(u, -1, (qy, qx), br)
        sv = fluid_rule._sample(v, -2, (qy, qx), br)
        nx, _ = _clamp_decided(br, dx + dt * su, -X, float(W - 1) - X)
        ny, _ = _clamp_decided(br, dy + dt * sv, -Y, float(H - 1) - Y)
        return torch.stack([nx, ny], dim=-3)
    su = fluid_rule._sample(u, -1, (Y, X), br)               # the density advection's samples, clamps and floors, in its order
    sv = fluid_rule._sample(v, -2, (Y, X), br)
    mx, my = dt * su, dt * sv
    px, pass_x = _clamp_decided(br, X - mx, 0.0, float(W - 1))
    py, pass_y = _clamp_decided(br, Y - my, 0.0, float(H - 1))
    ix = torch.where(pass_x, -mx, px - X)
    iy = torch.where(pass_y, -my, py - Y)
    moved = fluid_rule._interpolate(disp, (py.unsqueeze(-3), px.unsqueeze(-3)), br)          # both components at one set of taps
    return moved + torch.stack([ix, iy], dim=-3)


def _differences(f, nd=2):
    """(d f / d x, d f / d y) -- with nd = 3 also d f / d z -- of f [..., H, W] at unit spacing: central with a factor 0.5 inside, one-sided
    on the first and last index of each axis."""
    out = []
    for dim in (-1, -2, -3)[:nd]:
        n = f.shape[dim]
        inner = 0.5 * (f.narrow(dim, 2, n - 2) - f.narrow(dim, 0, n - 2))
        first = f.narrow(dim, 1, 1) - f.narrow(dim, 0, 1)
        last = f.narrow(dim, n - 1, 1) - f.narrow(dim, n - 2, 1)
        out.append(torch.cat([first, inner, last], dim=dim))
    return out


def ftle_rule(disp, horizon: float):
    """The FTLE field [..., H, W] of the map x + disp over a window of `horizon` = n_steps * dt > 0 time units (module docstring), in
    disp's dtype."""
    if disp.dim() < 3 or disp.shape[-3] != 2 or min(disp.shape[-2:]) < 3:
        raise ValueError(f"ftle_rule: disp must be [..., 2, H, W] with H, W >= 3, got {tuple(disp.shape)}")
    if not float(horizon) > 0:
        raise ValueError(f"ftle_rule: horizon > 0, got {horizon}")
    ax, ay = _differences(disp[..., 0, :, :])
    bx, by = _differences(disp[..., 1, :, :])
    exx = ax + 0.5 * (ax * ax + bx * bx)
    eyy = by + 0.5 * (ay * ay + by * by)
    exy = 0.5 * (ay + bx) + 0.5 * (ax * ay + bx * by)
    m, d = 0.5 * (exx + eyy), 0.5 * (exx - eyy)
    emax = m + torch.sqrt(d * d + exy * exy)
    return torch.log1p(torch.clamp_min(2.0 * emax, LO)) / (2.0 * float(horizon))


@dataclass
class FtleResult:
    """ftle [B, H, W]: the field, per unit time.  displacement [B, 2, H, W]: the map's (dx, dy) in cells.  mean, max [B] fp64: of each
    grid's field.  state: (u, v, p, density) after the last step.  Un-batched states: everything without the B.  Of a volume's flow
    (flow_map3d.py): ftle [B, D, H, W], displacement [B, 3, D, H, W] = (dx, dy, dz), state (u, v, w, p, density)."""
    ftle: torch.Tensor
    displacement: torch.Tensor
    mean: torch.Tensor
    max: torch.Tensor
    state: Tuple[torch.Tensor, ...]


# ------------------------------------------------------------------------------------------------ what 2-D and 3-D share, over one record
@dataclass(frozen=True)
class MapRoute:
    """What the shared code needs to know about a dimension's flow map: the HipRoute record of its stepper, the public names as the error
    texts spell them, the two rules, the three entry points (map step, FTLE field, its workspace query) and the hip route's limits."""
    dim: HipRoute
    step_name: str
    field_name: str
    flow_name: str
    step_rule: Callable
    ftle_rule: Callable
    entries: Tuple[str, str, str]
    limits: str


def _check_window(n_steps, dt, what):
    if int(n_steps) < 1:
        raise ValueError(f"{what}: n_steps >= 1")
    if not float(dt) > 0:
        raise ValueError(f"{what}: dt > 0")


def _result(ftle, disp, mean, top, state, batched):
    if not batched:
        ftle, disp, mean, top, state = ftle[0], disp[0], mean[0], top[0], tuple(s[0] for s in state)
    return FtleResult(ftle, disp, mean, top, tuple(state))


def _stats64(ftle):
    """(mean, max) per grid of a field [B, ...] in fp64 by torch."""
    flat = ftle.double().flatten(1)
    return flat.mean(dim=1), flat.max(dim=1).values


def _check_hip(tensors, what):
    dev = tensors[0].device
    _lib.require_cuda(dev, f"{what}(route='hip')")
    for t in tensors:
        if t.dtype != torch.float32 or t.device != dev:
            raise ValueError(f"{what}(route='hip'): the operands must be float32 tensors on one device")


def _route(route, what):
    if route not in ("hip", "torch"):
        raise ValueError(f"{what}: route is 'hip' or 'torch', got {route!r}")
    return route == "hip"


def _launch_map_step(m, direction, vel, disp, out, dims, dt, dev):
    """The map-step entry point on device stores: vel = the velocity components, dims = (B, *grid, pitch_c, pitch_v, pitch_m)."""
    _lib.check(getattr(_lib.load(), m.entries[0])(direction, *[c.data_ptr() for c in vel], disp.data_ptr(), out.data_ptr(), *dims,
                                                  float(dt), _lib.stream_ptr(dev)))


def route_flow_ftle_rule(m, state, n_steps, dt, viscosity, jacobi_iters, direction, branches) -> FtleResult:
    """flow_ftle_rule / flow_ftle3d_rule: fluid_rule.step and the map step's rule chained from a zero displacement, then the FTLE's."""
    dim = m.dim
    _direction(direction, m.flow_name)
    _check_window(n_steps, dt, m.flow_name)
    check_state(dim, state)
    batched = state[-1].dim() == dim.nd + 1
    state = tuple(t.detach() if batched else t.detach()[None] for t in state)
    disp = state[-1].new_zeros(state[-1].shape[0], dim.nd, *state[-1].shape[1:])
    for _ in range(int(n_steps)):
        state = fluid_rule.step(state, dt, viscosity, jacobi_iters, branches)
        disp = m.step_rule(disp, *state[:dim.nd], dt=dt, direction=direction, branches=branches)
    ftle = m.ftle_rule(disp, int(n_steps) * float(dt))
    return _result(ftle, disp, *_stats64(ftle), state, batched)


def route_map_step(m, disp, vel, dt, direction, route):
    """flow_map_step / flow_map_step3d: the checks, then the rule or one launch on dense tensors."""
    dim = m.dim
    code = _direction(direction, m.step_name)
    if not _route(route, m.step_name):
        return m.step_rule(disp, *vel, dt=dt, direction=direction)
    grid = _check_disp(dim, disp, vel, m.step_name)
    _check_hip((disp, *vel), m.step_name)
    batched = disp.dim() == dim.nd + 2
    d, *vv = (t.detach().contiguous() if batched else t.detach()[None].contiguous() for t in (disp, *vel))
    out = torch.empty_like(d)
    W = grid[-1]
    with torch.cuda.device(d.device):
        _launch_map_step(m, code, vv, d, out, (d.shape[0], *grid, W, W + 1, W), dt, d.device)
    return out if batched else out[0]


def route_ftle_field(m, disp, horizon, route):
    """ftle_field / ftle_field3d: the checks, then the rule with torch's fp64 statistics or the entry point's two launches."""
    dim, what = m.dim, m.field_name
    nd = dim.nd
    if disp.dim() not in (nd + 1, nd + 2) or disp.shape[-nd - 1] != nd or min(disp.shape[-nd:]) < 3:
        raise ValueError(f"{what}: disp must be [{nd}, {dim.axes}] or [B, {nd}, {dim.axes}] with {dim.axes} >= 3, got {tuple(disp.shape)}")
    if not float(horizon) > 0:
        raise ValueError(f"{what}: horizon > 0, got {horizon}")
    batched = disp.dim() == nd + 2
    d = disp.detach() if batched else disp.detach()[None]
    if _route(route, what):
        _check_hip((d,), what)
        d = d.contiguous()
        B, grid = d.shape[0], tuple(d.shape[2:])
        L = _lib.load()
        nbytes = int(getattr(L, m.entries[2])(B, *grid))
        if nbytes < 0:
            raise ValueError(f"{what}: B={B}, grid {' x '.join(str(n) for n in grid)} is not supported ({m.limits})")
        ftle = torch.empty(B, *grid, dtype=torch.float32, device=d.device)
        stats = torch.empty(B, 2, dtype=torch.float64, device=d.device)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=d.device)
        with torch.cuda.device(d.device):
            _lib.check(getattr(L, m.entries[1])(d.data_ptr(), ftle.data_ptr(), stats.data_ptr(), B, *grid, grid[-1], float(horizon),
                                                ws.data_ptr(), nbytes, _lib.stream_ptr(d.device)))
        mean, top = stats[:, 0], stats[:, 1]
    else:
        ftle = m.ftle_rule(d, horizon)
        mean, top = _stats64(ftle)
    return (ftle, mean, top) if batched else (ftle[0], mean[0], top[0])


def route_flow_ftle(m, state, n_steps, dt, viscosity, jacobi_iters, direction, route) -> FtleResult:
    """flow_ftle / flow_ftle3d: the checks, then the rule or the chained loop on the cached stepper -- every step is step_into(None, 1)
    followed by the map step straight on the stepper's padded velocity stores, two displacement buffers swapping; then the FTLE's two
    launches; one host synchronisation, where the stepper reports its status."""
    dim, what = m.dim, m.flow_name
    code = _direction(direction, what)
    if not _route(route, what):
        return route_flow_ftle_rule(m, state, n_steps, dt, viscosity, jacobi_iters, direction, None)
    _check_window(n_steps, dt, what)
    check_state(dim, state)
    _check_hip(state, what)
    if int(jacobi_iters) < 0:
        raise ValueError(f"{what}: jacobi_iters >= 0")
    batched = state[-1].dim() == dim.nd + 1
    state = tuple(t.detach() if batched else t.detach()[None] for t in state)
    B, *grid = state[-1].shape
    dev = state[-1].device
    with torch.no_grad(), torch.cuda.device(dev):
        sim = simulator(dim, B, grid, dt, viscosity, jacobi_iters, dev)
        for name, t in zip(dim.fields, state):
            setattr(sim, name, t)
        vel = [getattr(sim, "_" + name) for name in dim.fields[:dim.nd]]
        dims = (B, *grid, sim._pc, sim._pv, grid[-1])
        disp, other = torch.zeros(B, dim.nd, *grid, device=dev), torch.empty(B, dim.nd, *grid, device=dev)
        for _ in range(int(n_steps)):
            sim.step_into(None, 1)
            _launch_map_step(m, code, vel, disp, other, dims, dt, dev)
            disp, other = other, disp
        ftle, mean, top = route_ftle_field(m, disp, int(n_steps) * float(dt), "hip")
        state = sim.state()
        check = getattr(sim, "check", None)                  # the frames leave the stepper: a timed-out projection is reported here
        if check is not None:                                # (by the stepper that can time out: the 3-D one has no check(), and then
            check()                                          # the call does not synchronise at all)
    return _result(ftle, disp, mean, top, state, batched)


# ------------------------------------------------------------------------------------------------ the public functions, 2-D
def flow_ftle_rule(u, v, p, density, n_steps: int, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                   direction: str = "backward", branches: Optional[Branches] = None) -> FtleResult:
    """n_steps of fluid_rule.step from the state (u, v, p, density), each followed by flow_map_step_rule with the step's output
    velocities, from a zero displacement; then ftle_rule over n_steps * dt.  Any dtype and device; mean and max in fp64 by torch."""
    return route_flow_ftle_rule(MAP2, (u, v, p, density), n_steps, dt, viscosity, jacobi_iters, direction, branches)


def flow_map_step(disp, u, v, *, dt: float = 0.01, direction: str = "backward", route: str = "hip"):
    """One map step -> disp' (module docstring).  disp [B, 2, H, W], u [B, H+1, W], v [B, H, W+1] (or all without the B): the velocities
    are the output of the step() the map is composed with.  route="hip": fp32 ROCm tensors, smk_flow_map_step (one launch);
    route="torch": flow_map_step_rule, any dtype and device."""
    return route_map_step(MAP2, disp, (u, v), dt, direction, route)


def ftle_field(disp, horizon: float, route: str = "hip"):
    """(ftle [B, H, W], mean [B] fp64, max [B] fp64) of the map x + disp, disp [B, 2, H, W] (or without the B), over a window of
    `horizon` = n_steps * dt > 0 time units.  route="hip": fp32 ROCm tensor, smk_ftle_field (two launches, no host synchronisation);
    route="torch": ftle_rule, the statistics in fp64 by torch."""
    return route_ftle_field(MAP2, disp, horizon, route)


def flow_ftle(u, v, p, density, n_steps: int, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
              direction: str = "backward", route: str = "hip") -> FtleResult:
    """The FTLE field of the flow over n_steps further steps from the state (u, v, p, density) -> FtleResult.  State in the reference's
    shapes u [B, H+1, W], v [B, H, W+1], p, density [B, H, W] (or without the B).  route="hip": fp32 ROCm tensors; the state is set into
    the cached stepper fluid_step uses, every step is step_into(None, 1) (bit-identical to step()) followed by smk_flow_map_step
    straight on the stepper's velocity stores, then smk_ftle_field; one host synchronisation, at the end, to check the stepper's status.
    route="torch": flow_ftle_rule, any dtype and device."""
    return route_flow_ftle(MAP2, (u, v, p, density), n_steps, dt, viscosity, jacobi_iters, direction, route)


MAP2 = MapRoute(HIP2, "flow_map_step", "ftle_field", "flow_ftle", flow_map_step_rule, ftle_rule,
                ("smk_flow_map_step", "smk_ftle_field", "smk_ftle_workspace"), "B <= 65535, 3 <= H, W <= 32766")
