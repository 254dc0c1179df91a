"""The flow map of the 3-D stepper and its finite-time Lyapunov exponent (FTLE) field, on libsmokehip (csrc/flow_map3d.hip).  DESIGN.md
section 3.15; the 3-D counterpart of flow_map.py (section 3.14), whose checks, result packing, single calls and chained loop it runs over
the record MAP3: this module holds the 3-D rule and binds the shared code to the 3-D argument lists.

A displacement disp [B, 3, D, H, W] = (dx, dy, dz) at the cell centres, in cells, stands for the map x -> x + disp; component k acts along
the axis velocity component k of the state (u, v, w, p, density) acts along (dx along W, dy along H, dz along D).  After every step() the
step's own first-order trace, with its output velocities, is composed into it, backward or forward, as in 2-D.

  flow_map_step3d_rule(disp, u, v, w, ...)     the rule of one map step in torch ops over fluid_rule's _sample / _interpolate / Branches.
  ftle3d_rule(disp, horizon)                   the FTLE field of a displacement volume.
  flow_ftle3d_rule(u, v, w, p, density, n)     fluid_rule.step and the map step chained: route="torch", and the tests' oracle.
  flow_map_step3d / ftle_field3d / flow_ftle3d the public functions; route="hip": smk_flow_map3d_step and smk_ftle3d_field.

The rule, one rounding per listed op.  Backward, at cell (Z, Y, X): su, sv, sw = the density advection's velocity samples; per axis
a = X - dt s, p = clamp(a, 0, n - 1), in the order px, py, pz; the increment -(dt s) where 0 <= a <= n - 1 (bounds included), p - X
otherwise (never p - X where the clamp passes: flow_map.py says why); disp' = interp(disp; pz, py, px) + increment, the three components at
one set of eight taps.  Forward: per axis q = clamp(X + d, 0, n - 1), sample positions only; s = the component sampled at (qz, qy, qx) by
the _sample rule; d' = min(max(d + dt s, -X), n - 1 - X).

FTLE: with g[k][j] the difference of component k along axis j (x, y, z) at unit spacing (central with a factor 0.5 inside, one-sided on
the first and last index of each axis), the Green-Lagrange strain formed so that the identity never enters --
  E_ii = g[i][i] + 0.5 ((g[x][i]^2 + g[y][i]^2) + g[z][i]^2),
  E_ij = 0.5 (g[i][j] + g[j][i]) + 0.5 ((g[x][i] g[x][j] + g[y][i] g[y][j]) + g[z][i] g[z][j]),
its largest eigenvalue emax by strain_emax3d, and ftle = log1p(max(2 emax, lo)) / (2 horizon), lo = -1 + 2^-24.

strain_emax3d is cyclic Jacobi with exactly 4 sweeps and no early exit, rotations in the order (x, y), (x, z), (y, z), each elementwise and
branch-free:  theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), sign(theta) = +1 for theta >= 0;  where
a_pq == 0 the divide is by 1 and t = 0 is selected;  c = 1 / sqrt(t^2 + 1), s = t c;  a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0;
a_rp' = c a_rp - s a_rq, a_rq' = s a_rp + c a_rq.  The result is the maximum of the three diagonal entries (a NaN wins).  Only adds,
multiplies, correctly rounded divides and square roots, and selects: the kernel is the rule operation for operation.  Against
torch.linalg.eigvalsh in fp64 it is within 2.5e-7 ||E||_F in fp32 and 2.0e-15 ||E||_F in fp64 (3 sweeps: 4.7e-10 in fp64); the
trigonometric closed form loses 2.2e-4 ||E||_F in fp32 where two eigenvalues coincide, and is not used.

Out of scope: a dataset label built from the statistics, derivatives of the map, higher-order particle integration."""
from typing import Optional

import torch

from . import fluid_rule
from .flow_map import (LO, FtleResult, MapRoute, _check_disp, _clamp_decided, _differences, _direction, route_flow_ftle, route_flow_ftle_rule,
                       route_ftle_field, route_map_step)
from .fluid_grad3d import HIP3
from .fluid_rule import Branches

__all__ = ["flow_ftle3d", "flow_ftle3d_rule", "flow_map_step3d", "flow_map_step3d_rule", "ftle3d_rule", "ftle_field3d", "strain_emax3d"]

SWEEPS = 4
ACTS = (-1, -2, -3)                                          # the axis component k of the displacement, and of the velocity, acts along


# ------------------------------------------------------------------------------------------------ the rule in torch ops
def flow_map_step3d_rule(disp, u, v, w, *, dt: float = 0.01, direction: str = "backward", branches: Optional[Branches] = None):
    """One map step in torch ops (module docstring): disp [..., 3, D, H, W], u [..., D, H+1, W], v [..., D, H, W+1], w [..., D+1, H, W] of
    any floating dtype on any device -> disp'.  branches: a Branches recorder (filled) or replayer (followed); None: decisions are made
    and not kept."""
    forward = _direction(direction, "flow_map_step3d_rule")
    grid = _check_disp(HIP3, disp, (u, v, w), "flow_map_step3d_rule")
    br = Branches() if branches is None else branches
    index = torch.meshgrid(*[torch.arange(n, dtype=disp.dtype, device=disp.device) for n in grid], indexing="ij")     # (Z, Y, X)
    at = [index[a] for a in ACTS]                            # X, Y, Z: the index along the axis component k acts on
    top = [float(grid[a] - 1) for a in ACTS]
    d = [disp[..., k, :, :, :] for k in range(3)]
    if forward:
        q = [br.clamp(at[k] + d[k], 0.0, top[k]) for k in range(3)]
        where = (q[2], q[1], q[0])
        s = [fluid_rule._sample(c, ACTS[k], where, br) for k, c in enumerate((u, v, w))]
        return torch.stack([_clamp_decided(br, d[k] + dt * s[k], -at[k], top[k] - at[k])[0] for k in range(3)], dim=-4)
    s = [fluid_rule._sample(c, ACTS[k], index, br) for k, c in enumerate((u, v, w))]     # the density advection's samples, in its order
    m = [dt * x for x in s]
    p, inc = [], []
    for k in range(3):                                       # px, py, pz, as fluid_rule.advect clamps
        pk, passed = _clamp_decided(br, at[k] - m[k], 0.0, top[k])
        p.append(pk)
        inc.append(torch.where(passed, -m[k], pk - at[k]))
    moved = fluid_rule._interpolate(disp, tuple(p[k].unsqueeze(-4) for k in (2, 1, 0)), br)     # the three components at one set of taps
    return moved + torch.stack(inc, dim=-4)


def _rotate(a, p, q, r):
    """One Jacobi rotation of the symmetric 3 x 3 matrices a (a dict of the six entries keyed by sorted index pairs) that annihilates
    a[p, q]; r is the third index."""
    key = lambda i, j: (i, j) if i <= j else (j, i)          # noqa: E731
    app, aqq, apq, arp, arq = a[p, p], a[q, q], a[key(p, q)], a[key(r, p)], a[key(r, q)]
    one = torch.ones_like(apq)
    flat = apq == 0
    theta = (aqq - app) / torch.where(flat, one, 2.0 * apq)
    t = torch.where(theta >= 0, one, -one) / (theta.abs() + torch.sqrt(theta * theta + 1.0))
    t = torch.where(flat, torch.zeros_like(t), t)
    c = 1.0 / torch.sqrt(t * t + 1.0)
    s = t * c
    a[p, p], a[q, q], a[key(p, q)] = app - t * apq, aqq + t * apq, torch.zeros_like(apq)
    a[key(r, p)], a[key(r, q)] = c * arp - s * arq, s * arp + c * arq


def strain_emax3d(exx, eyy, ezz, exy, exz, eyz):
    """The largest eigenvalue of the symmetric matrices [[exx, exy, exz], [exy, eyy, eyz], [exz, eyz, ezz]], elementwise over tensors of
    one shape and dtype: cyclic Jacobi, 4 sweeps (module docstring).  The zero matrix gives exactly 0; a NaN entry gives NaN."""
    a = {(0, 0): exx, (1, 1): eyy, (2, 2): ezz, (0, 1): exy, (0, 2): exz, (1, 2): eyz}
    for _ in range(SWEEPS):
        _rotate(a, 0, 1, 2)
        _rotate(a, 0, 2, 1)
        _rotate(a, 1, 2, 0)
    return torch.maximum(torch.maximum(a[0, 0], a[1, 1]), a[2, 2])


def ftle3d_rule(disp, horizon: float):
    """The FTLE field [..., D, H, W] of the map x + disp over a window of `horizon` = n_steps * dt > 0 time units (module docstring), in
    disp's dtype."""
    if disp.dim() < 4 or disp.shape[-4] != 3 or min(disp.shape[-3:]) < 3:
        raise ValueError(f"ftle3d_rule: disp must be [..., 3, D, H, W] with D, H, W >= 3, got {tuple(disp.shape)}")
    if not float(horizon) > 0:
        raise ValueError(f"ftle3d_rule: horizon > 0, got {horizon}")
    g = [_differences(disp[..., k, :, :, :], 3) for k in range(3)]          # g[k][j] = d disp_k / d axis_j, axes x, y, z

    def dots(i, j):
        return (g[0][i] * g[0][j] + g[1][i] * g[1][j]) + g[2][i] * g[2][j]
    diag = [g[i][i] + 0.5 * dots(i, i) for i in range(3)]
    off = {(i, j): 0.5 * (g[i][j] + g[j][i]) + 0.5 * dots(i, j) for i, j in ((0, 1), (0, 2), (1, 2))}
    emax = strain_emax3d(diag[0], diag[1], diag[2], off[0, 1], off[0, 2], off[1, 2])
    return torch.log1p(torch.clamp_min(2.0 * emax, LO)) / (2.0 * float(horizon))


def flow_ftle3d_rule(u, v, w, p, density, n_steps: int, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                     direction: str = "backward", branches: Optional[Branches] = None) -> FtleResult:
    """n_steps of fluid_rule.step from the state (u, v, w, p, density), each followed by flow_map_step3d_rule with the step's output
    velocities, from a zero displacement; then ftle3d_rule over n_steps * dt.  Any dtype and device; mean and max in fp64 by torch."""
    return route_flow_ftle_rule(MAP3, (u, v, w, p, density), n_steps, dt, viscosity, jacobi_iters, direction, branches)


MAP3 = MapRoute(HIP3, "flow_map_step3d", "ftle_field3d", "flow_ftle3d", flow_map_step3d_rule, ftle3d_rule,
                ("smk_flow_map3d_step", "smk_ftle3d_field", "smk_ftle3d_workspace"), "B * (D + 1) <= 65535, 3 <= D, H, W <= 32766")


# ------------------------------------------------------------------------------------------------ the public functions
def flow_map_step3d(disp, u, v, w, *, dt: float = 0.01, direction: str = "backward", route: str = "hip"):
    """One map step -> disp' (module docstring).  disp [B, 3, D, H, W], u [B, D, H+1, W], v [B, D, H, W+1], w [B, D+1, H, W] (or all
    without the B): the velocities are the output of the step() the map is composed with.  route="hip": fp32 ROCm tensors,
    smk_flow_map3d_step (one launch); route="torch": flow_map_step3d_rule, any dtype and device."""
    return route_map_step(MAP3, disp, (u, v, w), dt, direction, route)


def ftle_field3d(disp, horizon: float, route: str = "hip"):
    """(ftle [B, D, H, W], mean [B] fp64, max [B] fp64) of the map x + disp, disp [B, 3, D, H, W] (or without the B), over a window of
    `horizon` = n_steps * dt > 0 time units.  route="hip": fp32 ROCm tensor, smk_ftle3d_field (two launches, no host synchronisation);
    route="torch": ftle3d_rule, the statistics in fp64 by torch."""
    return route_ftle_field(MAP3, disp, horizon, route)


def flow_ftle3d(u, v, w, p, density, n_steps: int, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                direction: str = "backward", route: str = "hip") -> FtleResult:
    """The FTLE field of a volume's flow over n_steps further steps from the state (u, v, w, p, density) -> FtleResult.  State in SPEC_3D.md
    section 1's shapes u [B, D, H+1, W], v [B, D, H, W+1], w [B, D+1, H, W], p, density [B, D, H, W] (or without the B).  route="hip":
    fp32 ROCm tensors; the state is set into the cached stepper fluid_step3d uses, every step is step_into(None, 1) (bit-identical to
    step()) followed by smk_flow_map3d_step straight on the stepper's velocity stores, then smk_ftle3d_field.  route="torch":
    flow_ftle3d_rule, any dtype and device."""
    return route_flow_ftle(MAP3, (u, v, w, p, density), n_steps, dt, viscosity, jacobi_iters, direction, route)
