"""The differentiable fluid step in torch ops, written once for a 2-D or a 3-D grid: the rule behind physics/fluid_grad.py (DESIGN.md section
3.9), fluid_grad3d.py (3.10) and fluid_tangent.py (3.11), whose *_rule functions bind it to their argument lists.  It is driven by the
per-dimension table oracle/ns_nd.py uses, and in fp32 on the CPU it is that oracle's step bit for bit (tests/test_fluid_rule_host.py).

A state is (velocity components ..., p, density), every tensor with any leading dimensions; axes are counted from the end (-1: x, -2: y,
-3: z).  Operation order is the reference's (navier_stokes.py; SPEC_3D.md sections 3-6), one rounding per listed op: neighbour sums left to
right in NEIGHBOURS' order, interpolation weights (x-factor * y-factor) * z-factor, taps first axis slowest, x fastest, low before high."""
import numpy as np
import torch

SIXTH = float(np.float32(1.0 / 6.0))       # SPEC_3D.md section 4: the fp32 value nearest to the double 1/6, in every dtype

# Velocity components in state order as (staggered axis, axis it acts along): u (y, x), v (x, y), w (z, z).
COMPONENTS = {2: ((-2, -1), (-1, -2)), 3: ((-2, -1), (-1, -2), (-3, -3))}
NEIGHBOURS = {2: (-2, -1), 3: (-2, -1, -3)}          # Laplacian / Jacobi sums: up, down, left, right, then front, back
JACOBI_SCALE = {2: 0.25, 3: SIXTH}
BUOYANT = 1                                          # buoyancy goes into v (navier_stokes.py:154-155)


class Branches:
    """Recorder / replayer of every integer decision of the step rule: each floor (the int64 index) and each coordinate clamp (which
    elements lay below lo, which above hi), in call order.  Record with Branches(), hand replayer() to a second run -- in another dtype,
    say -- and that run takes the recorded decisions instead of making its own: the fp64 rule along the fp32 run's branches."""

    def __init__(self, log=None):
        self.log, self.replay, self.pos = ([] if log is None else log), log is not None, 0

    def replayer(self):
        return Branches(self.log)

    def _next(self, make):
        if self.replay:
            item = self.log[self.pos]
            self.pos += 1
            return item
        item = make()
        self.log.append(item)
        return item

    def floor(self, x):
        return self._next(lambda: torch.floor(x.detach()).to(torch.int64))

    def clamp(self, x, lo, hi):
        lt, gt = self._next(lambda: (x.detach() < lo, x.detach() > hi))
        return torch.where(lt, x.new_tensor(lo), torch.where(gt, x.new_tensor(hi), x))


class _NoBranches:
    """The rule without a recorder: the same two operations, nothing kept."""

    @staticmethod
    def floor(x):
        return torch.floor(x.detach()).to(torch.int64)

    @staticmethod
    def clamp(x, lo, hi):
        return torch.clamp(x, lo, hi)           # (its backward passes the gradient where lo <= x <= hi, as Branches.clamp does)


def _shift(f, dim, lo):
    """The replicate-padded neighbour along dim: lo=True f[i-1] (f[0] at i = 0), lo=False f[i+1] (f[n-1] at i = n-1)."""
    n = f.shape[dim]
    if lo:
        return torch.cat([f.narrow(dim, 0, 1), f.narrow(dim, 0, n - 1)], dim=dim)
    return torch.cat([f.narrow(dim, 1, n - 1), f.narrow(dim, n - 1, 1)], dim=dim)


def _inner(f, nd, axis=None, start=1):
    """f without its boundary shell on the last nd axes; along `axis` the window starts at `start` (0: low neighbour, 2: high)."""
    for a in range(-nd, 0):
        f = f.narrow(a, start if a == axis else 1, f.shape[a] - 2)
    return f


def _diffuse(f, coef, nd):
    """diffusion_step (navier_stokes.py:50-72; SPEC_3D.md section 3): replicate padding, the neighbours summed left to right, - 2 nd f,
    f + (dt * viscosity) * lap."""
    lap = None
    for a in NEIGHBOURS[nd]:
        lap = _shift(f, a, True) if lap is None else lap + _shift(f, a, True)
        lap = lap + _shift(f, a, False)
    lap = lap - (2.0 * nd) * f
    return f + coef * lap


def _interpolate(f, coords, br):
    """bilinear_interpolate (navier_stokes.py:111-131; SPEC_3D.md section 5) at coords (first axis first): floor, clamp the INDICES, weights
    from the clamped indices.  The floors are recorded in the order x, y, (z)."""
    nd = len(coords)
    idx, wgt = [None] * nd, [None] * nd
    for a in reversed(range(nd)):
        c, n = coords[a], f.shape[a - nd]
        i0 = br.floor(c)
        i0, i1 = i0.clamp(0, n - 1), (i0 + 1).clamp(0, n - 1)
        idx[a], wgt[a] = (i0, i1), (i1.to(f.dtype) - c, c - i0.to(f.dtype))
    r = None
    for tap in range(1 << nd):
        bits = [(tap >> (nd - 1 - a)) & 1 for a in range(nd)]
        at, w = None, None
        for a in range(nd):                                  # the flat index, first axis slowest
            at = idx[a][bits[a]] if at is None else at * f.shape[a - nd] + idx[a][bits[a]]
        for a in reversed(range(nd)):
            w = wgt[a][bits[a]] if w is None else w * wgt[a][bits[a]]
        at = at.expand(f.shape[:-nd] + at.shape[-nd:])
        term = w * f.flatten(-nd).gather(-1, at.flatten(-nd)).view(at.shape)
        r = term if r is None else r + term
    return r


def _sample(c, act, grid, br):
    """interpolate_velocity_u / _v (navier_stokes.py:97-109): a component sampled at the index grid shifted +0.5 along the axis it acts on;
    every coordinate is clamped to the component's extent, slowest axis first (SPEC_3D.md section 5)."""
    nd = len(grid)
    coords = [br.clamp(g + 0.5 if a - nd == act else g, 0.0, float(c.shape[a - nd] - 1)) for a, g in enumerate(grid)]
    return _interpolate(c, coords, br)


def advect(field, vel, dt, branches=None):
    """advection_step(field; vel) (navier_stokes.py:74-95; SPEC_3D.md section 5); no decay.  The back-trace clamps go px, py, (pz)."""
    br = _NoBranches if branches is None else branches
    nd = len(vel)
    shape = field.shape[-nd:]
    grid = torch.meshgrid(*[torch.arange(n, dtype=field.dtype, device=field.device) for n in shape], indexing="ij")
    samples = [_sample(c, act, grid, br) for c, (_, act) in zip(vel, COMPONENTS[nd])]
    prev = list(grid)
    for s, (_, act) in zip(samples, COMPONENTS[nd]):
        prev[act] = br.clamp(grid[act] - dt * s, 0.0, float(shape[act] - 1))
    return _interpolate(field, prev, br)


def buoy_diffuse(vel, density, dt, viscosity):
    """Buoyancy into v[..., :-1] (navier_stokes.py:154-155), then diffusion_step of every component and the density -> (vel, density)."""
    nd = len(vel)
    vel, v = list(vel), vel[BUOYANT]
    n = v.shape[-1] - 1
    vel[BUOYANT] = torch.cat([v.narrow(-1, 0, n) + dt * (density * 0.1), v.narrow(-1, n, 1)], dim=-1)
    return [_diffuse(c, dt * viscosity, nd) for c in vel], _diffuse(density, dt * (viscosity * 0.1), nd)


def project(vel, p, dt, jacobi_iters):
    """pressure_projection (navier_stokes.py:133-149; SPEC_3D.md section 4): the divergence ((u_hi - u_lo) + v_hi) - v_lo (+ w_hi) - w_lo
    with a true divide by dt, jacobi_iters sweeps from the carried-over p with the boundary shell forced to 0, the gradient subtraction on
    the inner faces of every component -> (vel, p)."""
    nd = len(vel)
    div = None
    for c, (stag, _) in zip(vel, COMPONENTS[nd]):
        n = c.shape[stag] - 1
        div = c.narrow(stag, 1, n) - c.narrow(stag, 0, n) if div is None else (div + c.narrow(stag, 1, n)) - c.narrow(stag, 0, n)
    div = div / dt
    for _ in range(jacobi_iters):
        s = None
        for a in NEIGHBOURS[nd]:
            s = _inner(p, nd, a, 0) if s is None else s + _inner(p, nd, a, 0)
            s = s + _inner(p, nd, a, 2)
        p = torch.nn.functional.pad(JACOBI_SCALE[nd] * (s - _inner(div, nd)), (1, 1) * nd)
    out = []
    for c, (stag, _) in zip(vel, COMPONENTS[nd]):
        n = p.shape[stag] - 1
        grad = p.narrow(stag, 1, n) - p.narrow(stag, 0, n)
        out.append(torch.cat([c.narrow(stag, 0, 1), c.narrow(stag, 1, n) - dt * grad, c.narrow(stag, n + 1, 1)], dim=stag))
    return out, p


def step(state, dt, viscosity, jacobi_iters, branches=None):
    """One step() stage by stage as the reference orders them: buoy_diffuse, project, the sequentially dependent advections (each component
    with the components advected before it, then the density with all of them), and the 0.995 decay.  state: (components ..., p, density)."""
    *vel, p, density = state
    vel, density = buoy_diffuse(vel, density, dt, viscosity)
    vel, p = project(vel, p, dt, jacobi_iters)
    for k in range(len(vel)):
        vel[k] = advect(vel[k], vel, dt, branches)
    density = advect(density, vel, dt, branches) * 0.995
    return (*vel, p, density)
