"""Differentiable 2-D fluid step: one NavierStokesSimulator.step() (navier_stokes.py:151-173) as a function of its whole state
(u, v, p, density), with its derivative on libsmokehip (csrc/fluid_grad.hip) behind torch autograd.  DESIGN.md section 3.9.

  fluid_step(u, v, p, density, ...)      one step; route="hip": the stepper's own stage kernels forward (bit-identical to step()), the
                                         adjoint kernels smk_advect_backward / smk_project_backward / smk_buoy_diffuse_backward backward;
                                         route="torch": fluid_step_rule under torch autograd.
  fluid_rollout(u, v, p, density, n)     n chained steps -> (state, frames [B, n, H, W]).
  fluid_step_rule(u, v, p, density, ...) the executable rule in torch ops (any dtype and device, differentiable): the tests' oracle.
  FluidRollout(steps=k, ...)             the settings object PerturbationTester.adversarial_test(simulate=...) takes.

Derivative conventions: that of the expressions as written -- floor and integer casts have derivative 0, a clamp of a coordinate passes
its gradient where lo <= x <= hi (bounds included: in still regions X - dt * 0 sits exactly on the bound), the interpolation weights are
formed from the clamped indices as in the forward; dt, viscosity and jacobi_iters are constants.

Limit of the hip route: its advection backward gathers over the 3 x 3 destinations around a source cell, which holds while every
back-trace of the three advections moves less than one cell (with dt = 0.01 that is a velocity below 100 cells per unit time).  A grid
that breaks this gets NaN in all four of its gradients (no host synchronisation; the other grids of the batch are untouched);
route="torch" has no such limit, and the forward is unaffected either way.

Memory: a step whose input requires a gradient saves five fields per grid (u, v after the projection, the diffused density, u and v after
their advections; the last two are the step's own outputs): 5 * 4 * H * W bytes per grid and step -- 84 MB per step at 64 x 256^2.  Without
a gradient request nothing is saved."""
from dataclasses import dataclass
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from .. import _lib

__all__ = ["Branches", "FluidRollout", "advect_rule", "buoy_diffuse_rule", "fluid_rollout", "fluid_step", "fluid_step_rule", "project_rule"]


# ------------------------------------------------------------------------------------------------ the rule in torch ops
class Branches:
    """Recorder / replayer of every integer decision of fluid_step_rule: each floor (the int64 index) and each coordinate clamp (which
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
    """fluid_step_rule without a recorder: the same two operations, nothing kept."""

    @staticmethod
    def floor(x):
        return torch.floor(x.detach()).to(torch.int64)

    @staticmethod
    def clamp(x, lo, hi):
        return torch.clamp(x, lo, hi)           # (its backward passes the gradient where lo <= x <= hi, as Branches.clamp does)


def _diffuse(f, coef):
    """diffusion_step (navier_stokes.py:50-72): replicate padding, ((((up + down) + left) + right) - 4 f), f + (dt * viscosity) * lap."""
    up = torch.cat([f[..., :1, :], f[..., :-1, :]], dim=-2)
    down = torch.cat([f[..., 1:, :], f[..., -1:, :]], dim=-2)
    left = torch.cat([f[..., :, :1], f[..., :, :-1]], dim=-1)
    right = torch.cat([f[..., :, 1:], f[..., :, -1:]], dim=-1)
    lap = up + down
    lap = lap + left
    lap = lap + right
    lap = lap - 4.0 * f
    return f + coef * lap


def _take(f, yi, xi):
    """f[..., yi, xi] for index tensors that broadcast to [..., R, C]."""
    idx = yi * f.shape[-1] + xi
    idx = idx.expand(f.shape[:-2] + idx.shape[-2:])
    return f.flatten(-2).gather(-1, idx.flatten(-2)).view(idx.shape)


def _interpolate(f, y, x, br):
    """bilinear_interpolate (navier_stokes.py:111-131): floor, clamp the INDICES, weights from the clamped indices."""
    h, w = f.shape[-2:]
    x0, y0 = br.floor(x), br.floor(y)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = x0.clamp(0, w - 1), x1.clamp(0, w - 1)
    y0, y1 = y0.clamp(0, h - 1), y1.clamp(0, h - 1)
    fx0, fx1, fy0, fy1 = (t.to(f.dtype) for t in (x0, x1, y0, y1))
    wa = (fx1 - x) * (fy1 - y)
    wb = (x - fx0) * (fy1 - y)
    wc = (fx1 - x) * (y - fy0)
    wd = (x - fx0) * (y - fy0)
    r = wa * _take(f, y0, x0) + wb * _take(f, y0, x1)
    r = r + wc * _take(f, y1, x0)
    r = r + wd * _take(f, y1, x1)
    return r


def advect_rule(field, u, v, *, dt: float = 0.01, branches: Optional[Branches] = None):
    """advection_step(field; u, v) (navier_stokes.py:74-95) with interpolate_velocity_u / _v (:97-109); no decay."""
    br = _NoBranches if branches is None else branches
    f = field
    R, Cc = f.shape[-2:]
    Y, X = torch.meshgrid(torch.arange(R, dtype=f.dtype, device=f.device), torch.arange(Cc, dtype=f.dtype, device=f.device), indexing="ij")
    ui = _interpolate(u, br.clamp(Y, 0.0, float(u.shape[-2] - 1)), br.clamp(X + 0.5, 0.0, float(u.shape[-1] - 1)), br)
    vi = _interpolate(v, br.clamp(Y + 0.5, 0.0, float(v.shape[-2] - 1)), br.clamp(X, 0.0, float(v.shape[-1] - 1)), br)
    px = br.clamp(X - dt * ui, 0.0, float(Cc - 1))
    py = br.clamp(Y - dt * vi, 0.0, float(R - 1))
    return _interpolate(f, py, px, br)


def buoy_diffuse_rule(u, v, density, *, dt: float = 0.01, viscosity: float = 0.001):
    """Buoyancy into v[:, :-1] (navier_stokes.py:154-155), then diffusion_step of u, v and density (:158-160) -> (u, v, density)."""
    b = density * 0.1
    v = torch.cat([v[..., :, :-1] + dt * b, v[..., :, -1:]], dim=-1)
    return _diffuse(u, dt * viscosity), _diffuse(v, dt * viscosity), _diffuse(density, dt * (viscosity * 0.1))


def project_rule(u, v, p, *, dt: float = 0.01, jacobi_iters: int = 20):
    """pressure_projection (navier_stokes.py:133-149): divergence with a true divide by dt, jacobi_iters sweeps from the carried-over p
    with the ring forced to 0, the gradient subtraction on u[1:-1] and v[:, 1:-1] -> (u, v, p)."""
    div = u[..., 1:, :] - u[..., :-1, :]
    div = div + v[..., :, 1:]
    div = div - v[..., :, :-1]
    div = div / dt
    for _ in range(jacobi_iters):
        s = p[..., :-2, 1:-1] + p[..., 2:, 1:-1]
        s = s + p[..., 1:-1, :-2]
        s = s + p[..., 1:-1, 2:]
        p = torch.nn.functional.pad(0.25 * (s - div[..., 1:-1, 1:-1]), (1, 1, 1, 1))
    u = torch.cat([u[..., :1, :], u[..., 1:-1, :] - dt * (p[..., 1:, :] - p[..., :-1, :]), u[..., -1:, :]], dim=-2)
    v = torch.cat([v[..., :, :1], v[..., :, 1:-1] - dt * (p[..., :, 1:] - p[..., :, :-1]), v[..., :, -1:]], dim=-1)
    return u, v, p


def fluid_step_rule(u, v, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                    branches: Optional[Branches] = None):
    """One step() in torch ops, stage by stage as the reference orders them: buoy_diffuse_rule, project_rule, the three sequentially
    dependent advections u <- adv(u; u, v), v <- adv(v; u_new, v), density <- adv(density; u_new, v_new), and the 0.995 decay -- one
    rounding per reference op, so in fp32 on the CPU it is the reference's step bit for bit.  State [..., H+1, W], [..., H, W+1],
    [..., H, W], [..., H, W] of any floating dtype on any device; differentiable.
    branches: a Branches recorder (filled) or replayer (followed); None: decisions are made and not kept."""
    u, v, density = buoy_diffuse_rule(u, v, density, dt=dt, viscosity=viscosity)
    u, v, p = project_rule(u, v, p, dt=dt, jacobi_iters=jacobi_iters)
    u = advect_rule(u, u, v, dt=dt, branches=branches)
    v = advect_rule(v, u, v, dt=dt, branches=branches)
    density = advect_rule(density, u, v, dt=dt, branches=branches)
    density = density * 0.995
    return u, v, p, density


# ------------------------------------------------------------------------------------------------ the hip route
_SIMS = {}


def _simulator(B, H, W, dt, viscosity, jacobi_iters, dev):
    """The cached stepper whose stage kernels run the forward: one per (B, H, W, dt, viscosity, jacobi_iters, device)."""
    from .navier_stokes import NavierStokesSimulator
    key = (B, H, W, float(dt), float(viscosity), int(jacobi_iters), dev.index)
    sim = _SIMS.get(key)
    if sim is None:
        sim = _SIMS[key] = NavierStokesSimulator((H, W), dt=dt, viscosity=viscosity, device=dev, batch_size=B, jacobi_iters=jacobi_iters)
    return sim


def _nan_where_far(far, *grads):
    bad = (far != 0)[:, None, None]
    return tuple(torch.where(bad, g.new_tensor(float("nan")), g) for g in grads)


class _FluidStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, p, density, dt, viscosity, jacobi_iters):
        B, H, W = density.shape
        dev = density.device
        sim = _simulator(B, H, W, dt, viscosity, jacobi_iters, dev)
        with torch.cuda.device(dev):
            sim.u, sim.v, sim.p, sim.density = u, v, p, density
            keep = any(ctx.needs_input_grad[:4])
            if keep:                                     # stage by stage (bit-identical to step()), keeping what the backward needs
                sim.run_stage(_lib.STAGE_BUOY_DIFFUSE)
                sim.run_stage(_lib.STAGE_PROJECT)        # (a timed-out persistent projection is reported as step() reports it)
                u_p, v_p, d_d = sim.u.clone(), sim.v.clone(), sim.density.clone()
                sim.run_stage(_lib.STAGE_ADVECT_U)
                sim.run_stage(_lib.STAGE_ADVECT_V)
                sim.run_stage(_lib.STAGE_ADVECT_D)
            else:
                sim.step_into(None, 1)
            u_a, v_a, p_n, d_n = sim.state()
        if keep:
            ctx.save_for_backward(u_p, v_p, d_d, u_a, v_a)
        ctx.settings = (float(dt), float(viscosity), int(jacobi_iters))
        return u_a, v_a, p_n, d_n

    @staticmethod
    @once_differentiable
    def backward(ctx, gu, gv, gp, gd):
        u_p, v_p, d_d, u_a, v_a = ctx.saved_tensors
        dt, viscosity, jacobi_iters = ctx.settings
        B, H, W = d_d.shape
        dev = d_d.device
        L = _lib.load()
        gu, gv, gp, gd = (g.contiguous() for g in (gu, gv, gp, gd))
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            far = torch.empty(3, B, dtype=torch.int32, device=dev)

            def advect_backward(stage, which, field, uu, vv, gout):
                df, du, dv = torch.empty_like(field), torch.empty_like(uu), torch.empty_like(vv)
                _lib.check(L.smk_advect_backward(which, field.data_ptr(), uu.data_ptr(), vv.data_ptr(), gout.data_ptr(), df.data_ptr(),
                                                 du.data_ptr(), dv.data_ptr(), far[stage].data_ptr(), B, H, W, W, W + 1, dt, st))
                return df, du, dv
            # reverse stage order: density <- adv(d_d; u_a, v_a) * 0.995, v_a <- adv(v_p; u_a, v_p), u_a <- adv(u_p; u_p, v_p)
            g_dd, du, dv = advect_backward(0, 2, d_d, u_a, v_a, gd)
            g_ua, g_va = gu + du, gv + dv
            df, du, dv = advect_backward(1, 1, v_p, u_a, v_p, g_va)
            g_ua, g_vp = g_ua + du, df + dv
            df, du, dv = advect_backward(2, 0, u_p, u_p, v_p, g_ua)
            g_up, g_vp = df + du, g_vp + dv
            # projection, then diffusion + buoyancy
            nbytes = int(L.smk_project_backward_workspace(B, H, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            du, dv, dp = torch.empty_like(g_up), torch.empty_like(g_vp), torch.empty_like(gp)
            _lib.check(L.smk_project_backward(g_up.data_ptr(), g_vp.data_ptr(), gp.data_ptr(), du.data_ptr(), dv.data_ptr(), dp.data_ptr(),
                                              B, H, W, W, W + 1, jacobi_iters, dt, ws.data_ptr(), nbytes, st))
            ou, ov, od = torch.empty_like(du), torch.empty_like(dv), torch.empty_like(g_dd)
            _lib.check(L.smk_buoy_diffuse_backward(du.data_ptr(), dv.data_ptr(), g_dd.data_ptr(), ou.data_ptr(), ov.data_ptr(),
                                                   od.data_ptr(), B, H, W, W, W + 1, dt, viscosity, st))
            ou, ov, dp, od = _nan_where_far(far.amax(dim=0), ou, ov, dp, od)
        return ou, ov, dp, od, None, None, None


def _check_state(u, v, p, density):
    if density.dim() not in (2, 3):
        raise ValueError(f"fluid_step: density must be [H, W] or [B, H, W], got {tuple(density.shape)}")
    lead, (H, W) = tuple(density.shape[:-2]), density.shape[-2:]
    want = {"u": lead + (H + 1, W), "v": lead + (H, W + 1), "p": lead + (H, W)}
    for name, t in (("u", u), ("v", v), ("p", p)):
        if tuple(t.shape) != want[name]:
            raise ValueError(f"fluid_step: {name} must be {want[name]} beside density {tuple(density.shape)}, got {tuple(t.shape)}")
    if H < 3 or W < 3:
        raise ValueError("fluid_step: H, W >= 3")


def fluid_step(u, v, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip"):
    """One NavierStokesSimulator.step() as a differentiable function of the state -> (u, v, p, density).  State in the reference's shapes
    u [B, H+1, W], v [B, H, W+1], p, density [B, H, W] (or without the B).  route="hip": fp32 ROCm tensors; the forward runs the stepper's
    stage kernels and is bit-identical to step() on the same state, the backward runs the adjoint kernels (module docstring: far grids
    come back NaN).  route="torch": fluid_step_rule under torch autograd, any dtype and device."""
    _check_state(u, v, p, density)
    if route == "torch":
        return fluid_step_rule(u, v, p, density, dt=dt, viscosity=viscosity, jacobi_iters=jacobi_iters)
    if route != "hip":
        raise ValueError(f"fluid_step: route is 'hip' or 'torch', got {route!r}")
    _lib.require_cuda(density.device, "fluid_step(route='hip')")
    for name, t in (("u", u), ("v", v), ("p", p), ("density", density)):
        if t.dtype != torch.float32 or t.device != density.device:
            raise ValueError(f"fluid_step(route='hip'): {name} must be a float32 tensor on the density's device")
    if int(jacobi_iters) < 0:
        raise ValueError("fluid_step: jacobi_iters >= 0")
    batched = density.dim() == 3
    state = (u, v, p, density) if batched else tuple(t[None] for t in (u, v, p, density))
    out = _FluidStepFn.apply(*state, dt, viscosity, jacobi_iters)
    return out if batched else tuple(t[0] for t in out)


def fluid_rollout(u, v, p, density, n_steps: int, **settings):
    """n_steps chained fluid_step calls -> ((u, v, p, density) after the last, frames [B, n_steps, H, W] of the densities; [n_steps, H, W]
    for an un-batched state).  settings: fluid_step's keywords.  With a gradient request every step saves its five fields (module
    docstring: 84 MB per step at 64 x 256^2), so memory grows linearly with n_steps."""
    if n_steps < 1:
        raise ValueError("fluid_rollout: n_steps >= 1")
    state, frames = (u, v, p, density), []
    for _ in range(n_steps):
        state = fluid_step(*state, **settings)
        frames.append(state[3])
    return state, torch.stack(frames, dim=-3)


@dataclass(frozen=True)
class FluidRollout:
    """PerturbationTester.adversarial_test(simulate=FluidRollout(steps=k, ...)): initial densities at rest (u = v = p = 0) -> the density
    after `steps` steps, differentiably."""
    steps: int = 4
    dt: float = 0.01
    viscosity: float = 0.001
    jacobi_iters: int = 20
    route: str = "hip"

    def __call__(self, density):
        """density [B, H, W] -> density after `steps` steps from rest."""
        B, H, W = density.shape
        u, v, p = density.new_zeros(B, H + 1, W), density.new_zeros(B, H, W + 1), density.new_zeros(B, H, W)
        state, _ = fluid_rollout(u, v, p, density, self.steps, dt=self.dt, viscosity=self.viscosity, jacobi_iters=self.jacobi_iters,
                                 route=self.route)
        return state[3]
