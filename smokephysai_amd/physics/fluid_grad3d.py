"""Differentiable 3-D fluid step: one NavierStokesSimulator3D.step() (SPEC_3D.md sections 3-6) as a function of its whole state
(u, v, w, p, density), with its derivative on libsmokehip (csrc/fluid_grad3d.hip) behind torch autograd.  DESIGN.md section 3.10; the
3-D counterpart of fluid_grad.py (section 3.9), whose Branches recorder it reuses unchanged.

  fluid_step3d(u, v, w, p, density, ...)      one step; route="hip": the stepper's own stage kernels forward (bit-identical to step()),
                                              the adjoint kernels smk_advect3d_backward / smk_project3d_backward /
                                              smk_buoy_diffuse3d_backward backward; route="torch": fluid_step3d_rule under torch autograd.
  fluid_rollout3d(u, v, w, p, density, n)     n chained steps -> (state, frames [B, n, D, H, W]).
  fluid_step3d_rule(u, v, w, p, density, ...) the executable rule in torch ops (any dtype and device, differentiable): the tests' oracle.
  FluidRollout3D(steps=k, ...)                the settings object PerturbationTester.adversarial_test(simulate=...) takes for volumes.

Derivative conventions (section 3.9's, unchanged): floor and integer casts have derivative 0, a clamp of a coordinate passes its gradient
where lo <= x <= hi (bounds included), the interpolation weights are formed from the clamped indices as in the forward (so the upper-edge
quirk cancels itself); dt, viscosity and jacobi_iters are constants.  The velocity sample coordinates are index grids, constants: with
respect to a component the sample is linear, 0.5 / 0.5 on c[z, y, x] and its +1 neighbour along the acting axis where the sample is not
on the component's upper edge, exactly 0 elsewhere.

Limit of the hip route: its advection backward gathers over the 3 x 3 x 3 destinations around a source cell, which holds while every
back-trace of the four advections moves less than one cell on every axis.  A grid that breaks this gets NaN in all five of its gradients
(no host synchronisation; the other grids of the batch are untouched); route="torch" has no such limit, and the forward is unaffected.

Memory: a step whose input requires a gradient saves seven fields per grid (u, v, w after the projection, the diffused density, u, v, w
after their advections; the last three are the step's own outputs): 7 * 4 * D * H * W bytes per grid and step -- 3.8 GB per step at
8 x 64 x 512 x 512.  Without a gradient request nothing is saved."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .fluid_grad import Branches, _NoBranches

__all__ = ["FluidRollout3D", "advect3d_rule", "buoy_diffuse3d_rule", "fluid_rollout3d", "fluid_step3d", "fluid_step3d_rule",
           "project3d_rule"]

SIXTH = float(np.float32(1.0 / 6.0))       # SPEC_3D.md section 4: the fp32 value nearest to the double 1/6, in every dtype


# ------------------------------------------------------------------------------------------------ the rule in torch ops
def _shift(f, dim, lo):
    """The replicate-padded neighbour along dim: lo=True f[i-1] (f[0] at i = 0), lo=False f[i+1] (f[n-1] at i = n-1)."""
    n = f.shape[dim]
    if lo:
        return torch.cat([f.narrow(dim, 0, 1), f.narrow(dim, 0, n - 1)], dim=dim)
    return torch.cat([f.narrow(dim, 1, n - 1), f.narrow(dim, n - 1, 1)], dim=dim)


def _diffuse3(f, coef):
    """diffusion_step (SPEC_3D.md section 3): replicate padding on six faces, up + down + left + right + front + back - 6 f summed left to
    right, f + (dt * viscosity) * lap."""
    lap = _shift(f, -2, True) + _shift(f, -2, False)
    lap = lap + _shift(f, -1, True)
    lap = lap + _shift(f, -1, False)
    lap = lap + _shift(f, -3, True)
    lap = lap + _shift(f, -3, False)
    lap = lap - 6.0 * f
    return f + coef * lap


def _take3(f, zi, yi, xi):
    """f[..., zi, yi, xi] for index tensors that broadcast to [..., Z, Y, X]."""
    idx = (zi * f.shape[-2] + yi) * f.shape[-1] + xi
    idx = idx.expand(f.shape[:-3] + idx.shape[-3:])
    return f.flatten(-3).gather(-1, idx.flatten(-3)).view(idx.shape)


def _interpolate3(f, z, y, x, br):
    """interpolate (SPEC_3D.md section 5): floor, clamp the INDICES, weights from the clamped indices, (wx * wy) * wz, eight terms z-low
    plane first, x fastest, low before high.  Three floors, recorded in the order x, y, z."""
    d, h, w = f.shape[-3:]
    x0, y0, z0 = br.floor(x), br.floor(y), br.floor(z)
    x1, y1, z1 = x0 + 1, y0 + 1, z0 + 1
    x0, x1 = x0.clamp(0, w - 1), x1.clamp(0, w - 1)
    y0, y1 = y0.clamp(0, h - 1), y1.clamp(0, h - 1)
    z0, z1 = z0.clamp(0, d - 1), z1.clamp(0, d - 1)
    wx = (x1.to(f.dtype) - x, x - x0.to(f.dtype))
    wy = (y1.to(f.dtype) - y, y - y0.to(f.dtype))
    wz = (z1.to(f.dtype) - z, z - z0.to(f.dtype))
    xs, ys, zs = (x0, x1), (y0, y1), (z0, z1)
    r = None
    for k in range(2):
        for j in range(2):
            for i in range(2):
                term = ((wx[i] * wy[j]) * wz[k]) * _take3(f, zs[k], ys[j], xs[i])
                r = term if r is None else r + term
    return r


def _sample3(c, act, Z, Y, X, br):
    """A velocity component sampled at the index grid, shifted +0.5 along the axis it acts on (-1: x, -2: y, -3: z); every coordinate
    clamped to the component's extent (SPEC_3D.md section 5)."""
    coords = {-3: Z, -2: Y, -1: X}
    coords[act] = coords[act] + 0.5
    cz, cy, cx = (br.clamp(coords[a], 0.0, float(c.shape[a] - 1)) for a in (-3, -2, -1))
    return _interpolate3(c, cz, cy, cx, br)


def advect3d_rule(field, u, v, w, *, dt: float = 0.01, branches: Optional[Branches] = None):
    """advection_step(field; u, v, w) (SPEC_3D.md section 5); no decay."""
    br = _NoBranches if branches is None else branches
    f = field
    Df, Hf, Wf = f.shape[-3:]
    Z, Y, X = torch.meshgrid(*[torch.arange(n, dtype=f.dtype, device=f.device) for n in (Df, Hf, Wf)], indexing="ij")
    ui = _sample3(u, -1, Z, Y, X, br)
    vi = _sample3(v, -2, Z, Y, X, br)
    wi = _sample3(w, -3, Z, Y, X, br)
    px = br.clamp(X - dt * ui, 0.0, float(Wf - 1))
    py = br.clamp(Y - dt * vi, 0.0, float(Hf - 1))
    pz = br.clamp(Z - dt * wi, 0.0, float(Df - 1))
    return _interpolate3(f, pz, py, px, br)


def buoy_diffuse3d_rule(u, v, w, density, *, dt: float = 0.01, viscosity: float = 0.001):
    """Buoyancy into v[..., :-1] (SPEC_3D.md section 6.1), then diffusion_step of u, v, w and density -> (u, v, w, density)."""
    b = density * 0.1
    v = torch.cat([v[..., :, :-1] + dt * b, v[..., :, -1:]], dim=-1)
    return (_diffuse3(u, dt * viscosity), _diffuse3(v, dt * viscosity), _diffuse3(w, dt * viscosity),
            _diffuse3(density, dt * (viscosity * 0.1)))


def project3d_rule(u, v, w, p, *, dt: float = 0.01, jacobi_iters: int = 20):
    """pressure_projection (SPEC_3D.md section 4): divergence with a true divide by dt, jacobi_iters sweeps from the carried-over p with
    the boundary shell forced to 0, the gradient subtraction on the inner faces of u, v, w -> (u, v, w, p)."""
    div = u[..., :, 1:, :] - u[..., :, :-1, :]
    div = div + v[..., :, :, 1:]
    div = div - v[..., :, :, :-1]
    div = div + w[..., 1:, :, :]
    div = div - w[..., :-1, :, :]
    div = div / dt
    for _ in range(jacobi_iters):
        s = p[..., 1:-1, :-2, 1:-1] + p[..., 1:-1, 2:, 1:-1]
        s = s + p[..., 1:-1, 1:-1, :-2]
        s = s + p[..., 1:-1, 1:-1, 2:]
        s = s + p[..., :-2, 1:-1, 1:-1]
        s = s + p[..., 2:, 1:-1, 1:-1]
        p = torch.nn.functional.pad(SIXTH * (s - div[..., 1:-1, 1:-1, 1:-1]), (1, 1, 1, 1, 1, 1))
    u = torch.cat([u[..., :, :1, :], u[..., :, 1:-1, :] - dt * (p[..., :, 1:, :] - p[..., :, :-1, :]), u[..., :, -1:, :]], dim=-2)
    v = torch.cat([v[..., :, :, :1], v[..., :, :, 1:-1] - dt * (p[..., :, :, 1:] - p[..., :, :, :-1]), v[..., :, :, -1:]], dim=-1)
    w = torch.cat([w[..., :1, :, :], w[..., 1:-1, :, :] - dt * (p[..., 1:, :, :] - p[..., :-1, :, :]), w[..., -1:, :, :]], dim=-3)
    return u, v, w, p


def fluid_step3d_rule(u, v, w, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                      branches: Optional[Branches] = None):
    """One step() in torch ops, stage by stage as SPEC_3D.md section 6 orders them: buoy_diffuse3d_rule, project3d_rule, the four
    sequentially dependent advections u <- adv(u; u, v, w), v <- adv(v; u_new, v, w), w <- adv(w; u_new, v_new, w),
    density <- adv(density; u_new, v_new, w_new), and the 0.995 decay -- one rounding per listed op, so in fp32 on the CPU it is
    oracle/ns_nd.py's 3-D instance bit for bit.  State [..., D, H+1, W], [..., D, H, W+1], [..., D+1, H, W], [..., D, H, W] twice, of any
    floating dtype on any device; differentiable.
    branches: a Branches recorder (filled) or replayer (followed); None: decisions are made and not kept."""
    u, v, w, density = buoy_diffuse3d_rule(u, v, w, density, dt=dt, viscosity=viscosity)
    u, v, w, p = project3d_rule(u, v, w, p, dt=dt, jacobi_iters=jacobi_iters)
    u = advect3d_rule(u, u, v, w, dt=dt, branches=branches)
    v = advect3d_rule(v, u, v, w, dt=dt, branches=branches)
    w = advect3d_rule(w, u, v, w, dt=dt, branches=branches)
    density = advect3d_rule(density, u, v, w, dt=dt, branches=branches)
    density = density * 0.995
    return u, v, w, p, density


# ------------------------------------------------------------------------------------------------ the hip route
_SIMS = {}


def _simulator(B, D, H, W, dt, viscosity, jacobi_iters, dev):
    """The cached stepper whose stage kernels run the forward: one per (B, D, H, W, dt, viscosity, jacobi_iters, device)."""
    from .navier_stokes3d import NavierStokesSimulator3D
    key = (B, D, H, W, float(dt), float(viscosity), int(jacobi_iters), dev.index)
    sim = _SIMS.get(key)
    if sim is None:
        sim = _SIMS[key] = NavierStokesSimulator3D((D, H, W), dt=dt, viscosity=viscosity, device=dev, batch_size=B,
                                                   jacobi_iters=jacobi_iters)
    return sim


def _nan_where_far(far, *grads):
    bad = (far != 0)[:, None, None, None]
    return tuple(torch.where(bad, g.new_tensor(float("nan")), g) for g in grads)


class _FluidStep3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, w, p, density, dt, viscosity, jacobi_iters):
        from . import navier_stokes3d as N
        B, D, H, W = density.shape
        dev = density.device
        sim = _simulator(B, D, H, W, dt, viscosity, jacobi_iters, dev)
        with torch.cuda.device(dev):
            sim.u, sim.v, sim.w, sim.p, sim.density = u, v, w, p, density
            keep = any(ctx.needs_input_grad[:5])
            if keep:                                     # stage by stage (bit-identical to step()), keeping what the backward needs
                sim.run_stage(N.STAGE3D_BUOY_DIFFUSE)
                sim.run_stage(N.STAGE3D_PROJECT)
                u_p, v_p, w_p, d_d = sim.u.clone(), sim.v.clone(), sim.w.clone(), sim.density.clone()
                sim.run_stage(N.STAGE3D_ADVECT_U)
                sim.run_stage(N.STAGE3D_ADVECT_V)
                sim.run_stage(N.STAGE3D_ADVECT_W)
                sim.run_stage(N.STAGE3D_ADVECT_D)
            else:
                sim.step_into(None, 1)
            u_a, v_a, w_a, p_n, d_n = sim.state()
        if keep:
            ctx.save_for_backward(u_p, v_p, w_p, d_d, u_a, v_a, w_a)
        ctx.settings = (float(dt), float(viscosity), int(jacobi_iters))
        return u_a, v_a, w_a, p_n, d_n

    @staticmethod
    @once_differentiable
    def backward(ctx, gu, gv, gw, gp, gd):
        u_p, v_p, w_p, d_d, u_a, v_a, w_a = ctx.saved_tensors
        dt, viscosity, jacobi_iters = ctx.settings
        B, D, H, W = d_d.shape
        dev = d_d.device
        L = _lib.load()
        gu, gv, gw, gp, gd = (g.contiguous() for g in (gu, gv, gw, gp, gd))
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            far = torch.empty(4, B, dtype=torch.int32, device=dev)

            def advect_backward(stage, which, field, uu, vv, ww, gout):
                df, du, dv, dw = torch.empty_like(field), torch.empty_like(uu), torch.empty_like(vv), torch.empty_like(ww)
                _lib.check(L.smk_advect3d_backward(which, field.data_ptr(), uu.data_ptr(), vv.data_ptr(), ww.data_ptr(), gout.data_ptr(),
                                                   df.data_ptr(), du.data_ptr(), dv.data_ptr(), dw.data_ptr(), far[stage].data_ptr(),
                                                   B, D, H, W, W, W + 1, dt, st))
                return df, du, dv, dw
            # reverse stage order: density <- adv(d_d; u_a, v_a, w_a) * 0.995, w_a <- adv(w_p; u_a, v_a, w_p),
            # v_a <- adv(v_p; u_a, v_p, w_p), u_a <- adv(u_p; u_p, v_p, w_p)
            g_dd, du, dv, dw = advect_backward(0, 3, d_d, u_a, v_a, w_a, gd)
            g_ua, g_va, g_wa = gu + du, gv + dv, gw + dw
            df, du, dv, dw = advect_backward(1, 2, w_p, u_a, v_a, w_p, g_wa)
            g_ua, g_va, g_wp = g_ua + du, g_va + dv, df + dw
            df, du, dv, dw = advect_backward(2, 1, v_p, u_a, v_p, w_p, g_va)
            g_ua, g_vp, g_wp = g_ua + du, df + dv, g_wp + dw
            df, du, dv, dw = advect_backward(3, 0, u_p, u_p, v_p, w_p, g_ua)
            g_up, g_vp, g_wp = df + du, g_vp + dv, g_wp + dw
            # projection, then diffusion + buoyancy
            nbytes = int(L.smk_project3d_backward_workspace(B, D, H, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            du, dv, dw, dp = torch.empty_like(g_up), torch.empty_like(g_vp), torch.empty_like(g_wp), torch.empty_like(gp)
            _lib.check(L.smk_project3d_backward(g_up.data_ptr(), g_vp.data_ptr(), g_wp.data_ptr(), gp.data_ptr(), du.data_ptr(),
                                                dv.data_ptr(), dw.data_ptr(), dp.data_ptr(), B, D, H, W, W, W + 1, jacobi_iters, dt,
                                                ws.data_ptr(), nbytes, st))
            ou, ov, ow, od = torch.empty_like(du), torch.empty_like(dv), torch.empty_like(dw), torch.empty_like(g_dd)
            _lib.check(L.smk_buoy_diffuse3d_backward(du.data_ptr(), dv.data_ptr(), dw.data_ptr(), g_dd.data_ptr(), ou.data_ptr(),
                                                     ov.data_ptr(), ow.data_ptr(), od.data_ptr(), B, D, H, W, W, W + 1, dt, viscosity, st))
            ou, ov, ow, dp, od = _nan_where_far(far.amax(dim=0), ou, ov, ow, dp, od)
        return ou, ov, ow, dp, od, None, None, None


def _check_state(u, v, w, p, density):
    if density.dim() not in (3, 4):
        raise ValueError(f"fluid_step3d: density must be [D, H, W] or [B, D, H, W], got {tuple(density.shape)}")
    lead, (D, H, W) = tuple(density.shape[:-3]), density.shape[-3:]
    want = {"u": lead + (D, H + 1, W), "v": lead + (D, H, W + 1), "w": lead + (D + 1, H, W), "p": lead + (D, H, W)}
    for name, t in (("u", u), ("v", v), ("w", w), ("p", p)):
        if tuple(t.shape) != want[name]:
            raise ValueError(f"fluid_step3d: {name} must be {want[name]} beside density {tuple(density.shape)}, got {tuple(t.shape)}")
    if D < 3 or H < 3 or W < 3:
        raise ValueError("fluid_step3d: D, H, W >= 3")


def fluid_step3d(u, v, w, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip"):
    """One NavierStokesSimulator3D.step() as a differentiable function of the state -> (u, v, w, p, density).  State in SPEC_3D.md section
    1's shapes u [B, D, H+1, W], v [B, D, H, W+1], w [B, D+1, H, W], p, density [B, D, H, W] (or without the B).  route="hip": fp32 ROCm
    tensors; the forward runs the stepper's kernels and is bit-identical to step() on the same state, the backward runs the adjoint
    kernels (module docstring: far grids come back NaN).  route="torch": fluid_step3d_rule under torch autograd, any dtype and device."""
    _check_state(u, v, w, p, density)
    if route == "torch":
        return fluid_step3d_rule(u, v, w, p, density, dt=dt, viscosity=viscosity, jacobi_iters=jacobi_iters)
    if route != "hip":
        raise ValueError(f"fluid_step3d: route is 'hip' or 'torch', got {route!r}")
    _lib.require_cuda(density.device, "fluid_step3d(route='hip')")
    for name, t in (("u", u), ("v", v), ("w", w), ("p", p), ("density", density)):
        if t.dtype != torch.float32 or t.device != density.device:
            raise ValueError(f"fluid_step3d(route='hip'): {name} must be a float32 tensor on the density's device")
    if int(jacobi_iters) < 0:
        raise ValueError("fluid_step3d: jacobi_iters >= 0")
    batched = density.dim() == 4
    state = (u, v, w, p, density) if batched else tuple(t[None] for t in (u, v, w, p, density))
    out = _FluidStep3dFn.apply(*state, dt, viscosity, jacobi_iters)
    return out if batched else tuple(t[0] for t in out)


def fluid_rollout3d(u, v, w, p, density, n_steps: int, **settings):
    """n_steps chained fluid_step3d calls -> ((u, v, w, p, density) after the last, frames [B, n_steps, D, H, W] of the densities;
    [n_steps, D, H, W] for an un-batched state).  settings: fluid_step3d's keywords.  With a gradient request every step saves its seven
    fields per grid (module docstring: 3.8 GB per step at 8 x 64 x 512 x 512), so memory grows linearly with n_steps."""
    if n_steps < 1:
        raise ValueError("fluid_rollout3d: n_steps >= 1")
    state, frames = (u, v, w, p, density), []
    for _ in range(n_steps):
        state = fluid_step3d(*state, **settings)
        frames.append(state[4])
    return state, torch.stack(frames, dim=-4)


@dataclass(frozen=True)
class FluidRollout3D:
    """PerturbationTester.adversarial_test(simulate=FluidRollout3D(steps=k, ...)): initial volumes at rest (u = v = w = p = 0) -> the
    density after `steps` steps, differentiably."""
    steps: int = 4
    dt: float = 0.01
    viscosity: float = 0.001
    jacobi_iters: int = 20
    route: str = "hip"

    def __call__(self, density):
        """density [B, D, H, W] -> density after `steps` steps from rest."""
        B, D, H, W = density.shape
        z = density.new_zeros
        state, _ = fluid_rollout3d(z(B, D, H + 1, W), z(B, D, H, W + 1), z(B, D + 1, H, W), z(B, D, H, W), density, self.steps, dt=self.dt,
                                   viscosity=self.viscosity, jacobi_iters=self.jacobi_iters, route=self.route)
        return state[4]
