"""Differentiable 2-D fluid step: one NavierStokesSimulator.step() (navier_stokes.py:151-173) as a function of its whole state
(u, v, p, density), with its derivative on libsmokehip (csrc/fluid_grad.hip) behind torch autograd.  DESIGN.md section 3.9.

  fluid_step(u, v, p, density, ...)      one step; route="hip": the stepper's own stage kernels forward (bit-identical to step()), the
                                         adjoint kernels smk_advect_backward / smk_project_backward / smk_buoy_diffuse_backward backward;
                                         route="torch": fluid_step_rule under torch autograd.
  fluid_rollout(u, v, p, density, n)     n chained steps -> (state, frames [B, n, H, W]).
  fluid_step_rule(u, v, p, density, ...) the executable rule in torch ops (any dtype and device, differentiable): the tests' oracle.
  FluidRollout(steps=k, ...)             the settings object PerturbationTester.adversarial_test(simulate=...) takes.

Where things live: the rule itself is physics/fluid_rule.py, written once for 2-D and 3-D; the *_rule functions here bind its 2-D instance.
The hip route below is written once as well, over a per-dimension record (HIP2 here, HIP3 in fluid_grad3d.py): shape check, cached
stepper, staged forward (which fluid_tangent.py shares), autograd Function, step and rollout.

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
from operator import add
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import fluid_rule
from .fluid_rule import Branches
from .navier_stokes import NavierStokesSimulator

__all__ = ["Branches", "FluidRollout", "advect_rule", "buoy_diffuse_rule", "fluid_rollout", "fluid_step", "fluid_step_rule", "project_rule"]


# ------------------------------------------------------------------------------------------------ the rule in torch ops (fluid_rule.py, 2-D)
def advect_rule(field, u, v, *, dt: float = 0.01, branches: Optional[Branches] = None):
    """advection_step(field; u, v) (navier_stokes.py:74-95) with interpolate_velocity_u / _v (:97-109); no decay."""
    return fluid_rule.advect(field, (u, v), dt, branches)


def _diffuse(f, coef):
    """diffusion_step (navier_stokes.py:50-72) of one 2-D field: the host tests' handle on the rule's stencil."""
    return fluid_rule._diffuse(f, coef, 2)


def buoy_diffuse_rule(u, v, density, *, dt: float = 0.01, viscosity: float = 0.001):
    """Buoyancy into v[:, :-1] (navier_stokes.py:154-155), then diffusion_step of u, v and density (:158-160) -> (u, v, density)."""
    vel, density = fluid_rule.buoy_diffuse((u, v), density, dt, viscosity)
    return (*vel, density)


def project_rule(u, v, p, *, dt: float = 0.01, jacobi_iters: int = 20):
    """pressure_projection (navier_stokes.py:133-149): divergence with a true divide by dt, jacobi_iters sweeps from the carried-over p
    with the ring forced to 0, the gradient subtraction on u[1:-1] and v[:, 1:-1] -> (u, v, p)."""
    vel, p = fluid_rule.project((u, v), p, dt, jacobi_iters)
    return (*vel, p)


def fluid_step_rule(u, v, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                    branches: Optional[Branches] = None):
    """One step() in torch ops, stage by stage as the reference orders them: buoy_diffuse_rule, project_rule, the three sequentially
    dependent advections u <- adv(u; u, v), v <- adv(v; u_new, v), density <- adv(density; u_new, v_new), and the 0.995 decay -- one
    rounding per reference op, so in fp32 on the CPU it is the reference's step bit for bit.  State [..., H+1, W], [..., H, W+1],
    [..., H, W], [..., H, W] of any floating dtype on any device; differentiable.
    branches: a Branches recorder (filled) or replayer (followed); None: decisions are made and not kept."""
    return fluid_rule.step((u, v, p, density), dt, viscosity, jacobi_iters, branches)


# ------------------------------------------------------------------------------------------------ the hip route, once for 2-D and 3-D
@dataclass(frozen=True)
class HipRoute:
    """What the hip route needs to know about a dimension.  A state is (components ..., p, density); grid: the density's (H, W) or
    (D, H, W).  The C entry points all take (..., B, *grid, pitch_c = W, pitch_v = W + 1, ...)."""
    nd: int                           # grid axes = velocity components
    name: str                         # the public function's name, as the error texts spell it
    axes: str                         # "H, W" or "D, H, W", likewise
    fields: Tuple[str, ...]           # the stepper's state attributes, in state order
    simulator: type
    stages: Tuple[int, ...]           # run_stage's constants in step order: buoy-diffuse, project, then one advection per component, density
    grow: Tuple[Tuple[int, ...], ...]      # per component, then p: what its shape has more than the density's grid, per axis
    backward: Tuple[str, str, str, str]    # advect, project, buoy-diffuse backward and the projection's workspace query
    rule: object                      # the *_step_rule of route="torch"
    tangent: Tuple[str, str, str]     # advect tangent, tangent renorm and its workspace query (fluid_tangent.py, fluid_tangent3d.py)
    orthonormalize: Tuple[str, str]   # Gram-Schmidt over a grid's tangents and its workspace query (csrc/tangent_qr.hip)

    def shapes(self, lead, grid):
        """The shapes of the components and of p beside a density lead + grid."""
        return [lead + tuple(map(add, grid, g)) for g in self.grow]


HIP2 = HipRoute(2, "fluid_step", "H, W", ("u", "v", "p", "density"), NavierStokesSimulator,
                (_lib.STAGE_BUOY_DIFFUSE, _lib.STAGE_PROJECT, _lib.STAGE_ADVECT_U, _lib.STAGE_ADVECT_V, _lib.STAGE_ADVECT_D), ((1, 0), (0, 1), (0, 0)),
                ("smk_advect_backward", "smk_project_backward", "smk_buoy_diffuse_backward", "smk_project_backward_workspace"),
                fluid_step_rule, ("smk_advect_tangent", "smk_tangent_renorm", "smk_tangent_renorm_workspace"),
                ("smk_tangent_orthonormalize", "smk_tangent_orthonormalize_workspace"))

_SIMS = {}


def simulator(dim, B, grid, dt, viscosity, jacobi_iters, dev):
    """The cached stepper whose stage kernels run the forward: one per (B, grid, dt, viscosity, jacobi_iters, device)."""
    key = (B, tuple(grid), float(dt), float(viscosity), int(jacobi_iters), dev.index)
    sim = _SIMS.get(key)
    if sim is None:
        sim = _SIMS[key] = dim.simulator(tuple(grid), dt=dt, viscosity=viscosity, device=dev, batch_size=B, jacobi_iters=jacobi_iters)
    return sim


def staged_forward(dim, sim, state):
    """One step() of `sim` from `state`, stage by stage (bit-identical to step(); a timed-out persistent projection is reported as step()
    reports it) -> (the step's state, clones of the projected components and the diffused density: what the derivatives need)."""
    for name, t in zip(dim.fields, state):
        setattr(sim, name, t)
    sim.run_stage(dim.stages[0])
    sim.run_stage(dim.stages[1])
    kept = [getattr(sim, name).clone() for name in dim.fields[:dim.nd]] + [sim.density.clone()]
    for stage in dim.stages[2:]:
        sim.run_stage(stage)
    return sim.state(), kept


def _nan_where_far(far, *grads):
    bad = (far != 0).view(-1, *[1] * (grads[0].dim() - 1))
    return tuple(torch.where(bad, g.new_tensor(float("nan")), g) for g in grads)


def _ptrs(*tensors):
    return [t.data_ptr() for t in tensors]


class _FluidStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dim, dt, viscosity, jacobi_iters, *state):
        density = state[-1]
        dev = density.device
        sim = simulator(dim, density.shape[0], density.shape[1:], dt, viscosity, jacobi_iters, dev)
        with torch.cuda.device(dev):
            if any(ctx.needs_input_grad[4:]):            # keeping what the backward needs
                out, kept = staged_forward(dim, sim, state)
                ctx.save_for_backward(*kept, *out[:dim.nd])
            else:
                for name, t in zip(dim.fields, state):
                    setattr(sim, name, t)
                sim.step_into(None, 1)
                out = sim.state()
        ctx.dim, ctx.settings = dim, (float(dt), float(viscosity), int(jacobi_iters))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        dim, nd, saved = ctx.dim, ctx.dim.nd, ctx.saved_tensors
        vel_p, d_d, vel_a = saved[:nd], saved[nd], saved[nd + 1:]
        dt, viscosity, jacobi_iters = ctx.settings
        B, grid, dev = d_d.shape[0], d_d.shape[1:], d_d.device
        dims = (B, *grid, grid[-1], grid[-1] + 1)
        L = _lib.load()
        advect, project, buoy_diffuse, workspace = (getattr(L, name) for name in dim.backward)
        *g_a, gp, gd = (g.contiguous() for g in gouts)
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            far = torch.empty(nd + 1, B, dtype=torch.int32, device=dev)

            def advect_backward(stage, which, field, vel, gout):
                df, dvel = torch.empty_like(field), [torch.empty_like(c) for c in vel]
                _lib.check(advect(which, *_ptrs(field, *vel, gout, df, *dvel), far[stage].data_ptr(), *dims, dt, st))
                return df, dvel
            # reverse stage order.  density <- adv(d_d; the advected components) * 0.995, then component k <- adv(c_p[k]; the advected
            # components before it, the projected ones from itself on): 2-D v_a <- adv(v_p; u_a, v_p), u_a <- adv(u_p; u_p, v_p)
            g_dd, dvel = advect_backward(0, nd, d_d, vel_a, gd)
            g_a = [g + d for g, d in zip(g_a, dvel)]
            g_p = [None] * nd
            for stage, k in enumerate(reversed(range(nd)), 1):
                df, dvel = advect_backward(stage, k, vel_p[k], (*vel_a[:k], *vel_p[k:]), g_a[k])
                for j in range(k):
                    g_a[j] = g_a[j] + dvel[j]
                g_p[k] = df + dvel[k]                        # (the field is its own velocity component)
                for j in range(k + 1, nd):
                    g_p[j] = g_p[j] + dvel[j]
            # projection, then diffusion + buoyancy
            nbytes = int(workspace(B, *grid))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            d_vel, dp = [torch.empty_like(g) for g in g_p], torch.empty_like(gp)
            _lib.check(project(*_ptrs(*g_p, gp, *d_vel, dp), *dims, jacobi_iters, dt, ws.data_ptr(), nbytes, st))
            o_vel, od = [torch.empty_like(g) for g in d_vel], torch.empty_like(g_dd)
            _lib.check(buoy_diffuse(*_ptrs(*d_vel, g_dd, *o_vel, od), *dims, dt, viscosity, st))
            grads = _nan_where_far(far.amax(dim=0), *o_vel, dp, od)
        return (None, None, None, None, *grads)


def check_state(dim, state):
    density, nd = state[-1], dim.nd
    if density.dim() not in (nd, nd + 1):
        raise ValueError(f"{dim.name}: density must be [{dim.axes}] or [B, {dim.axes}], got {tuple(density.shape)}")
    lead, grid = tuple(density.shape[:-nd]), density.shape[-nd:]
    for name, t, g in zip(dim.fields, state, dim.grow):
        want = lead + tuple(map(add, grid, g))
        if t.shape != want:
            raise ValueError(f"{dim.name}: {name} must be {want} beside density {tuple(density.shape)}, got {tuple(t.shape)}")
    if min(grid) < 3:
        raise ValueError(f"{dim.name}: {dim.axes} >= 3")


def route_step(dim, state, dt=0.01, viscosity=0.001, jacobi_iters=20, route="hip"):
    """fluid_step / fluid_step3d: the checks, then the rule or the autograd Function."""
    check_state(dim, state)
    if route == "torch":
        return dim.rule(*state, dt=dt, viscosity=viscosity, jacobi_iters=jacobi_iters)
    if route != "hip":
        raise ValueError(f"{dim.name}: route is 'hip' or 'torch', got {route!r}")
    density = state[-1]
    _lib.require_cuda(density.device, f"{dim.name}(route='hip')")
    for name, t in zip(dim.fields, state):
        if t.dtype != torch.float32 or t.device != density.device:
            raise ValueError(f"{dim.name}(route='hip'): {name} must be a float32 tensor on the density's device")
    if int(jacobi_iters) < 0:
        raise ValueError(f"{dim.name}: jacobi_iters >= 0")
    batched = density.dim() == dim.nd + 1
    out = _FluidStepFn.apply(dim, dt, viscosity, jacobi_iters, *(state if batched else tuple(t[None] for t in state)))
    return out if batched else tuple(t[0] for t in out)


def route_rollout(dim, state, n_steps, settings):
    """fluid_rollout / fluid_rollout3d: n_steps chained steps -> (state, the densities stacked in front of the grid axes)."""
    if n_steps < 1:
        raise ValueError(f"{dim.name.replace('step', 'rollout')}: n_steps >= 1")
    frames = []
    for _ in range(n_steps):
        state = route_step(dim, state, **settings)
        frames.append(state[-1])
    return state, torch.stack(frames, dim=-dim.nd - 1)


def fluid_step(u, v, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip"):
    """One NavierStokesSimulator.step() as a differentiable function of the state -> (u, v, p, density).  State in the reference's shapes
    u [B, H+1, W], v [B, H, W+1], p, density [B, H, W] (or without the B).  route="hip": fp32 ROCm tensors; the forward runs the stepper's
    stage kernels and is bit-identical to step() on the same state, the backward runs the adjoint kernels (module docstring: far grids
    come back NaN).  route="torch": fluid_step_rule under torch autograd, any dtype and device."""
    return route_step(HIP2, (u, v, p, density), dt, viscosity, jacobi_iters, route)


def fluid_rollout(u, v, p, density, n_steps: int, **settings):
    """n_steps chained fluid_step calls -> ((u, v, p, density) after the last, frames [B, n_steps, H, W] of the densities; [n_steps, H, W]
    for an un-batched state).  settings: fluid_step's keywords.  With a gradient request every step saves its five fields (module
    docstring: 84 MB per step at 64 x 256^2), so memory grows linearly with n_steps."""
    return route_rollout(HIP2, (u, v, p, density), n_steps, settings)


@dataclass(frozen=True)
class FluidRollout:
    """PerturbationTester.adversarial_test(simulate=FluidRollout(steps=k, ...)): initial densities at rest (u = v = p = 0) -> the density
    after `steps` steps, differentiably."""
    steps: int = 4
    dt: float = 0.01
    viscosity: float = 0.001
    jacobi_iters: int = 20
    route: str = "hip"
    dim = HIP2                        # (not a field: FluidRollout3D overrides it)

    def __call__(self, density):
        """density [B, H, W] ([B, D, H, W] in 3-D) -> density after `steps` steps from rest."""
        rest = [density.new_zeros(s) for s in self.dim.shapes(density.shape[:1], density.shape[1:])]
        settings = dict(dt=self.dt, viscosity=self.viscosity, jacobi_iters=self.jacobi_iters, route=self.route)
        return route_rollout(self.dim, (*rest, density), self.steps, settings)[0][-1]
