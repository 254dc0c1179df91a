"""Differentiable 3-D fluid step: one NavierStokesSimulator3D.step() (SPEC_3D.md sections 3-6) as a function of its whole state
(u, v, w, p, density), with its derivative on libsmokehip (csrc/fluid_grad3d.hip) behind torch autograd.  DESIGN.md section 3.10; the
3-D counterpart of fluid_grad.py (section 3.9).  The rule is physics/fluid_rule.py's 3-D instance and the hip route is fluid_grad.py's, run
over the record HIP3 below: this module binds both to the 3-D argument lists.

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

from . import fluid_rule, navier_stokes3d as N
from .fluid_grad import FluidRollout, HipRoute, route_rollout, route_step
from .fluid_rule import SIXTH, Branches                                      # noqa: F401  (SIXTH: the tests' Jacobi scale)

__all__ = ["FluidRollout3D", "advect3d_rule", "buoy_diffuse3d_rule", "fluid_rollout3d", "fluid_step3d", "fluid_step3d_rule",
           "project3d_rule"]


# ------------------------------------------------------------------------------------------------ the rule in torch ops (fluid_rule.py, 3-D)
def advect3d_rule(field, u, v, w, *, dt: float = 0.01, branches: Optional[Branches] = None):
    """advection_step(field; u, v, w) (SPEC_3D.md section 5); no decay."""
    return fluid_rule.advect(field, (u, v, w), dt, branches)


def _diffuse3(f, coef):
    """diffusion_step (SPEC_3D.md section 3) of one 3-D field: the host tests' handle on the rule's stencil."""
    return fluid_rule._diffuse(f, coef, 3)


def buoy_diffuse3d_rule(u, v, w, density, *, dt: float = 0.01, viscosity: float = 0.001):
    """Buoyancy into v[..., :-1] (SPEC_3D.md section 6.1), then diffusion_step of u, v, w and density -> (u, v, w, density)."""
    vel, density = fluid_rule.buoy_diffuse((u, v, w), density, dt, viscosity)
    return (*vel, density)


def project3d_rule(u, v, w, p, *, dt: float = 0.01, jacobi_iters: int = 20):
    """pressure_projection (SPEC_3D.md section 4): divergence with a true divide by dt, jacobi_iters sweeps from the carried-over p with
    the boundary shell forced to 0, the gradient subtraction on the inner faces of u, v, w -> (u, v, w, p)."""
    vel, p = fluid_rule.project((u, v, w), p, dt, jacobi_iters)
    return (*vel, p)


def fluid_step3d_rule(u, v, w, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                      branches: Optional[Branches] = None):
    """One step() in torch ops, stage by stage as SPEC_3D.md section 6 orders them: buoy_diffuse3d_rule, project3d_rule, the four
    sequentially dependent advections u <- adv(u; u, v, w), v <- adv(v; u_new, v, w), w <- adv(w; u_new, v_new, w),
    density <- adv(density; u_new, v_new, w_new), and the 0.995 decay -- one rounding per listed op, so in fp32 on the CPU it is
    oracle/ns_nd.py's 3-D instance bit for bit.  State [..., D, H+1, W], [..., D, H, W+1], [..., D+1, H, W], [..., D, H, W] twice, of any
    floating dtype on any device; differentiable.
    branches: a Branches recorder (filled) or replayer (followed); None: decisions are made and not kept."""
    return fluid_rule.step((u, v, w, p, density), dt, viscosity, jacobi_iters, branches)


# ------------------------------------------------------------------------------------------------ the hip route (fluid_grad.py's, 3-D)
HIP3 = HipRoute(3, "fluid_step3d", "D, H, W", ("u", "v", "w", "p", "density"), N.NavierStokesSimulator3D,
                (N.STAGE3D_BUOY_DIFFUSE, N.STAGE3D_PROJECT, N.STAGE3D_ADVECT_U, N.STAGE3D_ADVECT_V, N.STAGE3D_ADVECT_W, N.STAGE3D_ADVECT_D),
                ((0, 1, 0), (0, 0, 1), (1, 0, 0), (0, 0, 0)),
                ("smk_advect3d_backward", "smk_project3d_backward", "smk_buoy_diffuse3d_backward", "smk_project3d_backward_workspace"),
                fluid_step3d_rule, ("smk_advect3d_tangent", "smk_tangent3d_renorm", "smk_tangent3d_renorm_workspace"),
                ("smk_tangent3d_orthonormalize", "smk_tangent3d_orthonormalize_workspace"))


def fluid_step3d(u, v, w, p, density, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip"):
    """One NavierStokesSimulator3D.step() as a differentiable function of the state -> (u, v, w, p, density).  State in SPEC_3D.md section
    1's shapes u [B, D, H+1, W], v [B, D, H, W+1], w [B, D+1, H, W], p, density [B, D, H, W] (or without the B).  route="hip": fp32 ROCm
    tensors; the forward runs the stepper's kernels and is bit-identical to step() on the same state, the backward runs the adjoint
    kernels (module docstring: far grids come back NaN).  route="torch": fluid_step3d_rule under torch autograd, any dtype and device."""
    return route_step(HIP3, (u, v, w, p, density), dt, viscosity, jacobi_iters, route)


def fluid_rollout3d(u, v, w, p, density, n_steps: int, **settings):
    """n_steps chained fluid_step3d calls -> ((u, v, w, p, density) after the last, frames [B, n_steps, D, H, W] of the densities;
    [n_steps, D, H, W] for an un-batched state).  settings: fluid_step3d's keywords.  With a gradient request every step saves its seven
    fields per grid (module docstring: 3.8 GB per step at 8 x 64 x 512 x 512), so memory grows linearly with n_steps."""
    return route_rollout(HIP3, (u, v, w, p, density), n_steps, settings)


@dataclass(frozen=True)
class FluidRollout3D(FluidRollout):
    """PerturbationTester.adversarial_test(simulate=FluidRollout3D(steps=k, ...)): initial volumes at rest (u = v = w = p = 0) -> the
    density after `steps` steps, differentiably.  FluidRollout's fields; density [B, D, H, W]."""
    dim = HIP3
