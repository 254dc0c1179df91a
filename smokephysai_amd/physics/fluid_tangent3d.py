"""Tangent-linear 3-D fluid step: one NavierStokesSimulator3D.step() (SPEC_3D.md sections 3-6) together with J t, the product of its
Jacobian with respect to the whole state (u, v, w, p, density) and tangent states t, on libsmokehip (csrc/fluid_tangent3d.hip), and the
Lyapunov exponents of a volume's flow that come from it (Benettin's method).  DESIGN.md section 3.12; the 3-D counterpart of
fluid_tangent.py (section 3.11), whose route, shape checks and Benettin loop it runs over the record HIP3: this module binds them to the
3-D argument lists.

  fluid_step3d_jvp(state, tangents, ...)       one step -> (state', tangents'); route="hip": the stepper's own stage kernels for the state
                                               (bit-identical to step()) and, on a stepper of B * T grids, for the tangents' linear stages
                                               (buoyancy + diffusion, projection), then smk_advect3d_tangent four times; route="torch":
                                               fluid_step3d_jvp_rule.
  fluid_step3d_jvp_rule(state, tangents, ...)  torch.autograd.forward_ad over fluid_step3d_rule (any dtype and device): the tests' oracle.
  fluid_tangent_rollout3d(state, tangents, n)  n chained fluid_step3d_jvp calls; nothing is saved between steps.
  lyapunov_exponents3d(u, v, w, p, density, n) the k largest Lyapunov exponents per unit time -> LyapunovResult (fluid_tangent.py's).
  flow_chaos3d(u, v, w, p, density, n)         the spectrum's summaries -> FlowChaos (fluid_tangent.py's): largest exponent, Kaplan-Yorke
                                               dimension, Kolmogorov-Sinai entropy bound.

Derivative conventions: fluid_grad3d's.  Unlike fluid_step3d's backward the hip route has no one-cell limit: the tangent of the advection
is a gather at the forward's own taps.  Limit of the hip route: B * T * (D + 1) <= 65535, smk_sim3d_create's limit for the stepper of
B * T grids that runs the tangents' linear stages.

Memory: nothing is saved between steps; a call holds the state, T tangent states per grid, the stepper's own buffers for B and for B * T
grids, and the step's intermediate clones -- of the order of (1 + T) * 3 states.

Hot path and what is not: for k = 1 the renormalisation is smk_tangent3d_renorm (two launches, no host synchronisation).  For k > 1 the
tangents are re-orthonormalised by modified Gram-Schmidt with fp64 coefficients: gram_schmidt="torch" (lyapunov_exponents3d's default, as
before) in plain torch operations, NOT a hot path; gram_schmidt="hip" (flow_chaos3d's default on the hip route) by
smk_tangent3d_orthonormalize (csrc/tangent_qr.hip: 2 k launches, no host synchronisation).  DESIGN.md section 3.13.

Out of scope: forward_ad through fluid_step3d itself (call fluid_step3d_jvp), and the dataset labels (the `lyapunov_exponent` /
`fractal_dimension` / `entropy` of the 3-D datasets stay the proxies; a labels="flow" dataset mode is not built)."""
from typing import Optional

from .fluid_grad3d import HIP3
from .fluid_rule import Branches
from .fluid_tangent import FlowChaos, LyapunovResult, route_flow_chaos, route_jvp, route_jvp_rule, route_lyapunov, route_tangent_rollout

__all__ = ["flow_chaos3d", "fluid_step3d_jvp", "fluid_step3d_jvp_rule", "fluid_tangent_rollout3d", "lyapunov_exponents3d"]


def fluid_step3d_jvp_rule(state, tangents, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                          branches: Optional[Branches] = None):
    """(state', tangents') of one step by torch.autograd.forward_ad over fluid_step3d_rule: any floating dtype, any device.  state
    (u, v, w, p, density) with leading dimensions [B] (or none); tangents state-shaped, or [B, T, ...]: then the state is expanded along T
    and one pass carries all T tangents (a Branches recorder then holds decisions of that expanded shape).  branches: as
    fluid_step3d_rule's."""
    return route_jvp_rule(HIP3, state, tangents, dt, viscosity, jacobi_iters, branches)


def fluid_step3d_jvp(state, tangents, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip"):
    """One NavierStokesSimulator3D.step() with the tangent-linear step beside it -> ((u, v, w, p, density)', (tu, tv, tw, tp, tdensity)').
    state: u [B, D, H+1, W], v [B, D, H, W+1], w [B, D+1, H, W], p, density [B, D, H, W] (or without the B); tangents: state-shaped, or
    [B, T, ...] for T tangents per grid.  route="hip": fp32 ROCm tensors; the returned state is bit-identical to step() on the same state;
    nothing is saved; no one-cell limit.  route="torch": fluid_step3d_jvp_rule, any dtype and device.  Not differentiable itself."""
    return route_jvp(HIP3, state, tangents, dt, viscosity, jacobi_iters, route)


def fluid_tangent_rollout3d(state, tangents, n_steps: int, **settings):
    """n_steps chained fluid_step3d_jvp calls -> (state, tangents) after the last.  settings: fluid_step3d_jvp's keywords.  Nothing is kept
    between steps, so memory does not grow with n_steps; the tangents are not renormalised (lyapunov_exponents3d does that)."""
    return route_tangent_rollout(HIP3, state, tangents, n_steps, settings)


def lyapunov_exponents3d(u, v, w, p, density, n_steps: int, *, k: int = 1, renorm_every: int = 1, tangent0=None, seed: int = 0,
                         dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip",
                         branches: Optional[Branches] = None, gram_schmidt: str = "torch") -> LyapunovResult:
    """The k largest Lyapunov exponents of the flow from the state (u, v, w, p, density), by Benettin's method: lyapunov_exponents'
    keywords and result, over fluid_step3d_jvp.  k = 1: smk_tangent3d_renorm on the hip route; 1 < k <= 8: modified Gram-Schmidt, in torch
    operations (gram_schmidt="torch", the default: not a hot path) or by smk_tangent3d_orthonormalize (gram_schmidt="hip").  tangent0: (tu, tv, tw, tp, tdensity), state-shaped (k = 1) or [B, k, ...]; default: unit-normal noise
    drawn on the CPU from `seed`."""
    return route_lyapunov(HIP3, (u, v, w, p, density), n_steps, k, renorm_every, tangent0, seed, dt, viscosity, jacobi_iters, route,
                          branches, gram_schmidt)


def flow_chaos3d(u, v, w, p, density, n_steps: int, *, k: int = 4, renorm_every: int = 1, seed: int = 0, dt: float = 0.01,
                 viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip", gram_schmidt: Optional[str] = None) -> FlowChaos:
    """flow_chaos for a volume's flow from the state (u, v, w, p, density): the k largest exponents by lyapunov_exponents3d -> FlowChaos.
    gram_schmidt: None = "hip" (smk_tangent3d_orthonormalize) on route="hip", "torch" on route="torch"."""
    return route_flow_chaos(HIP3, (u, v, w, p, density), n_steps, k, renorm_every, seed, dt, viscosity, jacobi_iters, route, gram_schmidt)
