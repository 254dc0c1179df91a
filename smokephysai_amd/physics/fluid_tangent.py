"""Tangent-linear 2-D fluid step: one NavierStokesSimulator.step() (navier_stokes.py:151-173) together with J t, the product of its
Jacobian with respect to the whole state (u, v, p, density) and tangent states t, on libsmokehip (csrc/fluid_tangent.hip), and the
Lyapunov exponents of the flow that come from it (Benettin's method).  DESIGN.md section 3.11.

  fluid_step_jvp(state, tangents, ...)        one step -> (state', tangents'); route="hip": the stepper's own stage kernels for the state
                                              (bit-identical to step()) and, on a stepper of B * T grids, for the tangents' linear stages
                                              (buoyancy + diffusion, projection), then smk_advect_tangent three times; route="torch":
                                              fluid_step_jvp_rule.
  fluid_step_jvp_rule(state, tangents, ...)   torch.autograd.forward_ad over fluid_step_rule (any dtype and device): the tests' oracle.
  fluid_tangent_rollout(state, tangents, n)   n chained fluid_step_jvp calls; nothing is saved between steps.
  lyapunov_exponents(u, v, p, density, n)     the k largest Lyapunov exponents per unit time, with renormalisation every renorm_every
                                              steps -> LyapunovResult(exponents [B, k], log_growth [B, n_renorms, k], state, tangents).
  flow_chaos(u, v, p, density, n)             the spectrum's three summaries -> FlowChaos(exponents sorted, lyapunov = the largest,
                                              kaplan_yorke, ks_entropy, truncated, log_growth); kaplan_yorke_dimension and ks_entropy
                                              are the two formulas on any spectrum (fp64 torch, any device).  DESIGN.md section 3.13.

Where things live: the rule under forward_ad is fluid_grad.fluid_step_rule, i.e. physics/fluid_rule.py's 2-D instance; the state's staged
forward, the shape check and the stepper cache are fluid_grad.py's (staged_forward, check_state, simulator over the record HIP2), shared
with fluid_step; the kernel's back-trace is csrc/fluid_trace.h, shared with csrc/fluid_grad.hip.  The route, the tangents' shape checks
and the Benettin loop below are written once over that per-dimension record (the route_* functions); the public functions here bind them
to HIP2, those of fluid_tangent3d.py to HIP3.

Derivative conventions: fluid_grad's -- that of the expressions as written (floor and integer casts have derivative 0, a clamp of a
coordinate passes its tangent where lo <= x <= hi, bounds included, the interpolation weights are formed from the clamped indices).
Unlike fluid_step's backward the hip route has no one-cell limit: the tangent of the advection is a gather at the forward's own taps, so a
back-trace may move any number of cells.

Hot path and what is not: for k = 1 the renormalisation is smk_tangent_renorm (two launches, no host synchronisation; the norms stay on
the device until the end).  For k > 1 the tangents are re-orthonormalised by modified Gram-Schmidt with fp64 coefficients: with
gram_schmidt="torch" (lyapunov_exponents' default, as before) in plain torch operations, k (k + 1) / 2 reductions and updates per
renormalisation and NOT a hot path; with gram_schmidt="hip" (flow_chaos' default on the hip route) by smk_tangent_orthonormalize
(csrc/tangent_qr.hip: 2 k launches, no host synchronisation, the same rule operation for operation).

Out of scope: torch.func.jvp / torch.autograd.forward_ad through fluid_step itself (call fluid_step_jvp), and the dataset labels (the
`lyapunov_exponent` / `fractal_dimension` / `entropy` of get_chaos_features() and of the datasets stay the reference's proxies; a
labels="flow" dataset mode that would put flow_chaos' quantities there is not built).  The 3-D step is fluid_tangent3d.py."""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.autograd.forward_ad as fwad

from .. import _lib
from .fluid_grad import HIP2, Branches, check_state, simulator, staged_forward

__all__ = ["FlowChaos", "LyapunovResult", "flow_chaos", "fluid_step_jvp", "fluid_step_jvp_rule", "fluid_tangent_rollout",
           "kaplan_yorke_dimension", "ks_entropy", "lyapunov_exponents"]

MAX_K = 8
MAX_PLANES = 65535          # B * T in 2-D, B * T * (D + 1) in 3-D: the launch grids' reach (include/smokehip.h)


# ------------------------------------------------------------------------------------------------ names and shapes, per dimension record
def _jvp_name(dim):
    return f"{dim.name}_jvp"                                   # fluid_step_jvp, fluid_step3d_jvp


def _lyapunov_name(dim):
    return "lyapunov_exponents" + ("" if dim.nd == 2 else f"{dim.nd}d")


def _tangent_names(dim):
    return "(" + ", ".join("t" + f for f in dim.fields) + ")"  # (tu, tv, tp, tdensity)


def _planes(dim, density, T):
    """(what the launch grids count, its value) for a batched density and T tangents per grid."""
    n = density.shape[0] * (T or 1)
    return ("B * T", n) if dim.nd == 2 else ("B * T * (D + 1)", n * (density.shape[1] + 1))


def _check_tangents(dim, state, tangents):
    """-> T, or None where the tangents are state-shaped.  state: checked [B, ...] tensors."""
    what = _jvp_name(dim)
    if len(tangents) != len(dim.fields):
        raise ValueError(f"{what}: tangents are {_tangent_names(dim)}")
    dims = {t.dim() - s.dim() for s, t in zip(state, tangents)}
    if dims not in ({0}, {1}):
        raise ValueError(f"{what}: tangents must all be state-shaped [B, ...] or all [B, T, ...]")
    extra = dims.pop()
    T = None if extra == 0 else int(tangents[0].shape[1])
    for name, s, t in zip(dim.fields, state, tangents):
        want = tuple(s.shape) if T is None else (s.shape[0], T) + tuple(s.shape[1:])
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: the tangent of {name} must be {want}, got {tuple(t.shape)}")
    if T is not None and T < 1:
        raise ValueError(f"{what}: T >= 1")
    counted, n = _planes(dim, state[-1], T)
    if n > MAX_PLANES:
        raise ValueError(f"{what}: {counted} = {n} exceeds {MAX_PLANES}")
    return T


def _batched(dim, state, tangents):
    """Un-batched states (grid-shaped; tangents likewise or [T, ...]) get their leading 1 -> (state, tangents, was batched)."""
    check_state(dim, state)
    if state[-1].dim() == dim.nd + 1:
        return tuple(state), tuple(tangents), True
    return tuple(t[None] for t in state), tuple(t[None] for t in tangents), False


# ------------------------------------------------------------------------------------------------ the rule: forward-mode AD of the step rule
def route_jvp_rule(dim, state, tangents, dt, viscosity, jacobi_iters, branches):
    """fluid_step_jvp_rule / fluid_step3d_jvp_rule: forward_ad over dim.rule."""
    state, tangents, batched = _batched(dim, state, tangents)
    T = _check_tangents(dim, state, tangents)
    if T is not None:
        state = tuple(s[:, None].expand(s.shape[0], T, *s.shape[1:]).contiguous() for s in state)
    with fwad.dual_level():
        duals = [fwad.make_dual(s.detach(), t.detach().to(s.dtype)) for s, t in zip(state, tangents)]
        outs = dim.rule(*duals, dt=dt, viscosity=viscosity, jacobi_iters=jacobi_iters, branches=branches)
        new, tan = [], []
        for o in outs:
            primal, tangent = fwad.unpack_dual(o)
            new.append(primal.detach())
            tan.append(torch.zeros_like(primal) if tangent is None else tangent.detach())
    if T is not None:
        new = [s[:, 0] for s in new]
    if not batched:
        new, tan = [s[0] for s in new], [t[0] for t in tan]
    return tuple(new), tuple(tan)


def fluid_step_jvp_rule(state, tangents, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20,
                        branches: Optional[Branches] = None):
    """(state', tangents') of one step by torch.autograd.forward_ad over fluid_step_rule: any floating dtype, any device.  state
    (u, v, p, density) with leading dimensions [B] (or none); tangents state-shaped, or [B, T, ...]: then the state is expanded along T and
    one pass carries all T tangents (a Branches recorder then holds decisions of that expanded shape).  branches: as fluid_step_rule's."""
    return route_jvp_rule(HIP2, state, tangents, dt, viscosity, jacobi_iters, branches)


# ------------------------------------------------------------------------------------------------ the hip route
def _hip_step(dim, state, tangents, T, dt, viscosity, jacobi_iters):
    """state [B, ...], tangents [B * T, ...] (fp32, on one ROCm device) -> (state', tangents' [B * T, ...])."""
    nd = dim.nd
    B, *grid = state[-1].shape
    dev = state[-1].device
    L = _lib.load()
    advect = getattr(L, dim.tangent[0])
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        # the base state, stage by stage as the differentiable step's forward runs it (fluid_grad.staged_forward: bit-identical to step();
        # a timed-out persistent projection is reported as step() reports it, here and for the tangents below)
        new, kept = staged_forward(dim, simulator(dim, B, grid, dt, viscosity, jacobi_iters, dev), state)
        vel_a, vel_p, d_d = list(new[:nd]), kept[:nd], kept[nd]
        # the tangents' linear stages: the same kernels on a stepper of B * T grids (buoyancy, diffusion and projection are linear and
        # homogeneous in the state, so their tangent is themselves, with the same rounding)
        tsim = simulator(dim, B * T, grid, dt, viscosity, jacobi_iters, dev)
        for name, t in zip(dim.fields, tangents):
            setattr(tsim, name, t)
        tsim.run_stage(dim.stages[0])
        tsim.run_stage(dim.stages[1])
        *tvel_p, tp_n, td_d = tsim.state()

        def advect_tangent(which, field, vel, tfield, tvel):
            out = torch.empty_like(tfield)
            _lib.check(advect(which, *[t.data_ptr() for t in (field, *vel, tfield, *tvel, out)], B, T, *grid, grid[-1], grid[-1] + 1, dt, st))
            return out
        # the advections with the forward's operand wiring: component k <- (c_p[k]; the advected components before it, the projected ones
        # from itself on), then density <- (d_d; the advected components) -- 2-D: u_a <- (u_p; u_p, v_p), v_a <- (v_p; u_a, v_p),
        # density <- (d_d; u_a, v_a).  Each call takes the tangents of its own velocity operands.
        tvel_a = []
        for k in range(nd):
            tvel_a.append(advect_tangent(k, vel_p[k], (*vel_a[:k], *vel_p[k:]), tvel_p[k], (*tvel_a[:k], *tvel_p[k:])))
        td_n = advect_tangent(nd, d_d, vel_a, td_d, tvel_a)
    return new, (*tvel_a, tp_n, td_n)


def _check_hip(state, tangents, jacobi_iters, what):
    _lib.require_cuda(state[-1].device, f"{what}(route='hip')")
    for t in tuple(state) + tuple(tangents):
        if t.dtype != torch.float32 or t.device != state[-1].device:
            raise ValueError(f"{what}(route='hip'): the state and the tangents must be float32 tensors on one device")
    if int(jacobi_iters) < 0:
        raise ValueError(f"{what}: jacobi_iters >= 0")


def route_jvp(dim, state, tangents, dt=0.01, viscosity=0.001, jacobi_iters=20, route="hip"):
    """fluid_step_jvp / fluid_step3d_jvp: the checks, then the rule or the hip route."""
    what = _jvp_name(dim)
    if route == "torch":
        return route_jvp_rule(dim, state, tangents, dt, viscosity, jacobi_iters, None)
    if route != "hip":
        raise ValueError(f"{what}: route is 'hip' or 'torch', got {route!r}")
    state, tangents, batched = _batched(dim, state, tangents)
    T = _check_tangents(dim, state, tangents)
    _check_hip(state, tangents, jacobi_iters, what)
    with torch.no_grad():
        flat = tuple(t.reshape(-1, *t.shape[-dim.nd:]) for t in tangents)
        new, tan = _hip_step(dim, state, flat, T or 1, float(dt), float(viscosity), int(jacobi_iters))
    tan = tuple(t.view(x.shape) for t, x in zip(tan, tangents))
    if not batched:
        new, tan = tuple(s[0] for s in new), tuple(t[0] for t in tan)
    return new, tan


def route_tangent_rollout(dim, state, tangents, n_steps, settings):
    """fluid_tangent_rollout / fluid_tangent_rollout3d: n_steps chained tangent steps."""
    if n_steps < 1:
        raise ValueError(f"fluid_tangent_rollout{'' if dim.nd == 2 else f'{dim.nd}d'}: n_steps >= 1")
    for _ in range(n_steps):
        state, tangents = route_jvp(dim, state, tangents, **settings)
    return state, tangents


def fluid_step_jvp(state, tangents, *, dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip"):
    """One NavierStokesSimulator.step() with the tangent-linear step beside it -> ((u, v, p, density)', (tu, tv, tp, tdensity)').
    state: u [B, H+1, W], v [B, H, W+1], p, density [B, H, W] (or without the B); tangents: state-shaped, or [B, T, ...] for T tangents
    per grid.  route="hip": fp32 ROCm tensors; the returned state is bit-identical to step() on the same state; nothing is saved; no
    one-cell limit.  route="torch": fluid_step_jvp_rule, any dtype and device.  Not differentiable itself (outputs carry no graph)."""
    return route_jvp(HIP2, state, tangents, dt, viscosity, jacobi_iters, route)


def fluid_tangent_rollout(state, tangents, n_steps: int, **settings):
    """n_steps chained fluid_step_jvp calls -> (state, tangents) after the last.  settings: fluid_step_jvp's keywords.  Nothing is kept
    between steps, so memory does not grow with n_steps; the tangents are not renormalised (lyapunov_exponents does that)."""
    return route_tangent_rollout(HIP2, state, tangents, n_steps, settings)


# ------------------------------------------------------------------------------------------------ Lyapunov exponents (Benettin)
@dataclass
class LyapunovResult:
    """exponents [B, k] fp64, per unit time: sum of log_growth / (n_steps * dt), largest first for k > 1 (Gram-Schmidt order).
    log_growth [B, n_renorms, k] fp64: the log of each tangent's norm at each renormalisation.  state: (u, v, p, density) -- in 3-D
    (u, v, w, p, density) -- after the last step; tangents: the k unit (k > 1: orthonormal) tangent states [B, k, ...] after the last
    renormalisation."""
    exponents: torch.Tensor
    log_growth: torch.Tensor
    state: Tuple[torch.Tensor, ...]
    tangents: Tuple[torch.Tensor, ...]


def _dot64(a, b):
    """<a, b> over whole states [B, ...] in fp64 -> [B]."""
    return sum((x.double() * y.double()).flatten(1).sum(dim=1) for x, y in zip(a, b))


def _per_grid(c, x):
    """A per-grid coefficient [B] in x's dtype, shaped to broadcast over x [B, ...]."""
    return c.to(x.dtype).view(-1, *[1] * (x.dim() - 1))


def _gram_schmidt(tangents):
    """Modified Gram-Schmidt over the k tangent states [B, k, ...] with fp64 coefficients -> (orthonormal tangents, norms [B, k] fp64):
    vector j loses its components along the finished vectors 0 .. j-1 one after another, the norm of what remains is its growth.  A zero
    or non-finite remainder is left unscaled.  Plain torch operations: not a hot path."""
    k = tangents[0].shape[1]
    done, norms = [], []
    for j in range(k):
        vec = [t[:, j] for t in tangents]
        for q in done:
            c = _dot64(q, vec)
            vec = [x - _per_grid(c, x) * y for x, y in zip(vec, q)]
        n = _dot64(vec, vec).sqrt()
        norms.append(n)
        ok = (n > 0) & torch.isfinite(n)
        div = torch.where(ok, n, torch.ones_like(n))
        done.append([x / _per_grid(div, x) for x in vec])
    return tuple(torch.stack([q[i] for q in done], dim=1) for i in range(len(tangents))), torch.stack(norms, dim=1)


def _renorm_torch(tangents):
    """k = 1 in torch ops, as smk_tangent_renorm does it: fp64 norm of the whole state, a divide by the norm in the tangents' dtype."""
    n = _dot64([t[:, 0] for t in tangents], [t[:, 0] for t in tangents]).sqrt()
    ok = (n > 0) & torch.isfinite(n)
    div = torch.where(ok, n, torch.ones_like(n))
    return tuple(t / _per_grid(div, t) for t in tangents), n[:, None]


class _HipRenorm:
    """smk_tangent_renorm / smk_tangent3d_renorm on tangents [B, 1, ...] in place -- or, with entry = dim.orthonormalize,
    smk_tangent_orthonormalize / smk_tangent3d_orthonormalize on tangents [B, T, ...] -- its workspace allocated once."""

    def __init__(self, dim, B, T, grid, dev, entry=None):
        self.L, self.dims, self.dev = _lib.load(), (B, T, *grid), dev
        call, query = entry or dim.tangent[1:]
        self.renorm = getattr(self.L, call)
        self.nbytes = int(getattr(self.L, query)(B, T, *grid))
        if self.nbytes < 0:
            counted = "B * k" if dim.nd == 2 else "B * k * (D + 1)"
            raise ValueError(f"{_lyapunov_name(dim)}: B={B}, k={T}, grid {' x '.join(str(n) for n in grid)} is not supported "
                             f"({counted} <= {MAX_PLANES}, 3 <= {dim.axes} <= 32766)")
        self.ws = torch.empty(self.nbytes // 8, dtype=torch.float64, device=dev)

    def __call__(self, tangents, norms):
        W = self.dims[-1]
        tangents = tuple(t if t.is_contiguous() else t.contiguous() for t in tangents)
        with torch.cuda.device(self.dev):
            _lib.check(self.renorm(*[t.data_ptr() for t in tangents], norms.data_ptr(), *self.dims, W, W + 1,
                                   self.ws.data_ptr(), self.nbytes, _lib.stream_ptr(self.dev)))
        return tangents


def _draw_tangent0(state, k, seed):
    """Unit-normal noise for every field, drawn on the CPU from `seed` and copied: independent of the device's generator."""
    g = torch.Generator().manual_seed(int(seed))
    return tuple(torch.randn(s.shape[0], k, *s.shape[1:], generator=g, dtype=torch.float32).to(device=s.device, dtype=s.dtype) for s in state)


def route_lyapunov(dim, state, n_steps, k=1, renorm_every=1, tangent0=None, seed=0, dt=0.01, viscosity=0.001, jacobi_iters=20,
                   route="hip", branches=None, gram_schmidt="torch") -> LyapunovResult:
    """lyapunov_exponents / lyapunov_exponents3d: Benettin's loop over the dimension record."""
    what = _lyapunov_name(dim)
    if route not in ("hip", "torch"):
        raise ValueError(f"{what}: route is 'hip' or 'torch', got {route!r}")
    if gram_schmidt not in ("hip", "torch"):
        raise ValueError(f"{what}: gram_schmidt is 'torch' or 'hip', got {gram_schmidt!r}")
    if gram_schmidt == "hip" and route != "hip":
        raise ValueError(f"{what}: gram_schmidt='hip' goes with route='hip'")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"{what}: 1 <= k <= {MAX_K}, got {k}")
    if n_steps < 1 or renorm_every < 1 or n_steps % renorm_every:
        raise ValueError(f"{what}: n_steps >= 1 and a multiple of renorm_every >= 1")
    if branches is not None and route != "torch":
        raise ValueError(f"{what}: branches goes with route='torch'")
    k = int(k)
    check_state(dim, state)
    batched = state[-1].dim() == dim.nd + 1
    state = tuple(t.detach() if batched else t.detach()[None] for t in state)
    B, *grid = state[-1].shape
    if tangent0 is None:
        tangents = _draw_tangent0(state, k, seed)
    else:
        tangents = tuple(t.detach() if batched else t.detach()[None] for t in tangent0)
        if len(tangents) == len(state) and all(t.dim() == s.dim() for t, s in zip(tangents, state)):
            tangents = tuple(t[:, None] for t in tangents)
        if _check_tangents(dim, state, tangents) != k:
            raise ValueError(f"{what}: tangent0 must hold k = {k} tangents per grid")
        tangents = tuple(t.clone() for t in tangents)
    settings = dict(dt=dt, viscosity=viscosity, jacobi_iters=jacobi_iters)
    n_renorms = n_steps // renorm_every
    hip = route == "hip"
    if hip:
        _check_hip(state, tangents, jacobi_iters, what)
    norms = torch.empty(n_renorms + 1, B, k, dtype=torch.float64, device=state[-1].device)
    if k > 1 and gram_schmidt == "torch":
        def renorm(ts, i):
            ts, norms[i] = _gram_schmidt(ts)
            return ts
    elif hip:                                                # (k = 1: the renorm entry point; the orthonormalisation at T = 1 is the same bits)
        hip_renorm = _HipRenorm(dim, B, k, grid, state[-1].device, dim.orthonormalize if k > 1 else None)

        def renorm(ts, i):
            return hip_renorm(ts, norms[i])
    else:
        def renorm(ts, i):
            ts, norms[i] = _renorm_torch(ts)
            return ts
    with torch.no_grad():
        tangents = renorm(tangents, 0)                       # (the initial scale: not a growth factor)
        for i in range(n_renorms):
            for _ in range(renorm_every):
                if hip:
                    state, tangents = route_jvp(dim, state, tangents, route="hip", **settings)
                else:
                    state, tangents = route_jvp_rule(dim, state, tangents, branches=branches, **settings)
            tangents = renorm(tangents, i + 1)
    if hip:                                                  # the frames leave the steppers: a timed-out projection is reported here
        for batch in sorted({B, B * k}):                     # (by the steppers that can time out: the 3-D one has no check())
            check = getattr(simulator(dim, batch, grid, dt, viscosity, jacobi_iters, state[-1].device), "check", None)
            if check is not None:
                check()
    log_growth = norms[1:].log().permute(1, 0, 2).contiguous()
    exponents = log_growth.sum(dim=1) / (n_steps * float(dt))
    if not batched:
        state, tangents = tuple(s[0] for s in state), tuple(t[0] for t in tangents)
        exponents, log_growth = exponents[0], log_growth[0]
    return LyapunovResult(exponents, log_growth, tuple(state), tuple(tangents))


def lyapunov_exponents(u, v, p, density, n_steps: int, *, k: int = 1, renorm_every: int = 1, tangent0=None, seed: int = 0,
                       dt: float = 0.01, viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip",
                       branches: Optional[Branches] = None, gram_schmidt: str = "torch") -> LyapunovResult:
    """The k largest Lyapunov exponents of the flow from the state (u, v, p, density), by Benettin's method: k tangent states are pushed
    through n_steps tangent-linear steps (fluid_step_jvp) beside the state and renormalised every renorm_every steps (n_steps must be a
    multiple); the exponents are the summed logs of the growth factors per unit time, n_steps * dt.  k = 1: smk_tangent_renorm on the
    hip route.  1 < k <= 8: modified Gram-Schmidt with fp64 coefficients -- gram_schmidt="torch" (the default): in torch operations
    (module docstring: not a hot path); gram_schmidt="hip" (route="hip" only): smk_tangent_orthonormalize, 2 k launches, the same rule.
    tangent0: (tu, tv, tp, tdensity), state-shaped (k = 1) or [B, k, ...]; default: unit-normal noise drawn on the CPU from `seed`.  It is
    normalised (orthonormalised) first, so its scale does not matter.  route="torch": the rule, any dtype and device; branches: a
    Branches recorder / replayer handed to every step of that route (the tests' fp64 run along the fp32 run's decisions).
    The hip route synchronises once, at the end, to check the steppers' status."""
    return route_lyapunov(HIP2, (u, v, p, density), n_steps, k, renorm_every, tangent0, seed, dt, viscosity, jacobi_iters, route, branches,
                          gram_schmidt)


# ------------------------------------------------------------------------------------------------ the spectrum's summaries
@dataclass
class FlowChaos:
    """What the first k Lyapunov exponents say about a flow, per grid (un-batched states: without the B).  exponents [B, k] fp64 per unit
    time, sorted descending; lyapunov [B] = exponents[:, 0]; kaplan_yorke [B]: kaplan_yorke_dimension(exponents), a lower bound where
    truncated [B] (bool) is set -- the partial sums did not turn negative within k; ks_entropy [B]: the sum of the positive exponents
    (Pesin's bound on the Kolmogorov-Sinai entropy); log_growth [B, n_renorms, k]: LyapunovResult's, in Gram-Schmidt order."""
    exponents: torch.Tensor
    lyapunov: torch.Tensor
    kaplan_yorke: torch.Tensor
    ks_entropy: torch.Tensor
    truncated: torch.Tensor
    log_growth: torch.Tensor


def kaplan_yorke_dimension(exponents):
    """The Kaplan-Yorke (Lyapunov) dimension of spectra [..., k] -> (D [...] fp64, truncated [...] bool).  The exponents are sorted
    descending first; with S_j = the sum of the j largest, j* the largest j with S_j >= 0:  D = j* + S_j* / |lambda_(j*+1)|;  D = 0 where
    the largest exponent is negative;  where S_k >= 0 there is no crossing within the k exponents given: D = k and truncated is set -- a
    lower bound.  A spectrum holding a NaN gives NaN."""
    lam = torch.as_tensor(exponents).to(torch.float64).sort(dim=-1, descending=True).values
    k = lam.shape[-1]
    sums = lam.cumsum(dim=-1)
    j = (sums >= 0).sum(dim=-1)                              # (sorted descending, the sums rise and then fall: S_j >= 0 holds on a prefix)
    inside = (j > 0) & (j < k)
    s_j = sums.gather(-1, (j - 1).clamp(0, k - 1)[..., None])[..., 0]
    l_next = lam.gather(-1, j.clamp(0, k - 1)[..., None])[..., 0].abs()
    frac = torch.where(inside, s_j / torch.where(inside, l_next, torch.ones_like(l_next)), torch.zeros_like(s_j))
    dim = j.to(torch.float64) + frac
    return torch.where(torch.isnan(lam).any(dim=-1), torch.full_like(dim, float("nan")), dim), j == k


def ks_entropy(exponents):
    """The sum of the positive exponents of spectra [..., k] -> [...] fp64: Pesin's upper bound on the Kolmogorov-Sinai entropy."""
    return torch.as_tensor(exponents).to(torch.float64).clamp_min(0).sum(dim=-1)


def route_flow_chaos(dim, state, n_steps, k=4, renorm_every=1, seed=0, dt=0.01, viscosity=0.001, jacobi_iters=20, route="hip",
                     gram_schmidt=None) -> FlowChaos:
    """flow_chaos / flow_chaos3d: the spectrum, then the formulas."""
    if gram_schmidt is None:
        gram_schmidt = "hip" if route == "hip" else "torch"
    res = route_lyapunov(dim, state, n_steps, k, renorm_every, None, seed, dt, viscosity, jacobi_iters, route, None, gram_schmidt)
    exponents = res.exponents.sort(dim=-1, descending=True).values
    ky, truncated = kaplan_yorke_dimension(exponents)
    return FlowChaos(exponents, exponents[..., 0], ky, ks_entropy(exponents), truncated, res.log_growth)


def flow_chaos(u, v, p, density, n_steps: int, *, k: int = 4, renorm_every: int = 1, seed: int = 0, dt: float = 0.01,
               viscosity: float = 0.001, jacobi_iters: int = 20, route: str = "hip", gram_schmidt: Optional[str] = None) -> FlowChaos:
    """The dynamical-systems counterparts of the three chaos labels from the state (u, v, p, density): the k largest Lyapunov exponents
    by lyapunov_exponents (same keywords; tangent0 drawn from `seed`) -> FlowChaos: the largest exponent, the Kaplan-Yorke dimension of
    the attractor and the Kolmogorov-Sinai entropy bound.  gram_schmidt: None = "hip" (smk_tangent_orthonormalize) on route="hip",
    "torch" on route="torch"; or either by name.  k exponents bound the dimension by k: see FlowChaos.truncated."""
    return route_flow_chaos(HIP2, (u, v, p, density), n_steps, k, renorm_every, seed, dt, viscosity, jacobi_iters, route, gram_schmidt)
