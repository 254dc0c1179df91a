"""Draws, cases and the oracle of the flow-map tests (smokephysai_amd/physics/flow_map.py).  A plain helper module,
imported by tests/test_flow_map_host.py (CPU) and tests/test_hip_flow_map.py (device).

Oracle.   The rule in fp32 on the CPU with a Branches recorder, then the same rule in fp64 replaying those branches: the fp64 map along
          the fp32 run's floors and clamp decisions (tests/step_grad_oracle.py says why a free-running fp64 rule is the wrong yardstick).
Replay.   The fp32 CPU run itself: what fp32 arithmetic costs against the oracle.
Metric.   step_grad_oracle.metric: max|x - ref| / max|ref| per field; where max|ref| == 0 the field must be exactly 0.
Bound.    10 x the replay's worst over the same cases, per quantity."""
import functools

import torch

import step_grad_oracle as O
from smokephysai_amd.physics import Branches
from smokephysai_amd.physics.flow_map import flow_ftle_rule, flow_map_step_rule, ftle_rule

REPLAY_MARGIN = 10.0
DT, NU, J = 0.01, 0.001, 20
DIRECTIONS = ("backward", "forward")
GRIDS = [(3, 3), (4, 5), (12, 33), (9, 37), (64, 64)]


def dataset_like_state(batch=2):
    """64 x 64 from rest with the kind of sources draw_source_configs draws: grid 0 one source, grid 1 three (intensities 0.5 .. 2.0)."""
    H = W = 64
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")

    def source(x, y, radius, intensity):
        dist = torch.sqrt(((xx - x) ** 2 + (yy - y) ** 2).float())
        return torch.where(dist <= radius, intensity * torch.exp(-(dist * dist) / (2 * (radius / 3) ** 2)), torch.zeros(()))
    d = torch.stack([source(30, 40, 8, 0.5), source(20, 44, 8, 2.0) + source(41, 30, 6, 1.2) + source(30, 18, 10, 0.8)][:batch])
    return torch.zeros(batch, H + 1, W), torch.zeros(batch, H, W + 1), torch.zeros(batch, H, W), d


def draw_disp(shape, batch, amplitude, seed=0, smooth=1):
    """A drawn displacement field [batch, 2, H, W]: amplitude * (2 rand - 1), `smooth` passes of the 3 x 3 binomial filter."""
    g = O._gen(seed + 7, *shape, batch)
    d = amplitude * (2 * torch.rand(batch, 2, *shape, generator=g) - 1)
    for _ in range(smooth):
        d = O._smooth(d)
    return d


def quirk_state(shape, batch):
    """Uniform velocities of -50: with dt = 0.01 every trace moves half a cell towards the high indices, except on the last row and
    column, where the velocity sample itself sits on the last index (x0 == x1: it reads 0) and the trace stays on the last index, where
    the interpolation of the displacement reads 0 as well."""
    H, W = shape
    return torch.full((batch, H + 1, W), -50.0), torch.full((batch, H, W + 1), -50.0), torch.zeros(batch, H, W), torch.zeros(batch, H, W)


@functools.lru_cache(maxsize=None)
def cases():
    """[(id, state (u, v, p, density), disp0)]: every grid with B = 1 and 3 at amplitude 5; the state at rest; an amplitude-300 state
    whose traces leave the domain on all four sides; the last-index quirk.  disp0 is the displacement the single-kernel tests start from."""
    out = []
    for shape in GRIDS:
        for batch in (1, 3):
            out.append((f"{shape[0]}x{shape[1]}-B{batch}-a5", O.draw_state(shape, 5.0, seed=4, batch=batch), draw_disp(shape, batch, 1.5)))
    H, W = 9, 37
    rest = (torch.zeros(1, H + 1, W), torch.zeros(1, H, W + 1), torch.zeros(1, H, W), torch.zeros(1, H, W))
    out.append(("9x37-B1-rest", rest, torch.zeros(1, 2, H, W)))
    far = O.draw_state((12, 33), 300.0, seed=3, batch=3)
    out.append(("12x33-B3-a300", far, draw_disp((12, 33), 3, 4.0)))
    out.append(("4x5-B3-quirk", quirk_state((4, 5), 3), draw_disp((4, 5), 3, 1.0, smooth=0)))
    return out


def leaves_on_all_sides(state, dt=DT):
    """Whether back-traces of the state's own velocities (a bound: samples are convex combinations) cross all four sides."""
    u, v = state[0], state[1]
    return bool((dt * u[..., :, 0] > 0.5).any() and (dt * u[..., :, -1] < -0.5).any() and
                (dt * v[..., 0, :] > 0.5).any() and (dt * v[..., -1, :] < -0.5).any())


def map_step_oracle(disp, u, v, direction, dt=DT):
    """-> (oracle fp64, replay fp32) of one map step."""
    rec = Branches()
    replay = flow_map_step_rule(disp, u, v, dt=dt, direction=direction, branches=rec)
    oracle = flow_map_step_rule(disp.double(), u.double(), v.double(), dt=dt, direction=direction, branches=rec.replayer())
    return oracle, replay


def ftle_oracle(disp, horizon):
    """-> (oracle fp64, replay fp32) of the FTLE of an fp32 displacement field (no decisions to replay)."""
    return ftle_rule(disp.double(), horizon), ftle_rule(disp, horizon)


def flow_ftle_oracle(state, n_steps, direction, dt=DT, viscosity=NU, jacobi_iters=J, rule=flow_ftle_rule):
    """-> (oracle FtleResult fp64, replay FtleResult fp32) of the chained run."""
    rec = Branches()
    kw = dict(dt=dt, viscosity=viscosity, jacobi_iters=jacobi_iters, direction=direction)
    replay = rule(*state, n_steps, branches=rec, **kw)
    oracle = rule(*[s.double() for s in state], n_steps, branches=rec.replayer(), **kw)
    return oracle, replay
