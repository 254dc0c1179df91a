"""Draws, cases and the oracle of the 3-D flow-map tests (smokephysai_amd/physics/flow_map3d.py).  A plain helper module,
imported by tests/test_flow_map3d_host.py (CPU) and tests/test_hip_flow_map3d.py (device); the 3-D counterpart of flow_map_oracle.py.

Oracle.   The rule in fp32 on the CPU with a Branches recorder, then the same rule in fp64 replaying those branches: the fp64 map along
          the fp32 run's floors and clamp decisions.
Replay.   The fp32 CPU run itself: what fp32 arithmetic costs against the oracle.
Metric.   step_grad_oracle.metric: max|x - ref| / max|ref| per field; where max|ref| == 0 the field must be exactly 0.
Bound.    10 x the replay's worst over the same cases, per quantity."""
import functools

import torch

import step3d_grad_oracle as O3
from flow_map_oracle import DIRECTIONS, DT, J, NU, REPLAY_MARGIN, flow_ftle_oracle          # noqa: F401
from smokephysai_amd.physics import Branches, fluid_rule
from smokephysai_amd.physics.flow_map3d import flow_ftle3d_rule, flow_map_step3d_rule, ftle3d_rule

GRIDS = [(3, 3, 3), (4, 5, 7), (9, 19, 37), (12, 33, 40)]
FAR = ((6, 12, 16), 300.0, 4, 2)                 # shape, amplitude, seed, batch: its traces leave through all six faces
CHAIN_STEPS = (1, 4)
LONG_ROWS = (16, 272, 8)                         # D * H = 4352 > 4096: smk_ftle3d_field's runs exceed 16 rows (17, in 256 groups)


def dataset_like_state3d():
    """(16, 32, 32) from rest with Gaussian balls as flow_map_oracle.dataset_like_state draws its discs: grid 0 one source of intensity
    0.5, grid 1 two sources of intensities 2.0 and 1.2."""
    s = (16, 32, 32)
    d = torch.stack([O3._source(s, 15, 20, 8, 5, 0.5), O3._source(s, 10, 22, 8, 5, 2.0) + O3._source(s, 21, 14, 7, 4, 1.2)])
    return O3._at_rest(d)


def draw_disp3d(shape, batch, amplitude, seed=0, smooth=1):
    """A drawn displacement [batch, 3, D, H, W]: amplitude * (2 rand - 1), `smooth` passes of the 3 x 3 x 3 binomial filter."""
    g = O3._gen(seed + 7, *shape, batch)
    d = amplitude * (2 * torch.rand(batch, 3, *shape, generator=g) - 1)
    for _ in range(smooth):
        d = O3._smooth3(d)
    return d


def quirk_state3d(shape, batch):
    """Uniform velocities of -50: with dt = 0.01 every trace moves half a cell towards the high indices, except on the last index of an
    axis, where the velocity sample itself sits on the last index (it reads 0) and the trace stays there, where the interpolation of the
    displacement reads 0 as well."""
    D, H, W = shape
    z = torch.zeros(batch, D, H, W)
    return (torch.full((batch, D, H + 1, W), -50.0), torch.full((batch, D, H, W + 1), -50.0), torch.full((batch, D + 1, H, W), -50.0), z, z)


def _cid(shape, batch, tag):
    return f"{shape[0]}x{shape[1]}x{shape[2]}-B{batch}-{tag}"


@functools.lru_cache(maxsize=None)
def cases():
    """[(id, state (u, v, w, p, density), disp0)]: every grid with B = 1 and 3 at amplitude 5; the state at rest; the amplitude-300
    state; the last-index quirk.  disp0 is the displacement the single-kernel tests start from."""
    out = []
    for shape in GRIDS:
        for batch in (1, 3):
            out.append((_cid(shape, batch, "a5"), O3.draw_state3d(shape, 5.0, seed=4, batch=batch), draw_disp3d(shape, batch, 1.5)))
    rest = (9, 19, 37)
    out.append((_cid(rest, 1, "rest"), O3._at_rest(torch.zeros(1, *rest)), torch.zeros(1, 3, *rest)))
    shape, amplitude, seed, batch = FAR
    out.append((_cid(shape, batch, "a300"), O3.draw_state3d(shape, amplitude, seed=seed, batch=batch), draw_disp3d(shape, batch, 4.0)))
    out.append((_cid((4, 5, 7), 3, "quirk"), quirk_state3d((4, 5, 7), 3), draw_disp3d((4, 5, 7), 3, 1.0, smooth=0)))
    return out


def leaves_through_all_six_faces(state, dt=DT):
    """Whether the density advection's own back-traces of the state, before their clamp, cross every one of the six faces."""
    u, v, w = state[:3]
    grid = state[4].shape[-3:]
    index = torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in grid], indexing="ij")
    for c, act in zip((u, v, w), (-1, -2, -3)):
        a = index[act] - dt * fluid_rule._sample(c, act, index, fluid_rule._NoBranches)
        if not (bool((a < 0).any()) and bool((a > grid[act] - 1).any())):
            return False
    return True


def map_step3d_oracle(disp, u, v, w, direction, dt=DT):
    """-> (oracle fp64, replay fp32) of one map step."""
    rec = Branches()
    replay = flow_map_step3d_rule(disp, u, v, w, dt=dt, direction=direction, branches=rec)
    oracle = flow_map_step3d_rule(disp.double(), u.double(), v.double(), w.double(), dt=dt, direction=direction, branches=rec.replayer())
    return oracle, replay


def ftle3d_oracle(disp, horizon):
    """-> (oracle fp64, replay fp32) of the FTLE of an fp32 displacement (no decisions to replay)."""
    return ftle3d_rule(disp.double(), horizon), ftle3d_rule(disp, horizon)


def flow_ftle3d_oracle(state, n_steps, direction, rule=flow_ftle3d_rule):
    """-> (oracle FtleResult fp64, replay FtleResult fp32) of the chained run."""
    return flow_ftle_oracle(state, n_steps, direction, rule=rule)


@functools.lru_cache(maxsize=None)
def references(cid):
    """Every oracle and replay the device tests need of one case, computed once and left unchanged:
    {("map_step", direction) | ("ftle_field", "drawn" | "small") | ("flow_ftle", direction, n_steps): (oracle, replay)}."""
    _, state, disp0 = next(c for c in cases() if c[0] == cid)
    refs = {}
    for direction in DIRECTIONS:
        refs["map_step", direction] = map_step3d_oracle(disp0, *state[:3], direction)
        for n_steps in CHAIN_STEPS:
            refs["flow_ftle", direction, n_steps] = flow_ftle3d_oracle(state, n_steps, direction)
    for name, disp, horizon in field_inputs(disp0):
        refs["ftle_field", name] = ftle3d_oracle(disp, horizon)
    return refs


def field_inputs(disp0):
    """The two displacements smk_ftle3d_field is run on per case: the drawn one and 1e-4 of it."""
    return (("drawn", disp0, 0.08), ("small", 1e-4 * disp0, 0.2))
