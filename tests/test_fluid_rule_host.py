"""CPU checks that hold the N-d step rule (smokephysai_amd/physics/fluid_rule.py) honest as ONE rule for 2-D and 3-D: from a drawn state
on grids with a different extent on every axis -- the smallest shapes where an axis mix-up shows -- one step equals oracle/ns_nd.py's bit for
bit in fp32, and a Branches log recorded in fp32 is consumed exactly by the fp64 run, entry for entry."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step3d_grad_oracle as O3                                                                       # noqa: E402
import step_grad_oracle as O2                                                                         # noqa: E402
from oracle.ns_nd import OracleNSnd                                                                   # noqa: E402
from smokephysai_amd.physics import fluid_rule                                                        # noqa: E402

SHAPES = [(3, 4), (5, 7), (3, 4, 5), (4, 5, 7)]
SETTINGS = dict(dt=0.1, viscosity=0.001, jacobi_iters=3)
AMPLITUDE = 6.0                   # times dt: back-traces of more than half a cell, into the clamps at these sizes


def _draw(shape):
    return (O2.draw_state if len(shape) == 2 else O3.draw_state3d)(shape, AMPLITUDE)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_step_from_a_drawn_state_is_the_nd_oracles_bit_for_bit(shape):
    state = _draw(shape)
    got = fluid_rule.step(state, SETTINGS["dt"], SETTINGS["viscosity"], SETTINGS["jacobi_iters"])
    names = ("u", "v", "w")[:len(shape)] + ("p", "density")
    for b in range(state[-1].shape[0]):
        o = OracleNSnd(shape, **SETTINGS)
        for name, t in zip(names, state):
            assert getattr(o, name).shape == tuple(t[b].shape), name
            setattr(o, name, t[b].numpy().copy())
        o.step()
        for name, t in zip(names, got):
            assert np.array_equal(t[b].numpy().view(np.int32), getattr(o, name).view(np.int32)), (shape, b, name)
    assert not torch.equal(got[0], state[0]) and not torch.equal(got[-1], state[-1])                  # (something moved)


@pytest.mark.parametrize("shape", SHAPES[1::2], ids=lambda s: "x".join(map(str, s)))
def test_a_branch_log_recorded_in_fp32_replays_through_fp64_entry_for_entry(shape):
    nd, state = len(shape), _draw(shape)
    rec = fluid_rule.Branches()
    fluid_rule.step(state, branches=rec, **SETTINGS)
    # per advection: nd sample coordinates for each of nd components and nd back-trace coordinates are clamped, nd + 1 interpolations
    # floor nd coordinates each; a step has nd + 1 advections
    assert len(rec.log) == (nd + 1) * (nd * nd + nd + (nd + 1) * nd)
    rep = rec.replayer()
    out = fluid_rule.step(tuple(t.double() for t in state), branches=rep, **SETTINGS)
    assert rep.pos == len(rec.log) and len(rep.log) == len(rec.log)
    assert all(o.dtype == torch.float64 for o in out)
