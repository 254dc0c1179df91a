"""Bit-identity guard of the fluid step's derivative kernels (csrc/fluid_grad.hip, fluid_tangent.hip, fluid_grad3d.hip and the Python route
in front of them): the sha256 of the raw output bytes of the calls below equals what the build before csrc/fluid_trace.h and the shared
hip route gave (tests/fluid_derivative_bits_parent.json, recorded on an MI355X by running this file as a script at that commit).  The
kernels sum in one fixed order without atomics, so their bits are a property of the source, not of the run.

Inputs are drawn on the CPU by the oracles' own draw_state / draw_upstream with B = 2 (tangent k: draw_upstream with seed k).  Shapes: a grid
smaller than the 32 x 8 tile, and one with more than one tile and a remainder on both axes."""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step3d_grad_oracle as O3                                                                       # noqa: E402
import step_grad_oracle as O2                                                                         # noqa: E402
from smokephysai_amd import _lib                                                                      # noqa: E402
from smokephysai_amd.physics import fluid_step, fluid_step3d                                          # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "fluid_derivative_bits_parent.json")
SHAPES2 = ((5, 7), (33, 40))
SHAPES3 = ((4, 5, 7), (9, 19, 37))
DT, AMPLITUDE2, AMPLITUDE3, T = 0.01, 60.0, 50.0, 3          # the oracles' first regime: no back-trace is far


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _ptrs(*tensors):
    return [t.data_ptr() for t in tensors]


def _tangents(state, dev):
    """[B, T, ...] per field: tangent k is draw_upstream(state, seed=k)."""
    ups = [O2.draw_upstream(state, seed=k) for k in range(T)]
    return [torch.stack([ups[k][i] for k in range(T)], dim=1).contiguous().to(dev) for i in range(4)]


def _whole_step(step, state, ups, dev, J):
    leaves = [t.to(dev).requires_grad_(True) for t in state]
    out = step(*leaves, dt=DT, viscosity=0.001, jacobi_iters=J)
    grads = torch.autograd.grad(out, leaves, [g.to(dev) for g in ups])
    return _digest(*out, *grads)


def compute_digests():
    dev = torch.device("cuda:0")
    L, st, out = _lib.load(), _lib.stream_ptr(dev), {}
    for H, W in SHAPES2:
        cpu = O2.draw_state((H, W), AMPLITUDE2)
        B = cpu[3].shape[0]
        u, v, p, d = state = [t.to(dev) for t in cpu]
        gs = [g.to(dev) for g in O2.draw_upstream(cpu)]
        ts = _tangents(cpu, dev)
        dims = (H, W, W, W + 1)
        for which, i in enumerate((0, 1, 3)):
            df, du, dv, far = torch.empty_like(state[i]), torch.empty_like(u), torch.empty_like(v), torch.empty(B, dtype=torch.int32, device=dev)
            _lib.check(L.smk_advect_backward(which, *_ptrs(state[i], u, v, gs[i], df, du, dv, far), B, *dims, DT, st))
            out[f"smk_advect_backward/{H}x{W}/which{which}"] = _digest(df, du, dv, far)
            tout = torch.empty_like(ts[i])
            _lib.check(L.smk_advect_tangent(which, *_ptrs(state[i], u, v, ts[i], ts[0], ts[1], tout), B, T, *dims, DT, st))
            out[f"smk_advect_tangent/{H}x{W}/which{which}"] = _digest(tout)
    nbytes = int(L.smk_tangent_renorm_workspace(B, T, H, W))              # (the last shape: 33 x 40)
    ws, norms = torch.empty(nbytes // 8, dtype=torch.float64, device=dev), torch.empty(B, T, dtype=torch.float64, device=dev)
    _lib.check(L.smk_tangent_renorm(*_ptrs(*ts, norms), B, T, *dims, ws.data_ptr(), nbytes, st))
    out[f"smk_tangent_renorm/{H}x{W}"] = _digest(*ts, norms)
    out[f"fluid_step/{H}x{W}/J5"] = _whole_step(fluid_step, cpu, O2.draw_upstream(cpu), dev, 5)
    for shape in SHAPES3:
        cpu = O3.draw_state3d(shape, AMPLITUDE3)
        out["fluid_step3d/" + "x".join(map(str, shape)) + "/J3"] = _whole_step(fluid_step3d, cpu, O3.draw_upstream3d(cpu), dev, 3)
    return out


@pytest.mark.gpu
def test_the_derivative_kernels_give_the_recorded_bits():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = compute_digests()
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}


if __name__ == "__main__":
    print(json.dumps(compute_digests(), indent=1, sort_keys=True))
