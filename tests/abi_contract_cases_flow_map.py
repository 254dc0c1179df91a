"""The case table of tests/test_hip_flow_map_abi_contract.py: the stateless entry points of csrc/flow_map.hip -- smk_flow_map_step (both
directions) and smk_ftle_field -- laid out for the guarded arena (tests/guarded_arena.py) the way tests/abi_contract_cases_tangent.py lays
out the tangent's calls.

A field [B][rows][pitch] is an arena buffer of B * rows planes of `columns` elements, a displacement [B][2][H][pitch_m] one of B * 2 * H
planes, `pitch` elements apart (pitch_c = W + 3, pitch_v = W + 1 + 2, pitch_m = W + 5: strictly larger than the rows, so the padding of
every row is guard), every fp32 pointer 4-byte aligned and no better; the fp64 stats and the workspace 8-byte aligned and no better (what
the header asks for), the workspace exactly smk_ftle_workspace(B, H, W) bytes.  reference(): the same entry point on dense, aligned,
separately allocated tensors (abi_contract_cases.dense_reference) -- the call physics.flow_map_step / ftle_field make, held to the fp64
oracle by tests/test_hip_flow_map.py."""
import torch

from abi_contract_cases import F32, F64, Case, _gen, dense_reference
from guarded_arena import Buf

ENTRY_POINTS = ["smk_flow_map_step", "smk_ftle_field"]
B = 2
SHAPES = [(5, 7), (33, 40)]            # one tile with a ragged edge and one run of rows; 5 x 2 tiles and 3 runs, the last of each ragged
DT = 0.1
HORIZON = 0.4


def _pitches(W):
    return W + 3, W + 1 + 2, W + 5


def _draw(shape, seed):
    """u, v (|dt * velocity| up to 2.4 cells, so traces leave the domain) and a displacement of up to 2 cells, as [planes * rows, cols]
    CPU tensors."""
    H, W = shape
    g = _gen(seed, H, W)
    u = 24.0 * (2 * torch.rand(B * (H + 1), W, generator=g) - 1)
    v = 24.0 * (2 * torch.rand(B * H, W + 1, generator=g) - 1)
    disp = 2.0 * (2 * torch.rand(B * 2 * H, W, generator=g) - 1)
    return u, v, disp


def _map_step_case(shape, direction):
    H, W = shape
    pc, pv, pm = _pitches(W)
    bufs = [Buf("u", F32, W, B * (H + 1), pc), Buf("v", F32, W + 1, B * H, pv), Buf("disp_in", F32, W, B * 2 * H, pm),
            Buf("disp_out", F32, W, B * 2 * H, pm, role="out")]

    def inputs():
        u, v, disp = _draw(shape, 110 + direction)
        return {"u": u, "v": v, "disp_in": disp}

    def args(b):
        return [direction, b.ptr("u"), b.ptr("v"), b.ptr("disp_in"), b.ptr("disp_out"), B, H, W, b.stride("u"), b.stride("v"),
                b.stride("disp_in"), DT, b.stream]
    case = Case(f"flow_map_step-{H}x{W}-dir{direction}", "smk_flow_map_step", bufs, args, inputs, lambda: dense_reference(case))
    return case


def _ftle_case(shape):
    H, W = shape
    pm = _pitches(W)[2]
    bufs = [Buf("disp", F32, W, B * 2 * H, pm), Buf("ftle", F32, W, B * H, pm, role="out"), Buf("stats", F64, B * 2, align=8, role="out")]

    def inputs():
        return {"disp": _draw(shape, 120)[2]}

    def args(b):
        return [b.ptr("disp"), b.ptr("ftle"), b.ptr("stats"), B, H, W, b.stride("disp"), HORIZON, *b.workspace(), b.stream]
    case = Case(f"ftle_field-{H}x{W}", "smk_ftle_field", bufs, args, inputs, lambda: dense_reference(case),
                query=lambda lib: lib.smk_ftle_workspace(B, H, W), ws_align=8)
    return case


def all_cases():
    cases = [_map_step_case(shape, direction) for shape in SHAPES for direction in (0, 1)]
    cases += [_ftle_case(shape) for shape in SHAPES]
    return cases
