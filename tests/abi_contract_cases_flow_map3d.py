"""The case table of tests/test_hip_flow_map3d_abi_contract.py: the stateless entry points of csrc/flow_map3d.hip -- smk_flow_map3d_step
(both directions) and smk_ftle3d_field -- laid out for the guarded arena (tests/guarded_arena.py) the way
tests/abi_contract_cases_flow_map.py lays out the 2-D calls.

A field [B][planes][rows][pitch] is an arena buffer of B * planes * rows rows of `columns` elements, a displacement
[B][3][D][H][pitch_m] one of B * 3 * D * H rows, `pitch` elements apart (pitch_c = W + 3, pitch_v = W + 1 + 2, pitch_m = W + 5: strictly
larger than the rows, so the padding of every row is guard), every fp32 pointer 4-byte aligned and no better; the fp64 stats and the
workspace 8-byte aligned and no better (what the header asks for), the workspace exactly smk_ftle3d_workspace(B, D, H, W) bytes.
reference(): the same entry point on dense, aligned, separately allocated tensors (abi_contract_cases.dense_reference) -- the call
physics.flow_map_step3d / ftle_field3d make, held to the fp64 oracle by tests/test_hip_flow_map3d.py."""
import torch

from abi_contract_cases import F32, F64, Case, _gen, dense_reference
from guarded_arena import Buf

ENTRY_POINTS = ["smk_flow_map3d_step", "smk_ftle3d_field"]
B = 2
SHAPES = [(4, 5, 7), (6, 19, 37)]      # one ragged tile per plane and two runs of rows; 2 x 3 tiles per plane and 8 runs, the last of each ragged
DT = 0.1
HORIZON = 0.4


def _pitches(W):
    return W + 3, W + 1 + 2, W + 5


def _draw(shape, seed):
    """u, v, w (|dt * velocity| up to 2.4 cells, so traces leave the domain) and a displacement of up to 2 cells, as [rows, cols] CPU
    tensors."""
    D, H, W = shape
    g = _gen(seed, D, H, W)
    u = 24.0 * (2 * torch.rand(B * D * (H + 1), W, generator=g) - 1)
    v = 24.0 * (2 * torch.rand(B * D * H, W + 1, generator=g) - 1)
    w = 24.0 * (2 * torch.rand(B * (D + 1) * H, W, generator=g) - 1)
    disp = 2.0 * (2 * torch.rand(B * 3 * D * H, W, generator=g) - 1)
    return u, v, w, disp


def _map_step_case(shape, direction):
    D, H, W = shape
    pc, pv, pm = _pitches(W)
    bufs = [Buf("u", F32, W, B * D * (H + 1), pc), Buf("v", F32, W + 1, B * D * H, pv), Buf("w", F32, W, B * (D + 1) * H, pc),
            Buf("disp_in", F32, W, B * 3 * D * H, pm), Buf("disp_out", F32, W, B * 3 * D * H, pm, role="out")]

    def inputs():
        u, v, w, disp = _draw(shape, 130 + direction)
        return {"u": u, "v": v, "w": w, "disp_in": disp}

    def args(b):
        return [direction, b.ptr("u"), b.ptr("v"), b.ptr("w"), b.ptr("disp_in"), b.ptr("disp_out"), B, D, H, W, b.stride("u"),
                b.stride("v"), b.stride("disp_in"), DT, b.stream]
    case = Case(f"flow_map3d_step-{D}x{H}x{W}-dir{direction}", "smk_flow_map3d_step", bufs, args, inputs, lambda: dense_reference(case))
    return case


def _ftle_case(shape):
    D, H, W = shape
    pm = _pitches(W)[2]
    bufs = [Buf("disp", F32, W, B * 3 * D * H, pm), Buf("ftle", F32, W, B * D * H, pm, role="out"),
            Buf("stats", F64, B * 2, align=8, role="out")]

    def inputs():
        return {"disp": _draw(shape, 140)[3]}

    def args(b):
        return [b.ptr("disp"), b.ptr("ftle"), b.ptr("stats"), B, D, H, W, b.stride("disp"), HORIZON, *b.workspace(), b.stream]
    case = Case(f"ftle3d_field-{D}x{H}x{W}", "smk_ftle3d_field", bufs, args, inputs, lambda: dense_reference(case),
                query=lambda lib: lib.smk_ftle3d_workspace(B, D, H, W), ws_align=8)
    return case


def all_cases():
    cases = [_map_step_case(shape, direction) for shape in SHAPES for direction in (0, 1)]
    cases += [_ftle_case(shape) for shape in SHAPES]
    return cases
