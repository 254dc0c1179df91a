"""The case table of tests/test_hip_abi_contract_fluid_grad.py: the stateless entry points of csrc/fluid_grad.hip -- smk_advect_backward,
smk_project_backward, smk_buoy_diffuse_backward -- laid out for the guarded arena (tests/guarded_arena.py) the way
tests/abi_contract_cases.py lays out its calls.

A field [B][rows][pitch] is an arena buffer of B * rows planes of `columns` elements, `pitch` elements apart (pitch_c = W + 3,
pitch_v = W + 1 + 2: strictly larger than the rows, so the padding of every row is guard), every pointer 4-byte aligned and no better (the
header asks for nothing more, so there is no weaker alignment to refuse), the projection's workspace exactly
smk_project_backward_workspace(B, H, W) bytes.  reference(): the same entry point on dense, aligned, separately allocated tensors
(abi_contract_cases.dense_reference) -- the call physics.fluid_step's backward makes, held to the fp64 oracle by
tests/test_hip_fluid_grad.py."""
import torch

from abi_contract_cases import F32, I32, Case, _gen, dense_reference
from guarded_arena import Buf

ENTRY_POINTS = ["smk_advect_backward", "smk_project_backward", "smk_buoy_diffuse_backward"]
B = 2
SHAPES = [(5, 7), (33, 40)]            # one tile with a ragged edge; 5 x 2 tiles, the last of each axis ragged
DT, VISCOSITY = 0.1, 0.001


def _pitches(W):
    return W + 3, W + 1 + 2


def _field(name, rows, cols, pitch, role="in"):
    return Buf(name, F32, cols, B * rows, pitch, role=role)


def _draw(shape, seed):
    """u, v (|dt * velocity| <= 0.6: under the one-cell limit), density, and three upstream gradients, as [B * rows, cols] CPU tensors."""
    H, W = shape
    g = _gen(seed, H, W)
    u = 6.0 * (2 * torch.rand(B * (H + 1), W, generator=g) - 1)
    v = 6.0 * (2 * torch.rand(B * H, W + 1, generator=g) - 1)
    d = torch.rand(B * H, W, generator=g) ** 4 * 2
    return u, v, d, torch.randn(B * (H + 1), W, generator=g), torch.randn(B * H, W + 1, generator=g), torch.randn(B * H, W, generator=g)


def _advect_case(shape, which):
    H, W = shape
    pc, pv = _pitches(W)
    rows, cols, pitch = ((H + 1, W, pc), (H, W + 1, pv), (H, W, pc))[which]
    bufs = [_field("field", rows, cols, pitch), _field("u", H + 1, W, pc), _field("v", H, W + 1, pv), _field("gout", rows, cols, pitch),
            _field("dfield", rows, cols, pitch, "out"), _field("du", H + 1, W, pc, "out"), _field("dv", H, W + 1, pv, "out"),
            Buf("far", I32, B, role="out")]

    def inputs():
        u, v, d, gu, gv, gd = _draw(shape, 50 + which)
        return {"field": (u, v, d)[which].clone(), "u": u, "v": v, "gout": (gu, gv, gd)[which]}

    def args(b):
        return [which, b.ptr("field"), b.ptr("u"), b.ptr("v"), b.ptr("gout"), b.ptr("dfield"), b.ptr("du"), b.ptr("dv"), b.ptr("far"),
                B, H, W, b.stride("u"), b.stride("v"), DT, b.stream]
    case = Case(f"advect_backward-{H}x{W}-which{which}", "smk_advect_backward", bufs, args, inputs, lambda: dense_reference(case))
    return case


def _project_case(shape, J):
    H, W = shape
    pc, pv = _pitches(W)
    bufs = [_field("gu", H + 1, W, pc), _field("gv", H, W + 1, pv), _field("gp", H, W, pc),
            _field("du", H + 1, W, pc, "out"), _field("dv", H, W + 1, pv, "out"), _field("dp", H, W, pc, "out")]

    def inputs():
        _, _, _, gu, gv, gp = _draw(shape, 60 + J)
        return {"gu": gu, "gv": gv, "gp": gp}

    def args(b):
        return [b.ptr("gu"), b.ptr("gv"), b.ptr("gp"), b.ptr("du"), b.ptr("dv"), b.ptr("dp"), B, H, W, b.stride("gu"), b.stride("gv"), J,
                0.01, *b.workspace(), b.stream]
    case = Case(f"project_backward-{H}x{W}-J{J}", "smk_project_backward", bufs, args, inputs, lambda: dense_reference(case),
                query=lambda lib: lib.smk_project_backward_workspace(B, H, W))
    return case


def _buoy_diffuse_case(shape):
    H, W = shape
    pc, pv = _pitches(W)
    bufs = [_field("gu", H + 1, W, pc), _field("gv", H, W + 1, pv), _field("gd", H, W, pc),
            _field("du", H + 1, W, pc, "out"), _field("dv", H, W + 1, pv, "out"), _field("dd", H, W, pc, "out")]

    def inputs():
        _, _, _, gu, gv, gd = _draw(shape, 70)
        return {"gu": gu, "gv": gv, "gd": gd}

    def args(b):
        return [b.ptr("gu"), b.ptr("gv"), b.ptr("gd"), b.ptr("du"), b.ptr("dv"), b.ptr("dd"), B, H, W, b.stride("gu"), b.stride("gv"),
                DT, VISCOSITY, b.stream]
    case = Case(f"buoy_diffuse_backward-{H}x{W}", "smk_buoy_diffuse_backward", bufs, args, inputs, lambda: dense_reference(case))
    return case


def all_cases():
    cases = [_advect_case(shape, which) for shape in SHAPES for which in (0, 1, 2)]
    cases += [_project_case(shape, J) for shape in SHAPES for J in (0, 3)]
    cases += [_buoy_diffuse_case(shape) for shape in SHAPES]
    return cases
