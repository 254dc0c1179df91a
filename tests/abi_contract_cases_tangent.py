"""The case table of tests/test_hip_tangent_abi_contract.py: the stateless entry points of csrc/fluid_tangent.hip -- smk_advect_tangent and
smk_tangent_renorm -- laid out for the guarded arena (tests/guarded_arena.py) the way tests/abi_contract_cases_fluid_grad.py lays out the
adjoint's calls.

A base field [B][rows][pitch] is an arena buffer of B * rows planes of `columns` elements, a tangent field [B][T][rows][pitch] one of
B * T * rows planes, `pitch` elements apart (pitch_c = W + 3, pitch_v = W + 1 + 2: strictly larger than the rows, so the padding of every
row is guard), every fp32 pointer 4-byte aligned and no better; the fp64 norms and the workspace 8-byte aligned and no better (what the
header asks for), the workspace exactly smk_tangent_renorm_workspace(B, T, H, W) bytes.  The four fields of smk_tangent_renorm are
"inout": copied in, divided in place.  reference(): the same entry point on dense, aligned, separately allocated tensors
(abi_contract_cases.dense_reference) -- the call physics.fluid_step_jvp / lyapunov_exponents make, held to the fp64 oracle by
tests/test_hip_fluid_tangent.py."""
import torch

from abi_contract_cases import F32, F64, Case, _gen, dense_reference
from guarded_arena import Buf

ENTRY_POINTS = ["smk_advect_tangent", "smk_tangent_renorm"]
B, T = 2, 2
SHAPES = [(5, 7), (33, 40)]            # one tile with a ragged edge; 5 x 2 tiles, the last of each axis ragged
DT = 0.1


def _pitches(W):
    return W + 3, W + 1 + 2


def _field(name, rows, cols, pitch, role="in", planes=B):
    return Buf(name, F32, cols, planes * rows, pitch, role=role)


def _dims(shape, which):
    H, W = shape
    pc, pv = _pitches(W)
    return ((H + 1, W, pc), (H, W + 1, pv), (H, W, pc))[which]


def _draw(shape, seed):
    """u, v (|dt * velocity| up to 2.4 cells: there is no one-cell limit here), density, and the tangents of the three and of p, as
    [planes * rows, cols] CPU tensors."""
    H, W = shape
    g = _gen(seed, H, W)
    u = 24.0 * (2 * torch.rand(B * (H + 1), W, generator=g) - 1)
    v = 24.0 * (2 * torch.rand(B * H, W + 1, generator=g) - 1)
    d = torch.rand(B * H, W, generator=g) ** 4 * 2
    tu, tv = torch.randn(B * T * (H + 1), W, generator=g), torch.randn(B * T * H, W + 1, generator=g)
    tp, td = torch.randn(B * T * H, W, generator=g), torch.randn(B * T * H, W, generator=g)
    return u, v, d, tu, tv, tp, td


def _advect_case(shape, which):
    H, W = shape
    pc, pv = _pitches(W)
    rows, cols, pitch = _dims(shape, which)
    bufs = [_field("field", rows, cols, pitch), _field("u", H + 1, W, pc), _field("v", H, W + 1, pv),
            _field("tfield", rows, cols, pitch, planes=B * T), _field("tu", H + 1, W, pc, planes=B * T),
            _field("tv", H, W + 1, pv, planes=B * T), _field("tout", rows, cols, pitch, "out", planes=B * T)]

    def inputs():
        u, v, d, tu, tv, _, td = _draw(shape, 80 + which)
        return {"field": (u, v, d)[which].clone(), "u": u, "v": v, "tfield": (tu, tv, td)[which].clone(), "tu": tu, "tv": tv}

    def args(b):
        return [which, b.ptr("field"), b.ptr("u"), b.ptr("v"), b.ptr("tfield"), b.ptr("tu"), b.ptr("tv"), b.ptr("tout"),
                B, T, H, W, b.stride("u"), b.stride("v"), DT, b.stream]
    case = Case(f"advect_tangent-{H}x{W}-which{which}", "smk_advect_tangent", bufs, args, inputs, lambda: dense_reference(case))
    return case


def _renorm_case(shape):
    H, W = shape
    pc, pv = _pitches(W)
    bufs = [_field("tu", H + 1, W, pc, "inout", B * T), _field("tv", H, W + 1, pv, "inout", B * T), _field("tp", H, W, pc, "inout", B * T),
            _field("td", H, W, pc, "inout", B * T), Buf("norms", F64, B * T, align=8, role="out")]

    def inputs():
        _, _, _, tu, tv, tp, td = _draw(shape, 90)
        return {"tu": 3.0 * tu, "tv": tv, "tp": 0.25 * tp, "td": td}

    def args(b):
        return [b.ptr("tu"), b.ptr("tv"), b.ptr("tp"), b.ptr("td"), b.ptr("norms"), B, T, H, W, b.stride("tu"), b.stride("tv"),
                *b.workspace(), b.stream]
    case = Case(f"tangent_renorm-{H}x{W}", "smk_tangent_renorm", bufs, args, inputs, lambda: dense_reference(case),
                query=lambda lib: lib.smk_tangent_renorm_workspace(B, T, H, W), ws_align=8)
    return case


def all_cases():
    cases = [_advect_case(shape, which) for shape in SHAPES for which in (0, 1, 2)]
    cases += [_renorm_case(shape) for shape in SHAPES]
    return cases
