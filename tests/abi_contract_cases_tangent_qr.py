"""The case table of tests/test_hip_tangent_qr_abi_contract.py: the stateless entry points of csrc/tangent_qr.hip --
smk_tangent_orthonormalize and smk_tangent3d_orthonormalize -- laid out for the guarded arena (tests/guarded_arena.py) the way
tests/abi_contract_cases_tangent.py and tests/abi_contract_cases_tangent3d.py lay out the renorm entry points.

A tangent field [B][T][rows][pitch] (3-D: [B][T][planes][rows][pitch]) is an arena buffer of B * T * rows rows of `columns` elements,
`pitch` elements apart (pitch_c = W + 3, pitch_v = W + 1 + 2: strictly larger than the rows, so the padding of every row is guard), every
fp32 pointer 4-byte aligned and no better; the fp64 norms and the workspace 8-byte aligned and no better (what the header asks for), the
workspace exactly smk_tangent_orthonormalize_workspace(B, T, H, W) / smk_tangent3d_orthonormalize_workspace(B, T, D, H, W) bytes.  The four
or five fields are "inout": copied in, orthonormalised in place.  reference(): the same entry point on dense, aligned, separately allocated
tensors (abi_contract_cases.dense_reference) -- the call physics.lyapunov_exponents(gram_schmidt="hip") makes, held to the fp64 oracle by
tests/test_hip_tangent_qr.py."""
import torch

from abi_contract_cases import F32, F64, Case, _gen, dense_reference
from guarded_arena import Buf

ENTRY_POINTS = ["smk_tangent_orthonormalize", "smk_tangent3d_orthonormalize"]
B, T = 2, 3
SHAPE_2D, SHAPE_3D = (5, 7), (3, 4, 5)


def _pitches(W):
    return W + 3, W + 1 + 2


def _layout(shape):
    """[(name, rows per state, columns, pitch)] of a state's fields in the entry point's order."""
    W = shape[-1]
    pc, pv = _pitches(W)
    if len(shape) == 2:
        H = shape[0]
        return [("tu", H + 1, W, pc), ("tv", H, W + 1, pv), ("tp", H, W, pc), ("td", H, W, pc)]
    D, H = shape[:2]
    return [("tu", D * (H + 1), W, pc), ("tv", D * H, W + 1, pv), ("tw", (D + 1) * H, W, pc), ("tp", D * H, W, pc), ("td", D * H, W, pc)]


def _case(shape):
    lay = _layout(shape)
    names = [name for name, *_ in lay]
    entry = ENTRY_POINTS[len(shape) - 2]
    bufs = [Buf(name, F32, cols, B * T * rows, pitch, role="inout") for name, rows, cols, pitch in lay]
    bufs.append(Buf("norms", F64, B * T, align=8, role="out"))

    def inputs():
        g = _gen(95, *shape)
        scale = {"tu": 3.0, "tp": 0.25}                  # fields of different weight, vectors of different length
        return {name: scale.get(name, 1.0) * torch.randn(B * T * rows, cols, generator=g) for name, rows, cols, _ in lay}

    def args(b):
        return [*[b.ptr(n) for n in names], b.ptr("norms"), B, T, *shape, b.stride("tu"), b.stride("tv"), *b.workspace(), b.stream]
    case = Case(f"{entry[4:]}-{'x'.join(str(n) for n in shape)}", entry, bufs, args, inputs, lambda: dense_reference(case),
                query=lambda lib: getattr(lib, entry + "_workspace")(B, T, *shape), ws_align=8)
    return case


def all_cases():
    return [_case(SHAPE_2D), _case(SHAPE_3D)]
