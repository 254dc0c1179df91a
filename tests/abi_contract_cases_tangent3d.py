"""The case table of tests/test_hip_tangent3d_abi_contract.py: the stateless entry points of csrc/fluid_tangent3d.hip --
smk_advect3d_tangent and smk_tangent3d_renorm -- laid out for the guarded arena (tests/guarded_arena.py) the way
tests/abi_contract_cases_tangent.py lays out the 2-D two and tests/abi_contract_cases_fluid_grad3d.py the 3-D adjoint's.

A base field [B][planes][rows][pitch] is an arena buffer of B * planes * rows rows of `columns` elements, a tangent field
[B][T][planes][rows][pitch] one of B * T * planes * rows rows, `pitch` elements apart (pitch_c = W + 3, pitch_v = W + 1 + 2: strictly
larger than the rows, so the padding of every row is guard), every fp32 pointer 4-byte aligned and no better; the fp64 norms and the
workspace 8-byte aligned and no better (what the header asks for), the workspace exactly smk_tangent3d_renorm_workspace(B, T, D, H, W)
bytes.  The five fields of smk_tangent3d_renorm are "inout": copied in, divided in place.  reference(): the same entry point on dense,
aligned, separately allocated tensors (abi_contract_cases.dense_reference) -- the call physics.fluid_step3d_jvp / lyapunov_exponents3d
make, held to the fp64 oracle by tests/test_hip_fluid_tangent3d.py."""
import torch

from abi_contract_cases import F32, F64, Case, _gen, dense_reference
from guarded_arena import Buf

ENTRY_POINTS = ["smk_advect3d_tangent", "smk_tangent3d_renorm"]
B, T = 2, 2
SHAPES = [(4, 5, 7), (6, 19, 37)]      # one tile with a ragged edge; 3 x 2 tiles per plane, the last of each axis ragged
DT = 0.1


def _pitches(W):
    return W + 3, W + 1 + 2


def _layout(shape):
    """{name: (planes * rows, columns, pitch)} of u, v, w and a cell field."""
    D, H, W = shape
    pc, pv = _pitches(W)
    return {"u": (D * (H + 1), W, pc), "v": (D * H, W + 1, pv), "w": ((D + 1) * H, W, pc), "c": (D * H, W, pc)}


def _field(name, lay, role="in", grids=B):
    rows, cols, pitch = lay
    return Buf(name, F32, cols, grids * rows, pitch, role=role)


def _sid(shape):
    return "x".join(str(s) for s in shape)


def _draw(shape, seed):
    """u, v, w (|dt * velocity| up to 2.4 cells: there is no one-cell limit here), density, and the tangents of the four and of p, as
    [grids * rows, cols] CPU tensors: (u, v, w, d, tu, tv, tw, td, tp)."""
    lay = _layout(shape)
    g = _gen(seed, *shape)
    vel = [24.0 * (2 * torch.rand(B * lay[k][0], lay[k][1], generator=g) - 1) for k in "uvw"]
    d = torch.rand(B * lay["c"][0], lay["c"][1], generator=g) ** 4 * 2
    return vel + [d] + [torch.randn(B * T * lay[k][0], lay[k][1], generator=g) for k in "uvwcc"]


def _advect_case(shape, which):
    D, H, W = shape
    lay = _layout(shape)
    fl = lay["uvwc"[which]]
    bufs = [_field("field", fl), _field("u", lay["u"]), _field("v", lay["v"]), _field("w", lay["w"]),
            _field("tfield", fl, grids=B * T), _field("tu", lay["u"], grids=B * T), _field("tv", lay["v"], grids=B * T),
            _field("tw", lay["w"], grids=B * T), _field("tout", fl, "out", B * T)]

    def inputs():
        t = _draw(shape, 80 + which)
        return {"field": t[which].clone(), "u": t[0], "v": t[1], "w": t[2], "tfield": t[4 + which].clone(), "tu": t[4], "tv": t[5],
                "tw": t[6]}

    def args(b):
        return [which, b.ptr("field"), b.ptr("u"), b.ptr("v"), b.ptr("w"), b.ptr("tfield"), b.ptr("tu"), b.ptr("tv"), b.ptr("tw"),
                b.ptr("tout"), B, T, D, H, W, b.stride("u"), b.stride("v"), DT, b.stream]
    case = Case(f"advect3d_tangent-{_sid(shape)}-which{which}", "smk_advect3d_tangent", bufs, args, inputs, lambda: dense_reference(case))
    return case


def _renorm_case(shape):
    D, H, W = shape
    lay = _layout(shape)
    bufs = [_field("tu", lay["u"], "inout", B * T), _field("tv", lay["v"], "inout", B * T), _field("tw", lay["w"], "inout", B * T),
            _field("tp", lay["c"], "inout", B * T), _field("td", lay["c"], "inout", B * T), Buf("norms", F64, B * T, align=8, role="out")]

    def inputs():
        t = _draw(shape, 90)
        return {"tu": 3.0 * t[4], "tv": t[5], "tw": 0.5 * t[6], "tp": 0.25 * t[8], "td": t[7]}

    def args(b):
        return [b.ptr("tu"), b.ptr("tv"), b.ptr("tw"), b.ptr("tp"), b.ptr("td"), b.ptr("norms"), B, T, D, H, W, b.stride("tu"),
                b.stride("tv"), *b.workspace(), b.stream]
    case = Case(f"tangent3d_renorm-{_sid(shape)}", "smk_tangent3d_renorm", bufs, args, inputs, lambda: dense_reference(case),
                query=lambda lib: lib.smk_tangent3d_renorm_workspace(B, T, D, H, W), ws_align=8)
    return case


def all_cases():
    cases = [_advect_case(shape, which) for shape in SHAPES for which in (0, 1, 2, 3)]
    cases += [_renorm_case(shape) for shape in SHAPES]
    return cases
