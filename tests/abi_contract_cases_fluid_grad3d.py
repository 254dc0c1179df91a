"""The case table of tests/test_hip_abi_contract_fluid_grad3d.py: the stateless entry points of csrc/fluid_grad3d.hip --
smk_advect3d_backward, smk_project3d_backward, smk_buoy_diffuse3d_backward -- laid out for the guarded arena (tests/guarded_arena.py) exactly
as tests/abi_contract_cases_fluid_grad.py lays out the 2-D three.

A field [B][planes][rows][pitch] is an arena buffer of B * planes * rows rows of `columns` elements, `pitch` elements apart (pitch_c = W + 3,
pitch_v = W + 1 + 2: strictly larger than the rows, so the padding of every row is guard), every pointer 4-byte aligned and no better, the
projection's workspace exactly smk_project3d_backward_workspace(B, D, H, W) bytes.  reference(): the same entry point on dense, aligned,
separately allocated tensors (abi_contract_cases.dense_reference) -- the call physics.fluid_step3d's backward makes, held to the fp64 oracle
by tests/test_hip_fluid_grad3d.py."""
import torch

from abi_contract_cases import F32, I32, Case, _gen, dense_reference
from guarded_arena import Buf

ENTRY_POINTS = ["smk_advect3d_backward", "smk_project3d_backward", "smk_buoy_diffuse3d_backward"]
B = 2
SHAPES = [(4, 5, 7), (6, 19, 37)]      # one tile with a ragged edge; 3 x 2 tiles of the march and one ragged brick of the projection
DT, VISCOSITY = 0.1, 0.001
PB_T = 2                               # csrc/fluid_grad3d.h FG3_PB_T: transposed sweeps per launch


def _pitches(W):
    return W + 3, W + 1 + 2


def _layout(shape):
    """{name: (planes * rows, columns, pitch)} of u, v, w and a cell field."""
    D, H, W = shape
    pc, pv = _pitches(W)
    return {"u": (D * (H + 1), W, pc), "v": (D * H, W + 1, pv), "w": ((D + 1) * H, W, pc), "c": (D * H, W, pc)}


def _field(name, lay, role="in"):
    rows, cols, pitch = lay
    return Buf(name, F32, cols, B * rows, pitch, role=role)


def _draw(shape, seed):
    """u, v, w (|dt * velocity| <= 0.6: under the one-cell limit), density, and four upstream gradients, as [B * rows, cols] CPU tensors."""
    lay = _layout(shape)
    g = _gen(seed, *shape)
    vel = [6.0 * (2 * torch.rand(B * lay[k][0], lay[k][1], generator=g) - 1) for k in "uvw"]
    d = torch.rand(B * lay["c"][0], lay["c"][1], generator=g) ** 4 * 2
    return vel + [d] + [torch.randn(B * lay[k][0], lay[k][1], generator=g) for k in "uvwc"]


def _sid(shape):
    return "x".join(str(s) for s in shape)


def _advect_case(shape, which):
    D, H, W = shape
    lay = _layout(shape)
    fl = lay["uvwc"[which]]
    bufs = [_field("field", fl), _field("u", lay["u"]), _field("v", lay["v"]), _field("w", lay["w"]), _field("gout", fl),
            _field("dfield", fl, "out"), _field("du", lay["u"], "out"), _field("dv", lay["v"], "out"), _field("dw", lay["w"], "out"),
            Buf("far", I32, B, role="out")]

    def inputs():
        t = _draw(shape, 50 + which)
        return {"field": t[which].clone(), "u": t[0], "v": t[1], "w": t[2], "gout": t[4 + which]}

    def args(b):
        return [which, b.ptr("field"), b.ptr("u"), b.ptr("v"), b.ptr("w"), b.ptr("gout"), b.ptr("dfield"), b.ptr("du"), b.ptr("dv"),
                b.ptr("dw"), b.ptr("far"), B, D, H, W, b.stride("u"), b.stride("v"), DT, b.stream]
    case = Case(f"advect3d_backward-{_sid(shape)}-which{which}", "smk_advect3d_backward", bufs, args, inputs, lambda: dense_reference(case))
    return case


def _project_case(shape, J):
    D, H, W = shape
    lay = _layout(shape)
    bufs = [_field("gu", lay["u"]), _field("gv", lay["v"]), _field("gw", lay["w"]), _field("gp", lay["c"]),
            _field("du", lay["u"], "out"), _field("dv", lay["v"], "out"), _field("dw", lay["w"], "out"), _field("dp", lay["c"], "out")]

    def inputs():
        t = _draw(shape, 60 + J)
        return {"gu": t[4], "gv": t[5], "gw": t[6], "gp": t[7]}

    def args(b):
        return [b.ptr("gu"), b.ptr("gv"), b.ptr("gw"), b.ptr("gp"), b.ptr("du"), b.ptr("dv"), b.ptr("dw"), b.ptr("dp"), B, D, H, W,
                b.stride("gu"), b.stride("gv"), J, 0.01, *b.workspace(), b.stream]
    case = Case(f"project3d_backward-{_sid(shape)}-J{J}", "smk_project3d_backward", bufs, args, inputs, lambda: dense_reference(case),
                query=lambda lib: lib.smk_project3d_backward_workspace(B, D, H, W))
    return case


def _buoy_diffuse_case(shape):
    D, H, W = shape
    lay = _layout(shape)
    bufs = [_field("gu", lay["u"]), _field("gv", lay["v"]), _field("gw", lay["w"]), _field("gd", lay["c"]),
            _field("du", lay["u"], "out"), _field("dv", lay["v"], "out"), _field("dw", lay["w"], "out"), _field("dd", lay["c"], "out")]

    def inputs():
        t = _draw(shape, 70)
        return {"gu": t[4], "gv": t[5], "gw": t[6], "gd": t[7]}

    def args(b):
        return [b.ptr("gu"), b.ptr("gv"), b.ptr("gw"), b.ptr("gd"), b.ptr("du"), b.ptr("dv"), b.ptr("dw"), b.ptr("dd"), B, D, H, W,
                b.stride("gu"), b.stride("gv"), DT, VISCOSITY, b.stream]
    case = Case(f"buoy_diffuse3d_backward-{_sid(shape)}", "smk_buoy_diffuse3d_backward", bufs, args, inputs, lambda: dense_reference(case))
    return case


def all_cases():
    cases = [_advect_case(shape, which) for shape in SHAPES for which in (0, 1, 2, 3)]
    cases += [_project_case(shape, J) for shape in SHAPES for J in (0, PB_T + 1)]
    cases += [_buoy_diffuse_case(shape) for shape in SHAPES]
    return cases
