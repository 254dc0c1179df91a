"""The second half of the case table of tests/test_hip_abi_contract.py: the stateless entry points a training step calls -- the 2-D
training convolutions, the BatchNorm passes (NCHW and channels-last), the reconstruction head's convolutions, LayerNorm, the attention
forward / backward / delta, the linear weight gradient, the FFN's element-wise chain, the chaos term and the gradient exchange.  Same
rules as tests/abi_contract_cases.py: the smallest shapes at which the launcher's branches exist (the tile and chunk sizes stand above
every shape list, read from the launchers in csrc/), every pitch strictly larger than its row, every workspace exactly the bytes its
query returns, every pointer with the weakest alignment that the header and the entry point's SMK_REQUIRE lines in api.hip admit
(4 bytes where neither names one).

reference(): the Python wrapper's dense, aligned call wherever a wrapper makes the call of the case -- the autograd nodes of
models/conv.py (_HipConv1Fn, _HipConv2Fn: forward, data gradient, weight gradient with and without db) and models/decoder_train.py
(_HipConvT4s2Fn, _HipConv3SigmoidFn: the forwards with a bias, the weight gradient with db), _HipBnReluPoolFn's forward and the phase
calls of models/norm.py (_phase: what sync_bn.py and the frozen route run) and models/encoder3d.py (_bn_cl_phase), hip_layernorm, the
autograd backward of hip_layernorm_train, hip_attention_delta, hip_linear_wgrad, models/ffn.py's _run, utils.distributed.reduce_shards.
The other cases compare with dense_reference(case), the same entry point on separately allocated, dense, 256-byte aligned torch tensors
with a torch.empty workspace -- the call the wrapper would make, where the wrapper cannot make it alone: a NULL bias or db of the head
(decoder_train.py always passes both), a data gradient or a backward whose node first runs its own forward on other values
(smk_convt4s2_train_dgrad, smk_conv3_sigmoid_train_backward, smk_bn_relu_pool_backward with given statistics, smk_attention_backward with
a given lse and delta), the lse that _HipAttentionFn keeps to itself, and the chaos calls, which chaos_attention.py and hip_body.py make
from inside their modules with noise they draw themselves.  The paths are held to fp64 by test_hip_encoder.py, test_hip_bn_pool_sizes.py, test_hip_input_grad.py,
test_hip_head_train.py, test_hip_transformer.py, test_hip_attention_variants.py, test_hip_linear_backward.py, test_hip_exchange.py and
test_hip_encoder3d_train.py; the comparison here is bit for bit.

Branches that no case reaches because the smallest shape that does holds more than about 4M elements: a workgroup with several tiles in
smk_conv1_train_wgrad (more than 2 x CUs tiles of 4 x 64), smk_conv2_train_forward / _dgrad (more than CUs x occupancy tiles of 8 x 16),
the 8-channel form of smk_convt4s2_train_forward and the 16-channel form of its dgrad (1024 workgroups and more), a chunk with several
tiles in smk_convt4s2_train_wgrad and smk_conv3_sigmoid_train_backward, the one-workgroup-per-CU forms of smk_attention_forward_lse
(more than CUs query blocks), the grid-stride loops of smk_attention_delta, smk_ffn_elementwise and smk_reduce_shards (16 workgroups
per CU and more).  The attention key split needs a workspace, which smk_attention_forward_lse does not take."""
import ctypes as C
import functools
import math

import torch

from abi_contract_cases import F32, I32, U8, Case, dense_reference, _gen
from guarded_arena import Buf
from smokephysai_amd import _lib

BF16 = torch.bfloat16
STATS, APPLY, BWD_SUMS, BWD_DZ = 0, 1, 2, 3
PHASE_NAME = {STATS: "stats", APPLY: "apply", BWD_SUMS: "bwd_sums", BWD_DZ: "bwd_dz"}
EPS = 1e-5


def _mk(id, entry, bufs, args, inputs, query=None, ws_align=4, reference=None, **tags):
    case = Case(id, entry, bufs, args, inputs, reference, query=query, ws_align=ws_align)
    if reference is None:
        case.reference = functools.partial(dense_reference, case)
    case.tags = tags
    return case


def _randn(seed, *names_sizes_scales):
    """-> a function that draws {name: randn(n) * scale (+ shift)} from one seeded generator, in the order given."""
    def draw():
        g = _gen(*seed)
        out = {}
        for name, n, scale, *shift in names_sizes_scales:
            out[name] = torch.randn(n, generator=g) * scale + (shift[0] if shift else 0.0)
        return out
    return draw


def _conv_reference(fn_name, module, draw, xshape, wshape, out, extra=()):
    """A reference through the autograd Function `fn_name` of smokephysai_amd.models.`module` (the node its hip_* wrapper builds):
    out "z": its forward on (x, weight, bias or None);  "dx": its backward from dz with only x asking for a gradient (x itself does
    not enter the data gradient: zeros);  "dw": its backward with the weight -- and the bias, if the case has a db -- asking."""
    def reference():
        import importlib
        fn = getattr(importlib.import_module("smokephysai_amd.models." + module), fn_name)
        d = {k: v.cuda() for k, v in draw().items()}
        w = d["weight"].reshape(wshape) if "weight" in d else torch.zeros(wshape, device="cuda")
        if out == "z":
            return {"z": fn.apply(d["x"].reshape(xshape), w, d.get("bias"), *extra)}
        if out == "dx":
            x = torch.zeros(xshape, device="cuda", requires_grad=True)
            z = fn.apply(x, w, None, *extra)
            z.backward(d["dz"].reshape(z.shape))
            return {"dx": x.grad}
        w.requires_grad_(True)
        b = torch.zeros(wshape[0] if module == "conv" else wshape[1], device="cuda", requires_grad=True) if out == "dw_db" else None
        z = fn.apply(d["x"].reshape(xshape), w, b, *extra)
        z.backward(d["dz"].reshape(z.shape))
        return {"dw": w.grad, "db": b.grad} if b is not None else {"dw": w.grad}
    return reference


def _ld(b, buf):
    """The pitch argument of a row buffer: the arena's (or the dense tensors') pitch; a single row has no second row, and gets a pitch
    larger than the row all the same."""
    return b.stride(buf.name) if buf.planes > 1 else buf.elems + 4


def _rows(name, cols, rows, pad, align=16, role="in", dtype=F32):
    """`rows` rows of `cols` elements, `cols + pad` apart (one row: dense)."""
    return Buf(name, dtype, cols, rows, cols + pad if rows > 1 else None, align=align, role=role)


# ------------------------------------------------------------------------------------------------ encoder conv1 (2-D)
# forward: a workgroup owns 4 rows x 256 columns (64 lanes x float4 per row);  dgrad: 32 x 64 tiles (C1D_TH x C1D_TW), rows and columns
# past H, W masked;  wgrad: 4 x 64 tiles dealt to min(2 x CUs, tiles) workgroups, one finishing launch over the workgroups' partials.
CONV1_FORWARD_SHAPES = [(1, 1, 4), (2, 6, 12), (2, 6, 260)]           # one lane; ragged in a single tile; two column tiles + ragged rows
CONV1_DGRAD_SHAPES = [(1, 1, 4), (2, 6, 12), (2, 38, 68)]             # ... two tiles per axis, both ragged
CONV1_WGRAD_SHAPES = [(1, 4, 64), (2, 8, 128)]                        # one tile; 2 x 2 x 2 tiles


def conv1_cases():
    cases = []
    for shape in CONV1_FORWARD_SHAPES:
        B, H, W = shape
        for bias in ((False,) if shape == CONV1_FORWARD_SHAPES[0] else (True, False)):
            bufs = [Buf("x", F32, B * H * W), Buf("weight", F32, 64 * 49)] + ([Buf("bias", F32, 64)] if bias else []) + \
                   [Buf("z1", F32, B * 64 * H * W, role="out")]
            draws = [("x", B * H * W, 1.0), ("weight", 64 * 49, 0.1)] + ([("bias", 64, 0.1)] if bias else [])
            draw = _randn((31, *shape), *draws)
            ref = _conv_reference("_HipConv1Fn", "conv", draw, (B, 1, H, W), (64, 1, 7, 7), "z")
            cases.append(_mk(f"conv1_train_forward-{B}x{H}x{W}-{'bias' if bias else 'nobias'}", "smk_conv1_train_forward", bufs,
                             lambda b, d=(B, H, W): [b.ptr("x"), b.ptr("weight"), b.ptr("bias"), *d, b.ptr("z1"), b.stream],
                             draw, reference=lambda ref=ref: {"z1": ref()["z"]}, bias=bias))
    for shape in CONV1_DGRAD_SHAPES:
        B, H, W = shape
        bufs = [Buf("dz", F32, B * 64 * H * W, align=16), Buf("weight", F32, 64 * 49), Buf("dx", F32, B * H * W, align=16, role="out")]
        draw = _randn((32, *shape), ("dz", B * 64 * H * W, 1.0), ("weight", 64 * 49, 0.1))
        cases.append(_mk(f"conv1_train_dgrad-{B}x{H}x{W}", "smk_conv1_train_dgrad", bufs,
                         lambda b, d=(B, H, W): [b.ptr("dz"), b.ptr("weight"), *d, b.ptr("dx"), b.stream],
                         draw, reference=_conv_reference("_HipConv1Fn", "conv", draw, (B, 1, H, W), (64, 1, 7, 7), "dx")))
    for shape in CONV1_WGRAD_SHAPES:
        B, H, W = shape
        for db in ((True,) if shape == CONV1_WGRAD_SHAPES[0] else (True, False)):
            bufs = [Buf("dz", F32, B * 64 * H * W), Buf("x", F32, B * H * W), Buf("dw", F32, 64 * 49, role="out")] + \
                   ([Buf("db", F32, 64, role="out")] if db else [])
            draw = _randn((33, *shape), ("dz", B * 64 * H * W, 1.0), ("x", B * H * W, 1.0))
            cases.append(_mk(f"conv1_train_wgrad-{B}x{H}x{W}-{'db' if db else 'nodb'}", "smk_conv1_train_wgrad", bufs,
                             lambda b, d=(B, H, W): [b.ptr("dz"), b.ptr("x"), *d, b.ptr("dw"), b.ptr("db"), b.workspace()[0], b.stream],
                             draw, query=lambda lib: lib.smk_conv1_train_wgrad_workspace(), db=db,
                             reference=_conv_reference("_HipConv1Fn", "conv", draw, (B, 1, H, W), (64, 1, 7, 7), "dw_db" if db else "dw")))
    return cases


# ------------------------------------------------------------------------------------------------ encoder conv2 (2-D)
# 8 x 16 output tiles (B3_TH x B3_TW); forward and dgrad: a weight-split launch into the workspace, then min(CUs x occupancy, tiles)
# persistent workgroups;  wgrad: (2 CUs / 32) x 8 = 128 streams of tiles x 4 channel groups, then a finishing launch -- 136 tiles give
# the first eight streams a second tile.
CONV2_SHAPES = [(1, 8, 16), (2, 16, 48)]                               # one tile; 2 x 2 x 3 tiles
CONV2_WGRAD_SHAPES = CONV2_SHAPES + [(1, 64, 272)]                     # 8 x 17 = 136 tiles: streams that own two tiles


def conv2_cases():
    cases = []
    for shape in CONV2_SHAPES:
        B, H, W = shape
        px = B * H * W
        for bias in ((True,) if shape == CONV2_SHAPES[0] else (True, False)):
            bufs = [Buf("a1", F32, 64 * px), Buf("weight", F32, 128 * 64 * 9)] + ([Buf("bias", F32, 128)] if bias else []) + \
                   [Buf("z2", F32, 128 * px, role="out")]
            draws = [("a1", 64 * px, 1.0), ("weight", 128 * 64 * 9, 0.05)] + ([("bias", 128, 0.1)] if bias else [])
            draw = _randn((34, *shape), *draws)
            ref = _conv_reference("_HipConv2Fn", "conv", lambda draw=draw: {("x" if k == "a1" else k): v for k, v in draw().items()},
                                  (B, 64, H, W), (128, 64, 3, 3), "z", extra=(True, True))
            cases.append(_mk(f"conv2_train_forward-{B}x{H}x{W}-{'bias' if bias else 'nobias'}", "smk_conv2_train_forward", bufs,
                             lambda b, d=(B, H, W): [b.ptr("a1"), b.ptr("weight"), b.ptr("bias"), *d, b.ptr("z2"), b.workspace()[0], b.stream],
                             draw, query=lambda lib: lib.smk_conv2_train_workspace(), bias=bias, reference=lambda ref=ref: {"z2": ref()["z"]}))
        bufs = [Buf("dz", F32, 128 * px), Buf("weight", F32, 128 * 64 * 9), Buf("dx", F32, 64 * px, role="out")]
        draw = _randn((35, *shape), ("dz", 128 * px, 1.0), ("weight", 128 * 64 * 9, 0.05))
        cases.append(_mk(f"conv2_train_dgrad-{B}x{H}x{W}", "smk_conv2_train_dgrad", bufs,
                         lambda b, d=(B, H, W): [b.ptr("dz"), b.ptr("weight"), *d, b.ptr("dx"), b.workspace()[0], b.stream],
                         draw, query=lambda lib: lib.smk_conv2_train_workspace(),
                         reference=_conv_reference("_HipConv2Fn", "conv", draw, (B, 64, H, W), (128, 64, 3, 3), "dx", extra=(True, True))))
    for shape in CONV2_WGRAD_SHAPES:
        B, H, W = shape
        px = B * H * W
        for db in ((True, False) if shape == CONV2_SHAPES[1] else (True,)):
            bufs = [Buf("dz", F32, 128 * px), Buf("a1", F32, 64 * px), Buf("dw", F32, 128 * 64 * 9, role="out")] + \
                   ([Buf("db", F32, 128, role="out")] if db else [])
            draw = _randn((36, *shape), ("dz", 128 * px, 1.0), ("a1", 64 * px, 1.0))
            ref = _conv_reference("_HipConv2Fn", "conv", lambda draw=draw: {("x" if k == "a1" else k): v for k, v in draw().items()},
                                  (B, 64, H, W), (128, 64, 3, 3), "dw_db" if db else "dw", extra=(True, True))
            cases.append(_mk(f"conv2_train_wgrad-{B}x{H}x{W}-{'db' if db else 'nodb'}", "smk_conv2_train_wgrad", bufs,
                             lambda b, d=(B, H, W): [b.ptr("dz"), b.ptr("a1"), *d, b.ptr("dw"), b.ptr("db"), b.workspace()[0], b.stream],
                             draw, query=lambda lib: lib.smk_conv2_train_wgrad_workspace(), db=db, reference=ref))
    return cases


# ------------------------------------------------------------------------------------------------ BatchNorm 2-D
# A workgroup owns one chunk of one channel's plane: 4,096 floats at pool 1, 2 and 4, 16,384 at pool 8, 8,192 at pool 16, 32,768 at pool 32
# (one row of cells); grid (B x chunks per plane, C); k_bn_finish adds a channel's B x chunks partial pairs.  W == 32 x pool when
# pooling.  Every shape: two samples or two chunks per plane, so that the finishing pass adds more than one pair; pool 16 also at the
# smallest plane (one chunk, B = 1).  The element-wise phases at pool 1 take any plane of whole float4s: 6 x 10 is 15 of them.
BN_SHAPES = {1: [(2, 16, 32, 128)], 2: [(2, 16, 64, 64)], 4: [(2, 16, 32, 128)], 8: [(2, 16, 64, 256)],
             16: [(1, 16, 16, 512), (2, 16, 32, 512)], 32: [(1, 16, 32, 1024)]}
BN_FROZEN_SHAPE = (2, 16, 6, 10)


def _bn_draws(shape, pool):
    B, Cc, H, W = shape
    n, no = B * Cc * H * W, B * Cc * (H // pool) * (W // pool)
    return _randn((37, *shape, pool), ("z", n, 1.0), ("dout", no, 1.0), ("gamma", Cc, 0.2, 1.0), ("beta", Cc, 0.2), ("mean", Cc, 0.1),
                  ("rstd", Cc, 0.1, 1.0), ("dgamma", Cc, 1.0), ("dbeta", Cc, 1.0))


def _pick(draw, *names, zero=()):
    def inputs():
        d = draw()
        return {n: (torch.zeros_like(d[n]) if n in zero else d[n]) for n in names}
    return inputs


def _bn_phase_reference(inputs, phase, shape, pool, count, cl=None):
    """One phase through the wrappers' own call: models/norm.py's _phase (NCHW), or models/encoder3d.py's _bn_cl_phase with cl =
    (C, pooled) for z [B, D, H, W, C] -- dense tensors of their own, the workspace a torch.empty of the queried size."""
    def reference():
        L, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())
        d = {k: v.cuda() for k, v in inputs().items()}
        new = lambda *size: torch.empty(*size, device=dev, dtype=F32)           # noqa: E731
        if cl is None:
            B, Cc, H, W = shape
            z, no = d["z"].reshape(shape), (B, Cc, H // pool, W // pool)
            nbytes = L.smk_bn_train_workspace(B, Cc, H, W, pool)
        else:
            (B, D, H, W), (Cc, pooled) = shape, cl
            z, no = d["z"].reshape(B, D, H, W, Cc), ((B, 1024, Cc) if pooled else (B, D, H, W, Cc))
            nbytes = L.smk_bn_cl_workspace(B, D, H, W, Cc)
        ws = torch.empty(int(nbytes), device=dev, dtype=U8) if phase in (STATS, BWD_SUMS) else None
        stats = torch.stack([d["mean"], torch.zeros_like(d["mean"]), d["rstd"]]) if "mean" in d else new(3, Cc)
        gamma, beta = d.get("gamma", new(Cc)), d.get("beta", new(Cc))
        dout = d["dout"].reshape(no) if "dout" in d else None
        out = new(no) if phase == APPLY else None
        dz = torch.empty_like(z) if phase == BWD_DZ else None
        dwb = torch.stack([d["dgamma"], d["dbeta"]]) if phase == BWD_DZ else (new(2, Cc) if phase == BWD_SUMS else None)
        if cl is None:
            from smokephysai_amd.models.norm import _phase
            _phase(L, phase, z, dout, gamma, beta, EPS, stats[0], stats[1] if phase == STATS else None, stats[2], pool, out, dz,
                   None if dwb is None else dwb[0], None if dwb is None else dwb[1], count, ws, dev)
        else:
            from smokephysai_amd.models.encoder3d import _bn_cl_phase
            _bn_cl_phase(L, phase, z, dout, cl[1], gamma, beta, EPS, stats, out, dz, dwb, count, ws, dev)
        torch.cuda.synchronize()
        return {STATS: {"mean": stats[0], "var": stats[1], "rstd": stats[2]}, APPLY: {"out": out},
                BWD_SUMS: {"dgamma": None if dwb is None else dwb[0], "dbeta": None if dwb is None else dwb[1]}, BWD_DZ: {"dz": dz}}[phase]
    return reference


def _bn_forward_reference(inputs, shape, pool):
    def reference():
        from smokephysai_amd.models.norm import _HipBnReluPoolFn
        d = {k: v.cuda() for k, v in inputs().items()}
        out, stats = _HipBnReluPoolFn.apply(d["z"].reshape(shape), d["gamma"], d["beta"], EPS, pool)
        return {"out": out, "mean": stats[0], "var": stats[1], "rstd": stats[2]}
    return reference


def _bn_cases(shape, pool):
    B, Cc, H, W = shape
    n, no = B * Cc * H * W, B * Cc * (H // pool) * (W // pool)
    dims = [B, Cc, H, W]
    draw = _bn_draws(shape, pool)
    tag = f"{B}x{Cc}x{H}x{W}-pool{pool}"
    query = lambda lib: lib.smk_bn_train_workspace(B, Cc, H, W, pool)          # noqa: E731
    z, dout = Buf("z", F32, n, align=16), Buf("dout", F32, no, align=16)
    vec = lambda name, role="in": Buf(name, F32, Cc, role=role)                # noqa: E731
    cases = [
        _mk(f"bn_relu_pool_forward-{tag}", "smk_bn_relu_pool_forward",
            [z, vec("gamma"), vec("beta"), Buf("out", F32, no, align=16, role="out"), vec("mean", "out"), vec("var", "out"), vec("rstd", "out")],
            lambda b: [b.ptr("z"), *dims, b.ptr("gamma"), b.ptr("beta"), EPS, pool, b.ptr("out"), b.ptr("mean"), b.ptr("var"), b.ptr("rstd"),
                       b.workspace()[0], b.stream],
            _pick(draw, "z", "gamma", "beta"), query=query, ws_align=16, pool=pool,
            reference=_bn_forward_reference(_pick(draw, "z", "gamma", "beta"), shape, pool)),
        _mk(f"bn_relu_pool_backward-{tag}", "smk_bn_relu_pool_backward",
            [z, dout, vec("gamma"), vec("beta"), vec("mean"), vec("rstd"), Buf("dz", F32, n, align=16, role="out"), vec("dgamma", "out"),
             vec("dbeta", "out")],
            lambda b: [b.ptr("z"), b.ptr("dout"), *dims, b.ptr("gamma"), b.ptr("beta"), b.ptr("mean"), b.ptr("rstd"), pool, b.ptr("dz"),
                       b.ptr("dgamma"), b.ptr("dbeta"), b.workspace()[0], b.stream],
            _pick(draw, "z", "dout", "gamma", "beta", "mean", "rstd"), query=query, ws_align=16, pool=pool)]
    for phase in (STATS, APPLY, BWD_SUMS, BWD_DZ):
        cases.append(_bn_phase_case(shape, pool, phase, draw, f"bn_relu_pool_phase-{tag}-{PHASE_NAME[phase]}", frozen=False))
    return cases


def _bn_phase_case(shape, pool, phase, draw, id, frozen):
    B, Cc, H, W = shape
    n, no = B * Cc * H * W, B * Cc * (H // pool) * (W // pool)
    z, dout = Buf("z", F32, n, align=16), Buf("dout", F32, no, align=16)
    vec = lambda name, role="in": Buf(name, F32, Cc, role=role)                # noqa: E731
    given = [z, vec("gamma"), vec("beta")]
    count = 1.0 if frozen else float(B * H * W)
    if phase == STATS:
        bufs, ins = given + [vec("mean", "out"), vec("var", "out"), vec("rstd", "out")], ("z", "gamma", "beta")
    elif phase == APPLY:
        bufs, ins = given + [vec("mean"), vec("rstd"), Buf("out", F32, no, align=16, role="out")], ("z", "gamma", "beta", "mean", "rstd")
    elif phase == BWD_SUMS:
        bufs = given + [dout, vec("mean"), vec("rstd"), vec("dgamma", "out"), vec("dbeta", "out")]
        ins = ("z", "dout", "gamma", "beta", "mean", "rstd")
    else:
        bufs = given + [dout, vec("mean"), vec("rstd"), vec("dgamma"), vec("dbeta"), Buf("dz", F32, n, align=16, role="out")]
        ins = ("z", "dout", "gamma", "beta", "mean", "rstd", "dgamma", "dbeta")
    needs_ws = phase in (STATS, BWD_SUMS)

    def args(b):
        return [phase, b.ptr("z"), b.ptr("dout"), B, Cc, H, W, b.ptr("gamma"), b.ptr("beta"), EPS, b.ptr("mean"), b.ptr("var"), b.ptr("rstd"),
                pool, b.ptr("out"), b.ptr("dz"), b.ptr("dgamma"), b.ptr("dbeta"), count, b.workspace()[0] if needs_ws else None, b.stream]
    inputs = _pick(draw, *ins, zero=("dgamma", "dbeta") if frozen else ())
    return _mk(id, "smk_bn_relu_pool_phase", bufs, args, inputs, reference=_bn_phase_reference(inputs, phase, shape, pool, count),
               query=(lambda lib: lib.smk_bn_train_workspace(B, Cc, H, W, pool)) if needs_ws else None, ws_align=16,
               pool=pool, phase=phase, frozen=frozen)


def bn_cases():
    cases = [c for pool, shapes in BN_SHAPES.items() for shape in shapes for c in _bn_cases(shape, pool)]
    draw = _bn_draws(BN_FROZEN_SHAPE, 1)
    tag = "x".join(map(str, BN_FROZEN_SHAPE))
    for phase in (APPLY, BWD_DZ):
        cases.append(_bn_phase_case(BN_FROZEN_SHAPE, 1, phase, draw, f"bn_relu_pool_phase-{tag}-pool1-frozen-{PHASE_NAME[phase]}", frozen=True))
    return cases


# ------------------------------------------------------------------------------------------------ BatchNorm channels-last
# z [M = B D H W][C]; a workgroup's 256 threads hold 256 / (C / 4) rows of float4s (16 rows at C = 64, 8 at C = 128); min(1024, row groups)
# workgroups stride over the row groups and k_bncl_finish adds their fp64 partial rows; pooled: one thread per (token, float4 of
# channels) walks its D x (H / 32) x (W / 32) block.  Unpooled 1 x 1 x 8 x 16: 128 rows = 8 / 16 row groups; 2 x 3 x 8 x 16: 768 rows;
# 1 x 2 x 96 x 96 at C = 64: 18,432 rows = 1,152 row groups, so that 128 workgroups take a second one.  Pooled 32 x 32: blocks of one voxel
# per plane; 32 x 64: blocks of 1 x 2.
BN_CL_SHAPES = {0: [(1, 1, 8, 16), (2, 3, 8, 16)], 1: [(1, 2, 32, 32), (2, 1, 32, 64)]}
BN_CL_STRIDED_SHAPE = (1, 2, 96, 96)


def _bn_cl_case(shape, Cc, pooled, phase):
    B, D, H, W = shape
    M = B * D * H * W
    n, no = M * Cc, (B * 1024 * Cc if pooled else M * Cc)
    draw = _randn((38, *shape, Cc, pooled), ("z", n, 1.0), ("dout", no, 1.0), ("gamma", Cc, 0.2, 1.0), ("beta", Cc, 0.2), ("mean", Cc, 0.1),
                  ("rstd", Cc, 0.1, 1.0), ("dgamma", Cc, 1.0), ("dbeta", Cc, 1.0))
    z, dout = Buf("z", F32, n, align=16), Buf("dout", F32, no, align=16)
    vec = lambda name, role="in": Buf(name, F32, Cc, role=role)                # noqa: E731
    if phase == STATS:
        bufs, ins = [z, vec("mean", "out"), vec("var", "out"), vec("rstd", "out")], ("z",)
    elif phase == APPLY:
        bufs = [z, vec("gamma"), vec("beta"), vec("mean"), vec("rstd"), Buf("out", F32, no, align=16, role="out")]
        ins = ("z", "gamma", "beta", "mean", "rstd")
    elif phase == BWD_SUMS:
        bufs = [z, dout, vec("gamma"), vec("beta"), vec("mean"), vec("rstd"), vec("dgamma", "out"), vec("dbeta", "out")]
        ins = ("z", "dout", "gamma", "beta", "mean", "rstd")
    else:
        bufs = [z, dout, vec("gamma"), vec("beta"), vec("mean"), vec("rstd"), vec("dgamma"), vec("dbeta"), Buf("dz", F32, n, align=16, role="out")]
        ins = ("z", "dout", "gamma", "beta", "mean", "rstd", "dgamma", "dbeta")
    needs_ws = phase in (STATS, BWD_SUMS)

    def args(b):
        return [phase, b.ptr("z"), b.ptr("dout"), B, D, H, W, Cc, pooled, b.ptr("gamma"), b.ptr("beta"), EPS, b.ptr("mean"), b.ptr("var"),
                b.ptr("rstd"), b.ptr("out"), b.ptr("dz"), b.ptr("dgamma"), b.ptr("dbeta"), float(M), b.workspace()[0] if needs_ws else None,
                b.stream]
    return _mk(f"bn_cl_phase-{B}x{D}x{H}x{W}-C{Cc}-{'pooled' if pooled else 'dense'}-{PHASE_NAME[phase]}", "smk_bn_cl_phase", bufs, args,
               _pick(draw, *ins), query=(lambda lib: lib.smk_bn_cl_workspace(B, D, H, W, Cc)) if needs_ws else None, ws_align=8,
               reference=_bn_phase_reference(_pick(draw, *ins), phase, shape, None, float(M), cl=(Cc, pooled)),
               C=Cc, pooled=pooled, phase=phase)


def bn_cl_cases():
    cases = [_bn_cl_case(shape, Cc, pooled, phase) for pooled, shapes in BN_CL_SHAPES.items() for shape in shapes for Cc in (64, 128)
             for phase in (STATS, APPLY, BWD_SUMS, BWD_DZ)]
    return cases + [_bn_cl_case(BN_CL_STRIDED_SHAPE, 64, 0, phase) for phase in (STATS, APPLY, BWD_SUMS, BWD_DZ)]


# ------------------------------------------------------------------------------------------------ reconstruction head
# ConvTranspose: forward and dgrad tile the input in 16 x 16 positions (TT), grid (tiles, channel groups, B) -- two output channels /
# four input channels per workgroup below 1024 workgroups;  wgrad: tiles of 2 x 16 input positions (TW_R x TW_C) dealt to
# min(tiles, max(64, 1024 / channel blocks)) chunks x CIN / 16 (COUT 32) or CIN / 32 (COUT 16) channel blocks, then one finishing launch.
# (B, CIN, COUT, H, W, tok):
CONVT_SHAPES = [(1, 16, 32, 16, 16, 0), (2, 32, 16, 16, 32, 0), (2, 64, 32, 32, 16, 1), (1, 32, 16, 16, 16, 1)]
# Conv2d(16, 1, 3) + sigmoid: tiles of 8 x 32 pixels (T3_H x T3_W), grid (tiles, 1, B); the backward's weight gradient runs in
# min(tiles, 1024) chunks and one finishing workgroup.
CONV3_SHAPES = [(1, 8, 32), (2, 16, 64)]                              # one tile; 2 x 2 x 2 tiles


def head_cases():
    cases = []
    for i, (B, CIN, COUT, H, W, tok) in enumerate(CONVT_SHAPES):
        nx, nz, nw = B * CIN * H * W, B * COUT * 4 * H * W, CIN * COUT * 16
        dims = [B, CIN, COUT, H, W, tok]
        tag = f"{B}x{CIN}x{COUT}x{H}x{W}-{'tok' if tok else 'nchw'}"
        for bias in ((True, False) if i in (1, 2) else (True,)):
            bufs = [Buf("x", F32, nx, align=16), Buf("weight", F32, nw)] + ([Buf("bias", F32, COUT)] if bias else []) + \
                   [Buf("z", F32, nz, align=8, role="out")]
            draws = [("x", nx, 1.0), ("weight", nw, 0.05)] + ([("bias", COUT, 0.1)] if bias else [])
            draw = _randn((39, *dims), *draws)
            xshape = (B, H * W, CIN) if tok else (B, CIN, H, W)
            cases.append(_mk(f"convt4s2_train_forward-{tag}-{'bias' if bias else 'nobias'}", "smk_convt4s2_train_forward", bufs,
                             lambda b, d=dims: [b.ptr("x"), b.ptr("weight"), b.ptr("bias"), *d, b.ptr("z"), b.stream],
                             draw, COUT=COUT, tok=tok, bias=bias,             # (the wrapper always passes a bias: a NULL one is the direct call)
                             reference=_conv_reference("_HipConvT4s2Fn", "decoder_train", draw, xshape, (CIN, COUT, 4, 4), "z",
                                                       extra=(bool(tok), H, W)) if bias else None))
        cases.append(_mk(f"convt4s2_train_dgrad-{tag}", "smk_convt4s2_train_dgrad",
                         [Buf("dz", F32, nz), Buf("weight", F32, nw), Buf("dx", F32, nx, align=16, role="out")],
                         lambda b, d=dims: [b.ptr("dz"), b.ptr("weight"), *d, b.ptr("dx"), b.stream],
                         _randn((40, *dims), ("dz", nz, 1.0), ("weight", nw, 0.05)), COUT=COUT, tok=tok))      # (dense_reference: the wrapper's
        #                                                                                 node wants a bias, and its data gradient comes with a forward)
        for db in ((True, False) if i in (1, 2) else (True,)):
            bufs = [Buf("dz", F32, nz), Buf("x", F32, nx, align=16), Buf("dw", F32, nw, role="out")] + ([Buf("db", F32, COUT, role="out")] if db else [])
            draw = _randn((41, *dims), ("dz", nz, 1.0), ("x", nx, 1.0))
            xshape = (B, H * W, CIN) if tok else (B, CIN, H, W)
            cases.append(_mk(f"convt4s2_train_wgrad-{tag}-{'db' if db else 'nodb'}", "smk_convt4s2_train_wgrad", bufs,
                             lambda b, d=dims: [b.ptr("dz"), b.ptr("x"), *d, b.ptr("dw"), b.ptr("db"), b.workspace()[0], b.stream],
                             draw, reference=_conv_reference("_HipConvT4s2Fn", "decoder_train", draw, xshape, (CIN, COUT, 4, 4), "dw_db",
                                                             extra=(bool(tok), H, W)) if db else None,
                             query=lambda lib, d=dims: lib.smk_convt4s2_train_wgrad_workspace(*d[:5]), ws_align=16, COUT=COUT, tok=tok, db=db))
    for shape in CONV3_SHAPES:
        B, H, W = shape
        px = B * H * W
        for bias in (True, False):
            bufs = [Buf("x", F32, 16 * px), Buf("weight", F32, 144)] + ([Buf("bias", F32, 1)] if bias else []) + [Buf("y", F32, px, role="out")]
            draws = [("x", 16 * px, 1.0), ("weight", 144, 0.2)] + ([("bias", 1, 0.1)] if bias else [])
            draw = _randn((42, *shape), *draws)
            ref = _conv_reference("_HipConv3SigmoidFn", "decoder_train", draw, (B, 16, H, W), (1, 16, 3, 3), "z")
            cases.append(_mk(f"conv3_sigmoid_train_forward-{B}x{H}x{W}-{'bias' if bias else 'nobias'}", "smk_conv3_sigmoid_train_forward", bufs,
                             lambda b, d=(B, H, W): [b.ptr("x"), b.ptr("weight"), b.ptr("bias"), *d, b.ptr("y"), b.stream],
                             draw, bias=bias, reference=(lambda ref=ref: {"y": ref()["z"]}) if bias else None))
        for grads in (True, False):
            bufs = [Buf("dy", F32, px), Buf("y", F32, px), Buf("x", F32, 16 * px), Buf("weight", F32, 144), Buf("dx", F32, 16 * px, role="out")] + \
                   ([Buf("dw", F32, 144, role="out"), Buf("db", F32, 1, role="out")] if grads else [])

            def inputs(shape=shape, px=px):
                d = _randn((43, *shape), ("dy", px, 1.0), ("y", px, 1.0), ("x", 16 * px, 1.0), ("weight", 144, 0.2))()
                d["y"] = torch.sigmoid(d["y"])
                return d
            cases.append(_mk(f"conv3_sigmoid_train_backward-{B}x{H}x{W}-{'dw_db' if grads else 'dx_only'}", "smk_conv3_sigmoid_train_backward", bufs,
                             lambda b, d=(B, H, W): [b.ptr("dy"), b.ptr("y"), b.ptr("x"), b.ptr("weight"), *d, b.ptr("dx"), b.ptr("dw"), b.ptr("db"),
                                                     b.workspace()[0], b.stream],
                             inputs, query=lambda lib, d=(B, H, W): lib.smk_conv3_sigmoid_train_workspace(*d), ws_align=16, grads=grads))
    return cases


# ------------------------------------------------------------------------------------------------ LayerNorm
# One wave per row, four rows per workgroup, the row in registers as up to 8 float4 per lane: the kernels are instantiated for
# ceil(D / 256) <= 1, 2, 4, 8.  D = 4: one lane; 256: NV = 1 full; 2048: NV = 8.  37 rows: ten workgroups, the last with one row.  The
# backward runs min(1024, ceil(rows / 4)) workgroups that stride over the rows and a finishing launch over their partial rows: 4,100 rows
# give the first workgroup a second group of rows.
LN_ROWS = (1, 37)
LN_DIMS_F32, LN_DIMS_SPLIT = (4, 256, 2048), (8, 256)
LN_BWD_SHAPES = [(r, D) for r in LN_ROWS for D in LN_DIMS_F32] + [(4100, 4)]


def _ln_draws(rows, D):
    return _randn((44, rows, D), ("x", rows * D, 1.0, 0.3), ("dy", rows * D, 1.0), ("weight", D, 0.2, 1.0), ("bias", D, 0.2))


def _ln_module(d, D):
    ln = torch.nn.LayerNorm(D, eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(d["weight"])
        ln.bias.copy_(d["bias"])
    return ln


def layernorm_cases():
    cases = []
    for split, dims in ((0, LN_DIMS_F32), (1, LN_DIMS_SPLIT)):
        for rows in LN_ROWS:
            for D in dims:
                x = _rows("x", D, rows, 4)
                y = Buf("y", I32, rows * D, align=16, role="out") if split else _rows("y", D, rows, 8, role="out")      # split: dense rows
                draw = _ln_draws(rows, D)

                def args(b, x=x, y=y, rows=rows, D=D, split=split):
                    return [b.ptr("x"), rows, D, _ld(b, x), b.ptr("weight"), b.ptr("bias"), EPS, b.ptr("y"), D if split else _ld(b, y), split,
                            b.stream]

                def reference(draw=draw, rows=rows, D=D, split=split):
                    from smokephysai_amd.models.attention import hip_layernorm
                    d = draw()
                    out = hip_layernorm(d["x"].cuda().reshape(rows, D), _ln_module(d, D), out_split=bool(split))
                    return {"y": out.reshape(-1).view(I32) if split else out}
                cases.append(_mk(f"layernorm-{rows}x{D}-{'split' if split else 'f32'}", "smk_layernorm",
                                 [x, Buf("weight", F32, D, align=16), Buf("bias", F32, D, align=16), y], args,
                                 _pick(draw, "x", "weight", "bias"), reference=reference, split=split))
    for rows, D in LN_BWD_SHAPES:
        x, dy, dx = _rows("x", D, rows, 4), _rows("dy", D, rows, 8), _rows("dx", D, rows, 12, role="out")
        draw = _ln_draws(rows, D)

        def args(b, x=x, dy=dy, dx=dx, rows=rows, D=D):
            return [b.ptr("x"), b.ptr("dy"), rows, D, _ld(b, x), _ld(b, dy), b.ptr("weight"), EPS, b.ptr("dx"), _ld(b, dx), b.ptr("dweight"),
                    b.ptr("dbias"), b.workspace()[0], b.stream]

        def reference(draw=draw, rows=rows, D=D):
            from smokephysai_amd.models.attention import hip_layernorm_train
            d = draw()
            ln = _ln_module(d, D)
            xin = d["x"].cuda().reshape(rows, D).requires_grad_(True)
            hip_layernorm_train(xin, ln).backward(d["dy"].cuda().reshape(rows, D))
            return {"dx": xin.grad, "dweight": ln.weight.grad, "dbias": ln.bias.grad}
        cases.append(_mk(f"layernorm_backward-{rows}x{D}", "smk_layernorm_backward",
                         [x, dy, Buf("weight", F32, D, align=16), dx, Buf("dweight", F32, D, role="out"), Buf("dbias", F32, D, role="out")], args,
                         _pick(draw, "x", "dy", "weight"), query=lambda lib, D=D: lib.smk_layernorm_bwd_workspace(D), ws_align=16,
                         reference=reference))
    return cases


# ------------------------------------------------------------------------------------------------ attention (training form)
# A workgroup owns one (batch, head, 128-query block) and walks the keys in tiles of 64 (AT_QB, AT_KV); without a workspace and with
# at most one workgroup per CU the keys of a block are halved between two groups of waves (512 threads).  The backward runs one
# workgroup per 128-key block (dk, dv) and one per 128-query block (dq).  128 x 1 head: one block, two key tiles; 2 x 256 x 2: two blocks
# per (batch, head), four key tiles.  smk_attention_delta: one wave per row, four rows per workgroup, grid.y = ceil(H / 8): nine heads
# make a second, ragged group of heads.
ATTN_SHAPES = [(1, 128, 1), (2, 256, 2)]
DELTA_SHAPES = [(1, 1), (37, 9)]                                       # (rows, H)


@functools.lru_cache(maxsize=None)
def _attn_draws(shape):
    """q, k, v, dout [B L][H 64] and, in fp64 on the CPU, the forward's lse (log2 units) and delta = rowsum(dout * out) per head."""
    B, L, H = shape
    g = _gen(45, *shape)
    q, k, v, dout = (torch.randn(B, L, H, 64, generator=g) for _ in range(4))
    scale = 1.0 / 8.0
    s = torch.einsum("blhd,bmhd->bhlm", q.double(), k.double()) * (scale * math.log2(math.e))
    lse = torch.logsumexp(s * math.log(2.0), dim=-1) / math.log(2.0)                   # [B, H, L]
    p = torch.exp2(s - lse.unsqueeze(-1))
    out = torch.einsum("bhlm,bmhd->blhd", p, v.double())
    delta = (dout.double() * out).sum(-1)                                              # [B, L, H]
    flat = lambda t: t.reshape(B * L, H * 64).contiguous()                             # noqa: E731
    return {"q": flat(q), "k": flat(k), "v": flat(v), "dout": flat(dout), "lse": lse.permute(0, 2, 1).reshape(-1).float().contiguous(),
            "delta": delta.reshape(-1).float().contiguous()}


def attention_cases():
    cases = []
    for shape in ATTN_SHAPES:
        B, L, H = shape
        rows, cols = B * L, H * 64
        tag = f"{B}x{L}x{H}"
        q, k, v = _rows("q", cols, rows, 4), _rows("k", cols, rows, 8), _rows("v", cols, rows, 12)
        out = _rows("out", cols, rows, 16, role="out")
        cases.append(_mk(f"attention_forward_lse-{tag}", "smk_attention_forward_lse", [q, k, v, out, Buf("lse", F32, rows * H, role="out")],
                         lambda b, d=(B, L, H), t=(q, k, v, out): [b.ptr("q"), b.ptr("k"), b.ptr("v"), b.ptr("out"), b.ptr("lse"), *d, 64,
                                                                  *(_ld(b, x) for x in t), 0.125, b.stream],
                         lambda shape=shape: {n: _attn_draws(shape)[n] for n in ("q", "k", "v")}))
        dout = _rows("dout", cols, rows, 16)
        dq, dk, dv = _rows("dq", cols, rows, 20, role="out"), _rows("dk", cols, rows, 24, role="out"), _rows("dv", cols, rows, 28, role="out")
        cases.append(_mk(f"attention_backward-{tag}", "smk_attention_backward",
                         [q, k, v, dout, Buf("lse", F32, rows * H), Buf("delta", F32, rows * H), dq, dk, dv],
                         lambda b, d=(B, L, H), t=(q, k, v, dout, dq, dk, dv): [
                             b.ptr("q"), b.ptr("k"), b.ptr("v"), b.ptr("dout"), b.ptr("lse"), b.ptr("delta"), b.ptr("dq"), b.ptr("dk"), b.ptr("dv"),
                             *d, 64, *(_ld(b, x) for x in t), 0.125, b.stream],
                         lambda shape=shape: dict(_attn_draws(shape))))
    for rows, H in DELTA_SHAPES:
        cols = H * 64
        dout, out = _rows("dout", cols, rows, 4), _rows("out", cols, rows, 8)
        draw = _randn((46, rows, H), ("dout", rows * cols, 1.0), ("out", rows * cols, 1.0))

        def reference(draw=draw, rows=rows, H=H):
            from smokephysai_amd.models.attention import hip_attention_delta
            d = draw()
            return {"delta": hip_attention_delta(d["dout"].cuda().reshape(1, rows, H * 64), d["out"].cuda().reshape(1, rows, H * 64), H)}
        cases.append(_mk(f"attention_delta-{rows}x{H}", "smk_attention_delta", [dout, out, Buf("delta", F32, rows * H, role="out")],
                         lambda b, rows=rows, H=H, t=(dout, out): [b.ptr("dout"), b.ptr("out"), rows, H, 64, _ld(b, t[0]), _ld(b, t[1]),
                                                                  b.ptr("delta"), b.stream],
                         draw, reference=reference))
    return cases


# ------------------------------------------------------------------------------------------------ linear weight gradient
# The copying form: dY is transposed and padded to 64 x segments rows in the workspace, x is split behind it, the layer kernel runs over
# 128 x 128 tiles of dW and 1, 2, 4 ... segments of at least 1,024 rows, whose partial sums a last launch adds.  (1, 4, 32): the smallest;
# (300, 68, 96): ragged rows (300 = 4 x 64 + 44) and out_features (68 = 2 x 32 + 4); (2048, 4, 32): two segments.  The transposed-read form
# (out and in multiples of 128, rows >= 32, pitches multiples of 4, dy and x 16-byte aligned -- the header names all five): (512, 128, 128)
# gives it two segments of 256 rows, and runs a second time with dy and x 4-byte aligned and odd pitches, which sends the same shape to the
# copying form (its reference is the wrapper on a dy that starts 4 bytes into its storage: the two forms agree to rounding only).  At that
# shape the query returns the copying form's bytes, four times what the transposed-read form uses; at (512, 1024, 512) -- 8 x 4 tiles, two
# segments -- the transposed-read partials (4.2 MB) are the larger need, so the workspace ends exactly where they end.
#               shape, the form the case must take
WGRAD_CASES = [((1, 4, 32), "copy"), ((300, 68, 96), "copy"), ((2048, 4, 32), "copy"), ((512, 128, 128), "tr"), ((512, 128, 128), "copy"),
               ((512, 1024, 512), "tr")]


def linear_wgrad_cases():
    cases = []
    for shape, form in WGRAD_CASES:
        rows, out_f, in_f = shape
        fast_shape = out_f % 128 == 0 and in_f % 128 == 0 and rows >= 32
        assert form == "copy" or fast_shape
        tr = form == "tr"
        dy = _rows("dy", out_f, rows, 4 if tr else 3, align=16 if tr else 4)
        x = _rows("x", in_f, rows, 8 if tr else 5, align=16 if tr else 4)
        for db in ((False,) if shape == WGRAD_CASES[0][0] else ((True, False) if shape == WGRAD_CASES[1][0] else (True,))):
            bufs = [dy, x, Buf("dw", F32, out_f * in_f, align=16, role="out")] + ([Buf("db", F32, out_f, role="out")] if db else [])
            draw = _randn((47, *shape), ("dy", rows * out_f, 1.0), ("x", rows * in_f, 1.0))

            def reference(draw=draw, shape=shape, db=db, shifted=fast_shape and not tr):
                from smokephysai_amd.models.linear import hip_linear_wgrad
                d = draw()
                dy_t = d["dy"].cuda().reshape(shape[0], shape[1])
                if shifted:                                              # the copying form at a shape the other form would take
                    store = torch.empty(dy_t.numel() + 1, device="cuda")
                    store[1:].copy_(dy_t.reshape(-1))
                    dy_t = store[1:].view(shape[0], shape[1])
                    assert dy_t.data_ptr() % 16 == 4
                got = hip_linear_wgrad(dy_t, d["x"].cuda().reshape(shape[0], shape[2]), want_db=db)
                return {"dw": got[0], "db": got[1]} if db else {"dw": got}
            tag = f"linear_wgrad-{rows}x{out_f}x{in_f}-{'db' if db else 'nodb'}" + ("-copying" if fast_shape and not tr else "")
            cases.append(_mk(tag, "smk_linear_wgrad", bufs,
                             lambda b, s=shape, t=(dy, x): [b.ptr("dy"), _ld(b, t[0]), b.ptr("x"), _ld(b, t[1]), *s, b.ptr("dw"), b.ptr("db"),
                                                           *b.workspace(), b.stream],
                             draw, query=lambda lib, s=shape: lib.smk_linear_wgrad_workspace(*s), ws_align=16, db=db, form=form, reference=reference))
    return cases


# ------------------------------------------------------------------------------------------------ FFN element-wise chain
# One float4 per thread, min(16 x CUs, ceil(n / 1024)) workgroups; contiguous by contract, so the guards are the buffer ends.
# n = 4: one lane; n = 4,100: five workgroups, the last with one lane.
ELT_SIZES = [(4, 0.0, 0), (4100, 0.25, 0x1234_5678_9ABC)]             # (n, p, seed)
ELT_NAMES = ("gelu_dropout_fwd", "gelu_dropout_bwd", "dropout_add_fwd", "dropout_bwd")


def ffn_cases():
    cases = []
    for op, name in enumerate(ELT_NAMES):
        two = op in (1, 2)
        for n, p, seed in ELT_SIZES:
            bufs = [Buf("a", F32, n, align=16)] + ([Buf("b", F32, n, align=16)] if two else []) + [Buf("out", F32, n, align=16, role="out")]
            draw = _randn((48, op, n), ("a", n, 1.5), *([("b", n, 1.0)] if two else []))

            def reference(draw=draw, op=op, p=p, seed=seed, two=two):
                from smokephysai_amd.models.ffn import _run
                d = draw()
                return {"out": _run(op, d["a"].cuda(), d["b"].cuda() if two else None, p, seed)}
            cases.append(_mk(f"ffn_elementwise-{name}-{n}-p{p:g}", "smk_ffn_elementwise", bufs,
                             lambda b, op=op, n=n, p=p, seed=seed: [op, b.ptr("a"), b.ptr("b"), b.ptr("out"), n, p, seed, b.stream],
                             draw, reference=reference, op=op, p=p))
    return cases


# ------------------------------------------------------------------------------------------------ chaos term
# smk_lorenz_states: one thread per batch element, 64 per workgroup (B = 65: a second workgroup with one live lane).  smk_chaos_addend:
# one workgroup of 256 threads per batch element, striding over D (D = 260: a second pass with four live lanes); the batched form adds a
# grid axis over the layers.  addend [B][5][ld_addend]: columns D .. ld - 1 are guard.
CHAOS_SHAPES = [(1, 4), (3, 256), (65, 260)]                           # (B, D)
LORENZ = (10.0, 28.0, 8.0 / 3.0, 0.01)
CHAOS_LAYERS = 2


def _chaos_bufs(B, D, suffix="", pad=1):
    return [Buf("noise" + suffix, F32, 3 * B), Buf("proj_w" + suffix, F32, 3 * D), Buf("proj_b" + suffix, F32, D), Buf("gate_w" + suffix, F32, D),
            Buf("gate_b" + suffix, F32, 1), Buf("addend" + suffix, F32, D, 5 * B, D + pad, role="out")]


def _chaos_draws(B, D, suffix=""):
    return [("noise" + suffix, 3 * B, 1.0), ("proj_w" + suffix, 3 * D, 0.3), ("proj_b" + suffix, D, 0.1), ("gate_w" + suffix, D, 0.3),
            ("gate_b" + suffix, 1, 0.1)]


def chaos_cases():
    cases = []
    for B, D in CHAOS_SHAPES:
        cases.append(_mk(f"lorenz_states-{B}", "smk_lorenz_states", [Buf("noise", F32, 3 * B), Buf("states", F32, 15 * B, role="out")],
                         lambda b, B=B: [b.ptr("noise"), B, *LORENZ, b.ptr("states"), b.stream], _randn((49, B), ("noise", 3 * B, 1.0))))
        cases.append(_mk(f"chaos_addend-{B}x{D}", "smk_chaos_addend", _chaos_bufs(B, D),
                         lambda b, B=B, D=D: [b.ptr("noise"), B, D, b.ptr("proj_w"), b.ptr("proj_b"), b.ptr("gate_w"), b.ptr("gate_b"), 0.7, *LORENZ,
                                              b.ptr("addend"), b.stride("addend"), b.stream],
                         _randn((50, B, D), *_chaos_draws(B, D))))
    for B, D in CHAOS_SHAPES[:2]:
        bufs = [x for i in range(CHAOS_LAYERS) for x in _chaos_bufs(B, D, str(i), pad=1 + 2 * i)]
        draws = [x for i in range(CHAOS_LAYERS) for x in _chaos_draws(B, D, str(i))]

        def args(b, B=B, D=D):
            layers = (_lib.SmkChaosLayer * CHAOS_LAYERS)()
            for i in range(CHAOS_LAYERS):
                for f in ("noise", "proj_w", "proj_b", "gate_w", "gate_b", "addend"):
                    setattr(layers[i], f, b.ptr(f"{f}{i}"))
                layers[i].ld_addend, layers[i].strength = b.stride(f"addend{i}"), 0.7 + 0.2 * i
            return [CHAOS_LAYERS, C.cast(layers, C.c_void_p), B, D, *LORENZ, b.stream]
        cases.append(_mk(f"chaos_addend_batched-{B}x{D}-{CHAOS_LAYERS}layers", "smk_chaos_addend_batched", bufs, args, _randn((51, B, D), *draws),
                         layers=CHAOS_LAYERS))
    return cases


# ------------------------------------------------------------------------------------------------ gradient exchange
# Four elements per thread, 1,024 per workgroup, min(16 x CUs, ceil(n / 1024)) workgroups; a thread whose four elements cross n takes
# the scalar tail.  n = 4: one lane; 1,028: two workgroups; 1,030: the same with a tail of two (bf16 output: the buffer ends inside a
# 32-bit word).  Shards `stride` = n rounded up to a multiple of 4, + 4, elements apart (the header wants a multiple of 4).
WIRE = {F32: 0, BF16: 1}
#               world, in,   out,  n,    in place
SHARD_CASES = [(1, F32, F32, 4, False), (1, F32, BF16, 1028, False), (1, BF16, BF16, 4, False), (1, BF16, F32, 1028, False),
               (3, F32, F32, 1028, False), (3, F32, BF16, 4, False), (3, F32, BF16, 1030, False), (3, BF16, BF16, 1028, False),
               (3, BF16, F32, 4, False), (3, F32, F32, 1028, True), (3, BF16, BF16, 1030, True)]
DTYPE_NAME = {F32: "f32", BF16: "bf16"}


def _shard_case(world, tin, tout, n, in_place):
    stride = (n + 3) // 4 * 4 + 4
    align = {F32: 16, BF16: 8}
    shards = Buf("shards", tin, n, world, stride if world > 1 else None, align=align[tin], role="inout" if in_place else "in")
    bufs = [shards] + ([] if in_place else [Buf("out", tout, n, align=align[tout], role="out")])

    def inputs():
        t = torch.randn(world, n, generator=_gen(52, world, n, WIRE[tin], WIRE[tout])).to(tin)
        return {"shards": t if world > 1 else t.reshape(-1)}

    def args(b):
        return [b.ptr("shards"), WIRE[tin], world, n, stride, b.ptr("shards" if in_place else "out"), WIRE[tout],      # (one shard: no second one,
                #                                                                                      and a stride larger than n all the same)
                b.stream]

    def reference():
        from smokephysai_amd.utils.distributed import reduce_shards
        q = (n + 3) // 4 * 4                                            # the wrapper's shards are q = stride elements apart
        flat = torch.zeros(world, q, dtype=tin, device="cuda")
        flat[:, :n] = inputs()["shards"].cuda().reshape(world, n)
        out = flat[0] if in_place else torch.zeros(q, dtype=tout, device="cuda")
        reduce_shards(flat.reshape(-1), world, q, out)
        return {"shards": flat[:, :n].contiguous()} if in_place else {"out": out[:n].contiguous()}
    return _mk(f"reduce_shards-w{world}-{DTYPE_NAME[tin]}_{DTYPE_NAME[tout]}-{n}" + ("-inplace" if in_place else ""), "smk_reduce_shards", bufs, args,
               inputs, reference=reference, world=world, formats=(tin, tout), in_place=in_place)


def exchange_cases():
    return [_shard_case(*c) for c in SHARD_CASES]


# ------------------------------------------------------------------------------------------------ the table
def train_cases():
    return (conv1_cases() + conv2_cases() + bn_cases() + bn_cl_cases() + head_cases() + layernorm_cases() + attention_cases() +
            linear_wgrad_cases() + ffn_cases() + chaos_cases() + exchange_cases())


# (case id, buffer): the call with that one pointer half as well aligned as the entry point demands must come back with
# SMK_ERR_INVALID and touch nothing (test_a_weaker_alignment_is_refused).
REFUSED_ALIGNMENTS = [("conv1_train_dgrad-2x6x12", "dz"), ("conv1_train_dgrad-2x6x12", "dx"), ("bn_relu_pool_forward-2x16x64x64-pool2", "z"),
                      ("bn_relu_pool_forward-2x16x64x64-pool2", "workspace"), ("bn_relu_pool_backward-2x16x64x64-pool2", "dout"),
                      ("bn_relu_pool_phase-2x16x6x10-pool1-frozen-apply", "out"), ("bn_cl_phase-1x1x8x16-C64-dense-apply", "z"),
                      ("bn_cl_phase-1x1x8x16-C64-dense-stats", "workspace"), ("bn_cl_phase-1x2x32x32-C128-pooled-bwd_sums", "workspace"),
                      ("convt4s2_train_forward-1x16x32x16x16-nchw-bias", "x"), ("convt4s2_train_forward-1x16x32x16x16-nchw-bias", "z"),
                      ("convt4s2_train_dgrad-1x16x32x16x16-nchw", "dx"), ("convt4s2_train_wgrad-1x16x32x16x16-nchw-db", "workspace"),
                      ("conv3_sigmoid_train_backward-1x8x32-dw_db", "workspace"), ("layernorm-37x256-f32", "x"), ("layernorm-37x256-f32", "weight"),
                      ("layernorm_backward-37x256", "workspace"), ("attention_forward_lse-1x128x1", "k"), ("attention_backward-1x128x1", "dv"),
                      ("attention_delta-37x9", "out"), ("linear_wgrad-300x68x96-db", "dw"), ("linear_wgrad-300x68x96-db", "workspace"),
                      ("ffn_elementwise-dropout_add_fwd-4100-p0.25", "b"), ("reduce_shards-w3-f32_bf16-1030", "shards"),
                      ("reduce_shards-w3-f32_bf16-1030", "out")]
