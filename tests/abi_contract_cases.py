"""The case table of tests/test_hip_abi_contract.py: one entry per call of a stateless entry point of include/smokehip.h, with its
buffers as the guarded arena (tests/guarded_arena.py) lays them out, its ctypes argument list and a reference().

Every shape is the smallest at which the branches in question exist, every plane stride is strictly larger than its plane, every
workspace has exactly the bytes its smk_*_workspace query returns (NULL, 0 where that is 0), and every pointer has the weakest alignment
the header allows for it and nothing more (guarded_arena.weakest): 4 bytes for the renders' volumes, images and workspaces, the image
planes of quality.hip, the frames of the statistics and every tensor of the loss; 8 bytes for fp64 outputs, the flows and the workspaces
that hold fp64 partial sums; 16 bytes (not 32) for the loss workspace and every buffer of the 3-D training convolutions, whose
activations the header wants 16-byte aligned; 256 bytes for the optical-flow workspaces.  Where the header names no alignment the
element type's own is taken.

reference() returns the expected outputs from the project's ordinary path on dense, aligned, separately allocated tensors: the Python
wrapper (render_volumes and its autograd backward, render_orbit, render_camera, plane_quality_sums, plane_ssim's backward, chaos_stats,
frame_diff_norms, volume_stats, farneback_optical_flow, lucas_kanade_optical_flow, predict_and_score, the hip_conv3d_* functions of
models/encoder3d.py, HipAdamW.step() for the update without a clip), or -- for smk_grad_norm, the update with a caller's grad_scale and the
loss, whose wrappers keep part of what the entry points read or write to themselves (out[1], the scale, mass_diff) -- the same direct ABI
call the existing tests make (dense_reference).  Those paths are held to fp64 by the existing tests, so
the contract test needs no oracle of its own and compares bit for bit.  Inputs come from seeded CPU generators and are finite."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from guarded_arena import Buf                                    # noqa: E402
from render_oracle import AMBIENT, SIGMAS, density               # noqa: E402
from smokephysai_amd import _lib                                 # noqa: E402

F32, I32, U8, F64 = torch.float32, torch.int32, torch.uint8, torch.float64
LIGHT_ID = {"none": _lib.SMK_LIGHT_NONE, "+y": _lib.SMK_LIGHT_POS_Y, "-y": _lib.SMK_LIGHT_NEG_Y, "+z": _lib.SMK_LIGHT_POS_Z}


class Case:
    """id: the test id.  entry: the entry point.  bufs: its Buf list without the workspace.  query(lib) -> the workspace's bytes (None: the
    entry point takes none), ws_align its alignment.  inputs() -> {name: CPU tensor} of every "in" / "inout" buffer.  args(binder) -> the
    ctypes argument list.  reference() -> {name: expected device tensor} of every "out" / "inout" buffer."""

    def __init__(self, id, entry, bufs, args, inputs, reference, query=None, ws_align=4):
        self.id, self.entry, self.bufs, self.args, self.query, self.ws_align = id, entry, list(bufs), args, query, ws_align
        self.inputs = functools.lru_cache(maxsize=None)(inputs)
        self.reference = reference

    def workspace_bytes(self, lib) -> int:
        if self.query is None:
            return 0
        nbytes = int(self.query(lib))
        assert nbytes >= 0, f"{self.id}: the workspace query refused the shape ({nbytes})"
        return nbytes

    def buffers(self, lib):
        if self.query is None:
            return list(self.bufs)
        return self.bufs + [Buf("workspace", U8, self.workspace_bytes(lib), align=self.ws_align, role="ws")]

    def __repr__(self):
        return self.id


class DenseBinder:
    """The binder of dense_reference: every buffer an ordinary contiguous tensor of its own, dense strides."""

    def __init__(self, tensors, bufs, stream):
        self.t, self.bufs, self.stream = tensors, bufs, stream

    def ptr(self, name):
        return self.t[name].data_ptr() if name in self.t else None

    def stride(self, name):
        return self.bufs[name].elems

    def workspace(self, name="workspace"):
        return (self.t[name].data_ptr(), self.bufs[name].elems) if name in self.t else (None, 0)


def dense_reference(case):
    """The same entry point on ordinary tensors: contiguous, dense strides, each its own allocation (so 16-byte aligned and more), a
    workspace from torch.empty.  -> {name: tensor} of the outputs."""
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    bufs = {b.name: b for b in case.buffers(lib) if not (b.role == "ws" and b.elems == 0)}
    tensors, base = {}, {}
    for name, b in bufs.items():
        n = b.planes * b.elems
        base[name] = torch.empty(max(n, 1), dtype=b.dtype, device=dev)                  # (an empty row still has an address)
        tensors[name] = base[name][:n]
        assert base[name].data_ptr() % 256 == 0
    for name, t in case.inputs().items():
        tensors[name].copy_(t.reshape(-1))
    _lib.check(getattr(lib, case.entry)(*case.args(DenseBinder(base, bufs, _lib.stream_ptr(dev)))))
    torch.cuda.synchronize()
    return {n: tensors[n] for n, b in bufs.items() if b.role in ("out", "inout")}


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------ volume renders
RENDER_SHAPES = [(5, 37, 70), (17, 16, 65)]           # three 16-row segments + 5 rows, two 64-column chunks (6 live lanes), DMAX 8;
RENDER_N = 2                                           # one segment (forward workspace 0 -> NULL), DMAX 32 with 16 + 1 planes, a 1-lane chunk
SIGMA_VIEW, SIGMA_LIGHT = SIGMAS[0]
VIEWS = 2
AZIMUTHS, ELEVATIONS = (30.0, 200.0), (20.0, -35.0)


def _settings(light):
    from smokephysai_amd.physics import RenderSettings
    return RenderSettings(SIGMA_VIEW, SIGMA_LIGHT, AMBIENT, 1.0, light)


def _desc(light):
    return _lib.SmkRenderDesc(float(SIGMA_VIEW), float(SIGMA_LIGHT), float(AMBIENT), 1.0, LIGHT_ID[light])


def _render_vols(shape):
    return torch.from_numpy(density("sparse", (RENDER_N,) + shape, seed=sum(shape))).reshape(RENDER_N, -1)


def _render_grads(shape):
    g = _gen(11, *shape)
    D, H, W = shape
    return torch.randn(RENDER_N, H * W, generator=g), torch.randn(RENDER_N, H * W, generator=g)


def _render_case(shape, light, trans=True):
    D, H, W = shape
    cells, hw = D * H * W, H * W
    bufs = [Buf("vols", F32, cells, RENDER_N, cells + 3), Buf("image", F32, hw, RENDER_N, hw + 1, role="out")]
    if trans:
        bufs.append(Buf("trans", F32, hw, RENDER_N, hw + 2, role="out"))
    desc = _desc(light)

    def args(b):
        return [b.ptr("vols"), b.stride("vols"), RENDER_N, D, H, W, C.byref(desc), b.ptr("image"), b.stride("image"),
                b.ptr("trans") if trans else None, b.stride("trans") if trans else hw, *b.workspace(), b.stream]

    def reference():
        from smokephysai_amd.physics import render_volumes
        vols = _render_vols(shape).cuda().reshape(RENDER_N, D, H, W)
        if trans:
            img, T = render_volumes(vols, _settings(light), transmittance=True)
            return {"image": img, "trans": T}
        return {"image": render_volumes(vols, _settings(light))}
    return Case(f"render-{D}x{H}x{W}-{light}" + ("" if trans else "-notrans"), "smk_volume_render", bufs, args,
                lambda: {"vols": _render_vols(shape)}, reference,
                query=lambda lib: lib.smk_volume_render_workspace(RENDER_N, D, H, W, LIGHT_ID[light]))


def _render_backward_case(shape, light, use_g=True, use_gt=True):
    D, H, W = shape
    cells, hw = D * H * W, H * W
    bufs = [Buf("vols", F32, cells, RENDER_N, cells + 3)]
    if use_g:
        bufs.append(Buf("grad_image", F32, hw, RENDER_N, hw + 1))
    if use_gt:
        bufs.append(Buf("grad_trans", F32, hw, RENDER_N, hw + 2))
    bufs.append(Buf("grad_vols", F32, cells, RENDER_N, cells + 5, role="out"))
    desc = _desc(light)

    def inputs():
        G, Gt = _render_grads(shape)
        d = {"vols": _render_vols(shape)}
        if use_g:
            d["grad_image"] = G
        if use_gt:
            d["grad_trans"] = Gt
        return d

    def args(b):
        return [b.ptr("vols"), b.stride("vols"), RENDER_N, D, H, W, C.byref(desc),
                b.ptr("grad_image") if use_g else None, b.stride("grad_image") if use_g else hw,
                b.ptr("grad_trans") if use_gt else None, b.stride("grad_trans") if use_gt else hw,
                b.ptr("grad_vols"), b.stride("grad_vols"), *b.workspace(), b.stream]

    def reference():
        from smokephysai_amd.physics import render_volumes
        vols = _render_vols(shape).cuda().reshape(RENDER_N, D, H, W).requires_grad_(True)
        G, Gt = (t.cuda().reshape(RENDER_N, H, W) for t in _render_grads(shape))
        img, T = render_volumes(vols, _settings(light), transmittance=True)
        outs, grads = zip(*[(o, g) for o, g, use in ((img, G, use_g), (T, Gt, use_gt)) if use])
        torch.autograd.backward(outs, grads)
        return {"grad_vols": vols.grad}
    which = "" if use_g and use_gt else ("-G" if use_g else "-Gt")
    return Case(f"render_backward-{D}x{H}x{W}-{light}{which}", "smk_volume_render_backward", bufs, args, inputs, reference,
                query=lambda lib: lib.smk_volume_render_backward_workspace(RENDER_N, D, H, W, LIGHT_ID[light]))


def _moving_camera_case(kind, shape, light):
    D, H, W = shape
    cells, hw, planes = D * H * W, H * W, RENDER_N * VIEWS
    bufs = [Buf("vols", F32, cells, RENDER_N, cells + 3), Buf("image", F32, hw, planes, hw + 1, role="out"),
            Buf("trans", F32, hw, planes, hw + 2, role="out")]
    desc = _desc(light)
    az = (C.c_double * planes)(*(AZIMUTHS * RENDER_N))
    el = (C.c_double * planes)(*(ELEVATIONS * RENDER_N))

    def args(b):
        angles = [az] if kind == "orbit" else [az, el]
        return [b.ptr("vols"), b.stride("vols"), RENDER_N, D, H, W, C.byref(desc), *angles, VIEWS, b.ptr("image"), b.stride("image"),
                b.ptr("trans"), b.stride("trans"), *b.workspace(), b.stream]

    def reference():
        from smokephysai_amd.physics import render_camera, render_orbit
        vols = _render_vols(shape).cuda().reshape(RENDER_N, D, H, W)
        if kind == "orbit":
            img, T = render_orbit(vols, list(AZIMUTHS), _settings(light), transmittance=True)
        else:
            img, T = render_camera(vols, list(AZIMUTHS), list(ELEVATIONS), _settings(light), transmittance=True)
        return {"image": img, "trans": T}
    return Case(f"render_{kind}-{D}x{H}x{W}-{light}", f"smk_volume_render_{kind}", bufs, args, lambda: {"vols": _render_vols(shape)}, reference,
                query=lambda lib: getattr(lib, f"smk_volume_render_{kind}_workspace")(RENDER_N, D, H, W, LIGHT_ID[light]))


def render_cases():
    cases = []
    for shape in RENDER_SHAPES:
        cases += [_render_case(shape, light) for light in ("none", "+y", "-y", "+z")]
    cases.append(_render_case(RENDER_SHAPES[0], "-y", trans=False))
    for shape in RENDER_SHAPES:
        cases += [_render_backward_case(shape, light) for light in ("none", "+y", "-y", "+z")]
    cases += [_render_backward_case(RENDER_SHAPES[0], "+y", use_gt=False), _render_backward_case(RENDER_SHAPES[0], "+y", use_g=False)]
    for kind in ("orbit", "camera"):
        for shape in RENDER_SHAPES:
            cases += [_moving_camera_case(kind, shape, light) for light in ("none", "+y", "-y")]
    return cases


# ------------------------------------------------------------------------------------------------ image quality
Q_N, Q_H, Q_W, Q_WINDOW = 3, 37, 53, 11


def _quality_inputs():
    g = _gen(3, Q_H, Q_W)
    pred = torch.rand(Q_N, Q_H * Q_W, generator=g)
    target = (pred + 0.1 * torch.randn(Q_N, Q_H * Q_W, generator=g)).clamp(0, 1)
    return pred, target, torch.randn(Q_N, generator=g)


def quality_cases():
    from smokephysai_amd.evaluation.robustness_metrics import C1, C2
    hw = Q_H * Q_W
    planes = [Buf("pred", F32, hw, Q_N, hw + 1), Buf("target", F32, hw, Q_N, hw + 3)]

    def fwd_args(b):
        return [b.ptr("pred"), b.stride("pred"), b.ptr("target"), b.stride("target"), Q_N, Q_H, Q_W, Q_WINDOW, float(C1), float(C2),
                *b.workspace(), b.ptr("ssim_sum"), b.ptr("sqerr_sum"), b.stream]

    def fwd_reference():
        from smokephysai_amd.evaluation.robustness_metrics import plane_quality_sums
        pred, target, _ = (t.cuda() for t in _quality_inputs())
        ssim, sqerr = plane_quality_sums(pred.reshape(Q_N, Q_H, Q_W), target.reshape(Q_N, Q_H, Q_W), Q_WINDOW)
        return {"ssim_sum": ssim, "sqerr_sum": sqerr}

    def bwd_args(b):
        return [b.ptr("pred"), b.stride("pred"), b.ptr("target"), b.stride("target"), Q_N, Q_H, Q_W, Q_WINDOW, float(C1), float(C2),
                b.ptr("plane_grad"), *b.workspace(), b.ptr("dpred"), b.stride("dpred"), b.stream]

    def bwd_reference():
        from smokephysai_amd.evaluation.robustness_metrics import plane_ssim
        pred, target, g = (t.cuda() for t in _quality_inputs())
        pred = pred.reshape(Q_N, Q_H, Q_W).requires_grad_(True)
        plane_ssim(pred, target.reshape(Q_N, Q_H, Q_W), Q_WINDOW).backward(g)
        return {"dpred": pred.grad}
    return [Case("image_quality", "smk_image_quality",
                 planes + [Buf("ssim_sum", F64, Q_N, align=8, role="out"), Buf("sqerr_sum", F64, Q_N, align=8, role="out")], fwd_args,
                 lambda: dict(zip(("pred", "target"), _quality_inputs()[:2])), fwd_reference,
                 query=lambda lib: lib.smk_image_quality_workspace(Q_N, Q_H, Q_W), ws_align=8),
            Case("image_quality_backward", "smk_image_quality_backward",
                 planes + [Buf("plane_grad", F32, Q_N), Buf("dpred", F32, hw, Q_N, hw + 1, role="out")], bwd_args,
                 lambda: dict(zip(("pred", "target", "plane_grad"), _quality_inputs())), bwd_reference,
                 query=lambda lib: lib.smk_image_quality_backward_workspace(Q_N, Q_H, Q_W))]


# ------------------------------------------------------------------------------------------------ statistics
STAT_N, STAT_H, STAT_W = 3, 100, 76
VOLUME_STAT_SHAPES = [(13, 40, 70), (1, 33, 65)]


def _frames(n, cells, *seed):
    return torch.rand(n, cells, generator=_gen(*seed)) ** 3


def stats_cases():
    hw = STAT_H * STAT_W
    frames = Buf("frames", F32, hw, STAT_N, hw + 2)

    def stats_args(b):
        return [b.ptr("frames"), b.stride("frames"), STAT_N, STAT_H, STAT_W, b.ptr("means"), b.ptr("box_counts"), b.ptr("hist"), b.stream]

    def stats_reference():
        from smokephysai_amd.physics.smoke_simulator import chaos_stats
        means, box, hist = chaos_stats(_frames(STAT_N, hw, 5).cuda().reshape(STAT_N, STAT_H, STAT_W))
        return {"means": means, "box_counts": box, "hist": hist}

    def norms_args(b):
        return [b.ptr("frames"), b.stride("frames"), STAT_N, STAT_H, STAT_W, b.ptr("norms"), b.stream]

    def norms_reference():
        from smokephysai_amd.physics.smoke_simulator import frame_diff_norms
        return {"norms": frame_diff_norms(_frames(STAT_N, hw, 5).cuda().reshape(STAT_N, STAT_H, STAT_W))}
    cases = [Case("chaos_stats", "smk_chaos_stats",
                  [frames, Buf("means", F32, STAT_N, role="out"), Buf("box_counts", I32, 5 * STAT_N, role="out"), Buf("hist", I32, 256 * STAT_N, role="out")],
                  stats_args, lambda: {"frames": _frames(STAT_N, hw, 5)}, stats_reference),
             Case("frame_diff_norms", "smk_frame_diff_norms", [frames, Buf("norms", F32, STAT_N - 1, role="out")], norms_args,
                  lambda: {"frames": _frames(STAT_N, hw, 5)}, norms_reference)]
    for shape in VOLUME_STAT_SHAPES:
        cases.append(_volume_stats_case(shape))
    return cases


def _volume_stats_case(shape):
    D, H, W = shape
    cells = D * H * W

    def args(b):
        return [b.ptr("vols"), b.stride("vols"), STAT_N, D, H, W, b.ptr("means"), b.ptr("box_counts"), b.ptr("hist"), b.ptr("norms"),
                *b.workspace(), b.stream]

    def reference():
        from smokephysai_amd.physics.smoke_simulator import volume_stats
        vols = _frames(STAT_N, cells, 9, *shape).cuda()
        means, box, hist, norms = volume_stats(vols.reshape((STAT_N, H, W) if D == 1 else (STAT_N, D, H, W)), norms=True)
        return {"means": means, "box_counts": box, "hist": hist, "norms": norms}
    return Case(f"volume_stats-{D}x{H}x{W}", "smk_volume_stats",
                [Buf("vols", F32, cells, STAT_N, cells + 1), Buf("means", F32, STAT_N, role="out"), Buf("box_counts", I32, 5 * STAT_N, role="out"),
                 Buf("hist", I32, 256 * STAT_N, role="out"), Buf("norms", F32, STAT_N - 1, role="out")], args,
                lambda: {"vols": _frames(STAT_N, cells, 9, *shape)}, reference,
                query=lambda lib: lib.smk_volume_stats_workspace(STAT_N, D, H, W), ws_align=8)


# ------------------------------------------------------------------------------------------------ optical flow
FLOW_N = 3
FLOW_SHAPES = [(40, 72), (64, 96)]        # one pyramid level; two levels whose sizes differ per axis


@functools.lru_cache(maxsize=None)
def _flow_frames(shape):
    """Two shifted pairs of optical_flow_oracle and one pair of independent noise, uint8 [3, H*W] each; a seeded flow field for the warp."""
    from optical_flow_oracle import shifted_pair
    H, W = shape
    pairs = [shifted_pair(H, W, seed=H + W), shifted_pair(H, W, seed=H + W + 1, shift=(-3, 2))]
    rng = np.random.RandomState(H * W)
    pairs.append((rng.randint(0, 256, (H, W)).astype(np.uint8), rng.randint(0, 256, (H, W)).astype(np.uint8)))
    prev = torch.from_numpy(np.stack([np.ascontiguousarray(p[0]) for p in pairs])).reshape(FLOW_N, H * W)
    nxt = torch.from_numpy(np.stack([np.ascontiguousarray(p[1]) for p in pairs])).reshape(FLOW_N, H * W)
    flow = torch.randn(FLOW_N * H * W * 2, generator=_gen(17, H, W)) * 2.5
    return prev, nxt, flow


def _flow_cases(shape):
    H, W = shape
    hw = H * W
    prev, nxt = Buf("prev", U8, FLOW_N * hw), Buf("next", U8, FLOW_N * hw)
    frames = lambda: {"prev": _flow_frames(shape)[0].reshape(-1), "next": _flow_frames(shape)[1].reshape(-1)}         # noqa: E731

    def method_args(b):
        return [b.ptr("prev"), b.ptr("next"), FLOW_N, H, W, b.ptr("flow"), *b.workspace(), b.stream]

    def method_reference(fn):
        def reference():
            from smokephysai_amd.evaluation import optical_flow
            p, n, _ = _flow_frames(shape)
            return {"flow": getattr(optical_flow, fn)(p.cuda().reshape(FLOW_N, H, W), n.cuda().reshape(FLOW_N, H, W))}
        return reference

    def warp_args(b):
        return [b.ptr("prev"), b.ptr("flow"), b.ptr("next"), FLOW_N, H, W, b.ptr("pred"), b.ptr("mse"), *b.workspace(), b.stream]

    def warp_reference():
        from smokephysai_amd.evaluation.optical_flow import predict_and_score
        p, n, f = _flow_frames(shape)
        pred, mse = predict_and_score(p.cuda().reshape(FLOW_N, H, W), f.cuda().reshape(FLOW_N, H, W, 2), n.cuda().reshape(FLOW_N, H, W))
        return {"pred": pred, "mse": mse}
    flow_out = Buf("flow", F32, FLOW_N * hw * 2, align=8, role="out")
    return [Case(f"flow_farneback-{H}x{W}", "smk_flow_farneback", [prev, nxt, flow_out], method_args, frames, method_reference("farneback_optical_flow"),
                 query=lambda lib: lib.smk_flow_farneback_workspace(FLOW_N, H, W), ws_align=256),
            Case(f"flow_lucas_kanade-{H}x{W}", "smk_flow_lucas_kanade", [prev, nxt, flow_out], method_args, frames,
                 method_reference("lucas_kanade_optical_flow"), query=lambda lib: lib.smk_flow_lk_workspace(FLOW_N, H, W), ws_align=256),
            Case(f"warp_frames-{H}x{W}", "smk_warp_frames",
                 [prev, nxt, Buf("flow", F32, FLOW_N * hw * 2, align=8), Buf("pred", U8, FLOW_N * hw, role="out"), Buf("mse", F64, FLOW_N, align=8, role="out")],
                 warp_args, lambda: dict(frames(), flow=_flow_frames(shape)[2]), warp_reference,
                 query=lambda lib: lib.smk_warp_workspace(FLOW_N, H, W), ws_align=256)]


def flow_cases():
    return [c for shape in FLOW_SHAPES for c in _flow_cases(shape)]


# ------------------------------------------------------------------------------------------------ train-step tail: optimizer table
OPT_ROWS = [1, 3, 5, 1027, 8193, 0]
OPT_MISALIGNED = {3: ("param", "grad", "exp_avg", "exp_avg_sq"), 4: ("exp_avg",)}      # row -> the pointers that are 4-byte aligned only
OPT_FIELDS = ("param", "grad", "exp_avg", "exp_avg_sq")
LR, WD, BETAS, EPS, STEP, MAX_NORM, GRAD_SCALE = 1e-3, 0.01, (0.9, 0.999), 1e-8, 3, 1.0, 0.37


def _opt_bufs(roles):
    """Every param / grad / exp_avg / exp_avg_sq its own arena buffer.  Rows 0-2 and the empty row: 4-byte aligned only, as the 1027
    row; the 8193 row 16-byte aligned except exp_avg, so that the 16-byte path must be refused on account of one pointer."""
    bufs = []
    for i, n in enumerate(OPT_ROWS):
        for f in OPT_FIELDS:
            weak = i != 4 or f in OPT_MISALIGNED[4]
            bufs.append(Buf(f"{f}{i}", F32, n, align=4 if weak else 16, phase=4 if weak else 16, role=roles[f]))
    return bufs


def _opt_inputs():
    g = _gen(23)
    d = {}
    for i, n in enumerate(OPT_ROWS):
        d[f"param{i}"] = torch.randn(n, generator=g)
        d[f"grad{i}"] = torch.randn(n, generator=g) * 10.0 ** (i % 3 - 1)
        d[f"exp_avg{i}"] = torch.randn(n, generator=g) * 0.1
        d[f"exp_avg_sq{i}"] = torch.rand(n, generator=g) * 0.01
    return d


def _opt_table(b):
    rows = (_lib.SmkOptTensor * len(OPT_ROWS))()
    for i, n in enumerate(OPT_ROWS):
        for f in OPT_FIELDS:
            setattr(rows[i], f, b.ptr(f"{f}{i}"))
        rows[i].n = n
    return rows


def _opt_sizes_only():
    rows = (_lib.SmkOptTensor * len(OPT_ROWS))()
    for i, n in enumerate(OPT_ROWS):
        rows[i].n = n
    return rows


def optimizer_cases():
    def norm_args(b):
        return [_opt_table(b), len(OPT_ROWS), MAX_NORM, b.ptr("out"), *b.workspace(), b.stream]

    def step_args(write_grad):
        def args(b):
            return [_opt_table(b), len(OPT_ROWS), LR, BETAS[0], BETAS[1], EPS, WD, 1.0 - BETAS[0] ** STEP, 1.0 - BETAS[1] ** STEP,
                    b.ptr("grad_scale") if write_grad else None, write_grad, b.stream]
        return args
    read_only = dict.fromkeys(OPT_FIELDS, "in")
    updated = dict(param="inout", grad="in", exp_avg="inout", exp_avg_sq="inout")
    cases = [Case("grad_norm", "smk_grad_norm", _opt_bufs(read_only) + [Buf("out", F32, 2, role="out")], norm_args, _opt_inputs, None,
                  query=lambda lib: lib.smk_grad_norm_workspace(_opt_sizes_only(), len(OPT_ROWS)), ws_align=8),
             Case("adamw_step-keep_grad", "smk_adamw_step", _opt_bufs(updated), step_args(0), _opt_inputs, None),
             Case("adamw_step-write_grad", "smk_adamw_step", _opt_bufs(dict(updated, grad="inout")) + [Buf("grad_scale", F32, 1)], step_args(1),
                  lambda: dict(_opt_inputs(), grad_scale=torch.tensor([GRAD_SCALE])), None)]
    for c in cases:
        c.reference = functools.partial(dense_reference, c)
    cases[1].reference = _hip_adamw_reference          # no clip, write_grad = 0: exactly what HipAdamW.step() asks of the entry point
    return cases


def _hip_adamw_reference():
    """smk_adamw_step through HipAdamW: the rows as ordinary parameters with their gradients, the moments and step STEP - 1 as its state."""
    from smokephysai_amd.optim import HipAdamW
    d = {k: v.cuda() for k, v in _opt_inputs().items()}
    params = [torch.nn.Parameter(d[f"param{i}"]) for i in range(len(OPT_ROWS))]
    opt = HipAdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    for i, p in enumerate(params):
        p.grad = d[f"grad{i}"]
        opt.state[p] = {"step": torch.tensor(float(STEP - 1)), "exp_avg": d[f"exp_avg{i}"], "exp_avg_sq": d[f"exp_avg_sq{i}"]}
    opt.step()
    assert opt._table is not None and opt._table[1] is not None, "HipAdamW left the HIP route"
    out = {}
    for i, p in enumerate(params):
        out[f"param{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    return out


# ------------------------------------------------------------------------------------------------ train-step tail: loss
LOSS_NAMES = ("1x1_T1", "4x128_T20_256")            # the smallest and the largest entry of test_hip_train_tail.LOSS_SHAPES
LOSS_SHAPES = {"1x1_T1": ((1, 1, 1, 1), (1, 1, 1, 1)), "4x128_T20_256": ((4, 1, 128, 128), (4, 20, 256, 256))}
W_MASS, W_CONT, W_CHAOS, W_PHYS = 0.7, 1.3, 0.1, 0.05


def _loss_draws(name):
    from test_hip_train_tail import LOSS_SHAPES as THEIRS, _loss_inputs
    assert THEIRS[name] == LOSS_SHAPES[name] and (W_MASS, W_CONT, W_CHAOS, W_PHYS) == (0.7, 1.3, 0.1, 0.05)
    return _loss_inputs(name)


def _loss_cases(name):
    shape, seq_shape = LOSS_SHAPES[name]
    plane_elems = shape[-2] * shape[-1]
    planes = math.prod(shape) // plane_elems
    n_chaos = shape[0] * 3
    sb, sT, sp = seq_shape[0], seq_shape[1], seq_shape[2] * seq_shape[3]
    common = [Buf("pred", F32, planes * plane_elems), Buf("target", F32, planes * plane_elems), Buf("chaos_pred", F32, n_chaos),
              Buf("chaos_target", F32, n_chaos)]

    def fwd_inputs():
        pred, target, cp, ct, seq = _loss_draws(name)
        return {"pred": pred.reshape(-1), "target": target.reshape(-1), "chaos_pred": cp.reshape(-1), "chaos_target": ct.reshape(-1),
                "sequence": seq.reshape(-1)}

    def fwd_args(b):
        return [b.ptr("pred"), b.ptr("target"), planes, plane_elems, b.ptr("chaos_pred"), b.ptr("chaos_target"), n_chaos, b.ptr("sequence"),
                sb, sT, sp, W_CHAOS, W_PHYS, W_MASS, W_CONT, b.ptr("out"), b.ptr("mass_diff"), *b.workspace(), b.stream]

    def bwd_inputs():
        d = fwd_inputs()
        del d["sequence"]
        g = _gen(29, planes)
        d["mass_diff"] = torch.randn(planes, generator=g)
        d["grad_out"] = torch.randn(6, generator=g)
        return d

    def bwd_args(with_chaos):
        def args(b):
            return [b.ptr("pred"), b.ptr("target"), planes, plane_elems, b.ptr("mass_diff"), b.ptr("chaos_pred"), b.ptr("chaos_target"), n_chaos,
                    b.ptr("grad_out"), W_CHAOS, W_PHYS, W_MASS, b.ptr("d_pred"), b.ptr("d_chaos") if with_chaos else None, b.stream]
        return args
    bwd = common + [Buf("mass_diff", F32, planes), Buf("grad_out", F32, 6), Buf("d_pred", F32, planes * plane_elems, role="out")]
    cases = [Case(f"train_loss_forward-{name}", "smk_train_loss_forward",
                  common + [Buf("sequence", F32, sb * sT * sp), Buf("out", F32, 6, role="out"), Buf("mass_diff", F32, planes, role="out")],
                  fwd_args, fwd_inputs, None, query=lambda lib: lib.smk_train_loss_workspace(planes, plane_elems, sb, sT, sp), ws_align=16),
             Case(f"train_loss_backward-{name}", "smk_train_loss_backward", bwd + [Buf("d_chaos", F32, n_chaos, role="out")], bwd_args(True),
                  bwd_inputs, None)]
    if name == LOSS_NAMES[0]:
        cases.append(Case(f"train_loss_backward-{name}-no_d_chaos", "smk_train_loss_backward", bwd, bwd_args(False), bwd_inputs, None))
    for c in cases:
        c.reference = functools.partial(dense_reference, c)
    return cases


def loss_cases():
    return [c for name in LOSS_NAMES for c in _loss_cases(name)]


# ------------------------------------------------------------------------------------------------ 3-D training convolutions
CONV3D_SHAPES = [(2, 2, 8, 16), (1, 3, 16, 48)]


def _conv3d_draws(shape):
    from test_hip_conv3d_train import _reference
    return _reference(shape)


def _conv3d_cases(shape):
    B, D, H, W = shape
    vox = B * D * H * W

    def buf(name, n, role="in"):
        return Buf(name, F32, n, align=16, role=role)

    def draws(*names):
        return lambda: {n: _conv3d_draws(shape)[n].reshape(-1) for n in names}

    def dev(*names):
        r = _conv3d_draws(shape)
        return [r[n].cuda() for n in names]
    train_ws = lambda lib: lib.smk_conv3d_train_workspace()          # noqa: E731
    dims = [B, D, H, W]

    def s7_forward_reference():
        from smokephysai_amd.models.encoder3d import _HipConv3dS7TrainFn
        return {"z1": _HipConv3dS7TrainFn.apply(*dev("vol", "w1", "b1"))}

    def cl_forward_reference():
        from smokephysai_amd.models.encoder3d import hip_conv3d_cl_forward_raw
        return {"z2": hip_conv3d_cl_forward_raw(*dev("a1", "w2", "b2"))}

    def cl_dgrad_reference():
        from smokephysai_amd.models.encoder3d import hip_conv3d_cl_dgrad
        return {"da1": hip_conv3d_cl_dgrad(*dev("dz2", "w2"))}

    def cl_wgrad_reference():
        from smokephysai_amd.models.encoder3d import hip_conv3d_cl_wgrad
        dw, db = hip_conv3d_cl_wgrad(*dev("dz2", "a1"))
        return {"dw": dw, "db": db}

    def s7_dgrad_reference():
        from smokephysai_amd.models.encoder3d import hip_conv3d_s7_dgrad
        return {"dvol": hip_conv3d_s7_dgrad(*dev("dz1", "w1"))}
    tag = "x".join(map(str, shape))
    return [Case(f"conv3d_s7_train_forward-{tag}", "smk_conv3d_s7_train_forward",
                 [buf("vol", vox), buf("w1", 64 * 343), buf("b1", 64), buf("z1", vox * 64, "out")],
                 lambda b: [b.ptr("vol"), b.ptr("w1"), b.ptr("b1"), *dims, b.ptr("z1"), b.workspace()[0], b.stream],
                 draws("vol", "w1", "b1"), s7_forward_reference, query=train_ws, ws_align=16),
            Case(f"conv3d_cl_train_forward-{tag}", "smk_conv3d_cl_train_forward",
                 [buf("a1", vox * 64), buf("w2", 128 * 64 * 27), buf("b2", 128), buf("z2", vox * 128, "out")],
                 lambda b: [b.ptr("a1"), b.ptr("w2"), b.ptr("b2"), *dims, b.ptr("z2"), b.workspace()[0], b.stream],
                 draws("a1", "w2", "b2"), cl_forward_reference, query=train_ws, ws_align=16),
            Case(f"conv3d_cl_dgrad-{tag}", "smk_conv3d_cl_dgrad", [buf("dz2", vox * 128), buf("w2", 128 * 64 * 27), buf("da1", vox * 64, "out")],
                 lambda b: [b.ptr("dz2"), b.ptr("w2"), *dims, b.ptr("da1"), b.workspace()[0], b.stream],
                 draws("dz2", "w2"), cl_dgrad_reference, query=train_ws, ws_align=16),
            Case(f"conv3d_cl_wgrad-{tag}", "smk_conv3d_cl_wgrad",
                 [buf("dz2", vox * 128), buf("a1", vox * 64), buf("dw", 128 * 64 * 27, "out"), buf("db", 128, "out")],
                 lambda b: [b.ptr("dz2"), b.ptr("a1"), *dims, b.ptr("dw"), b.ptr("db"), b.workspace()[0], b.stream],
                 draws("dz2", "a1"), cl_wgrad_reference, query=lambda lib: lib.smk_conv3d_cl_wgrad_workspace(B, D, H, W), ws_align=16),
            Case(f"conv3d_s7_dgrad-{tag}", "smk_conv3d_s7_dgrad", [buf("dz1", vox * 64), buf("w1", 64 * 343), buf("dvol", vox, "out")],
                 lambda b: [b.ptr("dz1"), b.ptr("w1"), *dims, b.ptr("dvol"), b.workspace()[0], b.stream],
                 draws("dz1", "w1"), s7_dgrad_reference, query=train_ws, ws_align=16)]


def conv3d_cases():
    return [c for shape in CONV3D_SHAPES for c in _conv3d_cases(shape)]


# ------------------------------------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def all_cases():
    from abi_contract_cases_train import train_cases                 # (imported here: that module takes Case and dense_reference from this one)
    cases = render_cases() + quality_cases() + stats_cases() + flow_cases() + optimizer_cases() + loss_cases() + conv3d_cases() + train_cases()
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


ENTRY_POINTS = ("smk_volume_render", "smk_volume_render_backward", "smk_volume_render_orbit", "smk_volume_render_camera", "smk_image_quality",
                "smk_image_quality_backward", "smk_chaos_stats", "smk_frame_diff_norms", "smk_volume_stats", "smk_flow_farneback",
                "smk_flow_lucas_kanade", "smk_warp_frames", "smk_grad_norm", "smk_adamw_step", "smk_train_loss_forward", "smk_train_loss_backward",
                "smk_conv3d_s7_train_forward", "smk_conv3d_cl_train_forward", "smk_conv3d_cl_dgrad", "smk_conv3d_cl_wgrad", "smk_conv3d_s7_dgrad",
                # the training step's calls: tests/abi_contract_cases_train.py
                "smk_conv1_train_forward", "smk_conv1_train_wgrad", "smk_conv1_train_dgrad", "smk_conv2_train_forward", "smk_conv2_train_dgrad",
                "smk_conv2_train_wgrad", "smk_bn_relu_pool_forward", "smk_bn_relu_pool_backward", "smk_bn_relu_pool_phase", "smk_bn_cl_phase",
                "smk_convt4s2_train_forward", "smk_convt4s2_train_dgrad", "smk_convt4s2_train_wgrad", "smk_conv3_sigmoid_train_forward",
                "smk_conv3_sigmoid_train_backward", "smk_layernorm", "smk_layernorm_backward", "smk_attention_forward_lse", "smk_attention_backward",
                "smk_attention_delta", "smk_linear_wgrad", "smk_ffn_elementwise", "smk_lorenz_states", "smk_chaos_addend", "smk_chaos_addend_batched",
                "smk_reduce_shards")
