"""smk_volume_render_camera_backward held to what include/smokehip.h promises about memory and streams, in the harness of
tests/test_hip_abi_contract.py (tests/guarded_arena.py): every buffer of the call lies in one arena the test owns, the planes strided, the
pointers 4-byte aligned and no better, the workspace exactly as large as smk_volume_render_camera_backward_workspace says, every other byte
a guard.  The cases are built like _render_backward_case of tests/abi_contract_cases.py: its two shapes and two volumes, two
(azimuth, elevation) views per volume, the three lights of a moving camera, and G alone / Gt alone once each.

For every case: no guard word changes under a NaN fill or a zero fill; the outputs of the two runs are bit-equal, hold no fill word and are
finite (the call reads nothing foreign -- unwritten scratch included -- and writes every element of grad_vols); they equal the dense,
aligned call that render_camera(..., differentiable=True) makes; and the call runs on the caller's stream without waiting for it."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from abi_contract_cases import AZIMUTHS, ELEVATIONS, F32, LIGHT_ID, RENDER_N, RENDER_SHAPES, VIEWS, Case, _desc, _gen, _render_vols, _settings  # noqa: E402
from guarded_arena import FILL_NAN, FILL_ZERO, Buf, bits, holds_fill, run_guarded                                                  # noqa: E402
from test_hip_abi_contract import DELAY_SECONDS, independent_side_stream, sleep_cycles_per_second                                   # noqa: E402


def _grads(shape):
    g = _gen(17, *shape)
    D, H, W = shape
    return torch.randn(RENDER_N * VIEWS, H * W, generator=g), torch.randn(RENDER_N * VIEWS, H * W, generator=g)


def _camera_backward_case(shape, light, use_g=True, use_gt=True):
    D, H, W = shape
    cells, hw, planes = D * H * W, H * W, RENDER_N * VIEWS
    bufs = [Buf("vols", F32, cells, RENDER_N, cells + 3)]
    if use_g:
        bufs.append(Buf("grad_image", F32, hw, planes, hw + 1))
    if use_gt:
        bufs.append(Buf("grad_trans", F32, hw, planes, hw + 2))
    bufs.append(Buf("grad_vols", F32, cells, RENDER_N, cells + 5, role="out"))
    desc = _desc(light)
    az = (C.c_double * planes)(*(AZIMUTHS * RENDER_N))
    el = (C.c_double * planes)(*(ELEVATIONS * RENDER_N))

    def inputs():
        G, Gt = _grads(shape)
        d = {"vols": _render_vols(shape)}
        if use_g:
            d["grad_image"] = G
        if use_gt:
            d["grad_trans"] = Gt
        return d

    def args(b):
        return [b.ptr("vols"), b.stride("vols"), RENDER_N, D, H, W, C.byref(desc), az, el, VIEWS,
                b.ptr("grad_image") if use_g else None, b.stride("grad_image") if use_g else hw,
                b.ptr("grad_trans") if use_gt else None, b.stride("grad_trans") if use_gt else hw,
                b.ptr("grad_vols"), b.stride("grad_vols"), *b.workspace(), b.stream]

    def reference():
        from smokephysai_amd.physics import render_camera
        vols = _render_vols(shape).cuda().reshape(RENDER_N, D, H, W).requires_grad_(True)
        G, Gt = (t.cuda().reshape(RENDER_N, VIEWS, H, W) for t in _grads(shape))
        img, T = render_camera(vols, list(AZIMUTHS), list(ELEVATIONS), _settings(light), transmittance=True, differentiable=True)
        outs, grads = zip(*[(o, g) for o, g, use in ((img, G, use_g), (T, Gt, use_gt)) if use])
        torch.autograd.backward(outs, grads)
        return {"grad_vols": vols.grad}
    which = "" if use_g and use_gt else ("-G" if use_g else "-Gt")
    return Case(f"render_camera_backward-{D}x{H}x{W}-{light}{which}", "smk_volume_render_camera_backward", bufs, args, inputs, reference,
                query=lambda lib: lib.smk_volume_render_camera_backward_workspace(RENDER_N, D, H, W, LIGHT_ID[light]))


CASES = [_camera_backward_case(shape, light) for shape in RENDER_SHAPES for light in ("none", "+y", "-y")]
CASES += [_camera_backward_case(RENDER_SHAPES[0], "+y", use_gt=False), _camera_backward_case(RENDER_SHAPES[0], "-y", use_g=False)]
case_param = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
_RUNS = {}


def _fills(case):
    """The two guarded runs of a case, shared by its tests and left unchanged."""
    if case.id not in _RUNS:
        _RUNS[case.id] = (run_guarded(case, FILL_NAN), run_guarded(case, FILL_ZERO))
    return _RUNS[case.id]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


@case_param
def test_keeps_to_its_buffers(case):
    nan, zero = _fills(case)
    assert nan.damage == 0, f"{case.id}, NaN fill: {nan.damage}"
    assert zero.damage == 0, f"{case.id}, zero fill: {zero.damage}"


@case_param
def test_reads_nothing_foreign_and_writes_every_element(case):
    nan, zero = _fills(case)
    assert set(nan.outputs) == {"grad_vols"}
    out = nan.outputs["grad_vols"]
    assert _same_bits(out, zero.outputs["grad_vols"]), f"{case.id}: grad_vols depends on the memory around the buffers"
    assert holds_fill(out, FILL_NAN) == 0, f"{case.id}: {holds_fill(out, FILL_NAN)} elements of grad_vols were never written"
    assert bool(torch.isfinite(out).all()), f"{case.id}: grad_vols is not finite"
    given = case.inputs()
    for run in (nan, zero):
        for name, after in run.inputs.items():
            assert _same_bits(after.reshape(-1).cpu(), given[name].reshape(-1)), f"{case.id}: the input '{name}' was written to"


@case_param
def test_same_values_as_the_ordinary_path(case):
    nan, _ = _fills(case)
    want = case.reference()["grad_vols"].detach()
    out = nan.outputs["grad_vols"]
    assert want.dtype == out.dtype and want.numel() == out.numel()
    differ = bits(out.reshape(-1)) != bits(want.reshape(-1))
    assert not bool(differ.any()), f"{case.id}: grad_vols differs from the dense, aligned call in {int(differ.sum())} of {differ.numel()} elements"


@case_param
def test_runs_on_the_callers_stream_without_waiting(case):
    nan, _ = _fills(case)                         # (also: every kernel of the call is loaded before the timed one)
    side = independent_side_stream()
    assert side is not None, "no side stream runs independently of the null stream here: the stream check could not tell anything"
    run = run_guarded(case, FILL_NAN, stream=side, delay_cycles=DELAY_SECONDS * sleep_cycles_per_second())
    print(f"{case.id}: host time of the call {run.host_seconds * 1e3:.3f} ms behind a delay of {DELAY_SECONDS * 1e3:.0f} ms")
    assert run.host_ahead, (f"{case.id}: the event behind the {DELAY_SECONDS} s delay had completed when the call returned after "
                            f"{run.host_seconds:.4f} s of host time: the call waited for the stream, or the delay is too short to tell")
    assert run.damage == 0, f"{case.id}, side stream: {run.damage}"
    assert _same_bits(run.outputs["grad_vols"], nan.outputs["grad_vols"]), \
        f"{case.id}: grad_vols differs on a side stream: part of the call left the caller's stream"
