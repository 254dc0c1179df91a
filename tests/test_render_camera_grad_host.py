"""CPU tests of the free-camera render's gradient (SPEC_3D.md section 10, "Free camera -- Gradient"): the oracle
(tests/render_camera_grad_oracle.py) against torch's fp64 autograd of the forward rule, the properties the section states, what fp32
alone costs over the GPU test's full case list (the figure tests/test_hip_render_camera_grad.py holds the device to), the declarations
of include/smokehip.h, the workspace query, and the Python surface as far as it needs no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from render_camera_grad_oracle import (AMBIENT, CAMERA_LIGHTS, CASE_GROUPS, COMBOS, GPU_VIEWS, HOST_SHAPES, HOST_VIEWS, SIGMAS,
                                       camera_grad_autograd, camera_grad_fp64, camera_grad_view_cases_fp64, err, reference, scatter_fp64,
                                       upstream)
from render_camera_oracle import camera_grid, camera_samples_count, camera_samples_fp64
from render_grad_oracle import GAIN, render_grad_fp64
from render_oracle import DENSITIES, density

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The fp32 replay's worst `err` against the fp64 rule over the GPU test's full case list, as first measured (at (16,64,130), sparse,
# sigma = (4, 8), "none", Gt alone).  Below 1e-5, so the device's second bound -- ten times this -- is the one that binds (SPEC_3D.md).
REPLAY_WORST = 1.49e-6


def _pair(shape, V, seed=3):
    G, Gt = upstream(shape, 1, V, seed=seed)
    return G[0], Gt[0]


# ---- the oracle is the derivative of the forward rule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_oracle_is_torchs_fp64_autograd_of_the_forward_rule(shape):
    V = len(HOST_VIEWS)
    G, Gt = _pair(shape, V)
    for i, light in enumerate(CAMERA_LIGHTS):
        for j, kind in enumerate(DENSITIES):
            sv, sl = SIGMAS[(i + 2 * j) % len(SIGMAS)]
            rho = density(kind, shape, seed=5)
            got = camera_grad_fp64(rho, HOST_VIEWS, G, Gt, sv, sl, AMBIENT, GAIN, light)
            want = camera_grad_autograd(rho, HOST_VIEWS, G, Gt, sv, sl, AMBIENT, GAIN, light, torch.float64)
            e = err(got, want, V, G, Gt, sv, sl, AMBIENT, GAIN, light)
            assert e <= 1e-12, (shape, light, kind, e)
    for g, gt in ((G, None), (None, Gt)):                          # either gradient alone
        got = camera_grad_fp64(rho, HOST_VIEWS, g, gt, 0.5, 1.0, AMBIENT, GAIN, "-y")
        want = camera_grad_autograd(rho, HOST_VIEWS, g, gt, 0.5, 1.0, AMBIENT, GAIN, "-y", torch.float64)
        assert err(got, want, V, g, gt, 0.5, 1.0, AMBIENT, GAIN, "-y") <= 1e-12


def test_the_case_lists_shared_form_is_the_oracle():
    shape = (6, 5, 8)
    rho = density("dense", shape, seed=2)
    G, Gt = _pair(shape, 1)
    for view in ((37.5, 30.0), (90.0, 90.0), (720.001, 45.0)):
        cases = camera_grad_view_cases_fp64(rho, *view, G[0], Gt[0])
        assert set(cases) == {(sv, sl, light) for sv, sl in SIGMAS for light in CAMERA_LIGHTS}
        for (sv, sl, light), (dg, dt) in cases.items():
            for got, g, gt in ((dg + dt, G, Gt), (dg, G, None), (dt, None, Gt)):
                want = camera_grad_fp64(rho, [view], g, gt, sv, sl, AMBIENT, GAIN, light)
                assert err(got, want, 1, g, gt, sv, sl, AMBIENT, GAIN, light) <= 1e-13


# ---- the properties of the section -------------------------------------------------------------------------------------------------------
def _transpose_of_rays(K, shape, views):
    """sum over the views of B^T applied to a value K[k][y',x'] that every sample of a ray shares."""
    S = camera_samples_count(*shape)
    return sum(scatter_fp64(np.broadcast_to(K[k], (S,) + K[k].shape), camera_grid(shape, *view)) for k, view in enumerate(views))


@pytest.mark.parametrize("shape", [(3, 5, 7), (6, 5, 8), (8, 12, 5)], ids=str)
def test_unlit_and_empty_volume_closed_forms(shape):
    views = ((0.0, 0.0), (37.5, 30.0), (-123.0, -60.0), (200.25, 89.999))
    G, Gt = _pair(shape, len(views))
    G, Gt = np.abs(G) + 0.1, -np.abs(Gt) - 0.1                      # G > 0 > Gt: nothing cancels
    sv, sl = 0.5, 1.0
    rho = density("dense", shape, seed=4)
    trans = np.stack([np.exp(-sv * camera_samples_fp64(rho, *view).sum(axis=0)) for view in views])
    G64, Gt64 = G.astype(np.float64), Gt.astype(np.float64)
    want = sv * _transpose_of_rays(trans * (GAIN * G64 - Gt64), shape, views)
    got = camera_grad_fp64(rho, views, G, Gt, sv, sl, AMBIENT, GAIN, "none")
    assert err(got, want, len(views), G, Gt, sv, sl, AMBIENT, GAIN, "none") <= 1e-13
    empty = sv * _transpose_of_rays(GAIN * G64 - Gt64, shape, views)     # transmittance = 1, under every light: rho = 0 has a gradient
    assert np.abs(empty).max() > 0.1 * sv
    for light in CAMERA_LIGHTS:
        got = camera_grad_fp64(np.zeros(shape), views, G, Gt, sv, sl, AMBIENT, GAIN, light)
        assert err(got, empty, len(views), G, Gt, sv, sl, AMBIENT, GAIN, light) <= 1e-13


@pytest.mark.parametrize("shape", [(3, 5, 7), (6, 5, 8), (5, 33, 36)], ids=str)
def test_level_whole_turns_are_the_front_views_gradient(shape):
    G, Gt = _pair(shape, 1)
    rho = density("sparse", shape, seed=6)
    for light in CAMERA_LIGHTS:
        front = render_grad_fp64(rho, G[0], Gt[0], 0.5, 1.0, AMBIENT, GAIN, light)
        for view in ((0.0, 0.0), (720.0, 0.0)):
            got = camera_grad_fp64(rho, [view], G, Gt, 0.5, 1.0, AMBIENT, GAIN, light)
            assert err(got, front, 1, G, Gt, 0.5, 1.0, AMBIENT, GAIN, light) <= 1e-13


def rearranged(rho):
    """Property 3 of "Free camera": the samples of the top view (0, 90) of rho [D,H,W], D = H (mod 2), as an array [S,H,W], and the
    index arrays (z of image row y', y of sample s, which of them are inside the volume) that carry a gradient of it back."""
    D, H, W = rho.shape
    S = camera_samples_count(D, H, W)
    z = np.arange(H) + (D - H) // 2                                 # c_z + (y' - c_y)
    y = (H - 1 + S - 1) // 2 - np.arange(S)                         # c_y - (s - (S-1)/2)
    zin, yin = (z >= 0) & (z < D), (y >= 0) & (y < H)
    arr = np.zeros((S, H, W), rho.dtype)
    arr[np.ix_(yin, zin)] = np.asarray(rho)[z[zin]][:, y[yin]].transpose(1, 0, 2)
    return arr, (z, zin, y, yin)


def rearranged_back(d_arr, shape, index):
    """The gradient with respect to rearranged(rho)'s array -> with respect to rho (a voxel no image row sees gets 0)."""
    z, zin, y, yin = index
    d = np.zeros(shape, d_arr.dtype)
    d[np.ix_(z[zin], y[yin])] = d_arr[np.ix_(yin, zin)].transpose(1, 0, 2)
    return d


@pytest.mark.parametrize("shape", [(6, 6, 8), (3, 5, 7), (7, 3, 4)], ids=str)
def test_top_view_is_the_front_views_gradient_of_the_rearranged_array(shape):
    rho = density("dense", shape, seed=2).astype(np.float64)
    arr, index = rearranged(rho)
    assert np.abs(camera_samples_fp64(rho, 0.0, 90.0) - arr).max() == 0.0
    G, Gt = _pair(shape, 1)
    for sv, sl in SIGMAS:
        for light, front in (("none", "none"), ("-y", "+z")):       # the light from above travels along the ray
            want = rearranged_back(render_grad_fp64(arr, G[0], Gt[0], sv, sl, AMBIENT, GAIN, front), shape, index)
            got = camera_grad_fp64(rho, [(0.0, 90.0)], G, Gt, sv, sl, AMBIENT, GAIN, light)
            assert err(got, want, 1, G, Gt, sv, sl, AMBIENT, GAIN, light) <= 1e-13, (sv, sl, light)


def test_untapped_voxels_have_no_gradient():
    """A voxel no sample taps has B^T Q = B^T R = 0.  Unlit that is its gradient; lit, the shadow sum runs over the rows behind it, so it
    is 0 where none of those is tapped either -- where the whole line along y is untapped, as the planes a level or a top view looks
    past at D > W, D > H."""
    shape = (64, 40, 48)
    rho = density("dense", shape, seed=7)
    S = camera_samples_count(*shape)
    G, Gt = _pair(shape, 1)
    for view in ((90.0, 0.0), (0.0, 90.0), (37.5, 30.0)):
        wsum = scatter_fp64(np.ones((S,) + shape[1:]), camera_grid(shape, *view))
        untapped = wsum == 0.0
        assert untapped.any() and (~untapped).any() and wsum.max() <= 2.0, (view, wsum.max())
        lines = np.broadcast_to(untapped.all(axis=1, keepdims=True), shape)
        if view[1] in (0.0, 90.0):
            assert np.array_equal(lines, untapped)                   # whole planes
        for light in CAMERA_LIGHTS:
            d = camera_grad_fp64(rho, [view], G, Gt, 0.5, 1.0, AMBIENT, GAIN, light)
            assert np.all(d[untapped if light == "none" else lines] == 0.0) and np.abs(d).max() > 0, (view, light)


# ---- what fp32 alone costs ---------------------------------------------------------------------------------------------------------------
def _replay_worst(groups):
    worst, where = 0.0, None
    for shape, kind, light in groups:
        r = reference(shape, kind, light)
        assert len(r["replay"]) == len(SIGMAS) * len(COMBOS) and r["G"].shape[1] == len(GPU_VIEWS)
        e, key = r["replay_worst"]
        if e > worst:
            worst, where = e, (shape, kind, light) + tuple(key)
    return worst, where


@pytest.mark.parametrize("shape,kind,light", CASE_GROUPS, ids=lambda v: str(v).replace(" ", ""))
def test_fp32_replay_over_the_gpu_tests_case_list(shape, kind, light):
    worst, where = _replay_worst([(shape, kind, light)])
    print(f"camera gradient, fp32 replay {shape} {kind} {light}: worst err {worst:.3e} at {where}")
    assert worst < 2 * REPLAY_WORST and worst < 1e-5


def test_fp32_replay_figure_of_the_full_case_list():
    worst, where = _replay_worst(CASE_GROUPS)                          # (computed by the test above, group by group, and kept)
    print(f"camera gradient, fp32 replay over the GPU test's full case list: worst err {worst:.3e} at {where}")
    assert worst < 2 * REPLAY_WORST and worst < 1e-5


# ---- the header, the binding, the workspace query ----------------------------------------------------------------------------------------
def test_header_declares_the_two_entry_points():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    assert re.search(r"int64_t\s+smk_volume_render_camera_backward_workspace\(int32_t n, int32_t D, int32_t H, int32_t W, int32_t light\);", hdr)
    m = re.search(r"int\s+smk_volume_render_camera_backward\((.*?)\);\n", hdr, flags=re.S)
    assert m
    params = [re.sub(r"/\*.*?\*/", "", p, flags=re.S).strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "vols", "vol_stride", "n", "D", "H", "W", "desc", "azimuths", "elevations", "n_views", "grad_image", "grad_image_stride", "grad_trans",
        "grad_trans_stride", "grad_vols", "grad_vol_stride", "workspace", "workspace_bytes", "stream"]


def camera_backward_bytes(n, D, H, W, lit):
    """The workspace formula as include/smokehip.h states it."""
    S = camera_samples_count(D, H, W)
    row = (2 * S + 1) * W if lit else W
    fit = 2 ** 26 // row
    band = min(32, H, fit - 3)
    slots = min(band + 3, H)
    vols = min(n, 16, fit // slots)
    return ((2 * n * D * H * W if lit else 0) + vols * slots * row) * 4


def test_binding_and_workspace_query():
    from smokephysai_amd import _lib
    assert "smk_volume_render_camera_backward" in _lib.EXPORTS and "smk_volume_render_camera_backward_workspace" in _lib.EXPORTS
    assert len(_lib._SIGNATURES["smk_volume_render_camera_backward"]) == 19
    L = _lib.load()
    q = L.smk_volume_render_camera_backward_workspace
    assert q.argtypes == [C.c_int32] * 5 and q.restype == C.c_int64     # no view count: the same for any number of views by construction
    none, pos, neg, posz = _lib.SMK_LIGHT_NONE, _lib.SMK_LIGHT_POS_Y, _lib.SMK_LIGHT_NEG_Y, _lib.SMK_LIGHT_POS_Z
    assert q(1, 1, 1, 1, none) == 4 and q(2, 4, 6, 8, none) == 2 * 6 * 8 * 4 and q(40, 4, 6, 8, none) == 16 * 6 * 8 * 4
    assert q(8, 64, 512, 512, none) == 8 * 35 * 512 * 4                 # a band of 32 rows and its three neighbours
    for n, D, H, W in ((1, 1, 1, 1), (2, 4, 6, 8), (2, 24, 70, 64), (40, 3, 5, 7), (8, 64, 512, 512), (3, 64, 4096, 1024), (17, 64, 40, 48),
                       (1, 1, 4096, 1024), (5, 64, 1, 1024)):
        assert q(n, D, H, W, none) == camera_backward_bytes(n, D, H, W, False), (n, D, H, W)
        assert q(n, D, H, W, pos) == q(n, D, H, W, neg) == camera_backward_bytes(n, D, H, W, True), (n, D, H, W)
        assert q(n, D, H, W, neg) - 2 * n * D * H * W * 4 <= 1 << 28    # the scratch's cap
    assert q(2, 4, 6, 8, posz) == -1 and q(2, 65, 6, 8, none) == -1 and q(2, 4, 6, 1025, none) == -1 and q(0, 4, 6, 8, none) == -1
    assert q(1, 2, 4097, 4, none) == -1 and q(1, 2, 4096, 4, none) > 0  # the backward's own limit on H
    assert L.smk_volume_render_camera_workspace(1, 2, 4097, 4, none) == 0      # ... which the forward does not have


# ---- the Python surface, as far as it needs no device -----------------------------------------------------------------------------------
def test_python_surface():
    from smokephysai_amd import physics
    from smokephysai_amd.evaluation.perturbation_tests import PerturbationTester
    from smokephysai_amd.physics import (RenderSettings, camera_backward_supported, camera_backward_workspace, camera_supported,
                                         render_camera)
    # the keyword travels through **options (the named parameters stay the forward-only render's): keyword only, default False
    sig = inspect.signature(render_camera).parameters
    assert sig["options"].kind is inspect.Parameter.VAR_KEYWORD and "differentiable=False (the default)" in render_camera.__doc__
    with pytest.raises(TypeError, match="unexpected keyword argument 'differentiabel'"):
        render_camera(torch.zeros(2, 4, 6, 8), 0.0, 0.0, differentiabel=True)
    with pytest.raises(TypeError):                                   # keyword only: no eighth positional argument
        render_camera(torch.zeros(2, 4, 6, 8), 0.0, 0.0, None, True)
    assert "camera_backward_workspace" in physics.__all__ and "camera_backward_supported" in physics.__all__
    assert camera_backward_supported(64, 4096, 1024) and not camera_backward_supported(64, 4097, 8) and camera_supported(64, 4097, 8)
    assert not camera_backward_supported(65, 8, 8) and not camera_backward_supported(8, 8, 1025)
    vols = torch.zeros(2, 4, 6, 8)
    with pytest.raises(RuntimeError, match="no backward"):           # the refusal without the keyword stands
        render_camera(vols.clone().requires_grad_(), 0.0, 0.0)
    with pytest.raises(RuntimeError, match="no backward.*differentiable=True"):
        render_camera(vols.clone().requires_grad_(), [0.0, 30.0], 10.0, differentiable=False)
    for v in (vols, vols.clone().requires_grad_()):                  # what render_camera raises today for a tensor that is not on a GPU
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            render_camera(v, [0.0, 30.0], 10.0, differentiable=True)
    with pytest.raises(ValueError, match="out="):
        render_camera(vols.clone().requires_grad_(), 0.0, 0.0, differentiable=True, out=torch.zeros(2, 6, 8))
    with pytest.raises(TypeError):
        render_camera(vols.clone().requires_grad_(), 0.0, 0.0, {"light": "none"}, differentiable=True)
    with pytest.raises(ValueError, match=r"\+z"):
        render_camera(vols.clone().requires_grad_(), 0.0, 0.0, RenderSettings(light="+z"), differentiable=True)
    with pytest.raises(ValueError, match=r"\[-90, 90\]"):
        render_camera(vols.clone().requires_grad_(), 0.0, 91.0, differentiable=True)
    with pytest.raises(ValueError, match=r"\+z"):
        camera_backward_workspace(1, (4, 6, 8), "+z", "cpu")
    with pytest.raises(ValueError):
        camera_backward_workspace(1, (4, 4097, 8), "none", "cpu")
    ws = camera_backward_workspace(2, (4, 6, 8), "none", "cpu")
    assert ws.dtype == torch.float32 and ws.numel() == 2 * 6 * 8
    e = inspect.signature(PerturbationTester.adversarial_test).parameters["elevation"]
    assert e.kind is inspect.Parameter.KEYWORD_ONLY and e.default is None
    with pytest.raises(ValueError, match="render="):
        PerturbationTester().adversarial_test(torch.nn.Identity(), torch.zeros(1, 1, 4, 6, 8), elevation=[0.0, 30.0])
    with pytest.raises(ValueError, match="render="):
        PerturbationTester().adversarial_test(torch.nn.Identity(), torch.zeros(1, 1, 4, 6, 8), azimuth=10.0, elevation=30.0)
