"""GPU tests of the free-camera render's gradient (SPEC_3D.md section 10, "Free camera -- Gradient"): smk_volume_render_camera_backward
(csrc/render_camera_grad.hip) through the C ABI, through render_camera(..., differentiable=True) under autograd and through
PerturbationTester.adversarial_test(render=..., azimuth=..., elevation=...), against tests/render_camera_grad_oracle.py.

Shapes (render_camera_oracle.GPU_SHAPES, the smallest at which each part can go wrong): (1,1,1) one voxel; (3,5,7) everything odd;
(6,5,8) even D, the parity of S; (5,33,36) tile tails, two bands of image rows; (24,70,64) several chunks, three bands; (64,40,48) D > W,
unreached voxels, the depth limit, two bands; (16,64,130) five strips, the forward's worst spot.  Each with 2 volumes, both densities, the
eight GPU_VIEWS as ONE call of V = 8, the four sigma pairs, the three lights, and G with Gt, G alone, Gt alone.  The output and the
workspace are pre-filled with NaN.

Bounds, in err = max|d - ref| / max(max|ref|, V s) against the float64 rule:
  1e-4, the project's bar, for every case; and
  the device's worst over all cases is at most 10 times the worst of the fp32 replay (torch's fp32 autograd of the rule) over the same
  cases: 1.49e-6 (tests/test_render_camera_grad_host.py), so 1.49e-5 binds.  test_device_error_is_within_ten_times_the_replays prints both.
The float64 references and the replay of a group of cases (a shape, a density kind, a light) are computed once
(render_camera_grad_oracle.reference; threads share its 16 volume-view pairs) and left unchanged.  Everything stated as "equal" is bit for
bit (torch.equal)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import rel_err                                                                                                # noqa: E402
from render_camera_grad_oracle import (AMBIENT, BOUND, CAMERA_LIGHTS, CASE_GROUPS, COMBOS, GPU_VIEWS, SIGMAS, combo_grads, err,   # noqa: E402
                                       reference, render_camera_torch, scatter_fp64, upstream)
from render_camera_oracle import camera_grid, camera_samples_count, camera_samples_fp64                                     # noqa: E402
from render_grad_oracle import GAIN                                                                                         # noqa: E402
from render_oracle import DENSITIES, density                                                                                # noqa: E402
from smokephysai_amd import _lib                                                                                            # noqa: E402
from smokephysai_amd.physics import RenderSettings, camera_backward_workspace, render_camera, render_volumes                # noqa: E402

DEV = "cuda"
NAN = float("nan")
_DEVICE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _backward(vols, views, settings, G, Gt, fill=NAN, ws_fill=NAN):
    """smk_volume_render_camera_backward on n dense volumes [n,D,H,W]; views: V (azimuth, elevation) pairs (every volume's) or n lists of
    V pairs; G / Gt: [n,V,H,W] device tensors or None.  The output is pre-filled with `fill`, the workspace with `ws_fill`."""
    n, D, H, W = vols.shape
    table = np.asarray(views, np.float64)
    table = np.broadcast_to(table, (n,) + table.shape).copy() if table.ndim == 2 else table       # [n, V, 2]
    V = table.shape[1]
    L = _lib.load()
    grad = torch.full((n, D, H, W), fill, device=DEV)
    ws = camera_backward_workspace(n, (D, H, W), settings.light, DEV)
    ws.fill_(ws_fill)                                              # nothing may be read from the workspace before it is written
    desc = settings.desc()
    az = (C.c_double * (n * V))(*table[..., 0].reshape(-1).tolist())
    el = (C.c_double * (n * V))(*table[..., 1].reshape(-1).tolist())
    _lib.check(L.smk_volume_render_camera_backward(vols.data_ptr(), D * H * W, n, D, H, W, C.byref(desc), az, el, V,
                                                   None if G is None else G.data_ptr(), H * W, None if Gt is None else Gt.data_ptr(), H * W,
                                                   grad.data_ptr(), D * H * W, ws.data_ptr(), ws.numel() * 4, _lib.stream_ptr(vols.device)))
    return grad


def _device_errors(shape, kind, light):
    """The device's err against the float64 rule for every case of one group (run once per group): (worst, its case, NaNs left)."""
    group = (shape, kind, light)
    if group not in _DEVICE:
        r = reference(shape, kind, light)
        V = len(GPU_VIEWS)
        dG, dGt, vol = _dev(r["G"]), _dev(r["Gt"]), _dev(r["vols"])
        worst, where, nans = 0.0, None, []
        for sv, sl in SIGMAS:
            s = RenderSettings(sv, sl, AMBIENT, GAIN, light)
            for combo in COMBOS:
                g, gt = combo_grads(combo, dG, dGt)
                got = _backward(vol, GPU_VIEWS, s, g, gt)
                key = (sv, sl, combo)
                if bool(torch.isnan(got).any()):
                    nans.append(key)
                got = got.cpu().numpy()
                for i in range(2):
                    hg, hgt = combo_grads(combo, r["G"][i], r["Gt"][i])
                    e = err(got[i], r["ref"][key][i], V, hg, hgt, sv, sl, AMBIENT, GAIN, light)
                    if not e <= worst:                     # (a NaN counts)
                        worst, where = e, key + (i,)
        _DEVICE[group] = (worst, where, nans)
    return _DEVICE[group]


# ---- a. against the fp64 rule through the ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind,light", CASE_GROUPS, ids=lambda v: str(v).replace(" ", ""))
def test_backward_matches_the_fp64_rule(shape, kind, light):
    e, where, nans = _device_errors(shape, kind, light)
    rp, rp_at = reference(shape, kind, light)["replay_worst"]
    print(f"camera gradient {shape} {kind} {light}: device worst err {e:.3e} at {where}; fp32 replay {rp:.3e} at {rp_at}")
    assert nans == [], f"NaN left in grad_vols: {nans[:4]}"       # every element written, nothing read before it is written
    assert e <= BOUND, (shape, kind, light, e, where)


def test_device_error_is_within_ten_times_the_replays():
    dev = max(_device_errors(*g)[0] for g in CASE_GROUPS)         # (every group was run by the test above, and kept)
    rep = max(reference(*g)["replay_worst"][0] for g in CASE_GROUPS)
    print(f"camera gradient, all cases: device worst err {dev:.3e}; fp32 replay worst err {rep:.3e}")
    assert dev <= 10 * rep and dev <= BOUND


# ---- b. bit-level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 33, 36), (64, 40, 48)], ids=str)
@pytest.mark.parametrize("light", CAMERA_LIGHTS)
def test_bit_level_properties(shape, light):
    s = RenderSettings(0.5, 1.0, AMBIENT, GAIN, light)
    V = len(GPU_VIEWS)
    views = [list(v) for v in GPU_VIEWS]
    G, Gt = upstream(shape, 2, V)
    dG, dGt = _dev(G), _dev(Gt)
    vol = _dev(np.stack([density("dense", shape, seed=i) for i in range(2)]))
    both = _backward(vol, views, s, dG, dGt)
    assert torch.equal(_backward(vol, views, s, dG, dGt, fill=-3.0, ws_fill=0.0), both)               # call to call, whatever the memory held
    alone = _backward(vol[1:2].contiguous(), views, s, dG[1:2].contiguous(), dGt[1:2].contiguous())
    assert torch.equal(alone[0], both[1])                                                            # independent of the batch mates
    assert torch.equal(_backward(vol, [views] * 2, s, dG, dGt), both)                                # [V] is the [n,V] table of equal rows
    mixed = _backward(vol, [views, views[::-1]], s, dG, dGt)                                         # one list per volume
    assert torch.equal(mixed[0], both[0])
    assert torch.equal(mixed[1], _backward(vol[1:2].contiguous(), views[::-1], s, dG[1:2].contiguous(), dGt[1:2].contiguous())[0])
    # V views in one call against the sum of V single-view calls: the same terms in another order of summation
    singles = sum(_backward(vol, [view], s, dG[:, k:k + 1].contiguous(), dGt[:, k:k + 1].contiguous()).double()
                  for k, view in enumerate(views)).cpu().numpy()
    for i in range(2):
        assert err(both[i].cpu().numpy(), singles[i], V, G[i], Gt[i], 0.5, 1.0, AMBIENT, GAIN, light) <= BOUND


# ---- c. closed forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 33, 36), (64, 40, 48)], ids=str)
def test_empty_volume_and_unlit_closed_forms(shape):
    views = ((0.0, 0.0), (37.5, 30.0), (-123.0, -60.0), (720.001, 45.0))
    V, S = len(views), camera_samples_count(*shape)
    G, Gt = upstream(shape, 2, V)
    G, Gt = np.abs(G) + 0.1, -np.abs(Gt) - 0.1                     # G > 0 > Gt: g G - Gt cannot cancel
    dG, dGt = _dev(G), _dev(Gt)
    K = GAIN * G.astype(np.float64) - Gt
    grids = [camera_grid(shape, *view) for view in views]

    def transpose(rays):                                           # [V,H,W'] -> sum over the views of B^T (the value on every sample)
        return sum(scatter_fp64(np.broadcast_to(rays[k], (S,) + rays[k].shape), grids[k]) for k in range(V))
    dense = np.stack([density("dense", shape, seed=i) for i in range(2)])
    zero = torch.zeros((2,) + shape, device=DEV)
    empty = [transpose(K[i]) for i in range(2)]
    for sv, sl in SIGMAS:
        for light in CAMERA_LIGHTS:                                # the empty volume: transmittance 1 under every light
            s = RenderSettings(sv, sl, AMBIENT, GAIN, light)
            got = _backward(zero, views, s, dG, dGt).cpu().numpy()
            for i in range(2):
                assert err(got[i], sv * empty[i], V, G[i], Gt[i], sv, sl, AMBIENT, GAIN, light) <= BOUND, (sv, sl, light)
        s = RenderSettings(sv, sl, AMBIENT, GAIN, "none")          # unlit: sigma_v B^T (transmittance (g G - Gt))
        got = _backward(_dev(dense), views, s, dG, dGt).cpu().numpy()
        for i in range(2):
            T = np.stack([np.exp(-sv * camera_samples_fp64(dense[i], *view, grid=grids[k]).sum(axis=0)) for k, view in enumerate(views)])
            assert err(got[i], sv * transpose(T * K[i]), V, G[i], Gt[i], sv, sl, AMBIENT, GAIN, "none") <= BOUND, sv


@pytest.mark.parametrize("shape", [(3, 5, 7), (6, 5, 8), (24, 70, 64)], ids=str)
def test_level_whole_turns_are_the_front_views_gradient(shape):
    G, Gt = upstream(shape, 2, 1)
    dG, dGt = _dev(G), _dev(Gt)
    for kind in DENSITIES:
        vol = _dev(np.stack([density(kind, shape, seed=i) for i in range(2)]))
        for sv, sl in SIGMAS:
            for light in CAMERA_LIGHTS:
                s = RenderSettings(sv, sl, AMBIENT, GAIN, light)
                v = vol.clone().requires_grad_(True)
                img, T = render_volumes(v, s, transmittance=True)
                (front,) = torch.autograd.grad((img * dG[:, 0]).sum() + (T * dGt[:, 0]).sum(), v)
                front = front.cpu().numpy()
                for view in ((0.0, 0.0), (720.0, 0.0)):
                    got = _backward(vol, [view], s, dG, dGt).cpu().numpy()
                    for i in range(2):
                        assert err(got[i], front[i], 1, G[i], Gt[i], sv, sl, AMBIENT, GAIN, light) <= BOUND, (kind, sv, sl, light, view)


def test_top_view_is_the_front_views_gradient_of_the_rearranged_volume():
    """(6,6,8), D = H: at (0, 90) every sample is a voxel, image row y' sees plane z = y' and the ray runs from y = 5 down to 0: the front
    view of rho[z, y, x] -> rho'[5 - y, z, x], and the light from above, which travels along the ray, is that view's "+z" light."""
    shape = (6, 6, 8)
    G, Gt = upstream(shape, 2, 1)
    dG, dGt = _dev(G), _dev(Gt)
    vol = _dev(np.stack([density("dense", shape, seed=i) for i in range(2)]))
    for sv, sl in SIGMAS:
        for light, front in (("none", "none"), ("-y", "+z")):
            turned = vol.permute(0, 2, 1, 3).flip(1).contiguous().requires_grad_(True)           # [2, 6 (depth: y descending), 6 (rows: z), 8]
            img, T = render_volumes(turned, RenderSettings(sv, sl, AMBIENT, GAIN, front), transmittance=True)
            (d,) = torch.autograd.grad((img * dG[:, 0]).sum() + (T * dGt[:, 0]).sum(), turned)
            want = d.flip(1).permute(0, 2, 1, 3).cpu().numpy()
            got = _backward(vol, [(0.0, 90.0)], RenderSettings(sv, sl, AMBIENT, GAIN, light), dG, dGt).cpu().numpy()
            for i in range(2):
                assert err(got[i], want[i], 1, G[i], Gt[i], sv, sl, AMBIENT, GAIN, light) <= BOUND, (sv, sl, light)


# ---- d. autograd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", CAMERA_LIGHTS)
def test_autograd_hands_out_the_abi_result(light):
    shape = (5, 33, 36)
    az, el = [0.0, 37.5, -123.0], [0.0, 30.0, -60.0]
    views = list(zip(az, el))
    V = len(views)
    s = RenderSettings(0.5, 1.0, AMBIENT, GAIN, light)
    G, Gt = upstream(shape, 2, V)
    dG, dGt = _dev(G), _dev(Gt)
    vol = _dev(np.stack([density("dense", shape, seed=i) for i in range(2)]))
    want = _backward(vol, views, s, dG, dGt)
    with torch.no_grad():
        image0, trans0 = render_camera(vol, az, el, s, transmittance=True)
    v = vol.clone().requires_grad_(True)
    image, trans = render_camera(v, az, el, s, transmittance=True, differentiable=True)
    assert image.requires_grad and trans.requires_grad and image.shape == (2, V) + shape[1:]
    assert torch.equal(image, image0) and torch.equal(trans, trans0)                         # the forward values are the plain call's
    (g,) = torch.autograd.grad((image * dG).sum() + (trans * dGt).sum(), v)
    assert g.shape == v.shape and torch.equal(g, want)
    # the image alone, and an unused output: the other gradient is absent, not a tensor of zeros
    v1 = vol.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad((render_camera(v1, az, el, s, differentiable=True) * dG).sum(), v1)
    assert torch.equal(g1, _backward(vol, views, s, dG, None))
    v2 = vol.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad((render_camera(v2, az, el, s, transmittance=True, differentiable=True)[1] * dGt).sum(), v2)
    assert torch.equal(g2, _backward(vol, views, s, None, dGt))
    # [n,V] tables, and a pair of numbers (no view dimension)
    v3 = vol.clone().requires_grad_(True)
    (g3,) = torch.autograd.grad((render_camera(v3, torch.tensor([az, az[::-1]]), torch.tensor([el, el[::-1]]), s, differentiable=True)
                                 * dG).sum(), v3)
    assert torch.equal(g3, _backward(vol, [views, views[::-1]], s, dG, None))
    v4 = vol.clone().requires_grad_(True)
    one = render_camera(v4, 37.5, 30.0, s, differentiable=True)
    assert one.shape == (2,) + shape[1:]
    (g4,) = torch.autograd.grad((one * dG[:, 1]).sum(), v4)
    assert torch.equal(g4, _backward(vol, [(37.5, 30.0)], s, dG[:, 1:2].contiguous(), None))
    # the [D,H,W] form
    v5 = vol[1].clone().requires_grad_(True)
    i5 = render_camera(v5, az, el, s, differentiable=True)
    assert i5.shape == (V,) + shape[1:]
    (g5,) = torch.autograd.grad((i5 * dG[1]).sum(), v5)
    assert g5.shape == shape and torch.equal(g5, _backward(vol[1:2].contiguous(), views, s, dG[1:2].contiguous(), None)[0])
    # a batch-strided input: every other volume of a larger batch, served run by run
    big = _dev(np.stack([density("dense", shape, seed=i) for i in range(4)])).requires_grad_(True)
    view = big[::2]
    assert not view.is_contiguous()
    iv, tv = render_camera(view, az, el, s, transmittance=True, differentiable=True)
    (gb,) = torch.autograd.grad((iv * dG).sum() + (tv * dGt).sum(), big)
    assert torch.equal(gb[::2], _backward(big.detach()[::2].contiguous(), views, s, dG, dGt)) and not bool(gb[1::2].any())
    # with nothing that requires a gradient, and under no_grad, it is the plain path, out= and all
    out = torch.empty(2, V, *shape[1:], device=DEV)
    assert render_camera(vol, az, el, s, out=out, differentiable=True) is out and torch.equal(out, image0)
    with torch.no_grad():
        assert render_camera(v, az, el, s, out=out, differentiable=True) is out
    with pytest.raises(ValueError, match="out="):
        render_camera(v, az, el, s, out=out, differentiable=True)
    with pytest.raises(RuntimeError, match="no backward"):        # without the keyword the refusal stands
        render_camera(v, az, el, s)
    # a second derivative is refused, in words
    image = render_camera(v, az, el, s, differentiable=True)
    weight = dG.clone().requires_grad_(True)
    (first,) = torch.autograd.grad((image * weight).sum(), v, create_graph=True)
    assert first.requires_grad
    with pytest.raises(RuntimeError, match="differentiate twice"):
        first.sum().backward()


# ---- e. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = _lib.load()
    desc = RenderSettings(light="+y").desc()
    n, D, H, W, V = 2, 4, 40, 8, 2
    cells, hw = D * H * W, H * W
    vol = torch.ones(n, D, H, W, device=DEV)
    G = torch.ones(n, V, H, W, device=DEV)
    grad = torch.full((n, D, H, W), -7.0, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    need = L.smk_volume_render_camera_backward_workspace(n, D, H, W, _lib.SMK_LIGHT_POS_Y)
    # the header's formula: row = (2 S + 1) W, a band of 32 rows and its three neighbours, both volumes in one unit
    assert need == (2 * n * cells + n * 35 * (2 * camera_samples_count(D, H, W) + 1) * W) * 4
    assert L.smk_volume_render_camera_backward_workspace(n, D, H, W, _lib.SMK_LIGHT_NONE) == n * 35 * W * 4
    assert L.smk_volume_render_camera_backward_workspace(1, D, 4097, W, _lib.SMK_LIGHT_NONE) == -1
    ws = torch.empty(need // 4, device=DEV)
    az = (C.c_double * (n * V))(0.0, 30.0, 0.0, 30.0)
    el = (C.c_double * (n * V))(0.0, 20.0, 0.0, -20.0)

    def call(D=4, H=40, W=8, vstride=cells, g=G.data_ptr(), gt=None, wbytes=need, d=desc, gstride=hw, a=az, e=el, views=V):
        small = D != 4 or W != 8 or H != 40
        return L.smk_volume_render_camera_backward(vol.data_ptr(), vstride, 1 if small else n, D, H if H != 40 or not small else 1, W,
                                                   C.byref(d), a, e, views, g, gstride, gt, hw, grad.data_ptr(), cells, ws.data_ptr(),
                                                   wbytes, st)
    assert call(d=RenderSettings(light="+z").desc()) == _lib.SMK_ERR_UNSUPPORTED and b"SMK_LIGHT_POS_Z" in L.smk_last_error()
    assert call(D=65) == _lib.SMK_ERR_UNSUPPORTED and b"D <= 64" in L.smk_last_error()
    assert call(W=1025) == _lib.SMK_ERR_UNSUPPORTED
    assert call(H=4097) == _lib.SMK_ERR_UNSUPPORTED and b"H <= 4096" in L.smk_last_error()
    assert call(wbytes=need - 4) == _lib.SMK_ERR_INVALID and b"workspace" in L.smk_last_error()
    assert call(g=None, gt=None) == _lib.SMK_ERR_INVALID and b"both null" in L.smk_last_error()
    assert call(d=_lib.SmkRenderDesc(0.1, 0.1, 0.25, 1.0, 7)) == _lib.SMK_ERR_INVALID
    assert call(vstride=cells - 1) == _lib.SMK_ERR_INVALID
    assert call(gstride=hw - 1) == _lib.SMK_ERR_INVALID
    assert call(views=0) == _lib.SMK_ERR_INVALID
    assert call(a=(C.c_double * (n * V))(0.0, NAN, 0.0, 30.0)) == _lib.SMK_ERR_INVALID and b"finite" in L.smk_last_error()
    assert call(e=(C.c_double * (n * V))(0.0, 90.5, 0.0, 30.0)) == _lib.SMK_ERR_INVALID and b"[-90, 90]" in L.smk_last_error()
    assert call(e=(C.c_double * (n * V))(0.0, 20.0, -91.0, 30.0)) == _lib.SMK_ERR_INVALID
    assert call(e=(C.c_double * (n * V))(0.0, float("inf"), 0.0, 30.0)) == _lib.SMK_ERR_INVALID
    assert call(e=(C.c_double * (n * V))(NAN, 20.0, 0.0, 30.0)) == _lib.SMK_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all())                              # grad_vols still holds its fill
    assert call() == _lib.SMK_OK
    torch.cuda.synchronize()
    assert not bool((grad == -7.0).any()) and bool(torch.isfinite(grad).all())
    with pytest.raises(ValueError):
        camera_backward_workspace(1, (65, 8, 8), "+y", DEV)
    with pytest.raises(ValueError):
        camera_backward_workspace(1, (4, 4097, 8), "+y", DEV)
    with pytest.raises(ValueError, match=r"\+z"):
        camera_backward_workspace(1, (8, 8, 8), "+z", DEV)
    tall = torch.zeros(1, 1, 4097, 2, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="no backward"):           # the forward takes the shape, the backward does not: said at the call
        render_camera(tall, 0.0, 10.0, differentiable=True)


# ---- f. PGD on the smoke, seen from where the camera stands ---------------------------------------------------------------------------------
PGD_AZIMUTHS, PGD_ELEVATIONS = [0.0, 37.5, -123.0], [0.0, 30.0, -60.0]


def _smoke_volumes():
    g = torch.Generator().manual_seed(21)
    return (torch.rand(2, 1, 8, 128, 128, generator=g) ** 4).to(DEV)          # mostly thin, as smoke; in [0, 1]


def test_volume_gradient_through_camera_render_and_model():
    """The first PGD step's gradient, d(-mse(reconstructed, target)) / d(volume) over the B x V frames, with render_camera in front of the
    model against the same model behind the free-camera render written as torch ops (render_camera_grad_oracle.render_camera_torch, fp32
    on the device): the model half is the same code on both sides, and it is linearised at the same frames on both sides -- the rule's
    frames carry the graph, the kernel's frames the values.  The frames of the two forwards differ by 3.1e-7 (relative, max-norm), and
    this model's gradient is not continuous: measured on MI355X, that difference alone moves the model's own gradient with respect to
    the frames of view (-123, -60) by 2.0e-3, and with it the figure of this test to 7.0e-4, while the two render backwards given one
    upstream gradient are 3.1e-7 apart (the orbit's test, whose frames differ by 1.9e-7, happens to cross no such kink: 3.4e-6).  With
    the model linearised at one point the test holds what it is about, the render's backward in front of the model."""
    from test_hip_input_grad import _small_model
    model = _small_model()
    assert model.input_grad == "hip"
    s = RenderSettings()
    vols = _smoke_volumes()
    V = len(PGD_AZIMUTHS)
    noise = torch.randn(1, 3, 2 * V, 1, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        shown = render_camera(vols[:, 0], PGD_AZIMUTHS, PGD_ELEVATIONS, s)
        target = F.adaptive_avg_pool2d(shown.reshape(-1, 1, 128, 128), (128, 128))

    def gradient(view):
        v = vols.clone().requires_grad_(True)
        out = model(view(v[:, 0]).reshape(-1, 1, 128, 128), chaos_noise=noise)["reconstructed"]
        (g,) = torch.autograd.grad(-F.mse_loss(out, target), v)
        return g

    def rule(v):
        frames = torch.stack([render_camera_torch(v, phi, theta, s.sigma_view, s.sigma_light, s.ambient, s.gain, s.light)[0]
                              for phi, theta in zip(PGD_AZIMUTHS, PGD_ELEVATIONS)], dim=1)
        assert rel_err(frames.detach().cpu().numpy(), shown.cpu().numpy()) <= 1e-5       # the two forwards agree ...
        return frames + (shown - frames).detach()                                        # ... and the model sees one set of values
    got = gradient(lambda v: render_camera(v, PGD_AZIMUTHS, PGD_ELEVATIONS, s, differentiable=True))
    want = gradient(rule)
    assert float(want.abs().max()) > 0
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"volume gradient through camera render + model, {V} views: rel err {e:.2e}")
    assert e <= 1e-4, e


def test_adversarial_test_perturbs_the_volume_from_pitched_views():
    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    from test_hip_input_grad import _Ops
    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()
    assert model.input_grad == "hip"
    vols = _smoke_volumes()
    eps = 0.1
    torch.manual_seed(5)
    with _Ops() as ops:
        res = PerturbationTester().adversarial_test(model, vols, eps, num_steps=2, render=RenderSettings(), azimuth=PGD_AZIMUTHS,
                                                    elevation=PGD_ELEVATIONS)
    assert set(res) == {"adversarial_feature_stability", "adversarial_perturbation_norm"}
    assert np.isfinite(res["adversarial_feature_stability"]) and np.isfinite(res["adversarial_perturbation_norm"])
    assert 0 < res["adversarial_perturbation_norm"] <= eps * np.sqrt(vols.numel()) * (1 + 1e-6)
    scans = sorted({n for n in ops.names if "cumsum" in n or "flip" in n or "grid_sampler" in n})
    assert scans == [], scans                                                  # the render and its backward are the kernels
    assert ops.conv_bn() == [], ops.conv_bn()                                  # ... and so is the model's half of the step
    assert all(p.grad is None and p.requires_grad for p in model.parameters())
    torch.manual_seed(5)                                                       # a single pair of numbers: B frames
    one = PerturbationTester().adversarial_test(model, vols, eps, num_steps=2, render=RenderSettings(), azimuth=37.5, elevation=30.0)
    assert 0 < one["adversarial_perturbation_norm"] <= eps * np.sqrt(vols.numel()) * (1 + 1e-6)
    torch.manual_seed(5)                                                       # the elevation alone: azimuth 0
    top = PerturbationTester().adversarial_test(model, vols, eps, num_steps=1, render=RenderSettings(), elevation=60.0)
    assert 0 < top["adversarial_perturbation_norm"] <= eps * np.sqrt(vols.numel()) * (1 + 1e-6)
    with pytest.raises(ValueError, match="render="):
        PerturbationTester().adversarial_test(model, vols, eps, num_steps=1, elevation=PGD_ELEVATIONS)
