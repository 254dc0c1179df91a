"""GPU tests of the gradient of the volume render (SPEC_3D.md section 10, "Gradient"): smk_volume_render_backward (csrc/render.hip) through
the C ABI, through render_volumes under autograd, and PerturbationTester.adversarial_test(render=...), against tests/render_grad_oracle.py.

Bounds:
  gradient: 1e-5 in the section's metric (render_grad_oracle.err: max|d - ref| over max(max|ref|, the size of one term)) against the
      float64 rule, for every shape, density kind, light and sigma pair of the shared case list, with both upstream gradients, the
      image's alone and the transmittance's alone.  torch's fp32 autograd of the rule stays within 4.2e-7 on these very shapes
      (tests/test_render_grad_host.py holds it below 1e-6); 1e-5 is ten times that bound, room for the device's exp and another summation
      order.  Measured on MI355X: 2.1e-7 at worst (at (64, 64, 64); 1.0e-7 at (1, 8, 8)), DESIGN.md 8.5.
  empty volume: rtol 1e-6 of sigma_view (g G - Gt) (four fp32 roundings; G > 0 > Gt there, so that the difference cannot cancel and a
      relative bound means something).
  through the model: 1e-4 max-norm relative, the project's bar.
  everything stated as "equal" is bit for bit (torch.equal)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import rel_err                                                                                       # noqa: E402
from render_grad_oracle import (AMBIENT, BOUND, DENSITIES, GAIN, LIGHTS, SHAPES, SIGMAS, density, err, render_grad_fp64,      # noqa: E402
                                render_torch, upstream)
from smokephysai_amd import _lib                                                                                   # noqa: E402
from smokephysai_amd.physics import RenderSettings, render_backward_workspace, render_volumes                      # noqa: E402

DEV = "cuda"
N = 3
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _backward(vols, settings, G, Gt, fill=NAN):
    """smk_volume_render_backward on contiguous [n, D, H, W] volumes; the output is pre-filled with `fill`."""
    n, D, H, W = vols.shape
    L = _lib.load()
    grad = torch.full((n, D, H, W), fill, device=DEV)
    ws = render_backward_workspace(n, (D, H, W), settings.light, DEV)
    if ws is not None:
        ws.fill_(NAN)                                          # nothing may be read from the workspace before it is written
    desc = settings.desc()
    _lib.check(L.smk_volume_render_backward(vols.data_ptr(), D * H * W, n, D, H, W, C.byref(desc),
                                            None if G is None else G.data_ptr(), H * W, None if Gt is None else Gt.data_ptr(), H * W,
                                            grad.data_ptr(), D * H * W, None if ws is None else ws.data_ptr(),
                                            0 if ws is None else ws.numel() * 4, _lib.stream_ptr(vols.device)))
    return grad


def _batch(kind, shape):
    return np.stack([density(kind, shape, seed=i) for i in range(N)])


# ---- 1, 2. against the fp64 oracle through the ABI; every element written; bit-level properties ------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_matches_the_fp64_rule(shape):
    G, Gt = upstream((N,) + shape)
    dG, dGt = _dev(G), _dev(Gt)
    worst = 0.0
    for kind in DENSITIES:
        rho = _batch(kind, shape)
        vol = _dev(rho)
        for sv, sl in SIGMAS:
            for light in LIGHTS:
                s = RenderSettings(sv, sl, AMBIENT, GAIN, light)
                ref_g = render_grad_fp64(rho, G, None, sv, sl, AMBIENT, GAIN, light)           # the rule is linear in (G, Gt)
                ref_t = render_grad_fp64(rho, None, Gt, sv, sl, AMBIENT, GAIN, light)
                both = _backward(vol, s, dG, dGt)
                for name, got, ref, g, gt in (("both", both, ref_g + ref_t, G, Gt), ("image", _backward(vol, s, dG, None), ref_g, G, None),
                                              ("transmittance", _backward(vol, s, None, dGt), ref_t, None, Gt)):
                    assert not torch.isnan(got).any(), (shape, kind, sv, sl, light, name)      # every element written
                    e = err(got.cpu().numpy(), ref, g, gt, sv, sl, AMBIENT, GAIN, light)
                    worst = max(worst, e)
                    assert e <= BOUND, (shape, kind, sv, sl, light, name, e)
                if (sv, sl) == (0.5, 1.0):
                    assert torch.equal(_backward(vol, s, dG, dGt, fill=-3.0), both)            # call to call
                    alone = _backward(vol[1:2].contiguous(), s, dG[1:2].contiguous(), dGt[1:2].contiguous())
                    assert torch.equal(alone[0], both[1])                                      # independent of the batch mates
    print(f"render gradient {shape}: worst err {worst:.2e} (bound {BOUND:.0e})")


# ---- 3. closed forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 33, 36), (64, 32, 130)], ids=str)
def test_empty_volume_and_unlit_closed_forms(shape):
    G, Gt = upstream((N,) + shape)
    G, Gt = np.abs(G) + 0.1, -np.abs(Gt) - 0.1                  # opposite signs: g G - Gt cannot cancel
    dG, dGt = _dev(G), _dev(Gt)
    zero = torch.zeros((N,) + shape, device=DEV)
    dense = _batch("dense", shape)
    for sv, sl in SIGMAS:
        for light in LIGHTS:
            s = RenderSettings(sv, sl, AMBIENT, GAIN, light)
            want = sv * (GAIN * G.astype(np.float64) - Gt)
            got = _backward(zero, s, dG, dGt).cpu().numpy()
            np.testing.assert_allclose(got, np.broadcast_to(want[:, None], got.shape), rtol=1e-6, atol=0, err_msg=f"{sv} {sl} {light}")
            np.testing.assert_allclose(_backward(zero, s, dG, None).cpu().numpy(), np.broadcast_to((sv * GAIN * G.astype(np.float64))[:, None], got.shape),
                                       rtol=1e-6, atol=0)
        s = RenderSettings(sv, sl, AMBIENT, GAIN, "none")
        T = np.exp(-sv * dense.astype(np.float64).sum(1))
        want = np.broadcast_to((sv * T * (GAIN * G.astype(np.float64) - Gt))[:, None], dense.shape)
        e = err(_backward(_dev(dense), s, dG, dGt).cpu().numpy(), want, G, Gt, sv, sl, AMBIENT, GAIN, "none")
        assert e <= BOUND, (sv, e)


# ---- 4. autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", LIGHTS)
def test_autograd_hands_out_the_abi_result(light):
    shape = (5, 33, 36)
    s = RenderSettings(0.5, 1.0, AMBIENT, GAIN, light)
    G, Gt = upstream((N,) + shape)
    dG, dGt = _dev(G), _dev(Gt)
    vol = _dev(_batch("dense", shape))
    want = _backward(vol, s, dG, dGt)
    with torch.no_grad():
        image0, trans0 = render_volumes(vol, s, transmittance=True)
    v = vol.clone().requires_grad_(True)
    image, trans = render_volumes(v, s, transmittance=True)
    assert image.requires_grad and trans.requires_grad
    assert torch.equal(image, image0) and torch.equal(trans, trans0)                         # the forward values are the plain call's
    (g,) = torch.autograd.grad((image * dG).sum() + (trans * dGt).sum(), v)
    assert g.shape == v.shape and torch.equal(g, want)
    # the image alone: the transmittance's gradient is absent, not a tensor of zeros
    v1 = vol.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad((render_volumes(v1, s) * dG).sum(), v1)
    assert torch.equal(g1, _backward(vol, s, dG, None))
    v2 = vol.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad((render_volumes(v2, s, transmittance=True)[1] * dGt).sum(), v2)
    assert torch.equal(g2, _backward(vol, s, None, dGt))
    # a strided [B, T, D, H, W] view: the gradient of every other step, served run by run
    B, T = 2, 3
    big = _dev(density("dense", (B, T) + shape, seed=5)).requires_grad_(True)
    view = big[:, ::2]
    assert not view.is_contiguous()
    Gv, Gtv = upstream((B, 2) + shape, seed=2)
    dGv, dGtv = _dev(Gv), _dev(Gtv)
    iv, tv = render_volumes(view, s, transmittance=True)
    assert iv.shape == (B, 2) + shape[1:]
    (gb,) = torch.autograd.grad((iv * dGv).sum() + (tv * dGtv).sum(), big)
    flat = big.detach()[:, ::2].contiguous().view((B * 2,) + shape)
    wantv = _backward(flat, s, dGv.view(B * 2, *shape[1:]), dGtv.view(B * 2, *shape[1:])).view((B, 2) + shape)
    assert torch.equal(gb[:, ::2], wantv) and not bool(gb[:, 1].any())
    with torch.no_grad():
        assert torch.equal(iv, render_volumes(big[:, ::2], s))
    # refusals of the autograd form
    with pytest.raises(ValueError, match="out="):
        render_volumes(v, s, out=torch.empty(N, *shape[1:], device=DEV))
    out = torch.empty(N, *shape[1:], device=DEV)
    with torch.no_grad():
        assert render_volumes(v, s, out=out) is out and torch.equal(out, image0)             # no_grad: the plain path, out= and all
    # a second derivative is refused, in words: the gradient is a function of the upstream gradient, and that graph is not built
    image, _ = render_volumes(v, s, transmittance=True)
    weight = dG.clone().requires_grad_(True)
    (first,) = torch.autograd.grad((image * weight).sum(), v, create_graph=True)
    assert first.requires_grad
    with pytest.raises(RuntimeError, match="differentiate twice"):
        first.sum().backward()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = _lib.load()
    s = RenderSettings(light="+y")
    desc = s.desc()
    vol = torch.ones(2, 4, 40, 8, device=DEV)
    G = torch.ones(2, 40, 8, device=DEV)
    grad = torch.full((2, 4, 40, 8), -7.0, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    need = L.smk_volume_render_backward_workspace(2, 4, 40, 8, _lib.SMK_LIGHT_POS_Y)
    assert need == (3 * 2 * 3 * 4 * 8 + 2 * 40 * 8) * 4
    ws = torch.empty(need // 4, device=DEV)

    def call(D=4, vstride=1280, g=G.data_ptr(), gt=None, wbytes=need, d=desc, gstride=320):
        return L.smk_volume_render_backward(vol.data_ptr(), vstride, 2 if D == 4 else 1, D, 40 if D == 4 else 1, 8, C.byref(d), g, gstride, gt, 320,
                                            grad.data_ptr(), 1280, ws.data_ptr(), wbytes, st)
    assert call(wbytes=need - 4) == _lib.SMK_ERR_INVALID and b"workspace" in L.smk_last_error()
    assert call(D=65) == _lib.SMK_ERR_UNSUPPORTED and b"D <= 64" in L.smk_last_error()
    assert call(g=None, gt=None) == _lib.SMK_ERR_INVALID and b"both null" in L.smk_last_error()
    assert call(d=_lib.SmkRenderDesc(0.1, 0.1, 0.25, 1.0, 7)) == _lib.SMK_ERR_INVALID
    assert call(vstride=1279) == _lib.SMK_ERR_INVALID
    assert call(gstride=319) == _lib.SMK_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all())
    assert call() == _lib.SMK_OK
    torch.cuda.synchronize()
    assert not bool((grad == -7.0).any())
    with pytest.raises(ValueError):
        render_backward_workspace(1, (65, 8, 8), "+y", DEV)


# ---- 6. PGD through the render ---------------------------------------------------------------------------------------------------------------
def _smoke_volumes():
    g = torch.Generator().manual_seed(21)
    return (torch.rand(2, 1, 8, 128, 128, generator=g) ** 4).to(DEV)          # mostly thin, as smoke; in [0, 1]


def test_volume_gradient_through_render_and_model():
    """d(-mse(reconstructed, target)) / d(volume) with render_volumes in front of the model against the same model behind the render written
    as torch ops (render_grad_oracle.render_torch, fp32 on the device): the model half is the same code on both sides."""
    from test_hip_input_grad import _small_model
    model = _small_model()
    assert model.input_grad == "hip"
    s = RenderSettings()
    vols = _smoke_volumes()
    noise = torch.randn(1, 3, 2, 1, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        target = F.adaptive_avg_pool2d(render_volumes(vols[:, 0], s)[:, None], (128, 128))

    def gradient(view):
        v = vols.clone().requires_grad_(True)
        out = model(view(v[:, 0])[:, None], chaos_noise=noise)["reconstructed"]
        (g,) = torch.autograd.grad(-F.mse_loss(out, target), v)
        return g
    got = gradient(lambda v: render_volumes(v, s))
    want = gradient(lambda v: render_torch(v, s.sigma_view, s.sigma_light, s.ambient, s.gain, s.light)[0])
    assert float(want.abs().max()) > 0
    e = rel_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"volume gradient through render + model: rel err {e:.2e}")
    assert e <= 1e-4, e


def test_adversarial_test_perturbs_the_volume():
    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    from test_hip_input_grad import _Ops
    torch.manual_seed(0)
    # the model of test_hip_input_grad.py's adversarial test: 64 output channels, so that the closing no_grad forwards run the fused eval head
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()
    assert model.input_grad == "hip"
    vols = _smoke_volumes()
    eps = 0.1
    torch.manual_seed(5)
    with _Ops() as ops:
        res = PerturbationTester().adversarial_test(model, vols, eps, num_steps=3, render=RenderSettings())
    assert set(res) == {"adversarial_feature_stability", "adversarial_perturbation_norm"}
    assert np.isfinite(res["adversarial_feature_stability"]) and np.isfinite(res["adversarial_perturbation_norm"])
    assert 0 < res["adversarial_perturbation_norm"] <= eps * np.sqrt(vols.numel()) * (1 + 1e-6)
    scans = sorted({n for n in ops.names if "cumsum" in n or "flip" in n})
    assert scans == [], scans                                                  # the render and its backward are the kernels
    assert ops.conv_bn() == [], ops.conv_bn()                                  # ... and so is the model's half of the step
    assert len(ops.names) > 20
    assert all(p.grad is None and p.requires_grad for p in model.parameters())
    # the recorder sees such ops when they run: the torch form of the render
    with _Ops() as seen:
        render_torch(vols[:, 0], light="-y")
    assert any("cumsum" in n for n in seen.names) and any("flip" in n for n in seen.names)
    # render=None is the code path without it: on frames, the call with and without the keyword is the same call
    with torch.no_grad():
        frames = render_volumes(vols[:, 0], RenderSettings())[:, None]
    results = []
    for kw in ({}, {"render": None}):
        torch.manual_seed(6)
        results.append(PerturbationTester().adversarial_test(model, frames, eps, num_steps=3, **kw))
    assert results[0]["adversarial_perturbation_norm"] == results[1]["adversarial_perturbation_norm"]
    assert results[0]["adversarial_feature_stability"] == pytest.approx(results[1]["adversarial_feature_stability"], abs=1e-6)
    with pytest.raises(TypeError):
        PerturbationTester().adversarial_test(model, vols, eps, num_steps=1, render={"light": "-y"})
    with pytest.raises(ValueError):
        PerturbationTester().adversarial_test(model, frames, eps, num_steps=1, render=RenderSettings())
