"""The differentiable SSIM on the MI355X: smk_image_quality_backward through the C ABI and through `plane_ssim` / `ssim_loss` under
autograd, against the float64 closed form of tests/ssim_grad_oracle.py (DESIGN.md 8.1 "Gradient") at the fp32-rounded inputs.

Metric: err = max|d - d64| / max|d64|.  Bound per case: 4 x the error of torch's fp32 CPU autograd of the reference's formula on the
same case (computed here, on the CPU), never below 1e-5 (the project's gradient bound, SPEC_3D 10/11).  The factor 4 (two bits) allows
for the kernel's direct k-term sums, which run in another order than avg_pool2d's and feed the E[x^2] - mu^2 cancellation.  A case whose
partner is so inexact that the bound would pass 2e-3 checks nothing, so the bound is capped there."""
import functools

import pytest
import torch
import torch.nn.functional as F

from smokephysai_amd import _lib
from smokephysai_amd.evaluation import plane_ssim
from smokephysai_amd.evaluation.robustness_metrics import C1, C2, ssim_torch
from smokephysai_amd.models.losses import ssim_loss
from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer

import ssim_grad_oracle as sgo

pytestmark = pytest.mark.gpu

BOUND_FLOOR, BOUND_CAP, BOUND_FACTOR = 1e-5, 2e-3, 4.0


def _seed(kind, n, H, W, k):
    return 100000 * sgo.KINDS.index(kind) + 10000 * n + 37 * H + 11 * W + k


@functools.lru_cache(maxsize=None)
def _case(kind, n, H, W, k):
    """Inputs, upstream gradient, the float64 gradient and plane means at the fp32-rounded inputs, and the case's bound."""
    seed = _seed(kind, n, H, W, k)
    p, t = sgo.make_case(kind, n, H, W, seed)
    up = sgo.make_upstream(n, seed)
    d64 = sgo.closed_form_grad(p.double(), t.double(), k, up.double())
    partner = sgo.grad_error(sgo.autograd_grad(p, t, k, up), d64)
    bound = min(max(BOUND_FACTOR * partner, BOUND_FLOOR), BOUND_CAP)
    return p, t, up, d64, sgo.plane_means(p.double(), t.double(), k), partner, bound


def _backward(pred, target, k, up, dpred=None, n=None, pred_stride=None, dpred_stride=None, workspace="auto", workspace_bytes=None):
    """smk_image_quality_backward on device planes [n, H, W] (dense rows); returns (status, dpred)."""
    L = _lib.load()
    H, W = pred.shape[-2:]
    n = pred.shape[0] if n is None else n
    if dpred is None:
        dpred = torch.full((n, H, W), float("nan"), device=pred.device)
    need = int(L.smk_image_quality_backward_workspace(pred.shape[0], H, W))
    ws = torch.empty(need, dtype=torch.uint8, device=pred.device) if workspace == "auto" else workspace
    rc = L.smk_image_quality_backward(pred.data_ptr(), pred.stride(0) if pred_stride is None else pred_stride, target.data_ptr(),
                                      target.stride(0), n, H, W, k, float(C1), float(C2), up.data_ptr(),
                                      None if ws is None else ws.data_ptr(), need if workspace_bytes is None else workspace_bytes,
                                      dpred.data_ptr(), dpred.stride(0) if dpred_stride is None else dpred_stride,
                                      _lib.stream_ptr(pred.device))
    torch.cuda.synchronize()
    return rc, dpred


@pytest.mark.parametrize("k", sgo.WINDOWS)
@pytest.mark.parametrize("kind", sgo.KINDS)
@pytest.mark.parametrize("shape", sgo.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradient_and_value_match_the_float64_closed_form(shape, kind, k):
    """The hardest case is 1x1-near-1: a single pixel with pred = target + 1e-3 N(0, 1) at window 1 has a gradient of about
    2 (y - x) / B1 ~ 1e-3 next to terms of size 1 / C2 ~ 1e3.  Torch's fp32 autograd is off by 1.9e-2 (n = 1) and 3.4e-3 (n = 3) there, so
    the bound is the 2e-3 cap; the kernel sums the two large terms of opposite sign first and stays below 1e-4."""
    H, W = shape
    for n in (1, 3):
        p, t, up, d64, means64, partner, bound = _case(kind, n, H, W, k)
        dp, dt, dup = p.cuda(), t.cuda(), up.cuda()
        rc, d = _backward(dp, dt, k, dup)
        assert rc == _lib.SMK_OK, _lib.load().smk_last_error()
        err = sgo.grad_error(d.cpu(), d64)
        print(f"ssim-grad {H}x{W} {kind} k={k} n={n}: kernel {err:.3e} torch-fp32 {partner:.3e} bound {bound:.3e} "
              f"ratio {err / max(partner, 1e-30):.2f}")
        # the same launch under autograd, and the forward value (tests/test_hip_evaluation.py's bound)
        q = dp.clone().requires_grad_()
        s = plane_ssim(q, dt, k)
        assert s.shape == (n,) and s.dtype == torch.float32 and "PlaneSsim" in type(s.grad_fn).__name__
        assert float((s.detach().cpu().double() - means64).abs().max()) <= 2e-6, n
        (s * dup).sum().backward()
        assert torch.equal(q.grad, d), n
        assert err <= bound, (n, err, partner, bound)


def test_every_element_is_written_once_and_calls_repeat():
    p, t, up, d64, _, _, bound = _case("smoke", 3, 33, 130, 11)
    dp, dt, dup = p.cuda(), t.cuda(), up.cuda()
    flat = torch.full((3 * 33 * 130 + 257,), float("nan"), device="cuda")
    rc, _ = _backward(dp, dt, 11, dup, dpred=flat[:3 * 33 * 130].view(3, 33, 130))
    assert rc == _lib.SMK_OK
    assert torch.isfinite(flat[:3 * 33 * 130]).all() and torch.isnan(flat[3 * 33 * 130:]).all()
    rc2, again = _backward(dp, dt, 11, dup)
    assert rc2 == _lib.SMK_OK and torch.equal(again.flatten(), flat[:3 * 33 * 130])
    # a plane's gradient does not depend on which planes share its call
    for i in range(3):
        rc1, alone = _backward(dp[i:i + 1], dt[i:i + 1], 11, dup[i:i + 1])
        assert rc1 == _lib.SMK_OK and torch.equal(alone[0], again[i]), i
    assert torch.equal(again[1], torch.zeros_like(again[1]))                # upstream gradient exactly 0
    assert sgo.grad_error(again.cpu(), d64) <= bound


def test_strided_planes_in_and_out():
    p, t, up, d64, _, _, bound = _case("uniform", 3, 37, 53, 3)
    big_p = torch.rand(3, 2, 37, 53, device="cuda")
    big_t = torch.rand(3, 2, 37, 53, device="cuda")
    big_p[:, 1], big_t[:, 0] = p.cuda(), t.cuda()
    vp, vt, dup = big_p[:, 1], big_t[:, 0], up.cuda()
    assert vp.stride(0) == 2 * 37 * 53 and not vp.is_contiguous()
    out = torch.full((3, 2, 37, 53), float("nan"), device="cuda")
    rc, _ = _backward(vp, vt, 3, dup, dpred=out[:, 0])
    assert rc == _lib.SMK_OK and torch.isnan(out[:, 1]).all()
    rc, dense = _backward(vp.contiguous(), vt.contiguous(), 3, dup)
    assert rc == _lib.SMK_OK and torch.equal(out[:, 0], dense)
    assert sgo.grad_error(dense.cpu(), d64) <= bound
    big_p.requires_grad_()
    (plane_ssim(big_p[:, 1], vt, 3) * dup).sum().backward()
    assert torch.equal(big_p.grad[:, 1], dense) and torch.equal(big_p.grad[:, 0], torch.zeros_like(dense))


def test_chunks_past_65535_planes():
    n, H, W, k = 65537, 2, 3, 3
    p, t, up, d64, means64, partner, bound = _case("uniform", n, H, W, k)
    q = p.cuda().requires_grad_()
    s = plane_ssim(q, t.cuda(), k)
    assert s.shape == (n,) and float((s.detach().cpu().double() - means64).abs().max()) <= 2e-6
    (s * up.cuda()).sum().backward()
    err = sgo.grad_error(q.grad.cpu(), d64)
    print(f"ssim-grad 65537 planes: kernel {err:.3e} torch-fp32 {partner:.3e} bound {bound:.3e}")
    assert err <= bound
    # the planes on both sides of the chunk boundary are the ones a call of their own gives
    rc, tail = _backward(q.detach()[65534:], t.cuda()[65534:], k, up.cuda()[65534:])
    assert rc == _lib.SMK_OK and torch.equal(tail, q.grad[65534:])


def test_refusals_leave_the_output_alone():
    p, t, up, *_ = _case("uniform", 3, 17, 65, 3)
    dp, dt, dup = p.cuda(), t.cuda(), up.cuda()
    hw = 17 * 65
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    refused = [dict(k=4), dict(k=33), dict(k=0), dict(k=3, pred_stride=hw - 1), dict(k=3, dpred_stride=hw - 1), dict(k=3, workspace=None),
               dict(k=3, workspace=small, workspace_bytes=16), dict(k=3, workspace_bytes=3 * hw * 3 * 4 - 1), dict(k=3, n=0),
               dict(k=3, n=65536)]
    for kw in refused:
        out = torch.full((3, 17, 65), -7.0, device="cuda")
        rc, _ = _backward(dp, dt, kw.pop("k"), dup, dpred=out, **kw)
        assert rc == _lib.SMK_ERR_INVALID, kw
        assert torch.equal(out, torch.full_like(out, -7.0)), kw


@pytest.mark.parametrize("kind", sgo.KINDS)
def test_ssim_loss_backward_on_the_device(kind):
    p, t, _, _, means64, _, _ = _case(kind, 3, 37, 53, 11)
    up = torch.full((6,), -1.0 / 6, dtype=torch.float64)                     # d(1 - mean)/d(plane mean), 6 planes
    p2, t2 = torch.cat([p, p.flip(0)]), torch.cat([t, t.flip(0)])
    d64 = sgo.closed_form_grad(p2.double(), t2.double(), 11, up)
    partner = sgo.grad_error(sgo.autograd_grad(p2, t2, 11, up.float()), d64)
    bound = min(max(BOUND_FACTOR * partner, BOUND_FLOOR), BOUND_CAP)
    q = p2.reshape(3, 2, 37, 53).cuda().requires_grad_()
    loss = ssim_loss(q, t2.reshape(3, 2, 37, 53).cuda())
    assert abs(loss.item() - (1 - float(means64.mean()))) <= 2e-6
    loss.backward()
    err = sgo.grad_error(q.grad.cpu().reshape(6, 37, 53), d64)
    print(f"ssim_loss {kind}: kernel {err:.3e} torch-fp32 {partner:.3e} bound {bound:.3e}")
    assert err <= bound
    # a target that wants a gradient is torch's; the kernel route is first order only
    tq = t2.reshape(3, 2, 37, 53).cuda().requires_grad_()
    s = plane_ssim(q, tq)
    assert "PlaneSsim" not in type(s.grad_fn).__name__
    s.sum().backward()
    assert tq.grad is not None and float(tq.grad.abs().max()) > 0
    first, = torch.autograd.grad((plane_ssim(q, tq.detach()) ** 2).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        first.sum().backward()


class _TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)
        self.head = torch.nn.Linear(16 * 16, 3)

    def forward(self, x):
        self.reconstructed = torch.sigmoid(self.conv(x))
        self.reconstructed.retain_grad()
        return {"reconstructed": self.reconstructed, "physics_features": self.head(self.reconstructed.flatten(1))}


def _all_torch_grad(recon, batch, model, reg, window, dtype):
    """d total / d reconstructed of train.py's decomposition plus 0.5 * (1 - mean SSIM), every term a torch formula on the CPU."""
    r = recon.to(dtype).requires_grad_()
    tgt, seq, ct = batch["target"].to(dtype), batch["sequence"].to(dtype), batch["chaos_features"].to(dtype)
    feats = F.linear(r.flatten(1), model.head.weight.detach().cpu().to(dtype), model.head.bias.detach().cpu().to(dtype))
    physics = reg({"density": r, "density_sequence": seq}, {"density": tgt})["total_physics_loss"]
    total = F.mse_loss(r, tgt) + 0.1 * F.mse_loss(feats, ct) + 0.05 * physics + 0.5 * (1 - ssim_torch(r, tgt, window).mean((-2, -1)).mean())
    total.backward()
    return r.grad


@pytest.mark.parametrize("route", ["hip", "torch"])
def test_batch_loss_terms_gradient_is_the_all_torch_formula(route):
    import train
    torch.manual_seed(5)
    model = _TinyNet().cuda()
    batch = {"input": torch.rand(3, 1, 16, 16), "target": torch.rand(3, 1, 16, 16), "chaos_features": torch.rand(3, 3),
             "sequence": torch.rand(3, 5, 16, 16)}
    reg = PhysicsRegularizer(conservation_weight=0.7, continuity_weight=1.3)
    (total, recon, phys, chaos), vec = train._batch_loss_terms(model, reg, batch, "cuda", losses=route, ssim_weight=0.5, ssim_window=5)
    assert (vec is not None) == (route == "hip")
    (base, recon0, phys0, chaos0), _ = train._batch_loss_terms(model, reg, batch, "cuda", losses=route)
    term = ssim_loss(model.reconstructed.detach(), batch["target"].cuda(), 5)
    assert abs(total.item() - base.item() - 0.5 * term.item()) <= 1e-6
    assert torch.equal(recon, recon0) and torch.equal(phys, phys0) and torch.equal(chaos, chaos0)
    (total, *_), _ = train._batch_loss_terms(model, reg, batch, "cuda", losses=route, ssim_weight=0.5, ssim_window=5)
    total.backward()
    got = model.reconstructed.grad.cpu()
    values = model.reconstructed.detach().cpu()
    d64 = _all_torch_grad(values, batch, model, reg, 5, torch.float64)
    partner = sgo.grad_error(_all_torch_grad(values, batch, model, reg, 5, torch.float32), d64)
    bound = min(max(BOUND_FACTOR * partner, BOUND_FLOOR), BOUND_CAP)
    err = sgo.grad_error(got, d64)
    print(f"_batch_loss_terms {route}: {err:.3e} torch-fp32 {partner:.3e} bound {bound:.3e}")
    assert err <= bound
