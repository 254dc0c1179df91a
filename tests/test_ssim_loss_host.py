"""Host-side contract of the differentiable SSIM (DESIGN.md 8.1 "Gradient"): the closed-form gradient against float64 autograd of the
reference's formula, the ABI surface of smk_image_quality_backward, `plane_ssim` / `ssim_loss` on CPU tensors (the torch route), the
`mi355x.ssim_weight` / `mi355x.ssim_window` settings of train.py and their effect on the loss terms.  No GPU: the kernels are tested in
tests/test_hip_ssim_loss.py."""
import os
import re

import pytest
import torch

from smokephysai_amd import _lib
from smokephysai_amd import evaluation
from smokephysai_amd.evaluation import RobustnessEvaluator, plane_ssim
from smokephysai_amd.models import losses
from smokephysai_amd.models.losses import ssim_loss
from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer

import ssim_grad_oracle as sgo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", sgo.KINDS)
@pytest.mark.parametrize("shape", sgo.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_closed_form_is_float64_autograd(shape, kind):
    H, W = shape
    for k in sgo.WINDOWS:
        p, t = sgo.make_case(kind, 3, H, W, seed=k)
        p, t, up = p.double(), t.double(), sgo.make_upstream(3, k).double()
        err = sgo.grad_error(sgo.closed_form_grad(p, t, k, up), sgo.autograd_grad(p, t, k, up))
        assert err <= 1e-10, (k, err)


def test_header_and_binding_declare_the_backward():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in ("smk_image_quality_backward", "smk_image_quality_backward_workspace"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/smokehip.h"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert len(_lib._SIGNATURES["smk_image_quality_backward"]) == 16
    assert len(L.smk_image_quality_backward_workspace.argtypes) == 3
    assert L.smk_image_quality_backward_workspace(2, 5, 7) == 2 * 5 * 7 * 3 * 4
    assert L.smk_image_quality_backward_workspace(0, 5, 7) == 0
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17
    assert "plane_ssim" in evaluation.__all__ and "ssim_loss" in losses.__all__


@pytest.mark.parametrize("window", [3, 11, 4])
def test_cpu_tensors_take_the_torch_route(window):
    p, t = sgo.make_case("smoke", 6, 37, 53, seed=2)
    p = p.reshape(3, 2, 37, 53).requires_grad_()
    t = t.reshape(3, 2, 37, 53)
    s = plane_ssim(p, t, window)
    assert s.shape == (3, 2) and s.dtype == torch.float32 and "PlaneSsim" not in type(s.grad_fn).__name__
    ev = RobustnessEvaluator(device="cpu")
    for i in range(3):
        for j in range(2):
            assert abs(s[i, j].item() - ev.compute_ssim(p[i:i + 1, j:j + 1].detach(), t[i:i + 1, j:j + 1], window)) <= 1e-6
    loss = ssim_loss(p, t, window)
    assert abs(loss.item() - (1 - s.mean().item())) <= 1e-7
    loss.backward()
    assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    if window % 2:
        up = torch.full((6,), -1.0 / 6, dtype=torch.float64)
        d64 = sgo.closed_form_grad(p.detach().reshape(6, 37, 53).double(), t.reshape(6, 37, 53).double(), window, up)
        assert sgo.grad_error(p.grad.reshape(6, 37, 53), d64) <= 2e-3
    assert plane_ssim(p[0, 0], t[0, 0]).shape == ()
    assert plane_ssim(p.detach().double(), t.double()).dtype == torch.float64


def test_a_target_that_requires_a_gradient_gets_one():
    p, t = sgo.make_case("uniform", 2, 16, 64, seed=3)
    p.requires_grad_()
    t.requires_grad_()
    ssim_loss(p, t, 3).backward()
    assert t.grad is not None and float(t.grad.abs().max()) > 0 and float(p.grad.abs().max()) > 0
    # SSIM is symmetric in its arguments: the target's gradient is the closed form with the roles swapped
    d64 = sgo.closed_form_grad(t.detach().double(), p.detach().double(), 3, torch.full((2,), -0.5, dtype=torch.float64))
    assert sgo.grad_error(t.grad, d64) <= 1e-5


def test_config_defaults_and_refusals():
    import train
    cfg = train.load_config(os.path.join(ROOT, "config", "config.yaml"))
    assert cfg["mi355x"]["ssim_weight"] == 0.0 and cfg["mi355x"]["ssim_window"] == 11
    assert train.ssim_settings(cfg) == (0.0, 11)
    assert train.ssim_settings({}) == (0.0, 11) and train.ssim_settings({"mi355x": None}) == (0.0, 11)
    assert train.ssim_settings({"mi355x": {"ssim_weight": 0.25, "ssim_window": 7}}) == (0.25, 7)
    for bad in ({"ssim_weight": -0.1}, {"ssim_weight": float("nan")}, {"ssim_window": 10}, {"ssim_window": 0}, {"ssim_window": 11.0},
                {"ssim_weight": 0.5, "ssim_window": -3}):
        with pytest.raises(ValueError, match="ssim_"):
            train.ssim_settings({"mi355x": bad})


class _TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)
        self.head = torch.nn.Linear(16 * 16, 3)

    def forward(self, x):
        y = torch.sigmoid(self.conv(x))
        return {"reconstructed": y, "physics_features": self.head(y.flatten(1))}


@pytest.mark.parametrize("route", ["torch", "hip"])
def test_batch_loss_terms_with_and_without_the_ssim_term(route):
    import train
    torch.manual_seed(5)
    model = _TinyNet()
    batch = {"input": torch.rand(3, 1, 16, 16), "target": torch.rand(3, 1, 16, 16), "chaos_features": torch.rand(3, 3),
             "sequence": torch.rand(3, 5, 16, 16)}
    reg = PhysicsRegularizer(conservation_weight=0.7, continuity_weight=1.3)
    parent, vec0 = train._batch_loss_terms(model, reg, batch, "cpu", losses=route)
    off, vec1 = train._batch_loss_terms(model, reg, batch, "cpu", losses=route, ssim_weight=0.0, ssim_window=5)
    assert vec0 is None and vec1 is None and len(off) == len(parent) == 4
    for a, b in zip(off, parent):
        assert torch.equal(a, b)
    on, _ = train._batch_loss_terms(model, reg, batch, "cpu", losses=route, ssim_weight=0.5, ssim_window=5)
    with torch.no_grad():
        term = ssim_loss(model(batch["input"])["reconstructed"], batch["target"], 5)
    assert float(term) > 0
    assert abs(on[0].item() - parent[0].item() - 0.5 * term.item()) <= 1e-6
    for a, b in zip(on[1:], parent[1:]):
        assert torch.equal(a, b)
    assert torch.equal(train.batch_losses(model, reg, batch, "cpu", losses=route, ssim_weight=0.5, ssim_window=5)[0], on[0])
    on[0].backward()
    assert all(p.grad is not None for p in model.parameters())
