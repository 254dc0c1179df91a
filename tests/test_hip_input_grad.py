"""Eval-mode input gradients on libsmokehip: the data gradient of the first convolution (smk_conv1_train_dgrad), BatchNorm + ReLU + pool from
the running statistics under autograd (hip_frozen_bn_relu_pool), and the 'hip_grad' route of SmokePhysNet that strings them together with
the conv2 and reconstruction-head nodes -- against float64 autograd, and with a recorder that shows no PyTorch convolution / BatchNorm op
is left on the route (forward or backward)."""
import copy
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.utils._python_dispatch import TorchDispatchMode

from conftest import rel_err
from smokephysai_amd import _lib

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3                 # SMK_ERR_UNSUPPORTED (include/smokehip.h)
_TORCH_CONV_BN = re.compile(r"^aten\.(convolution|miopen_|cudnn_|\w*batch_norm)")


class _Ops(TorchDispatchMode):
    """Every ATen op dispatched while active, on the calling thread and on autograd's device threads (the engine carries the mode over)."""

    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))

    def conv_bn(self):
        return sorted({n for n in self.names if _TORCH_CONV_BN.match(n)})


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
DGRAD_SHAPES = [(1, 1, 4), (2, 7, 12), (1, 8, 16), (3, 40, 48), (1, 5, 260), (2, 64, 64), (2, 128, 128)]


def _dgrad(dz, w):
    B, _, H, W = dz.shape
    dx = torch.full((B, 1, H, W), float("nan"), device="cuda")
    _lib.check(_lib.load().smk_conv1_train_dgrad(dz.data_ptr(), w.data_ptr(), B, H, W, dx.data_ptr(), _lib.stream_ptr(dz.device)))
    return dx


@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv1_dgrad_matches_float64_autograd(shape):
    """Bound: 1e-5 max-norm relative, what the project holds its fp32 convolution gradients to (test_hip_encoder.py: conv1's weight gradient)."""
    from smokephysai_amd.models.conv import hip_conv1_frozen, hip_conv1_frozen_supported
    B, H, W = shape
    torch.manual_seed(sum(shape))
    conv = nn.Conv2d(1, 64, 7, padding=3)
    dz = torch.randn(B, 64, H, W)
    x64 = torch.zeros(B, 1, H, W, dtype=torch.float64, requires_grad=True)
    copy.deepcopy(conv).double()(x64).backward(dz.double())
    ref = x64.grad.numpy()

    conv, dz = conv.cuda(), dz.cuda()
    w = conv.weight.detach().contiguous()
    dx = _dgrad(dz, w)
    assert not torch.isnan(dx).any()                             # every element written
    err = rel_err(dx.cpu().numpy(), ref)
    print(f"conv1 dgrad {shape}: rel err {err:.3e}")
    assert err < 1e-5, err
    assert torch.equal(_dgrad(dz, w), dx)                        # bit-identical when repeated
    # ... and the autograd node hands out exactly this
    x = torch.rand(B, 1, H, W, device="cuda", requires_grad=True)
    assert hip_conv1_frozen_supported(x, conv)
    hip_conv1_frozen(x, conv).backward(dz)
    assert torch.equal(x.grad, dx) and conv.weight.grad is None and conv.bias.grad is None


def test_conv1_dgrad_refuses_bad_shapes_without_launching():
    L = _lib.load()
    dz = torch.randn(1, 64, 4, 8, device="cuda")
    w = torch.randn(64, 7, 7, device="cuda")
    dx = torch.full((1, 1, 4, 8), float("nan"), device="cuda")
    st = _lib.stream_ptr(dz.device)
    assert L.smk_conv1_train_dgrad(dz.data_ptr(), w.data_ptr(), 1, 4, 6, dx.data_ptr(), st) == UNSUPPORTED      # W = 6
    assert b"multiple of 4" in L.smk_last_error()
    assert L.smk_conv1_train_dgrad(dz.data_ptr(), w.data_ptr(), 0, 4, 8, dx.data_ptr(), st) == UNSUPPORTED      # B = 0
    assert L.smk_conv1_train_dgrad(dz.data_ptr(), w.data_ptr(), 65536, 4, 8, dx.data_ptr(), st) == UNSUPPORTED
    assert L.smk_conv1_train_dgrad(dz.data_ptr(), w.data_ptr(), 1, 0, 8, dx.data_ptr(), st) == UNSUPPORTED
    assert L.smk_conv1_train_dgrad(dz.data_ptr() + 4, w.data_ptr(), 1, 4, 8, dx.data_ptr(), st) != 0           # alignment
    torch.cuda.synchronize()
    assert torch.isnan(dx).all()
    with pytest.raises(ValueError):
        from smokephysai_amd.models.conv import hip_conv1_frozen
        hip_conv1_frozen(torch.zeros(1, 1, 4, 6, device="cuda"), nn.Conv2d(1, 64, 7, padding=3).cuda())


# ---- BatchNorm (running statistics) + ReLU + pool -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("pool", [1, 4, 8])
def test_frozen_bn_relu_pool_matches_float64_autograd(pool, C):
    """Forward and dz against float64 adaptive_avg_pool2d(relu(batch_norm(eval))), both below 1e-5 max-norm relative.  No pre-activation lies
    within 1e-4 of zero (such entries are moved to 0.5), so no fp32 / fp64 ReLU mask can differ: the kernel is tested, not the rounding."""
    from smokephysai_amd.models.norm import hip_frozen_bn_relu_pool
    S = 32 * pool
    g = torch.Generator().manual_seed(100 * pool + C)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_((torch.rand(C, generator=g) + 0.5) * (1 - 2 * (torch.rand(C, generator=g) < 0.25).float()))     # some negative
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.3)
        bn.num_batches_tracked.fill_(7)
    bn.eval()
    bn64 = copy.deepcopy(bn).double()
    z = torch.randn(2, C, S, S, generator=g)
    with torch.no_grad():
        sc = (bn64.weight / torch.sqrt(bn64.running_var + bn.eps)).view(1, C, 1, 1)
        sh = bn64.bias.view(1, C, 1, 1) - bn64.running_mean.view(1, C, 1, 1) * sc
        near = (z.double() * sc + sh).abs() < 1e-4
        z = torch.where(near, ((0.5 - sh) / sc).expand_as(z).float(), z)
        assert float((z.double() * sc + sh).abs().min()) >= 1e-4
    dout = torch.randn(2, C, 32, 32, generator=g)
    z64 = z.double().requires_grad_(True)
    ref = F.adaptive_avg_pool2d(F.relu(bn64(z64)), (32, 32))
    ref.backward(dout.double())

    bn = bn.cuda()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    zc = z.cuda().requires_grad_(True)
    out = hip_frozen_bn_relu_pool(zc, bn, pool)
    assert out.shape == ref.shape
    out.backward(dout.cuda())
    e_out, e_dz = rel_err(out.detach().cpu().numpy(), ref.detach().numpy()), rel_err(zc.grad.cpu().numpy(), z64.grad.numpy())
    print(f"frozen bn pool {pool} C {C}: forward {e_out:.3e} dz {e_dz:.3e}")
    assert e_out < 1e-5 and e_dz < 1e-5, (e_out, e_dz)
    assert all(torch.equal(v, state[k]) for k, v in bn.state_dict().items())         # running statistics, num_batches_tracked, gamma, beta
    assert bn.weight.grad is None and bn.bias.grad is None


# ---- the whole model ---------------------------------------------------------------------------------------------------------------
def _small_model(frozen=True):
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4, output_channels=16)
    with torch.no_grad():                                        # running statistics of a trained model, not the 0 / 1 of a fresh one
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    model = model.cuda().eval()
    for p in model.parameters():
        p.requires_grad_(not frozen)
    return model


def _input_gradient(model, x, noise):
    """-mse(reconstructed, target) as adversarial_test states it (target: the clean frames, at the head's 128 x 128), d / d frames."""
    x = x.clone().requires_grad_(True)
    out = model(x, chaos_noise=noise)["reconstructed"]
    target = x.detach() if x.shape[-1] == out.shape[-1] else F.avg_pool2d(x.detach(), x.shape[-1] // out.shape[-1])
    (grad,) = torch.autograd.grad(-F.mse_loss(out, target), x)
    return out.detach(), grad


@pytest.fixture(scope="module")
def routes():
    """Per frame shape: the gradient and the output on 'hip', on 'torch' and on a float64 copy, and the ATen ops of the two fp32 runs."""
    cache = {}

    def get(shape):
        if shape not in cache:
            model = _small_model()
            g = torch.Generator().manual_seed(11)
            x = torch.rand(*shape, generator=g).cuda()
            noise = torch.randn(1, 3, shape[0], 1, generator=g).cuda()
            m64 = copy.deepcopy(model).double()
            for m in m64.modules():
                if "hip_train" in m.__dict__ or hasattr(type(m), "hip_train"):
                    m.hip_train = False
            res = {}
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                res["f64"] = _input_gradient(m64, x.double(), noise.double())      # (the module route, with its one-time hint)
                del caught[:]
                for route in ("hip", "torch"):
                    model.input_grad = route
                    with _Ops() as ops:
                        res[route] = _input_gradient(model, x, noise)
                    res[route + "_ops"] = ops
                    res[route + "_warned"] = any("eval forward with autograd" in str(w.message) for w in caught)
                    del caught[:]
            cache[shape] = res
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", [(2, 1, 128, 128), (1, 1, 256, 256)], ids=["2x128", "1x256"])
def test_input_gradient_stays_in_the_band_of_the_pytorch_route(routes, shape):
    """ReLU masks near zero flip in ANY fp32 forward, so the yardstick is PyTorch's own fp32 route against the same float64 model (the band
    rule of test_hip_pipeline.py): err_hip < max(2 err_torch, 1e-4); the two fp32 outputs agree within 1e-4."""
    r = routes(shape)
    ref = r["f64"][1].cpu().numpy()
    assert np.abs(ref).max() > 0
    err_hip, err_torch = rel_err(r["hip"][1].cpu().numpy(), ref), rel_err(r["torch"][1].cpu().numpy(), ref)
    out_diff = rel_err(r["hip"][0].cpu().numpy(), r["torch"][0].cpu().numpy())
    print(f"input gradient {shape}: hip {err_hip:.3e} torch {err_torch:.3e}; outputs differ by {out_diff:.3e}")
    assert err_hip < max(2.0 * err_torch, 1e-4), (err_hip, err_torch)
    assert out_diff < 1e-4, out_diff


@pytest.mark.parametrize("shape", [(2, 1, 128, 128), (1, 1, 256, 256)], ids=["2x128", "1x256"])
def test_no_pytorch_convolution_or_batchnorm_on_the_hip_route(routes, shape):
    r = routes(shape)
    seen = r["torch_ops"].conv_bn()
    # the recorder works, on the backward's thread too: PyTorch's route shows its convolutions, their backward and its BatchNorms
    assert any(n.startswith("aten.convolution_backward") for n in seen), seen
    assert any("batch_norm" in n for n in seen), seen
    assert r["torch_warned"]
    assert r["hip_ops"].conv_bn() == [], r["hip_ops"].conv_bn()
    assert not r["hip_warned"]
    assert len(r["hip_ops"].names) > 20


def test_adversarial_test_runs_without_pytorch_convolutions():
    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    # test_hip_evaluation.py's model: the default 64 output channels, so that the closing no_grad forwards run the fused eval head as well
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()
    assert model.input_grad == "hip"
    x = torch.rand(2, 1, 128, 128, device="cuda")
    eps = 0.1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with _Ops() as ops:
            res = PerturbationTester().adversarial_test(model, x, epsilon=eps, num_steps=3)
    assert ops.conv_bn() == [], ops.conv_bn()
    assert not any("eval forward with autograd" in str(m.message) for m in w)
    assert set(res) == {"adversarial_feature_stability", "adversarial_perturbation_norm"}
    assert 0 < res["adversarial_perturbation_norm"] <= eps * np.sqrt(x.numel()) * (1 + 1e-6)
    assert np.isfinite(res["adversarial_feature_stability"])
    assert all(p.grad is None for p in model.parameters())
    assert all(p.requires_grad for p in model.parameters())


def test_parameters_that_want_gradients_keep_the_module_route():
    model = _small_model(frozen=False)
    x = torch.rand(2, 1, 128, 128, device="cuda", requires_grad=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert model._encoder_route(x) == "modules"
        out = model(x)["reconstructed"]
    assert any("eval forward with autograd" in str(m.message) for m in w)
    (-F.mse_loss(out, x.detach())).backward()
    g = model.input_encoder[0].weight.grad
    assert g is not None and float(g.abs().max()) > 0 and x.grad is not None
    model.input_grad = "torch"
    for p in model.parameters():
        p.requires_grad_(False)
    assert model._encoder_route(x) == "modules"                  # the switch gives the former behaviour
    model.input_grad = "hip"
    assert model._encoder_route(x) == "hip_grad"
    assert model._encoder_route(torch.rand(2, 1, 64, 64, device="cuda", requires_grad=True)) == "modules"
    with torch.no_grad():
        assert model._encoder_route(x) == "hip"
