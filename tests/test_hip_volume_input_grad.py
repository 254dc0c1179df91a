"""Input gradients for volumes on libsmokehip (SPEC_3D.md section 11, "Input gradients"): Encoder3D's 'frozen' route -- the training
convolutions with BatchNorm3d from the running statistics and smk_conv3d_s7_dgrad at the end of the backward -- alone and inside
SmokePhysNet3D against float64 autograd, the same gradient in training mode, a recorder that shows no PyTorch convolution / BatchNorm op is
left on the route, and PerturbationTester / RobustnessEvaluator on a volume model."""
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

pytestmark = pytest.mark.gpu

_TORCH_CONV_BN = re.compile(r"^aten\.(convolution|miopen_|cudnn_|\w*batch_norm)")
VOLUMES = [(2, 1, 4, 32, 32), (1, 1, 3, 64, 32)]
IDS = ["2x4x32x32", "1x3x64x32"]


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


def _err(a, b):
    return rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _small_model(frozen=True):
    from smokephysai_amd.models import SmokePhysNet3D
    torch.manual_seed(0)
    model = SmokePhysNet3D(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4, output_channels=16)
    with torch.no_grad():                                        # running statistics of a trained model, not the 0 / 1 of a fresh one
        for m in model.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
            if isinstance(m, nn.BatchNorm3d):                    # away from the identity: a BatchNorm that scales and shifts
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    model = model.cuda().eval()
    if frozen:
        for p in model.parameters():
            p.requires_grad_(False)
    return model


def _float64(model):
    m64 = copy.deepcopy(model).double()
    m64.encoder3d.route = "torch"
    for m in m64.modules():
        if "hip_train" in m.__dict__ or hasattr(type(m), "hip_train"):
            m.hip_train = False
    return m64


def _rendered(x, size):
    """The front view of the clean volumes at the head's size: what adversarial_test compares the reconstruction with."""
    from smokephysai_amd.physics.render import render_volumes
    img = render_volumes(x[:, 0].detach().float().contiguous())[:, None]
    return img if img.shape[-2:] == tuple(size) else F.adaptive_avg_pool2d(img, size)


def _input_gradient(model, x, noise, target):
    x = x.clone().requires_grad_(True)
    out = model(x, chaos_noise=noise)["reconstructed"]
    (grad,) = torch.autograd.grad(-F.mse_loss(out, target.to(out.dtype)), x)
    return out.detach(), grad


@pytest.fixture(scope="module")
def routes():
    """Per volume shape: the gradient and the output on 'hip', on 'torch' and on a float64 copy, and the ATen ops of the two fp32 runs."""
    cache = {}

    def get(shape):
        if shape not in cache:
            model = _small_model()
            g = torch.Generator().manual_seed(11)
            x = torch.rand(*shape, generator=g).cuda()
            noise = torch.randn(1, 3, shape[0], 1, generator=g).cuda()
            target = _rendered(x, (128, 128))
            res = {}
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                res["f64"] = _input_gradient(_float64(model), x.double(), noise.double(), target)
                del caught[:]
                for route in ("hip", "torch"):
                    model.input_grad = route
                    with _Ops() as ops:
                        res[route] = _input_gradient(model, x, noise, target)
                    res[route + "_ops"] = ops
                    res[route + "_warnings"] = [str(w.message) for w in caught]
                    del caught[:]
            cache[shape] = res
        return cache[shape]
    return get


# ---- the encoder alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VOLUMES, ids=IDS)
def test_encoder3d_frozen_route_matches_float64(shape):
    """Tokens within 1e-5 and d (tokens * r).sum() / d volume within 1e-4 of a float64 copy on route="torch": the bounds
    test_hip_encoder3d_train.py holds the training route to."""
    enc = _small_model().encoder3d
    ref = copy.deepcopy(enc).double()
    ref.route = "torch"
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    x = torch.rand(*shape, device="cuda", generator=g).requires_grad_(True)
    r = torch.randn(shape[0], 1024, 128, device="cuda", generator=g)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    assert enc._route(x[:, 0]) == "frozen"
    tok = enc.tokens(x)
    assert "HipBn3dClFrozen" in type(tok.grad_fn).__name__ and tok.shape == (shape[0], 1024, 128)
    (grad,) = torch.autograd.grad((tok * r).sum(), x)
    x64 = x.detach().double().requires_grad_(True)
    tok64 = ref.tokens(x64)
    (grad64,) = torch.autograd.grad((tok64 * r.double()).sum(), x64)
    e_tok, e_grad = _err(tok, tok64), _err(grad, grad64)
    print(f"Encoder3D frozen {shape}: tokens {e_tok:.3e} volume gradient {e_grad:.3e}")
    assert float(grad64.abs().max()) > 0
    assert e_tok < 1e-5, e_tok
    assert e_grad < 1e-4, e_grad
    assert all(torch.equal(v, state[k]) for k, v in enc.state_dict().items())        # running statistics and num_batches_tracked untouched
    assert all(p.grad is None for p in enc.parameters())


# ---- the whole model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VOLUMES, ids=IDS)
def test_input_gradient_stays_in_the_band_of_the_pytorch_route(routes, shape):
    """The band rule of test_hip_input_grad.py, unchanged: ReLU masks near zero flip in ANY fp32 forward, so the yardstick is PyTorch's own
    fp32 route against the same float64 model: err_hip < max(2 err_torch, 1e-4); the two fp32 outputs agree within 1e-4."""
    r = routes(shape)
    ref = r["f64"][1].cpu().numpy()
    assert np.abs(ref).max() > 0
    err_hip, err_torch = rel_err(r["hip"][1].cpu().numpy(), ref), rel_err(r["torch"][1].cpu().numpy(), ref)
    out_diff = rel_err(r["hip"][0].cpu().numpy(), r["torch"][0].cpu().numpy())
    print(f"volume input gradient {shape}: hip {err_hip:.3e} torch {err_torch:.3e}; outputs differ by {out_diff:.3e}")
    assert err_hip < max(2.0 * err_torch, 1e-4), (err_hip, err_torch)
    assert out_diff < 1e-4, out_diff


@pytest.mark.parametrize("shape", VOLUMES, ids=IDS)
def test_no_pytorch_convolution_or_batchnorm_on_the_hip_route(routes, shape):
    r = routes(shape)
    seen = r["torch_ops"].conv_bn()
    # the recorder works, on the backward's thread too: PyTorch's route shows its convolutions, their backward and its BatchNorms
    assert any(n.startswith("aten.convolution_backward") for n in seen), seen
    assert any("batch_norm" in n for n in seen), seen
    assert r["hip_ops"].conv_bn() == [], r["hip_ops"].conv_bn()
    assert r["hip_warnings"] == [], r["hip_warnings"]
    assert len(r["hip_ops"].names) > 20


def test_routes():
    model = _small_model()
    enc = model.encoder3d
    x = torch.rand(2, 4, 32, 32, device="cuda", requires_grad=True)
    assert enc._route(x) == "frozen"
    assert enc._route(x, "torch") == "torch"                     # SmokePhysNet3D.input_grad = "torch": the A/B partner
    assert enc._route(x.detach()) == "torch"                     # nothing to differentiate on this route: the modules, as before
    with torch.no_grad():
        assert enc._route(x) == "eval"
    assert enc._route(torch.rand(2, 4, 48, 32, device="cuda", requires_grad=True)) == "torch"       # H = 48
    assert enc._route(x.double()) == "torch" and enc._route(x.cpu()) == "torch"
    enc.net[0].weight.requires_grad_(True)                       # a parameter wants a gradient: the modules
    assert enc._route(x) == "torch"
    enc.net[0].weight.requires_grad_(False)
    enc.net[1].train()                                           # a BatchNorm that is not frozen
    assert enc._route(x) == "torch"
    enc.net[1].eval()
    enc.route = "torch"
    assert enc._route(x) == "torch"
    enc.route = "hip"
    assert enc._route(x) == "frozen"
    enc.train()
    assert enc._route(x) == "train" and enc._route(x.detach()) == "train"
    enc.eval()
    # the model hands its switch down
    model.input_grad = "torch"
    with _Ops() as ops:
        model(x[:, None])
    assert any(n.startswith("aten.convolution") for n in ops.conv_bn())
    model.input_grad = "hip"
    with _Ops() as ops:
        out = model(x[:, None])["reconstructed"]
    assert ops.conv_bn() == [] and out.requires_grad


# ---- training mode ------------------------------------------------------------------------------------------------------------------
def test_training_mode_volume_gets_its_gradient():
    """Batch statistics: the volume gradient within 1e-4 of the float64 torch route, while the parameter gradients stay within the bounds of
    test_hip_encoder3d_train.py (weights 1e-4, dgamma / dbeta 1e-3, the two biases below 1e-3 of the largest gradient)."""
    enc = _small_model(frozen=False).encoder3d.train()
    ref = copy.deepcopy(enc).double()
    ref.route = "torch"
    shape = (2, 1, 4, 32, 32)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(*shape, device="cuda", generator=g).requires_grad_(True)
    r = torch.randn(2, 1024, 128, device="cuda", generator=g)
    assert enc._route(x[:, 0]) == "train"
    (enc.tokens(x) * r).sum().backward()
    x64 = x.detach().double().requires_grad_(True)
    (ref.tokens(x64) * r.double()).sum().backward()
    assert x.grad is not None and float(x64.grad.abs().max()) > 0
    grads, grads64 = {n: p.grad for n, p in enc.named_parameters()}, {n: p.grad for n, p in ref.named_parameters()}
    top = max(float(v.abs().max()) for v in grads64.values())
    e = {"volume": _err(x.grad, x64.grad)}
    for n in grads:
        e[n] = float(grads[n].abs().max()) / top if n in ("net.0.bias", "net.3.bias") else _err(grads[n], grads64[n])
    print("Encoder3D training, volume with requires_grad: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["volume"] < 1e-4, e["volume"]
    assert e["net.0.weight"] < 1e-4 and e["net.3.weight"] < 1e-4
    assert e["net.0.bias"] < 1e-3 and e["net.3.bias"] < 1e-3
    for n in ("net.1.weight", "net.1.bias", "net.4.weight", "net.4.bias"):
        assert e[n] < 1e-3, (n, e[n])


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------
def test_adversarial_test_on_volumes_runs_without_pytorch_convolutions():
    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet3D
    torch.manual_seed(0)
    # test_hip_input_grad.py's model: the default 64 output channels, so that the closing no_grad forwards run the fused eval head as well
    model = SmokePhysNet3D(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()
    assert model.input_grad == "hip"
    wanted = [p.requires_grad for p in model.parameters()]       # (the frozen 2-D input_encoder stays frozen)
    x = torch.rand(2, 1, 4, 32, 32, device="cuda")
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
    assert [p.requires_grad for p in model.parameters()] == wanted


def test_adversarial_test_on_frames_is_unchanged():
    """A 4-D call with target=None: the same seed gives the numbers of the reference's lines (perturbation_tests.py:54-98, with the gradient
    taken as the module docstring says), inlined here."""
    from smokephysai_amd.evaluation import PerturbationTester
    model = _small_model()
    x = torch.rand(2, 1, 128, 128, device="cuda")
    eps, steps = 0.1, 2

    torch.manual_seed(21)
    delta = torch.zeros_like(x, requires_grad=True)
    for _ in range(steps):
        output = model(torch.clamp(x + delta, 0, 1))
        loss = -F.mse_loss(output["reconstructed"], x)
        (grad,) = torch.autograd.grad(loss, delta)
        with torch.no_grad():
            delta += eps / steps * torch.sign(grad)
            delta.clamp_(-eps, eps)
    with torch.no_grad():
        base, adv = model(x), model(torch.clamp(x + delta, 0, 1))
        want = {"adversarial_feature_stability": F.cosine_similarity(base["latent_features"], adv["latent_features"], dim=1).mean().item(),
                "adversarial_perturbation_norm": torch.norm(delta.detach()).item()}

    torch.manual_seed(21)
    got = PerturbationTester().adversarial_test(model, x, epsilon=eps, num_steps=steps)
    assert got == want, (got, want)
    torch.manual_seed(21)
    assert PerturbationTester().adversarial_test(model, x, epsilon=eps, num_steps=steps, target=x) == want


def test_noise_and_quality_evaluations_take_volumes():
    from smokephysai_amd.evaluation import PerturbationTester, RobustnessEvaluator
    model = _small_model()
    x = torch.rand(2, 1, 4, 32, 32, device="cuda")
    res = PerturbationTester().gaussian_noise_test(model, x, noise_levels=[0.05, 0.1])
    assert set(res) == {"gaussian_0.05", "gaussian_0.1"}
    assert all(np.isfinite(v) for r in res.values() for v in r.values())
    q = RobustnessEvaluator().evaluate_reconstruction_quality(model, x, _rendered(x, (128, 128)))
    assert set(q) == {"ssim", "psnr", "mse"} and all(np.isfinite(v) for v in q.values())
