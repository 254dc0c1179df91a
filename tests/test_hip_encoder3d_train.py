"""Encoder3D and SmokePhysNet3D in training (SPEC_3D.md section 11): the module's hip route against a float64 copy on its torch route, the
eval mirror after an optimizer step, gradients through the whole model, and a short training run against the torch route."""
import copy

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _err(a, b):
    return rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _encoder(seed=7):
    from smokephysai_amd.models import Encoder3D
    torch.manual_seed(seed)
    enc = Encoder3D(route="hip").cuda().train()
    with torch.no_grad():                                     # away from the identity: a BatchNorm that scales and shifts
        for bn in (enc.net[1], enc.net[4]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    return enc


@pytest.mark.parametrize("shape", [(4, 32, 32), (3, 64, 32)], ids=lambda s: "x".join(map(str, s)))
def test_encoder3d_parameter_gradients_match_fp64(shape):
    """Tokens 1e-5, weight gradients 1e-4, dgamma / dbeta 1e-3, running statistics 1e-5 under the loss (tokens * r).sum().  The two convolution
    biases sit in front of a BatchNorm: their exact gradient is 0, checked as < 1e-3 of the largest gradient."""
    enc = _encoder()
    ref = copy.deepcopy(enc).double()
    ref.route = "torch"
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    x = torch.rand(2, 1, *shape, device="cuda", generator=g)
    r = torch.randn(2, 1024, 128, device="cuda", generator=g)
    tok = enc.tokens(x)
    assert "HipBn3dCl" in type(tok.grad_fn).__name__ and tok.shape == (2, 1024, 128)
    (tok * r).sum().backward()
    tok64 = ref.tokens(x.double())
    (tok64 * r.double()).sum().backward()
    grads = {n: p.grad for n, p in enc.named_parameters()}
    grads64 = {n: p.grad for n, p in ref.named_parameters()}
    top = max(float(v.abs().max()) for v in grads64.values())
    e = {"tokens": _err(tok, tok64)}
    for n in grads:
        if n in ("net.0.bias", "net.3.bias"):
            e[n] = float(grads[n].abs().max()) / top
        else:
            e[n] = _err(grads[n], grads64[n])
    for n in ("net.1.running_mean", "net.1.running_var", "net.4.running_mean", "net.4.running_var"):
        e[n] = _err(enc.state_dict()[n], ref.state_dict()[n])
    print(f"Encoder3D {shape}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["tokens"] < 1e-5
    assert e["net.0.weight"] < 1e-4 and e["net.3.weight"] < 1e-4
    assert e["net.0.bias"] < 1e-3 and e["net.3.bias"] < 1e-3
    for n in ("net.1.weight", "net.1.bias", "net.4.weight", "net.4.bias"):
        assert e[n] < 1e-3, (n, e[n])
    for n in ("net.1.running_mean", "net.1.running_var", "net.4.running_mean", "net.4.running_var"):
        assert e[n] < 1e-5, (n, e[n])
    assert int(enc.net[1].num_batches_tracked) == int(enc.net[4].num_batches_tracked) == 1


def test_eval_mirror_follows_an_optimizer_step():
    """eval() under no_grad runs the folded HipEncoder3D; after an optimizer step it is rebuilt from the new weights and running statistics."""
    from smokephysai_amd.models import HipEncoder3D
    enc = _encoder(8)
    opt = torch.optim.Adam(enc.parameters(), lr=0.01)                  # every weight moves by about 0.01, whatever the gradient's scale
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(2, 1, 4, 32, 32, device="cuda", generator=g)
    enc.eval()
    with torch.no_grad():
        before = enc.tokens(x)
    first = enc.hip_eval_encoder()
    assert isinstance(first, HipEncoder3D) and enc.hip_eval_encoder() is first
    enc.train()
    enc.tokens(x).square().sum().backward()
    opt.step()
    enc.eval()
    with torch.no_grad():
        after = enc.tokens(x)
        assert enc.hip_eval_encoder() is not first
        ref = copy.deepcopy(enc)
        ref.route = "torch"
        want = ref.tokens(x)
    assert _err(after, want) < 1e-4 and _err(before, want) > 1e-3


def _small_model(route):
    from smokephysai_amd.models import SmokePhysNet3D
    torch.manual_seed(3)
    return SmokePhysNet3D(input_dim=32, hidden_dim=64, num_layers=2, num_heads=4, output_channels=16, volume_encoder=route).cuda().train()


def test_smokephysnet3d_trains_its_3d_encoder():
    """forward on volumes with gradients: every encoder3d parameter but the two convolution biases gets a non-zero gradient, the frozen 2-D
    input_encoder none."""
    model = _small_model("hip")
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand(2, 1, 4, 32, 32, device="cuda", generator=g)
    noise = torch.randn(2, 3, 2, 1, device="cuda", generator=g)
    out = model(x, chaos_noise=noise)
    assert out["reconstructed"].shape == (2, 1, 128, 128)
    (out["reconstructed"].square().mean() + out["physics_features"].square().mean()).backward()
    for n, p in model.encoder3d.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        if n not in ("net.0.bias", "net.3.bias"):
            assert float(p.grad.abs().max()) > 0, n
    assert all(p.grad is None for p in model.input_encoder.parameters())


def test_short_volume_training_run_tracks_the_torch_route():
    """Five AdamW steps of train.batch_losses on a fixed batch in VolumeFrameDataset's item schema: the hip route's losses follow the torch
    route's within the band of test_short_training_run_tracks_the_all_pytorch_path (first three steps within 1e-2), and the loss falls."""
    import train

    def run(route):
        model = _small_model(route)
        opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01)
        g = torch.Generator().manual_seed(4)
        batch = {"input": torch.rand(2, 1, 4, 32, 32, generator=g), "target": torch.rand(2, 1, 32, 32, generator=g),
                 "chaos_features": torch.rand(2, 3, generator=g), "sequence": torch.rand(2, 20, 32, 32, generator=g)}
        torch.manual_seed(5)                                  # the same dropout masks and chaos draws on both routes
        losses = []
        for _ in range(5):
            opt.zero_grad()
            total, *_ = train.batch_losses(model, model.physics_regularizer, batch, "cuda")
            total.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            losses.append(float(total.detach()))
        return losses
    hip, ref = run("hip"), run("torch")
    print("volume training, hip route:", hip, "torch route:", ref)
    assert hip[-1] < hip[0] and ref[-1] < ref[0]
    for a, b in zip(hip[:3], ref[:3]):
        assert abs(a - b) <= 1e-2 * abs(b), (hip, ref)
