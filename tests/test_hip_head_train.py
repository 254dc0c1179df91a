"""GPU tests of the training route of the reconstruction head on libsmokehip (models/decoder_train.py, csrc/decoder_train.hip):
each convolution against float64 torch on the CPU, the whole head against the fp32 modules and fp64, the full training loss inside
PyTorch's own fp32 band, bit-reproducibility (no atomics), a training step with no MIOpen convolution or BatchNorm, and a short
training run that tracks the module route."""
import copy
import hashlib

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

from smokephysai_amd import _lib                                                          # noqa: E402
from smokephysai_amd.models import SmokePhysNet                                          # noqa: E402
from smokephysai_amd.models import smokephys_net                                         # noqa: E402
from smokephysai_amd.models.decoder_train import (hip_conv3_sigmoid_train, hip_convt4s2_train, hip_head_train,  # noqa: E402
                                                  hip_head_train_supported)

BATCHES = (1, 3, 8, 64)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _seeded(*shape, gen):
    return torch.randn(*shape, generator=gen)


# ---------------------------------------------------------------- each convolution alone, against float64 on the CPU
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("C0", (64, 16))
def test_first_convt_token_major_both_ends(B, C0):
    gen = torch.Generator().manual_seed(10 * B + C0)
    conv = nn.ConvTranspose2d(C0, 32, 4, stride=2, padding=1)
    tok, dz = _seeded(B, 1024, C0, gen=gen), _seeded(B, 32, 64, 64, gen=gen)
    c64, t64 = copy.deepcopy(conv).double(), tok.double().requires_grad_()
    z64 = c64(t64.transpose(1, 2).reshape(B, C0, 32, 32))
    z64.backward(dz.double())
    cg, tg = copy.deepcopy(conv).cuda(), tok.cuda().requires_grad_()
    z = hip_convt4s2_train(tg, cg, tokens=True)
    z.backward(dz.cuda())
    assert z.shape == (B, 32, 64, 64) and tg.grad.shape == (B, 1024, C0)
    assert _rel(z, z64) < 1e-5
    assert _rel(tg.grad, t64.grad) < 1e-5                       # the data gradient, written token-major
    assert _rel(cg.weight.grad, c64.weight.grad) < 5e-5
    assert _rel(cg.bias.grad, c64.bias.grad) < 5e-5


@pytest.mark.parametrize("B", BATCHES)
def test_second_convt(B):
    gen = torch.Generator().manual_seed(B)
    conv = nn.ConvTranspose2d(32, 16, 4, stride=2, padding=1)
    x, dz = _seeded(B, 32, 64, 64, gen=gen), _seeded(B, 16, 128, 128, gen=gen)
    c64, x64 = copy.deepcopy(conv).double(), x.double().requires_grad_()
    z64 = c64(x64)
    z64.backward(dz.double())
    cg, xg = copy.deepcopy(conv).cuda(), x.cuda().requires_grad_()
    z = hip_convt4s2_train(xg, cg)
    z.backward(dz.cuda())
    assert _rel(z, z64) < 1e-5 and _rel(xg.grad, x64.grad) < 1e-5
    assert _rel(cg.weight.grad, c64.weight.grad) < 5e-5 and _rel(cg.bias.grad, c64.bias.grad) < 5e-5


@pytest.mark.parametrize("B", BATCHES)
def test_conv3_sigmoid(B):
    gen = torch.Generator().manual_seed(100 + B)
    conv = nn.Conv2d(16, 1, 3, padding=1)
    x, dy = _seeded(B, 16, 128, 128, gen=gen).abs(), _seeded(B, 1, 128, 128, gen=gen)
    c64, x64 = copy.deepcopy(conv).double(), x.double().requires_grad_()
    y64 = torch.sigmoid(c64(x64))
    y64.backward(dy.double())
    cg, xg = copy.deepcopy(conv).cuda(), x.cuda().requires_grad_()
    y = hip_conv3_sigmoid_train(xg, cg)
    y.backward(dy.cuda())
    assert _rel(y, y64) < 1e-5 and _rel(xg.grad, x64.grad) < 1e-5
    assert _rel(cg.weight.grad, c64.weight.grad) < 5e-5 and _rel(cg.bias.grad, c64.bias.grad) < 5e-5


# ---------------------------------------------------------------- the whole head in train mode
@pytest.mark.parametrize("B", BATCHES)
def test_whole_head_against_modules_and_fp64(B):
    """hip_head_train against the fp32 modules and float64.  A train-mode BatchNorm + ReLU amplifies forward rounding: an activation
    within ~1e-7 of zero can fall on the other side of the ReLU in fp32 and fp64 (at batch 64 the head has 12.6 M of them), and one such
    flip moves a weight gradient by ~1e-3 of its max-norm.  So the float64 reference for the gradients takes the ReLU masks of the HIP
    forward; with equal masks what is left is the kernels' own rounding."""
    from smokephysai_amd.models.decoder_train import _bn_relu
    torch.manual_seed(7)
    head = SmokePhysNet().reconstruction_head.train()
    gen = torch.Generator().manual_seed(B)
    tok, r = _seeded(B, 1024, 64, gen=gen), _seeded(B, 1, 128, 128, gen=gen)

    h64, hf, hh = copy.deepcopy(head).double(), copy.deepcopy(head).cuda(), copy.deepcopy(head).cuda()
    assert hip_head_train_supported(hh, tok.cuda()) and not hip_head_train_supported(h64, tok.double())
    with torch.no_grad():                                       # the HIP forward's ReLU masks (bit-reproducible), on a copy
        hm = copy.deepcopy(hh)
        a1 = _bn_relu(hip_convt4s2_train(tok.cuda(), hm[0], tokens=True), hm[1])
        m1 = (a1 > 0).double().cpu()
        m2 = (_bn_relu(hip_convt4s2_train(a1, hm[3]), hm[4]) > 0).double().cpu()

    def run(h, t, route):
        t = t.clone().requires_grad_()
        img = t.transpose(1, 2).reshape(t.shape[0], 64, 32, 32)
        if route == "hip":
            y = hip_head_train(h, t)
        elif route == "modules":
            y = h(img)
        else:                                                   # float64 with the HIP masks in place of the ReLUs
            y = h[7](h[6](h[4](h[3](h[1](h[0](img)) * m1)) * m2))
        (y * r.to(y)).sum().backward()
        return y, t.grad, {k: p.grad for k, p in h.named_parameters()}

    y64, _, _ = run(copy.deepcopy(h64), tok.double(), "modules")
    ym, tm, gm = run(h64, tok.double(), "masked")
    yf, _, gf = run(hf, tok.cuda(), "modules")
    yh, th, gh = run(hh, tok.cuda(), "hip")
    assert _rel(yh, y64) < 1e-5 and _rel(yh, yf) < 1e-5 and _rel(yh, ym) < 1e-5
    scale = max(float(v.abs().max()) for v in gm.values())
    for k in gm:
        if k in ("0.bias", "3.bias"):                           # conv biases in front of a BatchNorm: exact gradient 0
            assert float(gh[k].abs().max()) <= max(10 * float(gf[k].abs().max()), 1e-5 * scale), k
            continue
        assert _rel(gh[k], gm[k]) < 1e-4, (k, _rel(gh[k], gm[k]), _rel(gf[k], gm[k]))
    assert _rel(th, tm) < 1e-4
    for i in (1, 4):
        for name in ("running_mean", "running_var"):
            assert _rel(getattr(hh[i], name), getattr(h64[i], name)) < 1e-5, (i, name)
            assert _rel(getattr(hh[i], name), getattr(hf[i], name)) < 1e-5, (i, name)
        assert int(hh[i].num_batches_tracked) == int(hf[i].num_batches_tracked) == int(h64[i].num_batches_tracked) == 1


def _grads(mod, loss_fn):
    mod.zero_grad()
    loss_fn(mod).backward()
    return {k: p.grad.detach().double().cpu() for k, p in mod.named_parameters() if p.grad is not None}


def test_full_loss_gradients_stay_in_the_fp32_band(golden, monkeypatch):
    """train.batch_losses on the fixture batch, as test_training_gradients_with_hip_linears (2): with the head on libsmokehip every
    live gradient stays inside the band PyTorch's own fp32 run keeps around fp64."""
    import train
    g = golden("train_batch.npz")
    model = SmokePhysNet(input_dim=32, hidden_dim=64, num_layers=2, num_heads=4, output_channels=16)
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w::")})
    model = model.cuda().train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    m64 = copy.deepcopy(model).double()
    gen = torch.Generator().manual_seed(5)
    noise = torch.randn(2, 3, 2, 1, generator=gen).cuda()
    batch = {"input": torch.from_numpy(g["inputs"]), "target": torch.from_numpy(g["targets"]),
             "chaos_features": torch.from_numpy(g["chaos_targets"]), "sequence": torch.zeros(2, 20, 128, 128)}
    b64 = {k: v.double() for k, v in batch.items()}
    calls = []
    real = smokephys_net.hip_head_train
    monkeypatch.setattr(smokephys_net, "hip_head_train", lambda h, t: calls.append(t.shape) or real(h, t))

    def full_loss(b, nz):
        return lambda mod: train.batch_losses(mod, mod.physics_regularizer, b, "cuda", chaos_noise=nz)[0]
    m64.head_train = "hip"                                       # float64: falls back to the modules
    ref = _grads(m64, full_loss(b64, noise.double()))
    assert not calls
    model.head_train = "hip"
    got = _grads(model, full_loss(batch, noise))
    assert calls == [(2, 1024, 16)]
    model.head_train = "torch"
    f32 = _grads(model, full_loss(batch, noise))
    assert len(calls) == 1
    scale = max(float(v.abs().max()) for v in ref.values())
    live = [k for k, v in ref.items() if float(v.abs().max()) > 1e-9 * scale]
    worst_f32 = max(_max_rel(f32[k], ref[k]) for k in live)
    worst_hip = max(_max_rel(got[k], ref[k]) for k in live)
    assert 1e-4 < worst_f32 < 5e-2
    assert worst_hip < max(2.0 * worst_f32, 1e-2), (worst_hip, worst_f32)


def _max_rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------- determinism, and no stale memory read
def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.mark.parametrize("B", (3, 64))
def test_repeated_calls_are_bit_identical_and_overwrite_nan(B):
    L = _lib.load()
    st = _lib.stream_ptr(torch.device("cuda"))
    gen = torch.Generator().manual_seed(B)
    tok = _seeded(B, 1024, 64, gen=gen).cuda()
    w1, b1 = _seeded(64, 32, 4, 4, gen=gen).cuda(), _seeded(32, gen=gen).cuda()
    x2, w2 = _seeded(B, 32, 64, 64, gen=gen).cuda(), _seeded(32, 16, 4, 4, gen=gen).cuda()
    dz1, dz2 = _seeded(B, 32, 64, 64, gen=gen).cuda(), _seeded(B, 16, 128, 128, gen=gen).cuda()
    x3, w3, b3 = _seeded(B, 16, 128, 128, gen=gen).cuda(), _seeded(16, 3, 3, gen=gen).cuda(), _seeded(1, gen=gen).cuda()
    dy = _seeded(B, 1, 128, 128, gen=gen).cuda()

    def once():
        out = {}
        z = _nan(B, 32, 64, 64)
        _lib.check(L.smk_convt4s2_train_forward(tok.data_ptr(), w1.data_ptr(), b1.data_ptr(), B, 64, 32, 32, 32, 1, z.data_ptr(), st))
        dx = _nan(B, 1024, 64)
        _lib.check(L.smk_convt4s2_train_dgrad(dz1.data_ptr(), w1.data_ptr(), B, 64, 32, 32, 32, 1, dx.data_ptr(), st))
        dw, db = _nan(64, 32, 4, 4), _nan(32)
        ws = _nan(L.smk_convt4s2_train_wgrad_workspace(B, 64, 32, 32, 32) // 4)
        _lib.check(L.smk_convt4s2_train_wgrad(dz1.data_ptr(), tok.data_ptr(), B, 64, 32, 32, 32, 1, dw.data_ptr(), db.data_ptr(),
                                              ws.data_ptr(), st))
        out.update(z1=z, dx1=dx, dw1=dw, db1=db)
        z = _nan(B, 16, 128, 128)
        _lib.check(L.smk_convt4s2_train_forward(x2.data_ptr(), w2.data_ptr(), b1.data_ptr(), B, 32, 16, 64, 64, 0, z.data_ptr(), st))
        dx = _nan(B, 32, 64, 64)
        _lib.check(L.smk_convt4s2_train_dgrad(dz2.data_ptr(), w2.data_ptr(), B, 32, 16, 64, 64, 0, dx.data_ptr(), st))
        dw, db = _nan(32, 16, 4, 4), _nan(16)
        ws = _nan(L.smk_convt4s2_train_wgrad_workspace(B, 32, 16, 64, 64) // 4)
        _lib.check(L.smk_convt4s2_train_wgrad(dz2.data_ptr(), x2.data_ptr(), B, 32, 16, 64, 64, 0, dw.data_ptr(), db.data_ptr(),
                                              ws.data_ptr(), st))
        out.update(z2=z, dx2=dx, dw2=dw, db2=db)
        y = _nan(B, 1, 128, 128)
        _lib.check(L.smk_conv3_sigmoid_train_forward(x3.data_ptr(), w3.data_ptr(), b3.data_ptr(), B, 128, 128, y.data_ptr(), st))
        dx, dw, db = _nan(B, 16, 128, 128), _nan(16, 3, 3), _nan(1)
        ws = _nan(L.smk_conv3_sigmoid_train_workspace(B, 128, 128) // 4)
        _lib.check(L.smk_conv3_sigmoid_train_backward(dy.data_ptr(), y.data_ptr(), x3.data_ptr(), w3.data_ptr(), B, 128, 128, dx.data_ptr(),
                                                      dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st))
        out.update(y3=y, dx3=dx, dw3=dw, db3=db)
        torch.cuda.synchronize()
        return out
    a, b = once(), once()
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- training steps
def _step_batches(B=8, N=128):
    gen = torch.Generator().manual_seed(11)
    batches = []
    for _ in range(2):
        x = torch.rand(B, 1, N, N, generator=gen)
        batches.append({"input": x, "target": torch.rand(B, 1, N, N, generator=gen), "chaos_features": torch.rand(B, 3, generator=gen),
                        "sequence": torch.rand(B, 20, N, N, generator=gen)})
    return batches


class _Null:
    def add_scalar(self, *a, **k):
        pass


def _two_steps(batches):
    import train
    from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
    torch.manual_seed(1234)
    model = SmokePhysNet(head_train="hip").cuda()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    torch.manual_seed(99)
    train.train_epoch(model, batches, opt, PhysicsRegularizer(), torch.device("cuda"), 0, _Null())
    torch.cuda.synchronize()
    hp, hg = hashlib.sha256(), hashlib.sha256()
    for p in model.parameters():
        hp.update(p.detach().cpu().numpy().tobytes())
        hg.update(p.grad.detach().cpu().numpy().tobytes())
    return hp.hexdigest(), hg.hexdigest(), model


def test_train_steps_are_bit_reproducible_without_miopen(monkeypatch):
    """Two train_epoch steps of the default model at 8 x 128^2 with head_train="hip", with MIOpen left non-deterministic: twice from
    the same seed, every parameter and gradient bit-identical; and a profiled step runs no convolution or BatchNorm op of PyTorch."""
    import train
    from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    batches = _step_batches()
    p1, g1, model = _two_steps(batches)
    p2, g2, _ = _two_steps(batches)
    assert p1 == p2 and g1 == g2
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        train.train_epoch(model, batches[:1], opt, PhysicsRegularizer(), torch.device("cuda"), 0, _Null())
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    bad = sorted(n for n in names if n.startswith(("aten::convolution", "aten::miopen", "aten::_convolution", "aten::cudnn"))
                 or (n.startswith("aten::") and "batch_norm" in n))
    assert not bad, bad
    assert any("AdamW" in n or "aten::_foreach" in n or "aten::add" in n for n in names)       # the profile did record the step


def test_short_training_run_tracks_the_module_head():
    """Five AdamW steps with head_train="hip" against "torch" from the same seed (test_short_training_run_tracks_the_all_pytorch_path)."""
    import train

    def run(route):
        torch.manual_seed(3)
        model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, output_channels=16, head_train=route).cuda().train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        g = torch.Generator().manual_seed(4)
        x = torch.rand(4, 1, 64, 64, generator=g)
        batch = {"input": x, "target": torch.nn.functional.interpolate(x, size=128, mode="bilinear"),
                 "chaos_features": torch.rand(4, 3, generator=g), "sequence": torch.rand(4, 20, 64, 64, generator=g)}
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
    assert hip[-1] < hip[0] and ref[-1] < ref[0]
    for a, b in zip(hip[:3], ref[:3]):
        assert abs(a - b) <= 1e-2 * abs(b), (hip, ref)
