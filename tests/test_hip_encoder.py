"""GPU parity of the fused HIP encoder (conv7x7+BN+ReLU -> conv3x3+BN+ReLU -> block-mean pool) against the
reference's captured features (tests/golden/encoder_io_*.npz) and the fp64-accumulating oracle.
Tolerance: 1e-4 relative (max-norm), the bar BASELINE.json states for CNN features."""
import numpy as np
import copy

import pytest
import torch

import oracle
from conftest import rel_err

pytestmark = pytest.mark.gpu

from smokephysai_amd.models.encoder import HipEncoder     # noqa: E402

TOL = 1e-4


@pytest.fixture(scope="module")
def enc(golden):
    return HipEncoder({k: torch.from_numpy(v) for k, v in golden("encoder_weights.npz").items()})


@pytest.mark.parametrize("N", [64, 128, 256])
def test_features_vs_reference(golden, enc, N):
    g = golden(f"encoder_io_{N}.npz")
    x = torch.from_numpy(g["frames"]).cuda()
    feats = enc(x[:, None], input_dim=128, dtype="f32").cpu().numpy()
    assert feats.shape == g["features"].shape
    for b in range(feats.shape[0]):
        assert rel_err(feats[b], g["features"][b]) < TOL, f"frame {b}"
    assert rel_err(feats, g["features"]) < 2e-5          # fp32 MFMA path is far inside the bar


@pytest.mark.parametrize("N", [64, 128, 256])
def test_features_bf16x3_within_1e4(golden, enc, N):
    """Split-bf16 MFMA path (hi*hi + hi*lo + lo*hi): still inside the 1e-4 bar vs the reference's fp32 features."""
    g = golden(f"encoder_io_{N}.npz")
    x = torch.from_numpy(g["frames"]).cuda()
    feats = enc(x[:, None], input_dim=128, dtype="bf16x3").cpu().numpy()
    for b in range(feats.shape[0]):
        assert rel_err(feats[b], g["features"][b]) < TOL, f"frame {b}"


@pytest.mark.parametrize("N", [64, 128, 256])
def test_features_i8x3_fixed_point_within_1e4(golden, enc, N):
    """int8 two-limb fixed point (per-tile activation scale, per-channel weight scale, exact i32 accumulation):
    inside the 1e-4 bar on every reference fixture (numpy emulation predicts 2e-5 .. 7e-5), opt-in."""
    g = golden(f"encoder_io_{N}.npz")
    x = torch.from_numpy(g["frames"]).cuda()
    feats = enc(x[:, None], input_dim=128, dtype="i8x3").cpu().numpy()
    errs = [rel_err(feats[b], g["features"][b]) for b in range(feats.shape[0])]
    print(f"i8x3 rel err at {N}: {errs}")
    assert max(errs) < 0.5 * TOL, errs           # measured 1e-5 .. 3e-5
    tok = enc.tokens(x, input_dim=128, dtype="i8x3")
    assert torch.equal(tok, torch.from_numpy(feats).cuda().flatten(2).transpose(1, 2))


@pytest.mark.parametrize("N", [64, 256])
def test_features_bf16_single_pass(golden, enc, N):
    """Single-pass bf16 MFMA: operands rounded to 8 significant bits, so the bar is bf16-class (2e-2), not 1e-4;
    this mode is opt-in and never used for the parity claims."""
    g = golden(f"encoder_io_{N}.npz")
    x = torch.from_numpy(g["frames"]).cuda()
    feats = enc(x[:, None], input_dim=128, dtype="bf16").cpu().numpy()
    assert rel_err(feats, g["features"]) < 2e-2


@pytest.mark.parametrize("dtype", ["bf16x3", "bf16"])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_token_major_output_is_the_same_data(golden, enc, dtype, N):
    """smk_encoder_forward_tokens writes [B,1024,128] = features.flatten(2).transpose(1,2) (smokephys_net.py:95), bitwise."""
    x = torch.from_numpy(golden(f"encoder_io_{N}.npz")["frames"]).cuda()
    nchw = enc(x, input_dim=128, dtype=dtype)
    tok = enc.tokens(x, input_dim=128, dtype=dtype)
    assert tok.shape == (x.shape[0], 1024, 128)
    assert torch.equal(tok, nchw.flatten(2).transpose(1, 2))


def test_conv1_activations(golden, enc):
    g = golden("encoder_io_64.npz")
    act = enc.conv1_activations(torch.from_numpy(g["frames"][:1]).cuda()).cpu().numpy()
    assert rel_err(act, g["conv1_act"]) < 1e-5


def test_vs_oracle_random_weights_and_batch():
    """Fresh random weights/BN stats and a batch of 3 random 64^2 frames vs the fp64 oracle."""
    rng = np.random.RandomState(0)
    w = dict(conv1_w=rng.randn(64, 1, 7, 7) * 0.2, conv1_b=rng.randn(64) * 0.1, bn1_w=rng.rand(64) + 0.5,
             bn1_b=rng.randn(64) * 0.1, bn1_mean=rng.randn(64) * 0.2, bn1_var=rng.rand(64) + 0.3,
             conv2_w=rng.randn(128, 64, 3, 3) * 0.05, conv2_b=rng.randn(128) * 0.1, bn2_w=rng.rand(128) + 0.5,
             bn2_b=rng.randn(128) * 0.1, bn2_mean=rng.randn(128) * 0.2, bn2_var=rng.rand(128) + 0.3)
    w = {k: v.astype(np.float32) for k, v in w.items()}
    frames = (rng.rand(3, 64, 64) * 1.8).astype(np.float32)
    ref = oracle.encoder_features(frames, w, input_dim=128)
    e = HipEncoder({k: torch.from_numpy(v) for k, v in w.items()})
    got = e(torch.from_numpy(frames).cuda(), input_dim=128).cpu().numpy()
    assert rel_err(got, ref) < 2e-5
    got3 = e(torch.from_numpy(frames).cuda(), input_dim=128, dtype="bf16x3").cpu().numpy()
    assert rel_err(got3, ref) < TOL
    goti = e(torch.from_numpy(frames).cuda(), input_dim=128, dtype="i8x3").cpu().numpy()
    print("i8x3 vs oracle, random weights:", [rel_err(goti[b], ref[b]) for b in range(3)])
    assert max(rel_err(goti[b], ref[b]) for b in range(3)) < TOL
    # input_dim=32 (small-model config): 64 -> 32 -> 32 composes to the same 2x2 block mean
    ref32 = oracle.encoder_features(frames[:1], w, input_dim=32)
    assert rel_err(e(torch.from_numpy(frames[:1]).cuda(), input_dim=32).cpu().numpy(), ref32) < 2e-5


def test_unsupported_shapes_fail_loudly(enc):
    from smokephysai_amd._lib import SmokeHipError
    with pytest.raises(SmokeHipError):
        enc(torch.zeros(1, 1, 96, 96, device="cuda"))
    with pytest.raises(SmokeHipError):
        enc(torch.zeros(1, 1, 64, 64, device="cuda"), input_dim=48)


def test_bf16x3_on_the_32x32x16_shape_still_matches(tmp_path):
    """SMK_ENC_SHAPE=32 selects k_encoder_bf16<true> (the 32x32x16 MFMA form kept for A/B against the default 16x16x32
    kernel).  The switch is read once per process, so this runs in a child process: same fixtures, same 1e-4 bar, both output
    layouts, and the two kernels agree with each other to 1e-5."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, "tests")
from conftest import rel_err
from smokephysai_amd.models.encoder import HipEncoder
w = {k: torch.from_numpy(v) for k, v in np.load("tests/golden/encoder_weights.npz").items()}
enc = HipEncoder(w)
for N in (64, 128, 256):
    g = np.load(f"tests/golden/encoder_io_{N}.npz")
    x = torch.from_numpy(g["frames"]).cuda()
    f = enc(x[:, None], input_dim=128, dtype="bf16x3")
    t = enc.tokens(x[:, None], input_dim=128, dtype="bf16x3")
    assert rel_err(f.cpu().numpy(), g["features"]) < 1e-4, N
    assert torch.equal(t, f.flatten(2).transpose(1, 2)), N
    np.save(f"{sys.argv[1]}/smk_feat32_{N}.npy", f.cpu().numpy())
print("ok32")
'''
    env = dict(os.environ, SMK_ENC_SHAPE="32")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok32" in out.stdout, out.stderr[-2000:]
    w = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(root, "tests/golden/encoder_weights.npz")).items()}
    enc16 = HipEncoder(w)
    for N in (64, 128, 256):
        g = np.load(os.path.join(root, f"tests/golden/encoder_io_{N}.npz"))
        f16 = enc16(torch.from_numpy(g["frames"]).cuda()[:, None], input_dim=128, dtype="bf16x3").cpu().numpy()
        assert rel_err(f16, np.load(tmp_path / f"smk_feat32_{N}.npy")) < 1e-5, N


# ---------------------------------------------------------------- training: BatchNorm (batch statistics) + ReLU + pool on libsmokehip
@pytest.mark.parametrize("B,C,H,pool", [(3, 64, 128, 1), (2, 128, 128, 4), (2, 128, 256, 8), (5, 16, 64, 1)])
def test_bn_relu_pool_training_kernels_match_fp64_autograd(B, C, H, pool):
    """smk_bn_relu_pool_forward / _backward against nn.BatchNorm2d(train) -> ReLU -> avg_pool2d in fp64: output, dz, dgamma, dbeta
    and the running-statistics update; deterministic."""
    from smokephysai_amd.models.norm import hip_bn_relu_pool
    torch.manual_seed(B * C + H + pool)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    ref_bn = torch.nn.BatchNorm2d(C).cuda().double().train()
    ref_bn.load_state_dict({k: v.double() if v.is_floating_point() else v.clone() for k, v in bn.state_dict().items()})
    z = (torch.randn(B, C, H, H, device="cuda") * 2.0 + 3.0 * torch.randn(1, C, 1, 1, device="cuda")).requires_grad_(True)
    dout = torch.randn(B, C, H // pool, H // pool, device="cuda")
    out = hip_bn_relu_pool(z, bn, pool)
    out.backward(dout)
    z64 = z.detach().double().requires_grad_(True)
    pre64 = ref_bn(z64)
    y64 = torch.relu(pre64)
    ref = y64 if pool == 1 else torch.nn.functional.avg_pool2d(y64, pool)
    ref.backward(dout.double())

    def err(a, b):
        return rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    # ReLU is discontinuous in its derivative: an activation within rounding of 0 (about one of the 1.7e7 elements here) takes the
    # other branch in fp32 than in fp64 -- as it does in PyTorch's own fp32 kernels; those elements are excluded from the dz check
    sure = (pre64.detach().abs() > 1e-5)
    assert float((~sure).sum()) < 1e-4 * sure.numel()
    assert err(out, ref) < 1e-5 and err(z.grad * sure, z64.grad * sure) < 1e-4
    # (the same flipped element enters the channel sums with a weight of |dout| / pool^2: up to a few 1e-4 of the largest dbeta)
    assert err(bn.weight.grad, ref_bn.weight.grad) < 1e-3 and err(bn.bias.grad, ref_bn.bias.grad) < 1e-3
    assert err(bn.running_mean, ref_bn.running_mean) < 1e-5 and err(bn.running_var, ref_bn.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == 1
    g1 = z.grad.clone()
    z.grad = None
    bn.zero_grad()
    hip_bn_relu_pool(z, bn, pool).backward(dout)
    assert torch.equal(z.grad, g1)


def test_training_encoder_path_on_hip_norm_blocks_matches_the_pytorch_path():
    """SmokePhysNet.encode_frames in train mode at 128^2: conv1 (MIOpen) + libsmokehip BatchNorm/ReLU/pool + conv2 forward / data
    gradient on libsmokehip against the all-PyTorch module path (linear_dtype='f32' disables the HIP route): features, input-encoder
    gradients (both against fp64), running statistics."""
    import copy
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(2)
    hip = SmokePhysNet(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4).cuda().train()
    ref = copy.deepcopy(hip)
    ref.linear_dtype = "f32"
    x = torch.rand(3, 1, 128, 128, device="cuda")
    g = torch.randn(3, 128, 32, 32, device="cuda")
    fh = hip.encode_frames(x)
    fr = ref.encode_frames(x)
    assert "HipBnReluPool" in type(fh.grad_fn).__name__ and "HipBnReluPool" not in type(fr.grad_fn).__name__
    fh.backward(g)
    fr.backward(g)

    def err(a, b):
        return rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    assert err(fh, fr) < 1e-5
    # gradients: this loss is ill-conditioned in fp32 (ReLU masks and batch statistics downstream of two convolutions: PyTorch-ROCm's own
    # fp32 path sits 1e-3 .. 1e-2 from fp64), so both fp32 routes are measured against the fp64 module path, not against each other
    r64 = copy.deepcopy(ref).double()
    r64.encode_frames(x.double()).backward(g.double())
    scale = max(float(q.grad.abs().max()) for q in r64.input_encoder.parameters())
    for (n, p), (_, q), (_, q64) in zip(hip.input_encoder.named_parameters(), ref.input_encoder.named_parameters(),
                                        r64.input_encoder.named_parameters()):
        if float(q64.grad.abs().max()) > 1e-3 * scale:
            e_hip, e_ref = err(p.grad.double(), q64.grad), err(q.grad.double(), q64.grad)
            assert e_hip < max(3.0 * e_ref, 5e-3), (n, e_hip, e_ref)
        else:                                                               # conv biases in front of a BatchNorm: gradient 0 (rounding noise)
            assert float(p.grad.abs().max()) < 1e-3 * scale, n
    for k in ("1.running_mean", "1.running_var", "4.running_mean", "4.running_var"):
        assert err(hip.input_encoder.state_dict()[k], ref.input_encoder.state_dict()[k]) < 1e-5, k


@pytest.mark.parametrize("pool,shape", [(1, (3, 8, 64, 64)), (8, (2, 16, 128, 256)), (4, (4, 8, 64, 128))])
def test_sync_bn_relu_pool_phases_equal_the_fused_call_and_full_batch_statistics(pool, shape):
    """SyncBatchNorm2d on libsmokehip (smk_bn_relu_pool_phase: statistics / apply / gradient sums / dz as separate passes with the
    host's all-reduce in between).  One process: identical to the fused training BatchNorm call.  Two shards of one batch processed
    with the COMBINED statistics (what the all-gather yields on two ranks): outputs, dz and the summed dgamma / dbeta equal the
    single-process full-batch result."""
    from smokephysai_amd.models import norm as N
    from smokephysai_amd.models.sync_bn import SyncBatchNorm2d
    torch.manual_seed(pool)
    B, C, H, W = shape
    z = (torch.randn(B, C, H, W, device="cuda") * 1.5 + 0.3).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    sbn = SyncBatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3)
        sbn.weight.copy_(bn.weight); sbn.bias.copy_(bn.bias)
    go = torch.randn(B, C, H // pool, W // pool, device="cuda")
    ref = N.hip_bn_relu_pool(z, bn, pool)
    ref.backward(go)
    gz_ref, gw_ref, gb_ref = z.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()
    z.grad = None
    out = N.hip_sync_bn_relu_pool(z, sbn, pool)                      # no process group: world size 1
    out.backward(go)
    assert torch.equal(out, ref) and torch.equal(z.grad, gz_ref)
    assert torch.equal(sbn.weight.grad, gw_ref) and torch.equal(sbn.bias.grad, gb_ref)
    assert torch.allclose(sbn.running_var, bn.running_var, rtol=1e-6) and torch.allclose(sbn.running_mean, bn.running_mean, rtol=1e-6, atol=1e-8)
    # two "ranks": shards [0:h] and [h:B]; statistics combined as _combine_stats does after the all-gather
    L = N._lib.load()
    dev = z.device
    h = B // 2 if B > 2 else 1
    shards = [z.detach()[:h].contiguous(), z.detach()[h:].contiguous()]
    gos = [go[:h].contiguous(), go[h:].contiguous()]
    w, b = bn.weight.detach(), bn.bias.detach()
    st = []
    for zs in shards:
        s = torch.empty(3, C, device=dev)
        ws = torch.empty(int(L.smk_bn_train_workspace(zs.shape[0], C, H, W, pool)), device=dev, dtype=torch.uint8)
        N._phase(L, N.BN_STATS, zs, None, w, b, bn.eps, s[0], s[1], s[2], pool, None, None, None, None, 0.0, ws, dev)
        st.append(s)
    n = torch.tensor([float(zs.shape[0] * H * W) for zs in shards], device=dev, dtype=torch.float64)[:, None]
    means = torch.stack([s[0] for s in st]).double(); vars_ = torch.stack([s[1] for s in st]).double()
    gmean = (means * n).sum(0) / n.sum()
    gvar = ((vars_ + (means - gmean) ** 2) * n).sum(0) / n.sum()
    gm, gr = gmean.float().contiguous(), torch.rsqrt(gvar.float() + bn.eps).contiguous()
    outs, sums = [], []
    for zs, g in zip(shards, gos):
        o = torch.empty(zs.shape[0], C, H // pool, W // pool, device=dev)
        N._phase(L, N.BN_APPLY, zs, None, w, b, bn.eps, gm, None, gr, pool, o, None, None, None, 0.0, None, dev)
        outs.append(o)
        d = torch.empty(2, C, device=dev)
        ws = torch.empty(int(L.smk_bn_train_workspace(zs.shape[0], C, H, W, pool)), device=dev, dtype=torch.uint8)
        N._phase(L, N.BN_BWD_SUMS, zs, g, w, b, 0.0, gm, None, gr, pool, None, None, d[0], d[1], 0.0, ws, dev)
        sums.append(d)
    tot = sums[0] + sums[1]
    dzs = []
    for zs, g in zip(shards, gos):
        dz = torch.empty_like(zs)
        N._phase(L, N.BN_BWD_DZ, zs, g, w, b, 0.0, gm, None, gr, pool, None, dz, tot[0], tot[1], float(n.sum()), None, dev)
        dzs.append(dz)
    scale = float(gz_ref.abs().max())
    assert float((torch.cat(outs) - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    assert float((torch.cat(dzs) - gz_ref).abs().max()) <= 2e-5 * scale
    assert torch.allclose(tot[0], gw_ref, rtol=1e-4, atol=1e-4 * float(gw_ref.abs().max()))
    assert torch.allclose(tot[1], gb_ref, rtol=1e-4, atol=1e-4 * float(gb_ref.abs().max()))


# (5, 128, 128): 640 tiles on 512 resident workgroups -- some workgroups walk two tiles and some one (the others: 0 or exactly 4 rounds)
@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 40, 48), (1, 8, 16), (4, 256, 256), (5, 128, 128)])
def test_training_conv2_forward_vs_fp64_and_gradients_vs_autograd(shape):
    """smk_conv2_train_forward (k_conv2_fwd_b16): input_encoder's Conv2d(64, 128, 3, padding=1) under autograd (smokephys_net.py:28):
    the forward within 2e-6 (max-norm) of an fp64 convolution, incl. frames that are not square, one tile only, and borders on every
    side; the data gradient (smk_conv2_train_dgrad, k_conv2_dgrad_b16) within 1e-5 of fp64 autograd; the weight / bias gradients equal
    PyTorch-ROCm's own (they ARE its convolution_backward on the saved tensors)."""
    from smokephysai_amd.models.conv import hip_conv2_train, hip_conv2_train_supported
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H)
    conv = torch.nn.Conv2d(64, 128, 3, padding=1).cuda()
    x = torch.rand(B, 64, H, W, device="cuda", generator=g) * 2.0 - 0.3
    x = torch.relu(x)                                           # what the first block hands over: non-negative with exact zeros
    assert hip_conv2_train_supported(x, conv)
    xa = x.clone().requires_grad_(True)
    z = hip_conv2_train(xa, conv, hip_forward=True)
    ref = torch.nn.functional.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1)
    err = float((z.double() - ref).abs().max() / ref.abs().max())
    assert err < 2e-6, err                                      # three bf16 terms per operand, six products (observed 9e-7; MIOpen fp32: 4e-7)
    dz = torch.randn(z.shape, device="cuda", generator=g)
    z.backward(dz)
    gw, gb, gx = conv.weight.grad.clone(), conv.bias.grad.clone(), xa.grad.clone()
    conv.zero_grad()
    xb = x.clone().requires_grad_(True)
    conv(xb).backward(dz)
    # all three gradients are libsmokehip's (k_conv2_dgrad_b16, k_conv2_wgrad_b16): against fp64 autograd
    xd = x.double().requires_grad_(True)
    c64 = copy.deepcopy(conv).double()
    c64.zero_grad()
    c64(xd).backward(dz.double())
    errx = float((gx.double() - xd.grad).abs().max() / xd.grad.abs().max())
    assert errx < 1e-5, errx
    errw = float((gw.double() - c64.weight.grad).abs().max() / c64.weight.grad.abs().max())
    errb = float((gb.double() - c64.bias.grad).abs().max() / c64.bias.grad.abs().max())
    assert errw < 1e-5 and errb < 1e-5, (errw, errb)
    for a, b_, name in ((gw, conv.weight.grad, "dW"), (gb, conv.bias.grad, "db")):       # and next to PyTorch-ROCm's fp32 ones
        assert float((a - b_).abs().max()) <= 1e-4 * float(b_.abs().max()), name
    # run-to-run: the partial sums are added in a fixed order
    conv.zero_grad()
    xc = x.clone().requires_grad_(True)
    hip_conv2_train(xc, conv, hip_forward=True).backward(dz)
    assert torch.equal(conv.weight.grad, gw) and torch.equal(conv.bias.grad, gb) and torch.equal(xc.grad, gx)
    assert float((gx - xb.grad).abs().max() / xb.grad.abs().max()) < 1e-4      # and next to PyTorch-ROCm's fp32 one
    # shapes the kernel is not built for are refused, not silently rerouted
    with pytest.raises(ValueError):
        hip_conv2_train(torch.zeros(1, 64, 12, 16, device="cuda"), conv)


@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 40, 128), (5, 256, 256)])
def test_training_conv1_forward_and_weight_gradient_vs_fp64(shape):
    """smk_conv1_train_forward / smk_conv1_train_wgrad: input_encoder's Conv2d(1, 64, 7, padding=3) under autograd (smokephys_net.py:25)
    in fp32 on the vector ALUs: forward within 2e-6 and dW / db within 1e-5 (max-norm) of fp64, run-to-run identical; a caller that asks
    for dX gets PyTorch-ROCm's."""
    from smokephysai_amd.models.conv import hip_conv1_train, hip_conv1_train_supported
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(B * 100 + W)
    conv = torch.nn.Conv2d(1, 64, 7, padding=3).cuda()
    x = torch.rand(B, 1, H, W, device="cuda", generator=g) * 1.5
    assert hip_conv1_train_supported(x, conv)
    z = hip_conv1_train(x, conv)
    c64 = copy.deepcopy(conv).double()
    ref = c64(x.double())
    assert float((z.double() - ref).abs().max() / ref.abs().max()) < 2e-6
    dz = torch.randn(z.shape, device="cuda", generator=g)
    z.backward(dz)
    gw, gb = conv.weight.grad.clone(), conv.bias.grad.clone()
    ref.backward(dz.double())
    assert float((gw.double() - c64.weight.grad).abs().max() / c64.weight.grad.abs().max()) < 1e-5
    assert float((gb.double() - c64.bias.grad).abs().max() / c64.bias.grad.abs().max()) < 1e-5
    conv.zero_grad()
    xr = x.clone().requires_grad_(True)
    hip_conv1_train(xr, conv).backward(dz)
    assert torch.equal(conv.weight.grad, gw) and torch.equal(conv.bias.grad, gb)
    xd = x.double().requires_grad_(True)
    c64(xd).backward(dz.double())
    assert float((xr.grad.double() - xd.grad).abs().max() / xd.grad.abs().max()) < 1e-5
    with pytest.raises(ValueError):
        hip_conv1_train(torch.zeros(1, 1, 30, 64, device="cuda"), conv)

