"""Training on 64^2, 512^2 and 1024^2 frames: the BatchNorm (batch statistics) + ReLU + mean-pool kernels at pools 2, 16 and 32 (smk_bn_relu_pool_*),
the training convolutions at the row pitches of those frames, the train-mode route of SmokePhysNet.encode_frames and the reproducibility of a
step -- against float64 autograd, with the tolerances of the tests of pools 1 / 4 / 8 (test_hip_encoder.py)."""
import copy
import hashlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _err(a, b):
    return rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())


# ---------------------------------------------------------------- the kernels against fp64 autograd
# one chunk per plane and several, a batch that is not a power of two, channel counts that are no multiple of anything, the encoder's own planes
BN_CASES = [(3, 5, 64, 64, 2), (2, 4, 128, 64, 2), (2, 3, 32, 512, 16), (1, 2, 512, 512, 16), (2, 3, 64, 1024, 32), (1, 2, 1024, 1024, 32)]


@pytest.mark.parametrize("B,C,H,W,pool", BN_CASES)
def test_bn_relu_pool_kernels_at_pools_2_16_32_match_fp64_autograd(B, C, H, W, pool):
    """The scheme of test_bn_relu_pool_training_kernels_match_fp64_autograd: output 1e-5, dz 1e-4 on the elements whose pre-activation is not
    within 1e-5 of the ReLU's kink (at most 1e-4 of the tensor: with gamma in [0.5, 1.5] the expected share is 2e-5 * phi(0) / 0.5 = 1.6e-5),
    dgamma / dbeta 1e-3, running statistics 1e-5, a second run bit-equal."""
    from smokephysai_amd.models.norm import hip_bn_relu_pool, hip_bn_relu_pool_supported
    torch.manual_seed(B * C + H + W + pool)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    ref_bn = torch.nn.BatchNorm2d(C).cuda().double().train()
    ref_bn.load_state_dict({k: v.double() if v.is_floating_point() else v.clone() for k, v in bn.state_dict().items()})
    z = (torch.randn(B, C, H, W, device="cuda") * 2.0 + 3.0 * torch.randn(1, C, 1, 1, device="cuda")).requires_grad_(True)
    assert hip_bn_relu_pool_supported(z, pool)
    dout = torch.randn(B, C, H // pool, W // pool, device="cuda")
    out = hip_bn_relu_pool(z, bn, pool)
    assert "HipBnReluPool" in type(out.grad_fn).__name__ and out.shape == dout.shape
    out.backward(dout)
    z64 = z.detach().double().requires_grad_(True)
    pre64 = ref_bn(z64)
    ref = F.avg_pool2d(torch.relu(pre64), pool)
    ref.backward(dout.double())
    sure = (pre64.detach().abs() > 1e-5)
    unsure = float((~sure).sum())
    e = dict(out=_err(out, ref), dz=_err(z.grad * sure, z64.grad * sure), dgamma=_err(bn.weight.grad, ref_bn.weight.grad),
             dbeta=_err(bn.bias.grad, ref_bn.bias.grad), mean=_err(bn.running_mean, ref_bn.running_mean), var=_err(bn.running_var, ref_bn.running_var))
    print(f"bn_relu_pool {(B, C, H, W, pool)}: excluded {unsure:.0f} of {sure.numel()}, " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert unsure < 1e-4 * sure.numel()
    assert e["out"] < 1e-5 and e["dz"] < 1e-4
    assert e["dgamma"] < 1e-3 and e["dbeta"] < 1e-3
    assert e["mean"] < 1e-5 and e["var"] < 1e-5
    assert int(bn.num_batches_tracked) == 1
    g1, gw1, gb1 = z.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()
    z.grad = None
    bn.zero_grad()
    out2 = hip_bn_relu_pool(z, bn, pool)
    out2.backward(dout)
    assert torch.equal(out2, out) and torch.equal(z.grad, g1) and torch.equal(bn.weight.grad, gw1) and torch.equal(bn.bias.grad, gb1)


# ---------------------------------------------------------------- which lanes make which cell
def _frozen_phase_args(C):
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    return one, zero, zero.clone(), one.clone()              # gamma, beta, mean, rstd: y = z


@pytest.mark.parametrize("pool", [16, 32])
def test_pool_cells_are_exact_blocks(pool):
    """The element-wise phases with y = z (gamma = rstd = 1, beta = mean = 0), three rows of cells (three chunks) per plane.  Forward: planes whose
    P x P blocks hold their own cell's number come out as exactly that number.  Backward: dout one-hot in a cell (every corner of the pooled
    plane, one interior cell; first and last plane) gives dz = 1 / P^2 on that cell's block and exactly zero elsewhere."""
    from smokephysai_amd.models import norm as N
    L = N._lib.load()
    B, C, oh, ow = 2, 2, 3, 32
    H, W = oh * pool, ow * pool
    dev = torch.device("cuda")
    gamma, beta, mean, rstd = _frozen_phase_args(C)
    cells = (torch.arange(B * C * oh * ow, device=dev, dtype=torch.float32) + 1.0).reshape(B, C, oh, ow)
    z = cells.repeat_interleave(pool, 2).repeat_interleave(pool, 3).contiguous()
    out = torch.full((B, C, oh, ow), float("nan"), device=dev)
    N._phase(L, N.BN_APPLY, z, None, gamma, beta, 0.0, mean, None, rstd, pool, out, None, None, None, 0.0, None, dev)
    assert torch.equal(out, cells)                              # P^2 equal integers below 2^24 / P^2: every partial sum is exact
    zero = torch.zeros(C, device=dev)
    for (b, c, i, j) in ((0, 0, 0, 0), (0, 1, 0, ow - 1), (1, 0, oh - 1, 0), (1, 1, oh - 1, ow - 1), (1, 0, 1, 13)):
        dout = torch.zeros(B, C, oh, ow, device=dev)
        dout[b, c, i, j] = float(pool * pool)
        dz = torch.full((B, C, H, W), float("nan"), device=dev)
        N._phase(L, N.BN_BWD_DZ, z, dout, gamma, beta, 0.0, mean, None, rstd, pool, None, dz, zero, zero, 1.0, None, dev)
        want = torch.zeros(B, C, H, W, device=dev)
        want[b, c, i * pool:(i + 1) * pool, j * pool:(j + 1) * pool] = 1.0
        assert torch.equal(dz, want), (b, c, i, j)


# ---------------------------------------------------------------- the phases (SyncBatchNorm2d)
@pytest.mark.parametrize("pool,shape", [(2, (4, 8, 64, 64)), (16, (2, 4, 32, 512)), (32, (2, 3, 64, 1024))])
def test_sync_bn_phases_at_pools_2_16_32(pool, shape):
    """test_sync_bn_relu_pool_phases_equal_the_fused_call_and_full_batch_statistics at the new pools: one process bit-equal to the fused call;
    two shards with the combined statistics equal to the full batch (same tolerances)."""
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


# ---------------------------------------------------------------- the training convolutions at rows of 512 and 1024
CONV_SHAPES = [(2, 16, 512), (1, 16, 1024)]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv1_training_node_at_wide_rows(shape):
    """hip_conv1_train (forward, weight / bias gradient, data gradient) against fp64: 2e-6 forward, 1e-5 gradients (test_hip_encoder.py /
    test_hip_input_grad.py)."""
    from smokephysai_amd.models.conv import hip_conv1_train, hip_conv1_train_supported
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(B * 100 + W)
    conv = torch.nn.Conv2d(1, 64, 7, padding=3).cuda()
    x = torch.rand(B, 1, H, W, device="cuda", generator=g) * 1.5
    xr = x.clone().requires_grad_(True)
    assert hip_conv1_train_supported(xr, conv)
    z = hip_conv1_train(xr, conv)
    assert "HipConv1" in type(z.grad_fn).__name__
    dz = torch.randn(z.shape, device="cuda", generator=g)
    z.backward(dz)
    c64 = copy.deepcopy(conv).double()
    c64.zero_grad()
    xd = x.double().requires_grad_(True)
    ref = F.conv2d(xd, c64.weight, c64.bias, padding=3)
    ref.backward(dz.double())
    e = dict(z=_err(z, ref), dw=_err(conv.weight.grad, c64.weight.grad), db=_err(conv.bias.grad, c64.bias.grad), dx=_err(xr.grad, xd.grad))
    print(f"conv1 train {shape}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["z"] < 2e-6 and e["dw"] < 1e-5 and e["db"] < 1e-5 and e["dx"] < 1e-5, e


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv2_training_node_at_wide_rows(shape):
    """hip_conv2_train (forward, data gradient, weight / bias gradient) against fp64: 2e-6 forward, 1e-5 gradients (test_hip_encoder.py)."""
    from smokephysai_amd.models.conv import hip_conv2_train, hip_conv2_train_supported
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + W)
    conv = torch.nn.Conv2d(64, 128, 3, padding=1).cuda()
    x = torch.relu(torch.rand(B, 64, H, W, device="cuda", generator=g) * 2.0 - 0.3)      # what the first block hands over
    xa = x.clone().requires_grad_(True)
    assert hip_conv2_train_supported(xa, conv)
    z = hip_conv2_train(xa, conv, hip_forward=True)
    assert "HipConv2" in type(z.grad_fn).__name__
    dz = torch.randn(z.shape, device="cuda", generator=g)
    z.backward(dz)
    c64 = copy.deepcopy(conv).double()
    c64.zero_grad()
    xd = x.double().requires_grad_(True)
    ref = F.conv2d(xd, c64.weight, c64.bias, padding=1)
    ref.backward(dz.double())
    e = dict(z=_err(z, ref), dx=_err(xa.grad, xd.grad), dw=_err(conv.weight.grad, c64.weight.grad), db=_err(conv.bias.grad, c64.bias.grad))
    print(f"conv2 train {shape}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["z"] < 2e-6 and e["dx"] < 1e-5 and e["dw"] < 1e-5 and e["db"] < 1e-5, e


# ---------------------------------------------------------------- the route
_ROUTE_REF = {}


def _route_reference(B, N):
    """The frames, the upstream gradient, the encoder's initial state and the fp64 module path's parameter gradients for a batch of B frames of
    N^2: computed once and shared by the input_dim cases (both adaptive pools compose to the same block mean whatever input_dim is)."""
    if (B, N) not in _ROUTE_REF:
        from smokephysai_amd.models import SmokePhysNet
        torch.manual_seed(2)
        m = SmokePhysNet(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4, linear_dtype="f32").cuda().train()
        state = copy.deepcopy(m.input_encoder.state_dict())
        gen = torch.Generator(device="cuda").manual_seed(N + B)
        x = torch.rand(B, 1, N, N, device="cuda", generator=gen)
        g = torch.randn(B, 128, 32, 32, device="cuda", generator=gen)
        r64 = m.double()
        r64.encode_frames(x.double()).backward(g.double())
        g64 = {n: p.grad.clone() for n, p in r64.input_encoder.named_parameters()}
        _ROUTE_REF[(B, N)] = (x, g, state, g64)
    return _ROUTE_REF[(B, N)]


@pytest.mark.parametrize("B,N,input_dim", [(3, 64, 128), (2, 512, 128), (2, 512, 32), (1, 1024, 128), (1, 1024, 32)])
def test_train_route_runs_on_libsmokehip_at_64_512_1024(B, N, input_dim):
    """SmokePhysNet.encode_frames in train mode: the HIP nodes serve the call; features within 1e-5 of the linear_dtype='f32' copy (the PyTorch
    modules); encoder parameter gradients, both routes measured against the fp64 module path, e_hip < max(3 e_ref, 5e-3); running statistics
    within 1e-5."""
    from smokephysai_amd.models import SmokePhysNet
    x, g, state, g64 = _route_reference(B, N)
    torch.manual_seed(3)
    hip = SmokePhysNet(input_dim=input_dim, hidden_dim=64, num_layers=1, num_heads=4).cuda().train()
    hip.input_encoder.load_state_dict(state)
    ref = copy.deepcopy(hip)
    ref.linear_dtype = "f32"
    fh = hip.encode_frames(x)
    fr = ref.encode_frames(x)
    assert "HipBnReluPool" in type(fh.grad_fn).__name__ and "HipBnReluPool" not in type(fr.grad_fn).__name__
    assert fh.shape == (B, 128, 32, 32)
    fh.backward(g)
    fr.backward(g)
    ef = _err(fh, fr)
    print(f"train route {B} x {N}^2, input_dim {input_dim}: features {ef:.2e}")
    assert ef < 1e-5
    scale = max(float(q.abs().max()) for q in g64.values())
    for (n, p), (_, q) in zip(hip.input_encoder.named_parameters(), ref.input_encoder.named_parameters()):
        q64 = g64[n]
        if float(q64.abs().max()) > 1e-3 * scale:
            e_hip, e_ref = _err(p.grad.double(), q64), _err(q.grad.double(), q64)
            print(f"  {n}: e_hip {e_hip:.2e} e_ref {e_ref:.2e}")
            assert e_hip < max(3.0 * e_ref, 5e-3), (n, e_hip, e_ref)
        else:                                                               # conv biases in front of a BatchNorm: gradient 0 (rounding noise)
            assert float(p.grad.abs().max()) < 1e-3 * scale, n
    for k in ("1.running_mean", "1.running_var", "4.running_mean", "4.running_var"):
        assert _err(hip.input_encoder.state_dict()[k], ref.input_encoder.state_dict()[k]) < 1e-5, k


# ---------------------------------------------------------------- a step
class _Null:
    def add_scalar(self, *a, **k):
        pass


def _two_steps(batches):
    import train
    from smokephysai_amd.models import SmokePhysNet
    from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
    torch.manual_seed(1234)
    model = SmokePhysNet(hidden_dim=64, num_layers=1, num_heads=4, head_train="hip").cuda()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    torch.manual_seed(99)
    train.train_epoch(model, batches, opt, PhysicsRegularizer(), torch.device("cuda"), 0, _Null())
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for p in model.parameters():
        assert bool(torch.isfinite(p).all())
        h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_two_steps_at_512_are_bit_reproducible(monkeypatch):
    """Two optimisation steps (train.train_epoch) at 2 x 512^2 with head_train='hip', twice from the same seed in one process, without
    mi355x.deterministic: the SHA-256 over all parameters is the same."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    gen = torch.Generator().manual_seed(11)
    batches = [{"input": torch.rand(2, 1, 512, 512, generator=gen), "target": torch.rand(2, 1, 512, 512, generator=gen),
                "chaos_features": torch.rand(2, 3, generator=gen), "sequence": torch.rand(2, 20, 512, 512, generator=gen)} for _ in range(2)]
    assert _two_steps(batches) == _two_steps(batches)
