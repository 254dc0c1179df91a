"""The attention-map kernels (csrc/transformer.hip, k_attention_recv<PROBS>) and everything above them: smk_attention_received /
smk_attention_probs element by element against fp64 on the inputs of the forward's variant tests (NaN-poisoned input padding, sentinel-filled
output padding, a repeated call, sub-ranges, the profiler's kernel names), the refusals, ChaosAttention.attention_maps against its PyTorch
route in fp64, and SmokePhysNet.attention_maps against the forward and a twin on the module route.

Bound (derived, not tuned on a device; notation and the score / lse terms as tests/attention_variant_cases.py derives them).  The kernel
forms s_ij exactly as the forward does (same split operands, same three products per k-step), so
    |ds_ij| <= 2^-14 A_ij + 2^-23 |s_ij - m_i|
and it subtracts the forward's own lse_i, which is within lse_bound_i of the fp64 value.  p = 2^(s - lse) moves by p ln 2 (ds + dlse) to
first order (1.1: room for the second-order terms and for the rounding of the fp32 difference s - lse, at most 2^-24 (|s - m| + log2 L),
which the 2^-23 |s - m| of ds and the 2^-21 of lse_bound cover); exp2 adds a relative 2^-22:
    |dp_ij| <= p_ij (1.1 ln 2 (|ds_ij| + lse_bound_i) + 2^-22) + 2^-126
(2^-126, the smallest normal fp32 number: the peaked rows hold weights below it, which the hardware exp2 returns as zero and which no fp32
output could hold to a relative 2^-22 -- the one term the output format adds to the relative bound).
received_j = (1 / L) sum_i p_ij carries the mean of those over i; its fp32 accumulation passes every term through at most L / 32 running
additions, a four-level tree, the exchange of the lane halves and the division, L / 32 + 6 roundings, all terms positive:
    |d received_j| <= mean_i |dp_ij| + (L / 32 + 8) 2^-24 received_j"""
import copy
import re

import pytest
import torch

from attention_maps_cases import module_inputs, peaked_module
from attention_variant_cases import (CUS, LN2, LOG2E, O_PAD, O_TAIL, SCALE, U, FwdSetup, assert_within, forward_route, outside_touched,
                                     parse_kernel, sentinel)
from conftest import rel_err

pytestmark = pytest.mark.gpu

RECV, PROBS = "k_attention_recv<false>", "k_attention_recv<true>"
_MAPS = re.compile(r"k_attention_recv(?:<\s*(true|false)\s*>|ILb([01])E)")
SHAPES = ((1, 128, 1), (1, 384, 1), (2, 256, 11), (1, 1024, 8))


def _lib():
    from smokephysai_amd import _lib as lib
    return lib


def profiled(fn):
    """(transformer.hip kernels the variant tables know, attention-map kernels, fn's result) of the GPU work fn() launched."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    known, maps = set(), set()
    for e in prof.events():
        k = parse_kernel(e.name)
        if k:
            known.add(k)
        m = _MAPS.search(e.name)
        if m:
            maps.add(RECV if (m.group(1) == "false" or m.group(2) == "0") else PROBS)
    return known, maps, res


def test_kernel_name_pattern():
    hit = lambda name: (lambda m: m and (m.group(1) or m.group(2)))(_MAPS.search(name))
    assert hit("void smk::k_attention_recv<true>(smk::AttnMapArgs)") == "true"
    assert hit("_ZN3smk16k_attention_recvILb0EEEvNS_11AttnMapArgsE") == "0"
    assert parse_kernel("void smk::k_attention_recv<false>(smk::AttnMapArgs)") is None      # the variant tables do not claim it


class MapsSetup:
    """FwdSetup's inputs for one (B, L, H), the forward's own lse, and per sampled (batch, head) the fp64 weights with their bound."""

    def __init__(self, B, L, H):
        self.B, self.L, self.H = B, L, H
        self.s = s = FwdSetup(B, L, H, seed=B * 1000 + L + H)
        _, lbuf = s.run(False, lse=True)
        self.lse = lbuf.view(torch.float32)[:B * L * H].clone()                       # [B][L][H]
        self.refs = {}
        for (b, h), (_, _, _, lse_bound) in s.refs.items():
            rows, cols = slice(b * L, (b + 1) * L), slice(64 * h, 64 * h + 64)
            qd = s.q[rows, cols].double() * (SCALE * LOG2E)
            kd = s.k32[rows, cols].double()
            sc = qd @ kd.t()
            A = qd.abs() @ kd.abs().t()
            m = sc.max(1, keepdim=True).values
            e = torch.exp2(sc - m)
            P = e / e.sum(1, keepdim=True)
            ds = 2.0 ** -14 * A + 2.0 ** -23 * (sc - m).abs()
            p_bound = P * (1.1 * LN2 * (ds + lse_bound[:, None]) + 2.0 ** -22) + 2.0 ** -126
            recv = P.mean(0)
            self.refs[(b, h)] = (P, p_bound, recv, p_bound.mean(0) + (L / 32 + 8) * U * recv)

    def received(self):
        lib = _lib()
        B, L, H, s = self.B, self.L, self.H, self.s
        buf = sentinel(B * H + O_TAIL, L + O_PAD)
        lib.check(lib.load().smk_attention_received(s.q.data_ptr(), s.k32.data_ptr(), self.lse.data_ptr(), buf.data_ptr(), B, L, H, 64,
                                                    s.q.stride(0), s.k32.stride(0), L + O_PAD, SCALE, lib.stream_ptr(torch.device("cuda"))))
        return buf

    def probs(self, b0, nb, h0, nh):
        lib = _lib()
        B, L, H, s = self.B, self.L, self.H, self.s
        buf = sentinel(nb * nh * L + O_TAIL, L + O_PAD)
        lib.check(lib.load().smk_attention_probs(s.q.data_ptr(), s.k32.data_ptr(), self.lse.data_ptr(), buf.data_ptr(), B, L, H, 64, b0, nb, h0, nh,
                                                 s.q.stride(0), s.k32.stride(0), L + O_PAD, SCALE, lib.stream_ptr(torch.device("cuda"))))
        return buf


_setups = {}


def maps_setup(B, L, H) -> MapsSetup:
    if (B, L, H) not in _setups:
        _setups.clear()                                     # (one at a time: the tests that share a shape are adjacent)
        _setups[(B, L, H)] = MapsSetup(B, L, H)
    return _setups[(B, L, H)]


@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[3:] + SHAPES[2:3], ids=lambda s: "x".join(map(str, s)))
def test_maps_kernels_against_fp64(shape):
    B, L, H = shape
    ms = maps_setup(B, L, H)
    acc = (L / 32 + 8) * U

    known, maps, rbuf = profiled(ms.received)
    assert (known, maps) == (set(), {RECV}), (sorted(known), sorted(maps))
    known, maps, pbuf = profiled(lambda: ms.probs(0, B, 0, H))
    assert (known, maps) == (set(), {PROBS}), (sorted(known), sorted(maps))
    assert outside_touched(rbuf, (slice(0, B * H), slice(0, L))) == 0, "received: words outside [B H][L] overwritten"
    assert outside_touched(pbuf, (slice(0, B * H * L), slice(0, L))) == 0, "probs: words outside [B H L][L] overwritten"
    assert torch.equal(rbuf, ms.received()) and torch.equal(pbuf, ms.probs(0, B, 0, H)), "a second call differs"

    recv = rbuf.view(torch.float32)[:B * H, :L].view(B, H, L)
    probs = pbuf.view(torch.float32)[:B * H * L, :L].view(B, H, L, L)
    total = recv.double().sum(-1)
    print(f"{shape}: max |sum_j received - 1| = {float((total - 1).abs().max()):.3e}")
    assert float((total - 1).abs().max()) < 1e-5
    for (b, h), (P, p_bound, r_ref, r_bound) in ms.refs.items():
        peak = float(r_ref.max()) * L
        own = probs[b, h].double().mean(0)
        print(f"{shape} ({b}, {h}): peak {peak:.1f}, worst err / bound: probs {float(((probs[b, h].double() - P).abs() / p_bound).max()):.3f}, "
              f"received {float(((recv[b, h].double() - r_ref).abs() / r_bound).max()):.3f}, received against its own probs "
              f"{float(((recv[b, h].double() - own).abs() / (acc * own + 1e-300)).max()):.3f}")
        assert peak > 2.0, f"batch {b} head {h}: the reference map is nearly uniform (max_j received * L = {peak:.2f})"
        assert_within(probs[b, h], P, p_bound, f"{shape} probs (batch {b}, head {h})")
        assert_within(recv[b, h], r_ref, r_bound, f"{shape} received (batch {b}, head {h})")
        assert_within(recv[b, h], own, acc * own + 1e-300, f"{shape} received against the column mean of its own probs (batch {b}, head {h})")
    # the all-zero queries of (0, 0) weigh every key 1 / L; the peaked queries of the last pair put (nearly) everything on their key
    assert float((probs[0, 0, :32].double() - 1.0 / L).abs().max()) < 2.0 ** -18 / L        # (a few ulp of lse = log2 L, times ln 2)
    assert float(probs[B - 1, H - 1, L - 32:].diagonal(L - 32).min()) > 0.99

    # sub-ranges: bit for bit the slice of the full call
    ranges = [(B - 1, 1, H - 1, 1), (0, 1, 0, 1)] + ([(1, 1, 3, 5)] if shape == (2, 256, 11) else [])
    for b0, nb, h0, nh in ranges:
        sub = ms.probs(b0, nb, h0, nh)
        assert outside_touched(sub, (slice(0, nb * nh * L), slice(0, L))) == 0
        got = sub.view(torch.float32)[:nb * nh * L, :L].view(nb, nh, L, L)
        assert torch.equal(got.view(torch.int32), probs[b0:b0 + nb, h0:h0 + nh].contiguous().view(torch.int32)), (b0, nb, h0, nh)


def test_wrapper_obtains_lse_and_takes_pitched_slices():
    """hip_attention_maps on q | k slices of one fused buffer: without lse it runs the forward for it (that kernel and the two map kernels are
    all the profiler shows) and returns bit for bit what the direct calls return with the forward's lse."""
    from smokephysai_amd.models.attention import hip_attention_maps
    B, L, H = 2, 256, 11
    D = 64 * H
    ms = maps_setup(B, L, H)
    qkv = torch.full((B, L, 3 * D + 8), float("nan"), device="cuda")
    qkv[..., :D] = ms.s.q.view(B, L, D)
    qkv[..., D:2 * D] = ms.s.k32.view(B, L, D)
    q, k = qkv[..., :D], qkv[..., D:2 * D]
    known, maps, (recv, probs) = profiled(lambda: hip_attention_maps(q, k, H, SCALE, probs_for=(1, 1, 3, 5)))
    assert maps == {RECV, PROBS}
    if torch.cuda.get_device_properties(0).multi_processor_count == CUS:
        assert known == {forward_route(B, L, H, False)[1]}, sorted(known)
    assert recv.shape == (B, H, L) and probs.shape == (1, 5, L, L)
    want_r = ms.received().view(torch.float32)[:B * H, :L].view(B, H, L)
    want_p = ms.probs(1, 1, 3, 5).view(torch.float32)[:5 * L, :L].view(1, 5, L, L)
    assert torch.equal(recv, want_r) and torch.equal(probs, want_p)
    known, maps, recv2 = profiled(lambda: hip_attention_maps(q, k, H, SCALE, lse=ms.lse.view(B, L, H)))
    assert (known, maps) == (set(), {RECV}) and torch.equal(recv2, recv)
    with pytest.raises(ValueError):
        hip_attention_maps(q[:, :192], k[:, :192], H, SCALE)
    with pytest.raises(ValueError):
        hip_attention_maps(q, k, H, SCALE, probs_for=(1, 2, 0, 1))


def test_refusals_write_nothing():
    lib = _lib()
    Lh = lib.load()
    st = lib.stream_ptr(torch.device("cuda"))
    B, L, H = 1, 256, 2
    D = 64 * H
    q = torch.randn(B, L, D, device="cuda")
    k = torch.randn(B, L, D, device="cuda")
    lse = torch.zeros(B, L, H, device="cuda")
    out = sentinel(B * H * L, L)

    def calls(L_, hd, ldq, ld_out=None):
        ld_out = L_ if ld_out is None else ld_out
        return (Lh.smk_attention_received(q.data_ptr(), k.data_ptr(), lse.data_ptr(), out.data_ptr(), B, L_, H, hd, ldq, ldq, ld_out, SCALE, st),
                Lh.smk_attention_probs(q.data_ptr(), k.data_ptr(), lse.data_ptr(), out.data_ptr(), B, L_, H, hd, 0, 1, 0, 1, ldq, ldq, ld_out,
                                       SCALE, st))
    big_L = (1 << 29) // D                                                   # B * L * ld = 2^29 floats: one past the 32-bit offset range
    assert big_L % 128 == 0
    cases = {"L = 192": (calls, (192, 64, D), lib.SMK_ERR_UNSUPPORTED), "head_dim = 32": (calls, (L, 32, D), lib.SMK_ERR_UNSUPPORTED),
             "offsets past 2^31 bytes": (calls, (big_L, 64, D), lib.SMK_ERR_INVALID), "output pitch < L": (calls, (L, 64, D, L - 4), lib.SMK_ERR_INVALID)}
    for what, (fn, args, status) in cases.items():
        known, maps, rcs = profiled(lambda: fn(*args))
        assert rcs == (status, status), (what, rcs)
        assert not known and not maps, (what, sorted(known | maps))
    bad_range = Lh.smk_attention_probs(q.data_ptr(), k.data_ptr(), lse.data_ptr(), out.data_ptr(), B, L, H, 64, 0, 2, 1, 2, D, D, L, SCALE, st)
    assert bad_range == lib.SMK_ERR_INVALID
    torch.cuda.synchronize()
    assert outside_touched(out, (slice(0, 0), slice(0, 0))) == 0, "a refused call wrote to its output"
    assert calls(L, 64, D) == (0, 0)                                         # ... and the same arguments within the limits run


def test_module_against_its_fp64_route():
    """ChaosAttention.attention_maps on libsmokehip against the PyTorch route of a float64 copy, on a module whose maps are far from uniform."""
    m = peaked_module().cuda()
    m64 = copy.deepcopy(m).double()
    x, noise = (t.cuda() for t in module_inputs())
    r64, p64 = m64.attention_maps(x.double(), noise=noise.double(), probs_for=(0, 2, 0, 2))
    peak = float((r64.max(-1).values * x.shape[1]).min())
    assert peak > 2.0, f"the reference maps are nearly uniform (min over (b, h) of max_j received * L = {peak:.2f})"
    known, maps, (r, p) = profiled(lambda: m.attention_maps(x, noise=noise, probs_for=(0, 2, 0, 2)))
    assert maps == {RECV, PROBS}, sorted(maps)
    assert r.dtype == torch.float32 and r.shape == (2, 2, 128) and p.shape == (2, 2, 128, 128)
    e_r, e_p = rel_err(r.cpu().numpy(), r64.cpu().numpy()), rel_err(p.cpu().numpy(), p64.cpu().numpy())
    print(f"module maps against fp64: received rel_err {e_r:.3e}, probs rel_err {e_p:.3e} (peak {peak:.2f})")
    assert e_r < 1e-4 and e_p < 1e-4
    # a mask takes the PyTorch route, in float32
    mask = torch.ones(2, 128, device="cuda")
    mask[:, 96:] = 0
    known, maps, rm = profiled(lambda: m.attention_maps(x, noise=noise, mask=mask))
    assert not maps and float(rm[..., 96:].abs().max()) == 0.0


def test_model_maps_leave_the_forward_bit_identical():
    """SmokePhysNet.attention_maps: the forward's outputs bit for bit, maps of the shape the figure takes, within 1e-4 (max-norm relative) of a
    twin model on the module route (linear_dtype="f32": PyTorch linears, ChaosAttention.attention_maps per layer), no state left behind."""
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(hidden_dim=128, num_heads=2, num_layers=2).cuda().eval()
    twin = SmokePhysNet(hidden_dim=128, num_heads=2, num_layers=2, linear_dtype="f32").cuda().eval()
    twin.load_state_dict(model.state_dict())
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(2, 1, 64, 64, device="cuda", generator=g)
    noise = torch.randn(2, 3, 2, 1, device="cuda", generator=g)
    keys = ("reconstructed", "physics_features", "latent_features")
    with torch.no_grad():
        before = model(x, chaos_noise=noise)
    known, maps, out = profiled(lambda: model.attention_maps(x, chaos_noise=noise, probs_for=(0, 1, 0, 1)))
    assert maps == {RECV, PROBS}, sorted(maps)
    assert not any(k.endswith("true>") for k in known if k.startswith("k_attention_x3")), sorted(known)      # captured layers: fp32 k | v
    for key in keys:
        assert torch.equal(out[key], before[key]), key
    assert sorted(out["attention_received"]) == [0, 1] and sorted(out["attention_probs"]) == [0, 1]
    ref = twin.attention_maps(x, chaos_noise=noise, probs_for=(0, 1, 0, 1))
    for li in (0, 1):
        r, p = out["attention_received"][li], out["attention_probs"][li]
        assert r.shape == (2, 2, 32, 32) and p.shape == (1, 1, 1024, 1024)
        assert float((r.double().sum((-1, -2)) - 1).abs().max()) < 1e-5
        own = p[0, 0].double().mean(0)
        assert_within(r[0, 0].reshape(-1), own, (1024 / 32 + 8) * U * own + 1e-300, f"layer {li}: received against the column mean of its probs")
        e_r = rel_err(r.cpu().numpy(), ref["attention_received"][li].cpu().numpy())
        e_p = rel_err(p.cpu().numpy(), ref["attention_probs"][li].cpu().numpy())
        print(f"layer {li}: received rel_err {e_r:.3e}, probs rel_err {e_p:.3e} against the module route")
        assert e_r < 1e-4 and e_p < 1e-4, (li, e_r, e_p)
    only = model.attention_maps(x, layers=[1], chaos_noise=noise)
    assert sorted(only["attention_received"]) == [1] and only["attention_probs"] == {}
    assert torch.equal(only["attention_received"][1], out["attention_received"][1])
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        model.attention_maps(x, chaos_noise=noise)
    model.eval()
    known, maps, after = profiled(lambda: _forward(model, x, noise))
    assert not maps
    for key in keys:
        assert torch.equal(after[key], before[key]), f"{key}: the forward changed after attention_maps"


def _forward(model, x, noise):
    with torch.no_grad():
        return model(x, chaos_noise=noise)
