"""Every form of the eval-mode reconstruction head (csrc/decoder.hip, models/decoder.py) and of the model's tail (smk_pooled_head,
csrc/transformer.hip) against fp64, element by element, with the buffers in a guarded arena the test owns.

launch_decoder picks one of three forms from (B, S) and the process-wide SMK_DECODER_SMALL (read once per process):

    small        B <= 8 (and SMK_DECODER_SMALL not 0)    k_convt4s2_small<64,32,true>, k_convt4s2_small<32,16,false>
    tiled, OG 2  otherwise, (S/16)^2 * 4 * B < 256        k_convt4s2<64,32,2,true>,     k_convt4s2<32,16,2,false>
    tiled, OG 8  otherwise                                k_convt4s2<64,32,8,true>,     k_convt4s2<32,16,8,false>

and k_conv3_sigmoid<8,32> follows in every form.  CASES reaches every row (the profiler's device events name the kernels that ran);
`python tests/test_hip_decoder.py child DIR` is the same run in a fresh process, which the test starts with SMK_DECODER_SMALL=0.

Error bounds.  u = 2^-24 (fp32 unit roundoff).  No constant below comes from a GPU measurement; they change only with a derivation.

Transposed-conv stage (CIN input channels), before the ReLU.  With s = gamma / sqrt(var + 1e-5) the kernels compute
    pre = sum_{c, 4 taps} x * fl(w s) + t,      t = fl(fl(fl(b - mean) * s~) + beta),
one fmaf chain of 4 CIN products from 0, then one addition of t.  s~ is s after four fp32 roundings (the sum under the root, the
root, the quotient -- both correctly rounded in this build -- and the product with w or with b - mean): each folded weight is within
4u (1 + 4u) of w s, and the fp32 spelling of 1e-5 moves s by less than 1e-5 * 2^-25 / var.  The chain adds gamma_{4 CIN} <= 4 CIN u (1 + ..)
of sum |x| |w s|, the last addition u |pre| <= u (sum |x| |w s| + |t|).  Together (4 CIN + 1 + 4) u plus second-order terms; the shift
carries u (subtraction) + 4u (s~ and the product) on |b - mean| |s|, u on the sum with beta, u from the last addition above:
    |pre - ref| <= (4 CIN + 16) u (|x| * |w s|) + 16 u (|b - mean| |s| + |beta|)
(`*`: the same transposed convolution on absolute values; 16 leaves room for every second-order term).  ReLU has slope <= 1 and
carries the bound unchanged.  A float32 numpy restatement with separately rounded products (one more u per product: 4 CIN u more
in the worst case, still first order in the same sum) is held against the same bound on the CPU in tests/test_decoder_host.py, which
also shows that swapped taps and a wrong border fall outside it.

Last stage.  acc = b3 followed by 144 fmaf: |acc - ref| <= gamma_144 (|x| * |w3| + |b3|) <= 146 u (..).  sigmoid' <= 1/4.  The result
1 / (1 + expf(-acc)) adds: expf within 1 ulp = 2u relative, which moves y = 1 / (1 + e) by y (1 - y) 2u <= u / 2; the sum 1 + e rounds
once (u y) and the correctly rounded quotient once more (u y); y <= 1, so 2.5 u <= 2^-22:
    |recon - ref| <= 0.25 * 146 u (|x| * |w3| + |b3|) + 2^-22.

Each stage's reference takes the GPU's own previous-stage output as its input, so no error travels between stages; the end-to-end
check is the old global bar (max-norm rel_err < 5e-6 against the fp64 chain from the tokens).

Pooled head (x [B][L][ldx], D columns used).  k_token_chunk_sums adds per = ceil(L / 32) tokens in order from 0 (per - 1 roundings),
k_pooled_hidden adds the 32 chunk sums in order (31) and divides by L (1): |pooled - ref| <= (per + 31) u mean_l |x|, stated as
    e_pooled = (ceil(L / 32) + 36) u mean_l |x|.
A hidden unit: a lane forms 4-term dot products (4 rounded products, 3 additions) and adds them over ceil(D / 256) steps, six
shuffle additions merge the lanes, the bias one more: at most 1 + 3 + ceil(D / 256) + 6 + 1 <= D + 16 roundings on any term,
    e_hidden = (D + 16) u (|w1| @ |pooled| + |b1|) + |w1| @ e_pooled            (ReLU: slope <= 1)
and an output unit the same way over ceil(H1 / 64) steps (1 + ceil(H1 / 64) + 6 + 1 <= H1 + 16):
    e_out = (H1 + 16) u (|w2| @ hidden + |b2|) + |w2| @ e_hidden.
The global bars of test_pooled_head_kernel_matches_torch (1e-6 on pooled, 1e-5 on out) stay beside them."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from conftest import rel_err      # noqa: E402
from guarded_arena import FILL_NAN, FILL_ZERO, GUARD, Arena      # noqa: E402,F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

SMALL = ("k_convt4s2_small<64,32,true>", "k_convt4s2_small<32,16,false>")
OG2 = ("k_convt4s2<64,32,2,true>", "k_convt4s2<32,16,2,false>")
OG8 = ("k_convt4s2<64,32,8,true>", "k_convt4s2<32,16,8,false>")
CONV3 = "k_conv3_sigmoid<8,32>"
FORMS = {"small": SMALL, "og2": OG2, "og8": OG8}
# (B, S, form).  S = 48: a tile without any image border, tiles_x not a power of two.  (63,16) is the last OG 2 batch (252 < 256),
# (64,16) and (16,32) the first OG 8 ones (exactly 256).
CASES = [(1, 16, "small"), (8, 32, "small"), (3, 48, "small"),
         (9, 16, "og2"), (63, 16, "og2"), (12, 32, "og2"),
         (64, 16, "og8"), (16, 32, "og8"), (9, 48, "og8")]
CHILD_CASES = [(1, 16, "og2"), (8, 32, "og2"), (8, 48, "og8")]           # with SMK_DECODER_SMALL=0
POOL_FRAMES = {16: 64, 32: 16, 48: 9}                                    # frames of the token pool per S: case (B, S) takes the first B
STAGES = ("tmp1", "tmp2", "recon")


# ------------------------------------------------------------------------------------------------ kernel names
_NAMES = "k_convt4s2_small|k_convt4s2|k_conv3_sigmoid"
_DEMANGLED = re.compile(rf"\b({_NAMES})<([^<>]*)>")
_MANGLED = re.compile(rf"\d+({_NAMES})I((?:L[ib]n?\d+E)+)E")


def parse_kernel(name: str):
    """A trace event's name -> 'k_convt4s2<64,32,8,true>', from either the demangled ('void smk::k_convt4s2<64, 32, 8, true>(float
    const*, ...)') or the mangled ('_ZN3smk10k_convt4s2ILi64ELi32ELi8ELb1EEEvPKfS2_S2_Pfii') spelling; None for any other kernel."""
    m = _DEMANGLED.search(name)
    if m:
        args = []
        for a in m.group(2).split(","):
            a = re.sub(r"^\((?:int|bool)\)", "", a.strip())          # (some demanglers print casts)
            args.append(a if a in ("true", "false") else str(int(a)))
        return f"{m.group(1)}<{','.join(args)}>"
    m = _MANGLED.search(name)
    if m:
        args = []
        for t, v in re.findall(r"L([ib])(n?\d+)E", m.group(2)):
            v = int(v.replace("n", "-"))
            args.append(("true" if v else "false") if t == "b" else str(v))
        return f"{m.group(1)}<{','.join(args)}>"
    return None


def launched_kernels(fn):
    """(the eval-decoder kernels the GPU ran during fn(), fn's result), by name from the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    return {k for k in (parse_kernel(e.name) for e in prof.events()) if k}, res


# ------------------------------------------------------------------------------------------------ fp64 references and bounds (no device code)
def head_params64(head) -> dict:
    from smokephysai_amd.models.decoder import decoder_weight_dict
    return {k: v.detach().double() for k, v in decoder_weight_dict(head).items()}


def tokens_as_image(tokens):
    """[B, S*S, 64] -> [B, 64, S, S] (smokephys_net.py:117), in fp64."""
    B, L, Cc = tokens.shape
    S = int(round(L ** 0.5))
    return tokens.double().transpose(1, 2).reshape(B, Cc, S, S)


def convt_stage_reference(x, w, b, gamma, beta, mean, var):
    """relu(bn(convT(x))) of one ConvTranspose2d(k4, s2, p1) + eval BatchNorm(eps 1e-5) + ReLU stage in fp64, from the modules' own
    (unfolded) formula, and the elementwise bound of the module docstring.  x [B, CIN, H, W] fp64, any device."""
    cin = w.shape[0]
    pre = F.batch_norm(F.conv_transpose2d(x, w, b, stride=2, padding=1), mean, var, gamma, beta, False, 0.0, 1e-5)
    s = gamma / torch.sqrt(var + 1e-5)
    A = F.conv_transpose2d(x.abs(), (w * s[None, :, None, None]).abs(), None, stride=2, padding=1)
    shift = (b - mean).abs() * s.abs() + beta.abs()
    return torch.relu(pre), (4 * cin + 16) * U * A + 16 * U * shift[None, :, None, None]


def conv3_stage_reference(x, w3, b3):
    """sigmoid(conv3x3(x) + b3) in fp64 and its elementwise bound.  x [B, 16, H, W] fp64."""
    A = F.conv2d(x.abs(), w3.abs(), None, padding=1) + b3.abs()
    return torch.sigmoid(F.conv2d(x, w3, b3, padding=1)), 0.25 * 146 * U * A + 2.0 ** -22


def stage_references(p, tokens, out):
    """[(name, ref, bound)] of the three stages, each from the GPU's own previous-stage output."""
    r1 = convt_stage_reference(tokens_as_image(tokens), p["ct1_w"], p["ct1_b"], p["bn1_w"], p["bn1_b"], p["bn1_mean"], p["bn1_var"])
    r2 = convt_stage_reference(out["tmp1"].double(), p["ct2_w"], p["ct2_b"], p["bn2_w"], p["bn2_b"], p["bn2_mean"], p["bn2_var"])
    r3 = conv3_stage_reference(out["tmp2"].double(), p["conv_w"], p["conv_b"])
    return [("tmp1",) + r1, ("tmp2",) + r2, ("recon",) + r3]


def chain_reference(p, tokens):
    """The whole head in fp64 from the tokens."""
    a1, _ = convt_stage_reference(tokens_as_image(tokens), p["ct1_w"], p["ct1_b"], p["bn1_w"], p["bn1_b"], p["bn1_mean"], p["bn1_var"])
    a2, _ = convt_stage_reference(a1, p["ct2_w"], p["ct2_b"], p["bn2_w"], p["bn2_b"], p["bn2_mean"], p["bn2_var"])
    return conv3_stage_reference(a2, p["conv_w"], p["conv_b"])[0]


def outside_bound(got, ref, bound):
    """(elements outside the bound, a NaN counting as outside; worst err / bound)."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(float("inf"))
    return bad, float(ratio.max())


def assert_within(got, ref, bound, what) -> float:
    """Every element of got within bound of ref; returns the worst err / bound."""
    bad, worst = outside_bound(got, ref, bound)
    if bool(bad.any()):
        idx = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {list(idx)}: got "
                             f"{float(got[idx])!r} ref {float(ref[idx])!r} bound {float(bound[idx]):.3e}; worst err / bound {worst:.3g}")
    return worst


def make_head(device, seed=7):
    """SmokePhysNet().reconstruction_head in eval mode with seeded random running statistics and affine parameters (as
    test_decoder_head_matches_torch makes it)."""
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(seed)
    head = SmokePhysNet().reconstruction_head.eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in head:
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.randn(m.num_features, generator=g) * 0.3 + 1.0)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    return head.to(device)


# ------------------------------------------------------------------------------------------------ the guarded arena (tests/guarded_arena.py)
def decoder_arena(B, S):
    return Arena([("tokens", B * S * S * 64, 0), ("tmp1", B * 32 * 4 * S * S, 2), ("tmp2", B * 16 * 16 * S * S, 2),
                  ("recon", B * 16 * S * S, 1)])


def decoder_shapes(B, S):
    return {"tmp1": (B, 32, 2 * S, 2 * S), "tmp2": (B, 16, 4 * S, 4 * S), "recon": (B, 1, 4 * S, 4 * S)}


class Decoder:
    """A smk_decoder handle for `head`, as HipDecoder.__init__ makes it."""

    def __init__(self, head):
        from smokephysai_amd import _lib
        from smokephysai_amd.models.decoder import _KEYS, decoder_weight_dict
        self.lib, self.L = _lib, _lib.load()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        wd = decoder_weight_dict(head)
        self.ws = {k: wd[k].detach().to(self.dev, torch.float32).contiguous() for k in _KEYS}
        packed = _lib.SmkDecoderWeights(*[self.ws[k].data_ptr() for k in _KEYS])
        self.handle = C.c_void_p()
        _lib.check(self.L.smk_decoder_create(C.byref(packed), self.dev.index, _lib.stream_ptr(self.dev), C.byref(self.handle)))
        torch.cuda.synchronize()

    def forward(self, arena, B, S, tokens_ptr=None):
        self.lib.check(self.L.smk_decoder_forward(self.handle, arena.ptr("tokens") if tokens_ptr is None else tokens_ptr, B, S,
                                                  arena.ptr("tmp1"), arena.ptr("tmp2"), arena.ptr("recon"), self.lib.stream_ptr(self.dev)))

    def run(self, tokens, fill):
        """One guarded call: every arena word but the tokens holds `fill` before it.  -> ({stage: tensor}, damaged guard words)"""
        B, S = tokens.shape[0], int(round(tokens.shape[1] ** 0.5))
        arena = decoder_arena(B, S)
        arena.fill(fill)
        arena.view("tokens").copy_(tokens.reshape(-1))
        self.forward(arena, B, S)
        torch.cuda.synchronize()
        out = {k: arena.view(k).clone().view(shape) for k, shape in decoder_shapes(B, S).items()}
        return out, arena.guard_damage(fill)


def run_case(dec, tokens):
    """Both fills (the NaN fill under the profiler).  -> dict(out, kernels, guard_damage, fill_equal, nan)"""
    kernels, (out, dmg_nan) = launched_kernels(lambda: dec.run(tokens, FILL_NAN))
    out0, dmg_zero = dec.run(tokens, FILL_ZERO)
    return dict(out=out, kernels=sorted(kernels), guard_damage=dmg_nan + dmg_zero,
                fill_equal={k: bool(torch.equal(out[k].view(torch.int32), out0[k].view(torch.int32))) for k in STAGES},
                nan={k: int(torch.isnan(out[k]).sum() + torch.isnan(out0[k]).sum()) for k in STAGES})


def token_pool(S, device="cuda"):
    g = torch.Generator().manual_seed(1000 + S)
    return torch.randn(POOL_FRAMES[S], S * S, 64, generator=g).to(device)


# ------------------------------------------------------------------------------------------------ part 1: the decoder's forms
@functools.lru_cache(maxsize=None)
def _head():
    return make_head("cuda")


@functools.lru_cache(maxsize=None)
def _decoder():
    return Decoder(_head())


@functools.lru_cache(maxsize=None)
def _params():
    return head_params64(_head())


@functools.lru_cache(maxsize=None)
def _pool(S):
    return token_pool(S)


@functools.lru_cache(maxsize=None)
def _result(B, S):
    return run_case(_decoder(), _pool(S)[:B])


def _ids(cases):
    return [f"B{B}-S{S}-{form}" for B, S, form in cases]


@pytest.mark.parametrize("B,S,form", CASES, ids=_ids(CASES))
def test_decoder_form_runs_its_kernels(B, S, form):
    assert _result(B, S)["kernels"] == sorted(FORMS[form] + (CONV3,))


@pytest.mark.parametrize("B,S,form", CASES, ids=_ids(CASES))
def test_decoder_stages_within_fp64_bound(B, S, form):
    r = _result(B, S)
    with torch.no_grad():
        worst = {name: assert_within(r["out"][name], ref, bound, f"B={B} S={S} {form} {name}")
                 for name, ref, bound in stage_references(_params(), _pool(S)[:B], r["out"])}
    print(f"decoder B={B} S={S} {form}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("B,S,form", CASES, ids=_ids(CASES))
def test_decoder_end_to_end(B, S, form):
    with torch.no_grad():
        ref = chain_reference(_params(), _pool(S)[:B])
    assert rel_err(_result(B, S)["out"]["recon"].cpu().numpy(), ref.cpu().numpy()) < 5e-6


@pytest.mark.parametrize("B,S,form", CASES, ids=_ids(CASES))
def test_decoder_keeps_to_its_buffers(B, S, form):
    """Guards untouched; the same bits and no NaN whether the arena around the tokens held NaNs or zeros: every output word is
    written, and nothing read outside the tokens or outside a stage's input plane reaches a result."""
    r = _result(B, S)
    assert r["guard_damage"] == 0
    assert r["fill_equal"] == {k: True for k in STAGES}
    assert r["nan"] == {k: 0 for k in STAGES}


def test_decoder_forms_give_the_same_bits():
    """decoder.hip: the small form is bit-identical to the tiled one, and OG 2 / OG 8 run the same chain per output element."""
    og8, og2, small = _result(16, 32), _result(12, 32), _result(8, 32)
    assert set(OG8) <= set(og8["kernels"]) and set(OG2) <= set(og2["kernels"]) and set(SMALL) <= set(small["kernels"])
    for k in STAGES:
        assert torch.equal(og8["out"][k][:8], small["out"][k]), k
        assert torch.equal(og2["out"][k][:8], small["out"][k]), k


def child_main(path):
    """The CHILD_CASES in this process (started with SMK_DECODER_SMALL=0): outputs and kernel names go to `path`."""
    inputs = torch.load(os.path.join(path, "inputs.pt"))
    head = make_head("cuda")
    head.load_state_dict(inputs["head"])
    dec = Decoder(head)
    report = []
    for B, S, _ in CHILD_CASES:
        r = run_case(dec, inputs["tokens"][S][:B].cuda())
        torch.save({k: v.cpu() for k, v in r["out"].items()}, os.path.join(path, f"out_{B}_{S}.pt"))
        report.append({"B": B, "S": S, "kernels": r["kernels"], "guard_damage": r["guard_damage"], "fill_equal": r["fill_equal"],
                       "nan": r["nan"]})
    with open(os.path.join(path, "report.json"), "w") as f:
        json.dump(report, f)
    print("child-ok")


def test_decoder_tiled_forms_at_small_batches(tmp_path):
    """SMK_DECODER_SMALL=0 keeps the tiled form at B <= 8: OG 2 for (1,16) and (8,32), OG 8 for (8,48); the same bits as the small form."""
    torch.save({"head": {k: v.cpu() for k, v in _head().state_dict().items()},
                "tokens": {S: _pool(S).cpu() for S in sorted({S for _, S, _ in CHILD_CASES})}}, tmp_path / "inputs.pt")
    env = dict(os.environ, SMK_DECODER_SMALL="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(tmp_path)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and "child-ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    report = json.load(open(tmp_path / "report.json"))
    assert [(r["B"], r["S"]) for r in report] == [(B, S) for B, S, _ in CHILD_CASES]
    for (B, S, form), r in zip(CHILD_CASES, report):
        assert r["kernels"] == sorted(FORMS[form] + (CONV3,)), (B, S)
        assert r["guard_damage"] == 0 and all(r["fill_equal"].values()) and not any(r["nan"].values()), (B, S)
        small = _result(B, S)
        assert small["kernels"] == sorted(SMALL + (CONV3,)), (B, S)
        tiled = torch.load(tmp_path / f"out_{B}_{S}.pt")
        for k in STAGES:
            assert torch.equal(tiled[k].cuda().view(torch.int32), small["out"][k].view(torch.int32)), (B, S, k)


def test_decoder_refuses_loudly_and_launches_nothing():
    from smokephysai_amd._lib import SmokeHipError
    from smokephysai_amd.models.decoder import HipDecoder, decoder_weight_dict
    dec = _decoder()
    arena = decoder_arena(1, 32)                        # room for every call below, had it launched
    arena.fill(FILL_NAN)
    hd = HipDecoder(decoder_weight_dict(_head()))

    def attempts():
        with pytest.raises((SmokeHipError, ValueError)):
            dec.forward(arena, 1, 24)
        with pytest.raises((SmokeHipError, ValueError)):
            dec.forward(arena, 1, 8)
        with pytest.raises((SmokeHipError, ValueError)):
            dec.forward(arena, 1, 32, tokens_ptr=arena.ptr("tokens") + 4)
        with pytest.raises((SmokeHipError, ValueError)):
            dec.forward(arena, 0, 32)
        with pytest.raises((SmokeHipError, ValueError)):
            hd(torch.zeros(1, 1000, 64, device="cuda"))
    kernels, _ = launched_kernels(attempts)
    assert kernels == set()
    assert arena.guard_damage(FILL_NAN, also=("tokens",) + STAGES) == 0


# ------------------------------------------------------------------------------------------------ part 2: the whole model
@functools.lru_cache(maxsize=None)
def _model():
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    return SmokePhysNet().cuda().eval()


def test_whole_model_at_the_first_og8_batch():
    """16 frames of 128^2: the default route (decoder in its OG 8 form) against the linear_dtype='f32' route (PyTorch-ROCm GEMMs and
    modules), all four outputs within 1e-4 max-norm -- the bar and the method of test_hip_body_matches_fp32_torch_body."""
    model = _model()
    assert model.linear_dtype == "bf16x3"
    g = torch.Generator().manual_seed(16)
    x = torch.rand(16, 1, 128, 128, generator=g).cuda()
    noise = torch.randn(len(model.chaos_layers), 3, 16, 1, generator=g).cuda()
    with torch.no_grad():
        kernels, hip = launched_kernels(lambda: model(x, return_features=True, chaos_noise=noise))
        model.linear_dtype = "f32"
        try:
            ref = model(x, return_features=True, chaos_noise=noise)
        finally:
            model.linear_dtype = "bf16x3"
    assert "k_convt4s2<64,32,8,true>" in kernels, kernels
    assert len(ref) == 4
    for k in ref:
        assert hip[k].shape == ref[k].shape
        assert rel_err(hip[k].cpu().numpy(), ref[k].cpu().numpy()) < 1e-4, k


def test_model_with_another_bn_eps_runs_the_modules():
    """k_fold_decoder folds with eps = 1e-5: a head with another eps must not reach it (hip_decoder_supported) and still be computed."""
    model = _model()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(1, 1, 128, 128, generator=g).cuda()
    noise = torch.randn(len(model.chaos_layers), 3, 1, 1, generator=g).cuda()
    bn = model.reconstruction_head[1]
    bn.eps = 1e-3
    try:
        with torch.no_grad():
            kernels, hip = launched_kernels(lambda: model(x, return_features=True, chaos_noise=noise))
            feats = model.output_decoder(hip["intermediate_features"])
            ref = model.reconstruction_head(feats.transpose(1, 2).reshape(1, 64, 32, 32))
    finally:
        bn.eps = 1e-5
    assert kernels == set()
    assert rel_err(hip["reconstructed"].cpu().numpy(), ref.cpu().numpy()) < 1e-4


# ------------------------------------------------------------------------------------------------ part 3: the pooled head
POOLED_CASES = [(1, 1, 4, 1, 1, 4), (2, 100, 132, 37, 3, 140), (3, 31, 512, 256, 3, 512), (2, 33, 256, 8, 5, 260),
                (64, 1024, 512, 256, 3, 512)]


def pooled_references(x, w1, b1, w2, b2):
    """fp64 (pooled, hidden, out) and their elementwise bounds (module docstring).  x [B, L, D] (a view: the padding is not read)."""
    L, D, H1 = x.shape[1], x.shape[2], w1.shape[0]
    xd, w1, b1, w2, b2 = x.double(), w1.double(), b1.double(), w2.double(), b2.double()
    pooled = xd.mean(dim=1)
    e_pooled = ((L + 31) // 32 + 36) * U * xd.abs().mean(dim=1)
    hidden = torch.relu(pooled @ w1.t() + b1)
    e_hidden = (D + 16) * U * (pooled.abs() @ w1.abs().t() + b1.abs()) + e_pooled @ w1.abs().t()
    out = hidden @ w2.t() + b2
    e_out = (H1 + 16) * U * (hidden @ w2.abs().t() + b2.abs()) + e_hidden @ w2.abs().t()
    return (pooled, e_pooled), (hidden, e_hidden), (out, e_out)


@pytest.mark.parametrize("B,L,D,H1,H2,ldx", POOLED_CASES)
def test_pooled_head_at_the_edges_of_its_abi(B, L, D, H1, H2, ldx):
    """smk_pooled_head where its kernels branch: clamped weight rows (H1 not a multiple of 8), empty token chunks (L < 32, L not a
    multiple of ceil(L / 32)), D / 4 not a multiple of 64, a pitched x with NaN in the padding -- and the model's own shape at batch 64."""
    from smokephysai_amd import _lib
    g = torch.Generator().manual_seed(B * 1000 + L + D + H1)
    xbuf = torch.full((B, L, ldx), float("nan"), device="cuda")
    x = xbuf[..., :D]
    x.copy_(torch.randn(B, L, D, generator=g))
    w1, b1 = (torch.randn(H1, D, generator=g) / D ** 0.5).cuda(), (torch.randn(H1, generator=g) * 0.1).cuda()
    w2, b2 = (torch.randn(H2, H1, generator=g) / H1 ** 0.5).cuda(), (torch.randn(H2, generator=g) * 0.1).cuda()
    assert w1.data_ptr() % 16 == 0 and x.stride() == (L * ldx, ldx, 1)
    arena = Arena([("pooled", B * D, 1), ("out", B * H2, 1), ("ws", B * (32 * D + H1), 1)])
    runs = []
    for fill in (FILL_NAN, FILL_ZERO):
        arena.fill(fill)
        _lib.check(_lib.load().smk_pooled_head(x.data_ptr(), B, L, D, ldx, w1.data_ptr(), b1.data_ptr(), H1, w2.data_ptr(), b2.data_ptr(), H2,
                                               arena.ptr("pooled"), arena.ptr("out"), arena.ptr("ws"), _lib.stream_ptr(x.device)))
        torch.cuda.synchronize()
        assert arena.guard_damage(fill) == 0
        runs.append({k: arena.view(k).clone() for k in ("pooled", "out", "ws")})
    for k in ("pooled", "out", "ws"):                   # (every workspace word is written: chunk sums, then the hidden vector)
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), k
        assert not bool(torch.isnan(runs[0][k]).any()), k
    pooled, out = runs[0]["pooled"].view(B, D), runs[0]["out"].view(B, H2)
    hidden = runs[0]["ws"][B * 32 * D:].view(B, H1)
    (p64, e_p), (h64, e_h), (o64, e_o) = pooled_references(x, w1, b1, w2, b2)
    worst = (assert_within(pooled, p64, e_p, "pooled"), assert_within(hidden, h64, e_h, "hidden"), assert_within(out, o64, e_o, "out"))
    print(f"pooled head B={B} L={L} D={D} H1={H1} H2={H2} ldx={ldx}: worst err / bound pooled {worst[0]:.3f}, hidden {worst[1]:.3f}, "
          f"out {worst[2]:.3f}")
    assert rel_err(pooled.cpu().numpy(), p64.cpu().numpy()) < 1e-6
    assert rel_err(out.cpu().numpy(), o64.cpu().numpy()) < 1e-5


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "child", "usage: test_hip_decoder.py child DIR"
    child_main(sys.argv[2])
