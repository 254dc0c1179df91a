"""Case tables and checks of tests/test_hip_attention_variants.py: every instantiation of the attention and LayerNorm kernels of
csrc/transformer.hip that its launchers pick (launch_attention_x3_t, launch_attention_bwd_x3, launch_attn_delta, launch_layernorm,
launch_layernorm_bwd), each reached by a row of the tables below, each checked element by element against fp64 with NaN-poisoned input
padding, sentinel-filled output padding and a repeated call.  Which kernel ran is read from the profiler.

Attention bound (element by element, against softmax attention in fp64).  The kernel works in log2 units: q' = q * scale * log2(e), scores
s_ij = q'_i . k_j, p_ij = 2^(s_ij - m_i).  A split-bf16 operand x = hi + lo misses x by at most 2^-16 |x| and the dropped lo * lo is at most
2^-16 of the product, so each of the 64 products of a score is off by 3 * 2^-16 of its magnitude; the MFMA accumulation of 3 * 64 of them adds
at most 200 * 2^-24 of the same sum:
    |ds_ij| <= 2^-14 A_ij + 2^-23 |s_ij - m_i|,   A_ij = |q'_i| . |k_j|        (2^-23: the fp32 s - m in front of exp2)
A score error moves the output by ln 2 sum_j p_ij (v_j - o_i) ds_ij (the derivative of a base-2 softmax); exp2 adds a relative 2^-22 to each
p, which moves the output by sum_j p_ij (v_j - o_i) 2^-22.  The P V products carry the same 3 * 2^-16 split error, and fp32 accumulation adds
at most (L / 4 + 80) 2^-24 of sum_j p_ij |v_j| (3 L / 16 MFMA updates and L / 64 rescales per output, the row sum l with L / 32 + 40
roundings, the split merges); normalising adds 2^-22 |o|:
    |o_id - ref| <= sum_j p_ij |v_jd - o_id| (1.1 ln 2 |ds_ij| + 2^-22) + (3 * 2^-16 + (L / 4 + 80) 2^-24) sum_j p_ij |v_jd| + 2^-22 |o_id|
(1.1: room for the second-order terms).  lse_i = m_i + log2 l_i (AttnArgs::lse: log2 of sum_j 2^(s_ij)) moves by sum_j p_ij ds_ij, by the
relative error of l over ln 2, and by the roundings of log2 and of the sum:
    |lse_i - ref| <= 1.1 sum_j p_ij |ds_ij| + (2^-22 + (L / 32 + 80) 2^-24) / ln 2 + 2^-21 + 2^-23 (|lse_i| + |m_i|)
No GPU measured these constants: they are derived.  The global max-norm rel_err < 5e-5 of the existing tests at this score spread stays
beside the bound.

LayerNorm bound (k_layernorm: one wave per row, pivot p = x[row][0]).  The kernel sums xs = x - p (NV float4 per lane, then a six-level
butterfly: every term passes at most NV + 9 roundings, the subtraction included), so mean - p is off by dm = (NV + 10) 2^-24 mean|xs|; each
d = xs - (mean - p) by dm + 2^-24 (|xs| + |d|).  The variance sum has the same depth plus the square, and its rounded d add 2 * 2^-24
sum |d| (|xs| + |d|); / D and + eps two roundings more; sqrt and the reciprocal a relative 2^-22 together:
    dvar = (NV + 9) 2^-24 var + 2 * 2^-24 mean(|d| (|xs| + |d|)) + 2 * 2^-24 (var + eps),   e_r = dvar / (2 (var + eps)) + 2^-22
    |y - ref| <= |w| (rstd |dd| + |xhat| (e_r + 2^-24)) + 2^-24 (|xhat w| + |y|)
The backward is held to the existing tests' rel_err < 1e-5 for dx, dw and db."""
import math
import os
import re
import sys
from dataclasses import dataclass
from typing import Optional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch            # noqa: E402

CUS = 256               # the table's shapes are derived for this many CUs (MI355X)


# ------------------------------------------------------------------------------------------------ kernel names
def _b(x):
    return str(bool(x)).lower()


def att(ks, sb=False, kvs=False):
    return f"k_attention_x3<{ks},{_b(sb)},{_b(kvs)}>"


def att_bwd(dkv):
    return f"k_attention_bwd_x3<{_b(dkv)}>"


def ln(nv):
    return f"k_layernorm<{nv}>"


def ln_bwd(nv):
    return f"k_layernorm_bwd<{nv}>"


COMBINE, DELTA, LN_FINISH = "k_attention_combine", "k_attn_delta", "k_layernorm_bwd_finish"

_TEMPLATED = "k_attention_x3|k_attention_bwd_x3|k_layernorm_bwd|k_layernorm"
_PLAIN = "k_attention_combine|k_attn_delta|k_layernorm_bwd_finish"
_DEMANGLED = re.compile(rf"\b({_TEMPLATED})<([^<>]*)>")
_DEMANGLED_PLAIN = re.compile(rf"\b({_PLAIN})\(")
_MANGLED = re.compile(rf"\d+({_TEMPLATED})I((?:L[ib]n?\d+E)+)E")
_MANGLED_PLAIN = re.compile(rf"\d+({_PLAIN})E")


def parse_kernel(name: str) -> Optional[str]:
    """A trace event's name -> the canonical form above, from either the demangled ('void smk::k_attention_x3<1, false, true>(smk::AttnArgs)')
    or the mangled ('_ZN3smk14k_attention_x3ILi1ELb0ELb1EEEvNS_8AttnArgsE') spelling; None for any other name."""
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
    m = _DEMANGLED_PLAIN.search(name) or _MANGLED_PLAIN.search(name)
    return m.group(1) if m else None


def launched_kernels(fn):
    """(the transformer.hip kernels the GPU ran during fn(), fn's result), by name from the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    return {k for k in (parse_kernel(e.name) for e in prof.events()) if k}, res


def attention_env() -> dict:
    """The diagnostic dispatch switches of launch_attention_x3_t (read once per process): the table needs them unset."""
    return {k: v for k, v in os.environ.items() if k in ("SMK_ATTN_SPLIT", "SMK_ATTN_KS", "SMK_ATTN_SB")}


# ------------------------------------------------------------------------------------------------ the tables
@dataclass(frozen=True)
class FwdCase:
    kernel: str                       # the unsplit instantiation: split-bf16 output, forward_lse, and fp32 output when nsplit == 1
    B: int
    L: int
    H: int
    nsplit: int = 1                   # fp32 output with the workspace the library asks for: keys dealt to nsplit workgroups + combine

    @property
    def kvs(self):
        return self.kernel.endswith("true>")

    @property
    def ws_kernels(self):
        return {att(2, False, self.kvs), COMBINE} if self.nsplit > 1 else {self.kernel}

    @property
    def name(self):
        return f"{self.kernel}:{self.B}x{self.L}x{self.H}" + (f"-split{self.nsplit}" if self.nsplit > 1 else "") + ("-kvsplit" if self.kvs else "")


def forward_route(B, L, H, kvs, cus=CUS):
    """(nsplit, unsplit instantiation) that launch_attention_x3_t picks, restated for the table test: nwg = B H L / 128 workgroups; keys split
    while nwg * 2n <= cus and every wave group keeps whole key tiles; KS = 2 when nwg <= cus; the single LDS buffer when nwg > 2 cus."""
    nwg = B * H * (L // 128)
    n = 1
    while n < 8 and nwg * n * 2 <= cus and (L // 64) % (n * 4) == 0:
        n *= 2
    if nwg <= cus and (L // 64) % 2 == 0:
        return n, att(2, False, kvs)
    return n, att(1, nwg > 2 * cus, kvs)


def _fwd(kvs):
    return (
        # split keys + k_attention_combine (hip_attention's workspace): nwg 64 -> 4 splits, 128 -> 2, 32 -> 8 (NT = 2 tiles per wave group)
        FwdCase(att(2, False, kvs), 1, 1024, 8, nsplit=4),
        FwdCase(att(2, False, kvs), 2, 1024, 8, nsplit=2),
        FwdCase(att(2, False, kvs), 1, 2048, 2, nsplit=8),
        # two wave groups, no split: nwg 256 = CUs (2 * 256 > 256); 3 workgroups (L / 64 = 6 is no multiple of 4), NT = 3, grid % 8 != 0; NT = 1
        FwdCase(att(2, False, kvs), 4, 1024, 8),
        FwdCase(att(2, False, kvs), 1, 384, 1),
        FwdCase(att(2, False, kvs), 1, 128, 8),
        # one group, double buffer: 256 < nwg <= 512 -- the training batch (8 frames: 512), and 261 (grid % 8 != 0, H * 64 = 1,856)
        FwdCase(att(1, False, kvs), 8, 1024, 8),
        FwdCase(att(1, False, kvs), 1, 1152, 29),
        # single buffer: nwg > 512 -- 576, the eval batch (4,096), 575 (L / 64 = 10, H * 64 = 1,472)
        FwdCase(att(1, True, kvs), 9, 1024, 8),
        FwdCase(att(1, True, kvs), 64, 1024, 8),
        FwdCase(att(1, True, kvs), 5, 640, 23),
    )


# each shape with fp32 k | v, then the same shape with k | v in SMK_FMT_SPLIT4_INPLACE (adjacent: they share one input setup)
FWD_CASES = tuple(c for pair in zip(_fwd(False), _fwd(True)) for c in pair)


@dataclass(frozen=True)
class BwdCase:
    B: int
    L: int
    H: int

    @property
    def name(self):
        return f"bwd:{self.B}x{self.L}x{self.H}"


# one 128-row outer block; 3 workgroups (grid % 8 != 0); odd H (k_attn_delta: a second blockIdx.y); the training batch
BWD_CASES = (BwdCase(1, 128, 2), BwdCase(1, 384, 1), BwdCase(2, 256, 11), BwdCase(8, 1024, 8))
BWD_KERNELS = frozenset({att_bwd(True), att_bwd(False)})


@dataclass(frozen=True)
class DeltaCase:
    rows: int
    H: int

    @property
    def name(self):
        return f"delta:{self.rows}x{self.H}"


# k_attn_delta: grid (min(rows / 4, CUs * 32), H / 8): 40,000 rows > 256 * 32 * 4 walk the grid-stride loop, H = 9 and 17 a partial 8-head group
DELTA_CASES = (DeltaCase(40000, 9), DeltaCase(1029, 17))


def ln_nv(D):
    """float4 per lane of launch_layernorm / launch_layernorm_bwd: ceil(D / 256) rounded up to 1, 2, 4 or 8."""
    n = (D + 255) // 256
    return next(v for v in (1, 2, 4, 8) if n <= v)


@dataclass(frozen=True)
class LnCase:
    kernel: str
    rows: int
    D: int

    @property
    def name(self):
        return f"{self.kernel}:{self.rows}x{self.D}"


# NV 1 (4, 64, 132), 2 (512), 4 (516: partial float4 group above NV = 1, 1024), 8 (1028, 2044 partial; 2048 full)
LN_DIMS = (4, 64, 132, 512, 516, 1024, 1028, 2044, 2048)
LN_CASES = tuple(LnCase(ln(ln_nv(D)), rows, D) for D in LN_DIMS for rows in (1, 3, 4099))
# backward: one workgroup (1, 5 rows), LN_BWD_WGS workgroups (4,099 rows), several rows per wave (70,000)
LN_BWD_CASES = tuple(LnCase(ln_bwd(ln_nv(D)), rows, D) for D in LN_DIMS for rows in (1, 5, 4099, 70000))
LN_OFFSET_DIMS = (512, 1024, 2048)

EXPECTED = frozenset({
    att(1), att(1, True), att(2), att(1, kvs=True), att(1, True, True), att(2, kvs=True), COMBINE,
    att_bwd(True), att_bwd(False), DELTA,
    ln(1), ln(2), ln(4), ln(8), ln_bwd(1), ln_bwd(2), ln_bwd(4), ln_bwd(8), LN_FINISH,
})


# ------------------------------------------------------------------------------------------------ shared helpers
SENT32 = 0x7FA5A5A5          # sentinel bits of an fp32 output word (a NaN no kernel writes)
SENT16 = 0x7FA5               # the same for a bf16 word of split output storage (int16)
Q_PAD, K_PAD, V_PAD, IN_TAIL = 12, 20, 8, 3          # pitch padding / rows past the end of the poisoned inputs
O_PAD, O_TAIL, FLAT_TAIL = 16, 5, 37                  # the same for the sentinel outputs; entries past the end of [rows][H] outputs
SCALE = 0.125
LOG2E, LN2, U = 1.4426950408889634, math.log(2.0), 2.0 ** -24


def _lib():
    from smokephysai_amd import _lib as lib
    return lib


def poisoned(x, pad, tail=IN_TAIL, bits=False):
    """x [R, C] copied into a NaN-filled [R + tail, C + pad] buffer; returns the [R, C] view.  bits: copy x's bit patterns (int32), not values."""
    R, C = x.shape
    buf = torch.full((R + tail, C + pad), float("nan"), device=x.device)
    if bits:
        buf.view(torch.int32)[:R, :C] = x.view(torch.int32)
    else:
        buf[:R, :C] = x
    return buf[:R, :C]


def sentinel(*shape, split=False):
    return torch.full(shape, SENT16 if split else SENT32, device="cuda", dtype=torch.int16 if split else torch.int32)


def outside_touched(buf, region, split=False) -> int:
    """Words of buf outside buf[region] that no longer hold the sentinel."""
    chk = buf.clone()
    sent = SENT16 if split else SENT32
    chk[region] = sent
    return int((chk != sent).sum())


def rel(a, b) -> float:
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)                                  # (NaN counts as outside)
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        ratio = (err / bound)[bad].nan_to_num(1e30)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {idx}: got "
                             f"{float(got[tuple(idx)])!r} ref {float(ref[tuple(idx)])!r} bound {float(bound[tuple(idx)]):.3e}; "
                             f"worst err / bound {float(ratio.max()):.3g}")


# ------------------------------------------------------------------------------------------------ attention forward
def attention_reference(q, k, v):
    """fp64 softmax attention of one (batch, head): q [nq, 64], k, v [L, 64] -> (o, o_bound, lse, lse_bound) as the module docstring derives."""
    L = k.shape[0]
    qd = q.double() * (SCALE * LOG2E)
    kd, vd = k.double(), v.double()
    s = qd @ kd.t()
    A = qd.abs() @ kd.abs().t()
    m = s.max(1, keepdim=True).values
    e = torch.exp2(s - m)
    l = e.sum(1, keepdim=True)
    P = e / l
    o = P @ vd
    ds = 2.0 ** -14 * A + 2.0 ** -23 * (s - m).abs()
    W = P * (1.1 * LN2 * ds + 2.0 ** -22)
    t1 = torch.cat([torch.einsum("ij,ijd->id", W[i:i + 64], (vd[None] - o[i:i + 64, None]).abs()) for i in range(0, q.shape[0], 64)])
    o_bound = t1 + (3 * 2.0 ** -16 + (L / 4 + 80) * U) * (P @ vd.abs()) + 2.0 ** -22 * o.abs()
    lse = (m + torch.log2(l)).squeeze(1)
    lse_bound = (1.1 * (P * ds).sum(1) + (2.0 ** -22 + (L / 32 + 80) * U) / LN2 + 2.0 ** -21
                 + 2.0 ** -23 * (lse.abs() + m.squeeze(1).abs()))
    return o, o_bound, lse, lse_bound


def sampled_pairs(B, H):
    """(batch, head) pairs the fp64 reference covers: all of them up to 16, else the first two, the middle two and the last two (the
    all-equal queries sit in the first pair, the peaked ones in the last)."""
    n = B * H
    idx = range(n) if n <= 16 else sorted({0, 1, n // 2 - 1, n // 2, n - 2, n - 1})
    return [(i // H, i % H) for i in idx]


class FwdSetup:
    """Inputs of one (B, L, H): q scaled by 2 (a widened score spread), keys growing along L (the running max moves across tiles and splits),
    queries 0..31 of (batch 0, head 0) all zero (equal scores: the output is the mean of v), the last 32 queries of (batch B-1, head H-1) each
    aimed at one of the last 32 keys (a strongly peaked softmax); q, k, v in NaN-poisoned pitched buffers, k | v also as split4 bits."""

    def __init__(self, B, L, H, seed):
        from smokephysai_amd.models.linear import split4_inplace
        self.B, self.L, self.H = B, L, H
        D, R = 64 * H, B * L
        g = torch.Generator(device="cuda").manual_seed(seed)
        q = torch.randn(B, L, D, device="cuda", generator=g) * 2.0
        k = torch.randn(B, L, D, device="cuda", generator=g) * torch.linspace(0.2, 2.0, L, device="cuda")[None, :, None]
        v = torch.randn(B, L, D, device="cuda", generator=g)
        q[0, :32, :64] = 0.0
        h = slice(64 * (H - 1), 64 * H)
        kk = k[B - 1, L - 32:, h]
        q[B - 1, L - 32:, h] = kk * (60.0 / (SCALE * (kk * kk).sum(1, keepdim=True)))      # natural-log score 60 on its key
        self.q = poisoned(q.view(R, D), Q_PAD)
        self.k32, self.v32 = poisoned(k.view(R, D), K_PAD), poisoned(v.view(R, D), V_PAD)
        self.ks = poisoned(split4_inplace(k.view(R, D)), K_PAD, bits=True)
        self.vs = poisoned(split4_inplace(v.view(R, D)), V_PAD, bits=True)
        self.refs = {}
        for b, hh in sampled_pairs(B, H):
            rows, cols = slice(b * L, (b + 1) * L), slice(64 * hh, 64 * hh + 64)
            self.refs[(b, hh)] = attention_reference(q.view(R, D)[rows, cols], k.view(R, D)[rows, cols], v.view(R, D)[rows, cols])

    def run(self, kvs, split=False, ws=None, lse=False):
        """One call on a fresh sentinel-filled output: fp32 [R + O_TAIL][D + O_PAD] (ldo = D + O_PAD) or split-bf16 [R + O_TAIL][D / 8][2][8];
        ws: the workspace tensor; lse: smk_attention_forward_lse (fp32 k | v) with a sentinel [R H + FLAT_TAIL] lse.  -> (out buffer, lse buffer)"""
        lib = _lib()
        Lh = lib.load()
        B, L, H = self.B, self.L, self.H
        D, R = 64 * H, B * L
        k, v = (self.ks, self.vs) if kvs else (self.k32, self.v32)
        st = lib.stream_ptr(torch.device("cuda"))
        obuf = sentinel(R + O_TAIL, D // 8, 2, 8, split=True) if split else sentinel(R + O_TAIL, D + O_PAD)
        ldo = D if split else D + O_PAD
        if lse:
            lbuf = sentinel(R * H + FLAT_TAIL)
            lib.check(Lh.smk_attention_forward_lse(self.q.data_ptr(), k.data_ptr(), v.data_ptr(), obuf.data_ptr(), lbuf.data_ptr(), B, L, H, 64,
                                                   self.q.stride(0), k.stride(0), v.stride(0), ldo, SCALE, st))
            return obuf, lbuf
        lib.check(Lh.smk_attention_kv(self.q.data_ptr(), k.data_ptr(), v.data_ptr(), obuf.data_ptr(), B, L, H, 64, self.q.stride(0), k.stride(0),
                                      v.stride(0), ldo, SCALE, lib.SMK_FMT_SPLIT_BF16 if split else lib.SMK_FMT_F32,
                                      lib.SMK_FMT_SPLIT4_INPLACE if kvs else lib.SMK_FMT_F32, None if ws is None else ws.data_ptr(),
                                      0 if ws is None else ws.numel(), st))
        return obuf, None

    def check_out(self, obuf, what):
        """The fp32 output against the fp64 reference (every sampled pair, element by element), global rel_err, sentinel outside [R][D]."""
        L, D, R = self.L, 64 * self.H, self.B * self.L
        o = obuf.view(torch.float32)[:R, :D]
        worst, top = 0.0, 0.0
        for (b, h), (ref, bound, _, _) in self.refs.items():
            got = o[b * L:(b + 1) * L, 64 * h:64 * h + 64]
            assert_within(got, ref, bound, f"{what} (batch {b}, head {h})")
            worst = max(worst, float((got.double() - ref).abs().max()))
            top = max(top, float(ref.abs().max()))
        assert worst / top < 5e-5, f"{what}: global rel_err {worst / top:.3e}"
        n = outside_touched(obuf, (slice(0, R), slice(0, D)))
        assert n == 0, f"{what}: {n} words outside [B L][H 64] overwritten"

    def check_lse(self, lbuf, what):
        L, H, R = self.L, self.H, self.B * self.L
        lse = lbuf.view(torch.float32)[:R * H].view(R, H)
        for (b, h), (_, _, ref, bound) in self.refs.items():
            assert_within(lse[b * L:(b + 1) * L, h], ref, bound, f"{what} lse (batch {b}, head {h})")
        n = outside_touched(lbuf, slice(0, R * H))
        assert n == 0, f"{what}: {n} lse words past B L H overwritten"


_fwd_setup = {}


def fwd_setup(case: FwdCase) -> FwdSetup:
    key = (case.B, case.L, case.H)
    if key not in _fwd_setup:
        _fwd_setup.clear()                                  # (the fp32 | split4 twins are adjacent in FWD_CASES: keep one setup)
        _fwd_setup[key] = FwdSetup(*key, seed=case.B * 1000 + case.L + case.H)
    return _fwd_setup[key]


def check_forward(case: FwdCase, want_kernel: bool = True) -> set:
    """Runs one forward row four ways and asserts, for each, the fp64 bound, the untouched sentinel padding and (want_kernel) the kernels:
      fp32 output with the workspace the library asks for (split + combine when nsplit > 1), repeated bit for bit;
      fp32 output without a workspace (the unsplit kernel), repeated bit for bit;
      split-bf16 output: bit for bit the hi / lo split of the unsplit fp32 output;
      smk_attention_forward_lse (fp32 k | v only): the unsplit output bit for bit, plus lse against fp64, repeated bit for bit;
    and for k | v in SMK_FMT_SPLIT4_INPLACE every output bit for bit the fp32 k | v route's.  Returns every kernel that ran."""
    from smokephysai_amd.models.linear import to_split
    s = fwd_setup(case)
    B, L, H = case.B, case.L, case.H
    D, R = 64 * H, B * L
    ws_bytes = int(_lib().load().smk_attention_workspace_bytes(B, L, H, 64))
    ws = torch.full((ws_bytes,), 0xFF, device="cuda", dtype=torch.uint8) if ws_bytes else None      # NaN-filled
    seen = set()

    def expect(kernels, want, what):
        seen.update(kernels)
        if want_kernel:
            assert kernels == want, f"{case.name} {what}: launched {sorted(kernels)}, expected {sorted(want)}"

    if want_kernel:
        assert (ws_bytes > 0) == (case.nsplit > 1), f"{case.name}: workspace {ws_bytes} bytes"
    k, (o_ws, _) = launched_kernels(lambda: s.run(case.kvs, ws=ws))
    expect(k, case.ws_kernels, "fp32 out + workspace")
    s.check_out(o_ws, f"{case.name} fp32 out + workspace")
    assert torch.equal(o_ws, s.run(case.kvs, ws=ws)[0]), f"{case.name}: a second call with the workspace differs"

    k, (o_pl, _) = launched_kernels(lambda: s.run(case.kvs))
    expect(k, {case.kernel}, "fp32 out")
    s.check_out(o_pl, f"{case.name} fp32 out")
    assert torch.equal(o_pl, s.run(case.kvs)[0]), f"{case.name}: a second call differs"
    if case.nsplit == 1:
        assert torch.equal(o_ws, o_pl), f"{case.name}: no split, yet the workspace changed the output"

    k, (o_sp, _) = launched_kernels(lambda: s.run(case.kvs, split=True))
    expect(k, {case.kernel}, "split-bf16 out")
    n = outside_touched(o_sp, slice(0, R), split=True)
    assert n == 0, f"{case.name} split-bf16 out: {n} words past row B L overwritten"
    want = to_split(o_pl.view(torch.float32)[:R, :D]).view(torch.int16)
    assert torch.equal(o_sp[:R], want), f"{case.name}: split-bf16 output differs from the split of the fp32 output in {int((o_sp[:R] != want).sum())} words"

    if case.kvs:                                           # the fp32 k | v twin: the same bits on every route
        assert torch.equal(o_ws, s.run(False, ws=ws)[0]) and torch.equal(o_pl, s.run(False)[0]), f"{case.name}: differs from the fp32 k | v route"
        assert torch.equal(o_sp, s.run(False, split=True)[0]), f"{case.name}: split-bf16 output differs from the fp32 k | v route"
    else:
        k, (o_l, lse) = launched_kernels(lambda: s.run(False, lse=True))
        expect(k, {case.kernel}, "forward_lse")
        assert torch.equal(o_l, o_pl), f"{case.name}: forward_lse output differs from the plain call"
        s.check_lse(lse, f"{case.name} forward_lse")
        assert torch.equal(lse, s.run(False, lse=True)[1]), f"{case.name}: a second forward_lse call differs in lse"
    return seen


# ------------------------------------------------------------------------------------------------ attention backward + delta
def delta_bound(dout, out, H):
    """fp64 rowsum(dout * out) per head and its bound: 8 fp32 roundings deep (the products, a three-level tree per lane, three shuffles)."""
    R = dout.shape[0]
    p = dout.double() * out.double()
    return p.view(R, H, 64).sum(-1), 8 * U * p.abs().view(R, H, 64).sum(-1)


def run_delta(dout, out, H):
    """smk_attention_delta into a sentinel [rows H + FLAT_TAIL] buffer -> the buffer."""
    lib = _lib()
    R = dout.shape[0]
    dbuf = sentinel(R * H + FLAT_TAIL)
    lib.check(lib.load().smk_attention_delta(dout.data_ptr(), out.data_ptr(), R, H, 64, dout.stride(0), out.stride(0), dbuf.data_ptr(),
                                             lib.stream_ptr(torch.device("cuda"))))
    return dbuf


def check_delta_result(dbuf, dout, out, H, what):
    R = dout.shape[0]
    ref, bound = delta_bound(dout, out, H)
    assert_within(dbuf.view(torch.float32)[:R * H].view(R, H), ref, bound, what)
    n = outside_touched(dbuf, slice(0, R * H))
    assert n == 0, f"{what}: {n} words past rows * H overwritten"


def check_delta(case: DeltaCase, want_kernel: bool = True) -> set:
    """k_attn_delta on pitched, NaN-poisoned dout / out: element by element against fp64, sentinel past [rows][H], repeated bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(case.rows + case.H)
    D = 64 * case.H
    dout = poisoned(torch.randn(case.rows, D, device="cuda", generator=g), 12)
    out = poisoned(torch.randn(case.rows, D, device="cuda", generator=g), 20)
    k, dbuf = launched_kernels(lambda: run_delta(dout, out, case.H))
    if want_kernel:
        assert k == {DELTA}, f"{case.name}: launched {sorted(k)}"
    check_delta_result(dbuf, dout, out, case.H, case.name)
    assert torch.equal(dbuf, run_delta(dout, out, case.H)), f"{case.name}: a second call differs"
    return k


def check_backward(case: BwdCase, want_kernel: bool = True) -> set:
    """The training route of _HipQKVAttentionFn: q | k | v and dq | dk | dv as column slices of one [B L][3 H 64 + pad] buffer each (inputs
    NaN-poisoned past 3 H 64 and past row B L, outputs sentinel-filled), the forward's own lse and delta.  dq, dk, dv and the forward output
    against fp64 autograd (rel_err < 2e-5, the existing bar), delta element by element, untouched sentinels, a bit-identical repeat."""
    lib = _lib()
    Lh = lib.load()
    B, L, H = case.B, case.L, case.H
    D, R = 64 * H, B * L
    st = lib.stream_ptr(torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + L + H)
    qkv_v = torch.randn(R, 3 * D, device="cuda", generator=g)
    dout = poisoned(torch.randn(R, D, device="cuda", generator=g), 12)
    qkv = poisoned(qkv_v, 16)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    ldi = qkv.stride(0)
    out = poisoned(torch.zeros(R, D, device="cuda"), 8)
    lse = torch.full((R * H,), float("nan"), device="cuda")
    lib.check(Lh.smk_attention_forward_lse(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, H, 64, ldi, ldi, ldi,
                                           out.stride(0), SCALE, st))
    kd, dbuf = launched_kernels(lambda: run_delta(dout, out, H))
    check_delta_result(dbuf, dout, out, H, f"{case.name} delta")
    delta = dbuf.view(torch.float32)[:R * H]
    seen = set(kd)

    def bwd():
        buf = sentinel(R + O_TAIL, 3 * D + 24)
        d = buf.view(torch.float32)
        ldd = d.stride(0)
        lib.check(Lh.smk_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                            d[:, :D].data_ptr(), d[:, D:].data_ptr(), d[:, 2 * D:].data_ptr(), B, L, H, 64, ldi, ldi, ldi,
                                            dout.stride(0), ldd, ldd, ldd, SCALE, st))
        return buf
    kb, gbuf = launched_kernels(bwd)
    seen |= kb
    if want_kernel:
        assert kd == {DELTA} and kb == BWD_KERNELS, f"{case.name}: launched {sorted(kd)} + {sorted(kb)}"
    n = outside_touched(gbuf, (slice(0, R), slice(0, 3 * D)))
    assert n == 0, f"{case.name}: {n} words outside [B L][3 H 64] overwritten"
    assert torch.equal(gbuf, bwd()), f"{case.name}: a second backward call differs"

    x = qkv_v.double().requires_grad_(True)
    q64, k64, v64 = (x[:, i * D:(i + 1) * D].reshape(B, L, H, 64).transpose(1, 2) for i in range(3))
    p = torch.softmax(q64 @ k64.transpose(-1, -2) * SCALE, dim=-1)
    ref = (p @ v64).transpose(1, 2).reshape(R, D)
    ref.backward(dout.double())
    e = rel(out, ref.detach())
    assert e < 2e-5, f"{case.name}: forward rel_err {e:.3e}"
    got = gbuf.view(torch.float32)[:R, :3 * D]
    for i, nm in enumerate(("dq", "dk", "dv")):
        e = rel(got[:, i * D:(i + 1) * D], x.grad[:, i * D:(i + 1) * D])
        assert e < 2e-5, f"{case.name}: {nm} rel_err {e:.3e}"
    return seen


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_inputs(rows, D, seed):
    """Rows of varied scale and offset (x = N(0, s^2) + c, s in [0.5, 2.5], c ~ N(0, 9)), weight and bias."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, D, device="cuda", generator=g) * (torch.rand(rows, 1, device="cuda", generator=g) * 2 + 0.5) \
        + torch.randn(rows, 1, device="cuda", generator=g) * 3
    return x, torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)


def ln_poisoned(x):
    """x in a NaN-filled pitched buffer (pad 12) with at least 2,048 NaN floats behind its last row."""
    return poisoned(x, 12, tail=2048 // (x.shape[1] + 12) + 2)


def layernorm_bound(x, w, b, eps=1e-5):
    """fp64 LayerNorm of the rows x [rows, D] and the bound of the module docstring."""
    D = x.shape[1]
    nv = ln_nv(D)
    xd, wd, bd = x.double(), w.double(), b.double()
    xs = xd - xd[:, :1]
    d = xs - xs.mean(1, keepdim=True)
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = d * rstd
    y = xhat * wd + bd
    dd = (nv + 10) * U * xs.abs().mean(1, keepdim=True) + U * (xs.abs() + d.abs())
    dvar = (nv + 9) * U * var + 2 * U * (d.abs() * (xs.abs() + d.abs())).mean(1, keepdim=True) + 2 * U * (var + eps)
    e_r = dvar / (2 * (var + eps)) + 2.0 ** -22
    bound = wd.abs() * (rstd * dd + xhat.abs() * (e_r + U)) + U * ((xhat * wd).abs() + y.abs())
    return y, bound


def run_layernorm(x, w, b, split=False):
    """smk_layernorm into a fresh sentinel buffer: fp32 [rows + O_TAIL][D + 20] or split-bf16 [rows + O_TAIL][D / 8][2][8]."""
    lib = _lib()
    rows, D = x.shape
    buf = sentinel(rows + O_TAIL, D // 8, 2, 8, split=True) if split else sentinel(rows + O_TAIL, D + 20)
    lib.check(lib.load().smk_layernorm(x.data_ptr(), rows, D, x.stride(0), w.data_ptr(), b.data_ptr(), 1e-5, buf.data_ptr(),
                                       D if split else D + 20, lib.SMK_FMT_SPLIT_BF16 if split else lib.SMK_FMT_F32,
                                       lib.stream_ptr(torch.device("cuda"))))
    return buf


def check_layernorm(case: LnCase, want_kernel: bool = True) -> set:
    """k_layernorm on a pitched NaN-poisoned x: y element by element against fp64, sentinel outside [rows][D], a bit-identical repeat, and
    (D % 8 == 0) the split-bf16 output bit for bit the split of the fp32 output."""
    from smokephysai_amd.models.linear import to_split
    rows, D = case.rows, case.D
    x, w, b = ln_inputs(rows, D, rows * 7 + D)
    xp = ln_poisoned(x)
    k, buf = launched_kernels(lambda: run_layernorm(xp, w, b))
    if want_kernel:
        assert k == {case.kernel}, f"{case.name}: launched {sorted(k)}"
    ref, bound = layernorm_bound(x, w, b)
    y = buf.view(torch.float32)[:rows, :D]
    assert_within(y, ref, bound, case.name)
    n = outside_touched(buf, (slice(0, rows), slice(0, D)))
    assert n == 0, f"{case.name}: {n} words outside [rows][D] overwritten"
    assert torch.equal(buf, run_layernorm(xp, w, b)), f"{case.name}: a second call differs"
    if D % 8 == 0:
        ks, sbuf = launched_kernels(lambda: run_layernorm(xp, w, b, split=True))
        if want_kernel:
            assert ks == {case.kernel}, f"{case.name} split: launched {sorted(ks)}"
        n = outside_touched(sbuf, slice(0, rows), split=True)
        assert n == 0, f"{case.name} split: {n} words past row {rows} overwritten"
        assert torch.equal(sbuf[:rows], to_split(y).view(torch.int16)), f"{case.name}: split-bf16 output differs from the split of the fp32 output"
    return k


def run_layernorm_bwd(x, dy, w):
    """smk_layernorm_backward: dx into a sentinel [rows + O_TAIL][D + 20], dw | db into one sentinel [2 (D + 12)] (gap after each), workspace
    NaN-filled -> (dx buffer, dw | db buffer)."""
    lib = _lib()
    Lh = lib.load()
    rows, D = x.shape
    dxb = sentinel(rows + O_TAIL, D + 20)
    wb = sentinel(2 * (D + 12))
    ws = torch.full((int(Lh.smk_layernorm_bwd_workspace(D)) // 4,), float("nan"), device="cuda")
    f = wb.view(torch.float32)
    lib.check(Lh.smk_layernorm_backward(x.data_ptr(), dy.data_ptr(), rows, D, x.stride(0), dy.stride(0), w.data_ptr(), 1e-5, dxb.data_ptr(),
                                        D + 20, f[:D].data_ptr(), f[D + 12:].data_ptr(), ws.data_ptr(), lib.stream_ptr(torch.device("cuda"))))
    return dxb, wb


def layernorm_grads(x, dy, w, b, eps=1e-5):
    """fp64 autograd of F.layer_norm: (dx, dw, db)."""
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    torch.nn.functional.layer_norm(x64, (x.shape[1],), w64, b64, eps).backward(dy.double())
    return x64.grad, w64.grad, b64.grad


def check_layernorm_bwd(case: LnCase, want_kernel: bool = True) -> set:
    """k_layernorm_bwd + k_layernorm_bwd_finish on pitched NaN-poisoned x and dy: dx, dw, db against fp64 autograd (rel_err < 1e-5, the existing
    bar), sentinel outside dx [rows][D] and between / after dw and db, a bit-identical repeat."""
    rows, D = case.rows, case.D
    x, _, _ = ln_inputs(rows, D, rows * 13 + D)
    g = torch.Generator(device="cuda").manual_seed(rows + D)
    w = torch.rand(D, device="cuda", generator=g) + 0.5
    dy = torch.randn(rows, D, device="cuda", generator=g)
    xp, dyp = ln_poisoned(x), poisoned(dy, 20)
    k, (dxb, wb) = launched_kernels(lambda: run_layernorm_bwd(xp, dyp, w))
    if want_kernel:
        assert k == {case.kernel, LN_FINISH}, f"{case.name}: launched {sorted(k)}"
    rdx, rdw, rdb = layernorm_grads(x, dy, w, torch.zeros_like(w))
    f = wb.view(torch.float32)
    for nm, got, ref in (("dx", dxb.view(torch.float32)[:rows, :D], rdx), ("dw", f[:D], rdw), ("db", f[D + 12:2 * D + 12], rdb)):
        e = rel(got, ref)
        assert e < 1e-5, f"{case.name}: {nm} rel_err {e:.3e}"
    n = outside_touched(dxb, (slice(0, rows), slice(0, D)))
    assert n == 0, f"{case.name}: {n} dx words outside [rows][D] overwritten"
    n = int((wb[D:D + 12] != SENT32).sum()) + int((wb[2 * D + 12:] != SENT32).sum())
    assert n == 0, f"{case.name}: {n} words beside dw / db overwritten"
    dxb2, wb2 = run_layernorm_bwd(xp, dyp, w)
    assert torch.equal(dxb, dxb2) and torch.equal(wb, wb2), f"{case.name}: a second call differs"
    return k


def offset_row_errors(D, rows=1029):
    """Rows whose mean dwarfs their spread (the fused LayerNorm test's rows: 50 + 0.1 randn, every 7th -300 + 0.01 randn): max-norm relative
    errors of y, dx, dw and db against fp64."""
    g = torch.Generator(device="cuda").manual_seed(D)
    x = 50.0 + 0.1 * torch.randn(rows, D, device="cuda", generator=g)
    x[::7] = -300.0 + 0.01 * torch.randn(x[::7].shape, device="cuda", generator=g)
    w = torch.rand(D, device="cuda", generator=g) + 0.5
    b = torch.randn(D, device="cuda", generator=g) * 0.3
    dy = torch.randn(rows, D, device="cuda", generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5)
    y = run_layernorm(x, w, b).view(torch.float32)[:rows, :D]
    dxb, wb = run_layernorm_bwd(x, dy, w)
    rdx, rdw, rdb = layernorm_grads(x, dy, w, b)
    f = wb.view(torch.float32)
    return {"y": rel(y, ref), "dx": rel(dxb.view(torch.float32)[:rows, :D], rdx), "dw": rel(f[:D], rdw), "db": rel(f[D + 12:2 * D + 12], rdb)}
