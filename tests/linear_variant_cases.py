"""Case table and checks of tests/test_hip_linear_variants.py: every forward instantiation that launch_linear_x3 (csrc/linear.hip) picks,
each reached by a row of the table below, each checked four ways (see check_case).  Also runs on its own, in a fresh process, for the
instantiations that only an SMK_LINEAR_* variable reaches (they are read once per process):

    SMK_LINEAR_KS=2 python tests/linear_variant_cases.py KS2

prints one JSON line {"setting", "ok", "cases": [{"name", "kernels"}]} and exits non-zero when a check fails.

Error bound (element by element, against the same chain in fp64).  A split-bf16 operand v = hi + lo (hi = RNE_bf16(v), lo =
RNE_bf16(v - hi)) misses v by at most 2^-8 |v - hi| <= 2^-17 |v|; the kernel sums hi*hi + hi*lo + lo*hi, dropping lo*lo <= 2^-16 |x w|.
Per product that is |x w| (2 * 2^-17 + 2^-16 + 2^-32) ~ 2^-15 |x w|, exact in fp32 (bf16 x bf16); accumulating K such products in fp32
adds at most K * 2^-24 of sum |x w| (the gamma_K bound), the epilogue's roundings (bias, addend, folded fp32 weights) a few 2^-24 more:
    |y - ref| <= c * (|x^| @ |W|^T) + 2^-22 |b|,   c = 2^-14 + (K + 16) * 2^-24      (2^-14: twice the product term)
x^ is the GEMM's actual operand: x itself (x_split: the decoded hi + lo it was given).  For the fused LayerNorm the kernel multiplies the
pivot-shifted row x - p (p = x[row][0]) by W' = W diag(gamma) and forms rstd ((x - p) W'^T - (mean - p) wsum) + b', so its operand sum is
    A = rstd (|x - p| @ |W'|^T) + rstd (|mean - p| + mean_k |x - p|) |wsum|
(the second term: the correction's product and the fp32 error of the row sum S1 times wsum), and the statistics add a relative error
(1 + z^2) (K / 64 + 16) 2^-24 of |x^ W'^T| (S2 summed in fp32 over K / 64 chunk steps and a 16-lane tree; var = S2 / K - (mean - p)^2
cancels by 1 + z^2, z = |mean - p| rstd).  The bound is applied before the activation and carried through it with the slope bound
(GELU <= 1.13, ReLU 1) plus the erf approximation's 2^-20 |pre|; residual and addend add their fp32 rounding (2^-23 of the operands),
a split-bf16 output its decode error (2^-16 |y|).  No GPU measured c: it is derived.  The global max-norm rel_err < 2e-5 stays beside it:
it sees a systematic loss (a dropped hi * lo product is 2^-9 of every element, inside the elementwise bound at K = 2,048)."""
import json
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
def x3(mb, nw, as_=False, ks=1, ring=4, lnf=False):
    return f"k_linear_x3<{mb},{nw},{str(as_).lower()},{ks},{ring},{str(lnf).lower()}>"


def b16(nw, r, lnf=False, conv=0):
    return f"k_linear_b16<{nw},{conv},{r},{str(lnf).lower()}>"


_DEMANGLED = re.compile(r"(k_linear_x3|k_linear_b16)<([^<>]*)>")
_MANGLED = re.compile(r"\d+(k_linear_x3|k_linear_b16)I((?:L[ib]n?\d+E)+)E")


def parse_kernel(name: str) -> Optional[str]:
    """A trace event's name -> the canonical form above, from either the demangled ('void smk::k_linear_x3<4, 8, false, 1, 4, true>
    (smk::LinearArgs)') or the mangled ('_ZN3smk11k_linear_x3ILi4ELi8ELb0ELi1ELi4ELb1EEEvNS_10LinearArgsE') spelling; None otherwise."""
    m = _DEMANGLED.search(name)
    if m:
        args = []
        for a in m.group(2).split(","):
            a = a.strip()
            a = re.sub(r"^\((?:int|bool)\)", "", a)         # (some demanglers print casts)
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


def launched_kernels(fn) -> set:
    """The linear-layer kernels the GPU ran during fn(), by name from the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {k for k in (parse_kernel(e.name) for e in prof.events()) if k}


# ------------------------------------------------------------------------------------------------ the table
@dataclass(frozen=True)
class Case:
    kernel: str                       # the instantiation this row must reach (256 CUs)
    M: int
    K: int
    N: int
    act: Optional[str] = None
    res: Optional[str] = None         # None | "res" (separate pitched tensor) | "inplace" (out aliases the residual)
    rpg: int = 0                      # periodic addend [M / rpg, 5, N] when > 0
    x_split: bool = False
    out_split: bool = False
    ln: bool = False                  # HipLinearLN.forward_ln (LayerNorm fused in front)
    split_from: Optional[int] = None  # forward_ln: columns >= split_from written as SMK_FMT_SPLIT4_INPLACE

    @property
    def name(self):
        f = [f"{self.M}x{self.K}->{self.N}"]
        for k in ("act", "res"):
            if getattr(self, k):
                f.append(f"{getattr(self, k)}")
        if self.rpg:
            f.append(f"padd{self.rpg}")
        if self.x_split:
            f.append("xsplit")
        if self.out_split:
            f.append("ysplit")
        if self.ln:
            f.append("ln")
        if self.split_from is not None:
            f.append(f"sf{self.split_from}")
        return self.kernel + ":" + "-".join(f)


# Derived from launch_linear_x3 at 256 CUs (the comment of each row: the deciding quantities).  N = 1056 / 288 / 480 / 224 / 160 / 96 leave a
# partial last column tile (256- or 128-column tiles); M = 8100, 16300, 33001, 4090, 1000, ... a ragged last row tile.
DEFAULT_CASES = (
    # fp32 in / out, 128-row tiles: k_linear_b16.  nw = 8: N >= 256 and cdiv(M,128) cdiv(N,256) >= 256; R = 4: K / 64 even
    Case(b16(8, 4), 8100, 128, 1056, act="gelu"),                               # 64 x 5 = 320 tiles
    Case(b16(8, 4), 8192, 256, 2048, rpg=1024),                                 # 64 x 8; addend groups of 1,024 rows
    Case(b16(4, 4), 16300, 256, 160, act="relu", res="res"),                    # N < 256: nw = 4, 128 x 2 = 256 tiles at mb = 4
    Case(b16(8, 2), 16300, 192, 288, res="inplace"),                            # K / 64 = 3 odd: R = 2
    Case(b16(4, 2), 32700, 64, 96, act="gelu"),                                 # K = 64: R = 2; 256 x 1 tiles
    # split-bf16 input: k_linear_x3<.., AS = true>, row blocks falling with M
    Case(x3(4, 8, True), 8100, 128, 1056, act="gelu", x_split=True),
    Case(x3(4, 4, True), 16300, 256, 160, res="res", x_split=True),
    Case(x3(2, 4, True), 20000, 192, 96, act="relu", x_split=True, out_split=True),   # 157 tiles at mb = 4 < 256, 313 at mb = 2
    Case(x3(1, 4, True), 1000, 512, 288, act="gelu", x_split=True),             # 8 x 3 / 16 x 3 < 256: mb = 1
    Case(x3(1, 4, True), 1024, 512, 288, rpg=32, x_split=True),
    # fp32 input, split output at mb = 4: k_linear_x3<.., AS = false>
    Case(x3(4, 8), 8100, 128, 1056, act="gelu", out_split=True),
    Case(x3(4, 4), 16300, 256, 160, out_split=True),
    # mb = 2: 64-row tiles; KS = 2 when the tiles fit one round and K >= 2,048 with K / 64 even
    Case(x3(2, 4, ks=2), 4090, 2048, 480, res="inplace"),                     # nw = 4 (32 x 2 < 256), 32 x 4 < 256 -> 64 x 4 = 256
    Case(x3(2, 4), 4090, 512, 480, act="gelu"),
    Case(x3(2, 4), 4096, 512, 480, rpg=64),
    Case(x3(2, 4), 8192, 256, 1024, rpg=64),                                   # nw = 8 chosen, addend rows_per_group % 128 != 0: mb 2, nw 4
    # mb = 1: 32-row tiles (a single frame)
    Case(x3(1, 4, ks=4), 1000, 2048, 480, act="gelu"),                         # 128 tiles <= 128, 32 chunks: KS = 4
    Case(x3(1, 4, ring=16), 1000, 512, 480, res="res"),                        # 8 chunks: KS = 1, 8 % 4 == 0 -> the 16-deep ring
    Case(x3(1, 4), 1000, 192, 480, act="relu"),                                # 3 chunks: the 4-deep ring
    Case(x3(1, 4), 1024, 192, 288, rpg=32),
    Case(x3(1, 4), 96, 128, 64),
    # LayerNorm fused (forward_ln): 128 x 256 tiles when cdiv(M,128) cdiv(N,256) >= 192; k_linear_b16 when mb = 4 and K / 64 even
    Case(b16(8, 2, True), 6000, 256, 1056, ln=True, split_from=512),          # 47 x 5 = 235 >= 192
    Case(b16(8, 2, True), 4096, 512, 1536, ln=True, rpg=1024),                 # batch 4 of the q | k | v layer
    Case(b16(4, 2, True), 33001, 128, 224, act="relu", ln=True),               # N < 256: 258 x 2 = 516 >= 512 at mb = 4
    Case(x3(4, 8, lnf=True), 40000, 64, 256, ln=True),                         # K = 64: the 8-wave x3 LNF kernel (its LDS tail)
    Case(x3(4, 8, lnf=True), 12200, 192, 288, act="gelu", ln=True, split_from=256),   # 96 x 2 = 192; K / 64 = 3 odd
    Case(x3(4, 4, lnf=True), 33001, 192, 160, ln=True),                        # N < 256, 516 tiles at mb = 4, K / 64 odd
    Case(x3(2, 4, lnf=True), 4096, 512, 1536, ln=True, rpg=64),                # nw 8 -> 4 (rows_per_group 64), mb 4 -> 2
    Case(x3(2, 4, lnf=True), 10000, 256, 480, act="gelu", ln=True),            # 79 x 4 = 316 < 512 at mb = 4, 628 at mb = 2
    Case(x3(1, 4, ring=16, lnf=True), 1024, 512, 1536, ln=True, rpg=1024, split_from=512),   # batch 1 q | k | v: 384 tiles <= 512
    Case(x3(1, 4, lnf=True), 4096, 512, 1536, ln=True, rpg=32),                # mb 1 by rows_per_group 32: 1,536 tiles > 512
    Case(x3(1, 4, lnf=True), 1000, 192, 288, act="relu", ln=True),             # one tile per workgroup, K / 64 = 3
)

# instantiations only an SMK_LINEAR_* variable reaches; one fresh process per setting
CHILD_SETTINGS = {
    "KS2": (("SMK_LINEAR_KS", "2"), (
        Case(x3(1, 4, ks=2), 1000, 2048, 480, act="gelu"),
        Case(x3(1, 4, ks=2), 1000, 512, 480, res="res"),
    )),
    "SHAPE32": (("SMK_LINEAR_SHAPE", "32"), (
        Case(x3(4, 8, lnf=True), 40000, 512, 256, ln=True),                    # LN, mb = 4, K / 64 even: the model's K on the x3 form
        Case(x3(4, 8, lnf=True), 4096, 512, 1536, ln=True, rpg=1024, split_from=512),
        Case(x3(4, 4), 16300, 256, 160, act="gelu", res="inplace"),
    )),
}

# every forward instantiation of launch_linear_x3 (CONV = 0): 22 reached by default, x3<1,4,false,2> only with SMK_LINEAR_KS=2
EXPECTED = frozenset({
    b16(8, 4), b16(4, 4), b16(8, 2), b16(4, 2),
    x3(4, 8, True), x3(4, 4, True), x3(2, 4, True), x3(1, 4, True),
    x3(4, 8), x3(4, 4), x3(2, 4, ks=2), x3(2, 4), x3(1, 4, ks=4), x3(1, 4, ks=2), x3(1, 4, ring=16), x3(1, 4),
    b16(8, 2, True), b16(4, 2, True),
    x3(4, 8, lnf=True), x3(4, 4, lnf=True), x3(2, 4, lnf=True), x3(1, 4, ring=16, lnf=True), x3(1, 4, lnf=True),
})
EXPECTED_BY_ENV_ONLY = frozenset({x3(1, 4, ks=2)})


# ------------------------------------------------------------------------------------------------ the checks
SENT32 = 0x7FA5A5A5          # sentinel bits of an fp32 output word (a NaN no kernel writes)
SENT16 = 0x7FA5               # the same for a bf16 word of split output storage (int16)
X_PAD, X_TAIL, Y_PAD, Y_TAIL = 12, 37, 20, 19      # pitch padding / rows past M of the poisoned input and the sentinel output


class Setup:
    """The inputs of one case, its layer handle and its fp64 reference + elementwise bound."""

    def __init__(self, case: Case, seed: int):
        from smokephysai_amd.models.linear import HipLinear, HipLinearLN, from_split, to_split
        c = self.case = case
        dev = "cuda"
        g = torch.Generator(device=dev).manual_seed(seed)
        M, K, N = c.M, c.K, c.N
        if c.ln:
            x = torch.randn(M, K, device=dev, generator=g) * 1.7 + torch.randn(M, 1, device=dev, generator=g) * 1.5
        else:
            x = torch.randn(M, K, device=dev, generator=g)
        w = torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)
        b = torch.randn(N, device=dev, generator=g)
        self.res = torch.randn(M, N, device=dev, generator=g) if c.res else None
        self.padd = torch.randn(M // c.rpg, 5, N, device=dev, generator=g) if c.rpg else None
        if c.ln:
            gamma = torch.rand(K, device=dev, generator=g) + 0.5
            beta = torch.randn(K, device=dev, generator=g) * 0.3
            self.lin = HipLinearLN(w, b, gamma, beta, 1e-5)
        else:
            self.lin = HipLinear(w, b)
        # the poisoned input: NaN in the pitch padding and in the rows after M (split: rows after M of the dense storage)
        if c.x_split:
            xs = to_split(x)
            buf = torch.full((M + X_TAIL,) + tuple(xs.shape[1:]), float("nan"), device=dev, dtype=torch.bfloat16)
            buf[:M] = xs
            self.x = buf[:M]
            xd = from_split(xs).double()                    # the GEMM's operand: the hi + lo it was given
        else:
            buf = torch.full((M + X_TAIL, K + X_PAD), float("nan"), device=dev)
            buf[:M, :K] = x
            self.x = buf[:M, :K]
            xd = x.double()
        wd, bd = w.double(), b.double()
        # fp64 reference (pre-activation) and the bound on the pre-activation error
        if c.ln:
            gd, bed = gamma.double(), beta.double()
            mean = xd.mean(1, keepdim=True)
            rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5)
            xhat = (xd - mean) * rstd
            pre = torch.nn.functional.layer_norm(xd, (K,), gd, bed, 1e-5) @ wd.t() + bd
            wf = (wd * gd[None, :]).float().double()        # the handle's folded fp32 weights
            wsum = wf.sum(1)
            piv = xd[:, :1]
            xp = (xd - piv).abs()
            A = rstd * (xp @ wf.abs().t()) + rstd * ((mean - piv).abs() + xp.mean(1, keepdim=True)) * wsum.abs()[None, :]
            z = (mean - piv).abs() * rstd
            stat = (1 + z * z) * (K / 64 + 16) * 2.0 ** -24 * (xhat @ wf.t()).abs()
            bias_abs = (wd @ bed + bd).abs()
        else:
            pre = xd @ wd.t() + bd
            A = xd.abs() @ wd.abs().t()
            stat = 0.0
            bias_abs = bd.abs()
        cK = 2.0 ** -14 + (K + 16) * 2.0 ** -24
        bound = cK * A + stat + 2.0 ** -22 * bias_abs[None, :]
        if c.rpg:
            idx = torch.arange(M, device=dev)
            pa = self.padd.double()[idx // c.rpg, (idx % c.rpg) % 5]
            pre = pre + pa
            bound = bound + 2.0 ** -23 * (pre.abs() + pa.abs())
        if c.act == "gelu":
            post = 0.5 * pre * (1 + torch.erf(pre / math.sqrt(2.0)))
            bound = 1.13 * bound + 2.0 ** -20 * pre.abs()
        elif c.act == "relu":
            post = torch.relu(pre)
        else:
            post = pre
        if self.res is not None:
            post = post + self.res.double()
            bound = bound + 2.0 ** -23 * (post.abs() + self.res.double().abs())
        if c.out_split or c.split_from is not None:
            bound = bound + 2.0 ** -16 * post.abs()
        self.ref, self.bound = post, bound

    def output_buffer(self):
        """A fresh sentinel-filled output buffer and the out= view the call writes into."""
        c = self.case
        if c.out_split:
            buf = torch.full((c.M + Y_TAIL, c.N // 8, 2, 8), SENT16, device="cuda", dtype=torch.int16)
            return buf, buf.view(torch.bfloat16)[:c.M]
        buf = torch.full((c.M + Y_TAIL, c.N + Y_PAD), SENT32, device="cuda", dtype=torch.int32)
        out = buf.view(torch.float32)[:c.M, :c.N]
        if c.res == "inplace":
            out.copy_(self.res)
        return buf, out

    def call(self, out):
        c = self.case
        if c.ln:
            return self.lin.forward_ln(self.x, activation=c.act, periodic_add=self.padd, rows_per_group=c.rpg, out=out, split_from=c.split_from)
        res = out if c.res == "inplace" else self.res
        return self.lin(self.x, activation=c.act, residual=res, periodic_add=self.padd, rows_per_group=c.rpg, out=out,
                        x_split=c.x_split, out_split=c.out_split)

    def decode(self, out):
        from smokephysai_amd.models.linear import from_split, unsplit4_inplace
        c = self.case
        if c.out_split:
            return from_split(out).double()
        y = out.double()
        if c.split_from is not None:
            y[:, c.split_from:] = unsplit4_inplace(out[:, c.split_from:].contiguous()).double()
        return y


def check_case(case: Case, seed: int = 0, want_kernel: bool = True) -> set:
    """Runs one case and asserts: (1) every element within the derived bound of the fp64 chain and the global rel_err < 2e-5; (2) no NaN from
    the poisoned pitch padding / rows past M; (3) every output word outside [M][N] still the sentinel, bit for bit; (4) a second call
    bit-identical.  Returns the kernels the first call launched; want_kernel: also assert that it is exactly the case's own."""
    s = Setup(case, seed)
    buf1, out1 = s.output_buffer()
    kernels = launched_kernels(lambda: s.call(out1))
    if want_kernel:
        assert kernels == {case.kernel}, f"{case.name}: launched {sorted(kernels)}"
    y = s.decode(out1)
    ref, bound = s.ref, s.bound
    err = (y - ref).abs()
    bad = ~(err <= bound)                                   # (NaN counts as outside)
    rel = float(err.max()) / max(float(ref.abs().max()), 1e-30)
    if bool(bad.any()):
        rows, cols = torch.nonzero(bad, as_tuple=True)
        r, col = int(rows[0]), int(cols[0])
        ratio = (err / bound)[bad]
        raise AssertionError(f"{case.name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at row {r} col {col}: "
                             f"y {float(y[r, col])!r} ref {float(ref[r, col])!r} bound {float(bound[r, col]):.3e}; rows {int(rows.min())}.."
                             f"{int(rows.max())}, cols {int(cols.min())}..{int(cols.max())}; worst err / bound {float(ratio.nan_to_num(1e30).max()):.3g}; "
                             f"global rel_err {rel:.3e}")
    assert rel < 2e-5, f"{case.name}: global rel_err {rel:.3e}"
    # (3) the sentinel outside [M][N]
    chk = buf1.clone()
    sent = SENT16 if case.out_split else SENT32
    if case.out_split:
        chk[:case.M] = sent
    else:
        chk[:case.M, :case.N] = sent
    n_touched = int((chk != sent).sum())
    assert n_touched == 0, f"{case.name}: {n_touched} words outside [M][N] overwritten"
    # (4) the same call again: the same bits everywhere
    buf2, out2 = s.output_buffer()
    s.call(out2)
    assert torch.equal(buf1, buf2), f"{case.name}: a second identical call differs in {int((buf1 != buf2).sum())} words"
    return kernels


def linear_env() -> dict:
    return {k: v for k, v in os.environ.items() if k.startswith("SMK_LINEAR_")}


def _child(setting: str) -> int:
    (var, val), cases = CHILD_SETTINGS[setting]
    env = linear_env()
    if env != {var: val}:
        print(json.dumps({"setting": setting, "ok": False, "error": f"SMK_LINEAR_* must be exactly {var}={val}, found {env}"}))
        return 2
    want = torch.cuda.get_device_properties(0).multi_processor_count == CUS
    out, ok = [], True
    for i, c in enumerate(cases):
        try:
            k = check_case(c, seed=1000 + i, want_kernel=want)
            out.append({"name": c.name, "kernels": sorted(k)})
        except AssertionError as e:
            ok = False
            out.append({"name": c.name, "error": str(e)})
    print(json.dumps({"setting": setting, "ok": ok, "cus_checked": want, "cases": out}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1]))
