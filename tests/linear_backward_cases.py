"""Case table and checks of tests/test_hip_linear_backward.py: every plan of the linear layers' backward (csrc/linear.hip) -- the weight
gradient smk_linear_wgrad on both of its routes (k_linear_wgrad_tr; k_transpose_pad + the layer kernel with K-segments), the bias gradient
that rides on either (k_col_finish), and the input-gradient handle filled from W read transposed (smk_linear_update).  The plans
(plan_wgrad_tr, plan_linear_wgrad, launch_linear_wgrad) are restated here in plain Python so that a host test can say which branch each row
of the table reaches; a GPU test holds the restated byte count against the library's own.  Also runs on its own, in a fresh process, for
the plans that only SMK_LINEAR_WGRAD_TR=0 reaches at the model's shapes (the variable is read once per process):

    SMK_LINEAR_WGRAD_TR=0 python tests/linear_backward_cases.py TR0

prints one JSON line {"setting", "ok", "cases": [{"name", "route", "nseg", "kernels", ...}]} and exits non-zero when a check fails.

Error bound (element by element, against dY^T X in fp64).  The argument is the forward table's (tests/linear_variant_cases.py): a
split-bf16 operand v = hi + lo (hi = RNE_bf16(v), lo = RNE_bf16(v - hi)) misses v by at most 2^-17 |v|; both kernels sum
hi*hi + hi*lo + lo*hi and drop lo*lo <= 2^-16 |dy x|.  Per product that is |dy x| (2 * 2^-17 + 2^-16 + 2^-32) ~ 2^-15 |dy x|, each
product exact in fp32 (bf16 x bf16).  The reduction runs over the token rows: fp32 accumulation of the `rows` products of one element
inside the segments (at most rows * 2^-24 of sum |dy x|, the gamma_n bound, whatever the chunk order), then k_sum_segments adds the nseg
partial slabs in segment order (nseg * 2^-24 more); 16 * 2^-24 covers the zero-padded rows and the merge of the layer kernel's wave groups:
    |dW - ref| <= c * (|dY|^T @ |X|),   c = 2^-14 + (rows + nseg + 16) * 2^-24           (2^-14: twice the product term)
The bias gradient is a plain fp32 sum of dY's own values (no split): partial column sums over row blocks, the blocks added in a fixed
order -- every value passes through fewer than rows + 16 additions:
    |db - ref| <= (rows + 16) * 2^-24 * sum_rows |dY|
No GPU measured c: it is derived.  The global max-norm rel_err < 2e-5 of tests/test_hip_linear.py stays beside it.

The exact case needs no bound at all: dY and X hold integers of [-8, 8] (bf16 numbers: lo = 0, every product exact) and every partial sum
stays below 64 * rows <= 2^24 for rows <= 262,144, so fp32 accumulation in ANY order is exact and dW, db must EQUAL the integer product
(formed in fp64, where |sums| < 2^53 are exact too).  A row dropped, doubled or taken from the neighbouring segment changes it."""
import json
import os
import re
import sys
from dataclasses import dataclass
from typing import Optional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch            # noqa: E402

CUS = 256               # the table's plans are derived for this many CUs (MI355X)


# ------------------------------------------------------------------------------------------------ kernel names
BACKWARD_KERNELS = ("k_linear_wgrad_tr", "k_transpose_pad", "k_sum_segments", "k_col_finish")
_BACKWARD = re.compile(r"(?<![A-Za-z0-9_])(" + "|".join(BACKWARD_KERNELS) + r")(?![A-Za-z0-9_])")
_BACKWARD_MANGLED = re.compile(r"_ZN3smk\d+(" + "|".join(BACKWARD_KERNELS) + r")E")


def parse_backward_kernel(name: str) -> Optional[str]:
    """A trace event's name -> one of BACKWARD_KERNELS, from either the demangled ('smk::k_linear_wgrad_tr(smk::WgradTrArgs)') or the mangled
    ('_ZN3smk17k_linear_wgrad_trENS_11WgradTrArgsE') spelling; None for every other kernel (k_linear_x3<..>, k_col_finish_v2, a memcpy)."""
    m = _BACKWARD_MANGLED.search(name)
    if m:
        return m.group(1)
    if name.startswith("_Z"):
        return None
    m = _BACKWARD.search(name)
    return m.group(1) if m else None


def launched_backward_kernels(fn) -> set:
    """The backward kernels (BACKWARD_KERNELS) the GPU ran during fn(), by name from the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {k for k in (parse_backward_kernel(e.name) for e in prof.events()) if k}


# ------------------------------------------------------------------------------------------------ the plans, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def plan_wgrad_tr(rows, out_f, in_f, cus, ld_dy=4, ldx=4, enabled=True) -> Optional[dict]:
    """plan_wgrad_tr (csrc/linear.hip): None when the transposed-read kernel does not take the call, else its segments.  seg_rows: the rows
    of each segment (0: an empty one); block_map: which branch of the kernel's block -> (tile, segment) map the launch takes."""
    if not (enabled and out_f % 128 == 0 and in_f % 128 == 0 and ld_dy % 4 == 0 and ldx % 4 == 0 and rows >= 32):
        return None
    tiles_m, tiles_n = out_f // 128, in_f // 128
    nseg = 2 * cus // (tiles_m * tiles_n)
    if nseg >= 8:
        nseg &= ~7
    nseg = max(1, min(nseg, max(rows // 256, 1)))                 # segments of at least 256 rows
    if nseg >= 8:
        nseg &= ~7
    rps = _cdiv(_cdiv(rows, nseg), 32) * 32
    return {"nseg": nseg, "tiles_m": tiles_m, "tiles_n": tiles_n, "rows_per_seg": rps,
            "bytes": (nseg * out_f * in_f + nseg * out_f) * 4,
            "block_map": "xcd" if nseg % 8 == 0 else "linear",
            "seg_rows": [max(0, min(rows, (s + 1) * rps) - s * rps) for s in range(nseg)]}


def plan_wgrad_fallback(rows, out_f, in_f) -> dict:
    """plan_linear_wgrad's own layout (before the maximum with the transposed-read form's bytes): dY^T [out][rows_pad] fp32, X split into the
    weight layout [rows_pad][in] x 2 bf16, (nseg > 1) the partial slabs, the bias gradient's partials [rows_pad / 32][out]."""
    tiles = _cdiv(out_f, 128) * _cdiv(in_f, 128)
    nseg = 1
    while nseg < 64 and tiles * nseg < 512 and rows // (2 * nseg) >= 1024:
        nseg *= 2
    unit = 64 * nseg
    rows_pad = _cdiv(rows, unit) * unit
    off_wq = out_f * rows_pad * 4
    off_part = off_wq + rows_pad * in_f * 2 * 2
    off_col = off_part + (nseg * out_f * in_f * 4 if nseg > 1 else 0)
    return {"nseg": nseg, "rows_pad": rows_pad, "off_wq": off_wq, "off_part": off_part, "off_col": off_col,
            "bytes": off_col + (rows_pad // 32) * out_f * 4}


def workspace_bytes(rows, out_f, in_f, cus, tr_enabled=True) -> int:
    """smk_linear_wgrad_workspace: the larger of the two routes' needs (the fast one asked at pitches it accepts: the pointers decide later)."""
    b = plan_wgrad_fallback(rows, out_f, in_f)["bytes"]
    t = plan_wgrad_tr(rows, out_f, in_f, cus, enabled=tr_enabled)
    return max(b, t["bytes"]) if t else b


# ------------------------------------------------------------------------------------------------ the table
@dataclass(frozen=True)
class BCase:
    rows: int
    out: int
    inf: int
    route: str                  # "tr" | "fallback": the route this row must take (256 CUs)
    nseg: int                   # ... and its segment count
    dy_pad: int = 8             # row pitch of dY = out + dy_pad floats
    x_pad: int = 4              # row pitch of X = in + x_pad
    dy_off: int = 0             # the view starts this many floats into a 16-byte-aligned buffer
    x_off: int = 0
    tag: str = ""

    @property
    def name(self):
        return f"{self.route}{self.nseg}:{self.rows}x{self.out}x{self.inf}" + (f"-{self.tag}" if self.tag else "")


def plan_route(c: BCase, cus: int, tr_enabled=True) -> dict:
    """launch_linear_wgrad's decision for one case: the route, its nseg, whether k_sum_segments runs, the workspace bytes."""
    t = plan_wgrad_tr(c.rows, c.out, c.inf, cus, c.out + c.dy_pad, c.inf + c.x_pad, tr_enabled)
    if t and c.dy_off % 4 == 0 and c.x_off % 4 == 0:
        r = {"route": "tr", "nseg": t["nseg"], "plan": t}
    else:
        f = plan_wgrad_fallback(c.rows, c.out, c.inf)
        r = {"route": "fallback", "nseg": f["nseg"], "plan": f}
    r["sum_segments"] = r["nseg"] > 1
    r["bytes"] = workspace_bytes(c.rows, c.out, c.inf, cus, tr_enabled)
    return r


def expected_kernels(route: dict, with_db: bool) -> set:
    k = {"k_linear_wgrad_tr"} if route["route"] == "tr" else {"k_transpose_pad"}
    if route["sum_segments"]:
        k.add("k_sum_segments")
    if with_db:
        k.add("k_col_finish")
    return k


# Derived from plan_wgrad_tr / plan_linear_wgrad at 256 CUs (512 slots / tiles, at most rows / 256 segments, rows_per_seg a multiple of 32).
DEFAULT_CASES = (
    # the transposed-read kernel; nseg 1 .. 7 take the plain block map, 8 / 16 / 24 the XCD slot map
    BCase(32, 128, 128, "tr", 1),                   # one full chunk, stored straight into dW
    BCase(33, 128, 256, "tr", 1),                   # a full chunk + a 1-row partial one; tiles_n = 2
    BCase(255, 256, 128, "tr", 1),                  # 7 full chunks + 31 rows; tiles_m = 2
    BCase(512, 128, 128, "tr", 2),
    BCase(777, 128, 384, "tr", 3),                  # rows_per_seg 288; the last segment has 201 rows
    BCase(1800, 384, 128, "tr", 7),                 # the last segment has 72 rows
    BCase(2051, 256, 384, "tr", 8),                 # 6 tiles (2 x 3), one octet of segments; the last has 35 rows
    BCase(4101, 256, 384, "tr", 16),                # two octets; segment 14 has 69 rows, segment 15 is empty
    BCase(6350, 128, 128, "tr", 24),                # segment 22 holds 14 rows (its first chunk is the partial one), segment 23 is empty
    # the fallback on shapes the fast route would take but for ...
    BCase(1, 128, 128, "fallback", 1),              # rows < 32
    BCase(31, 256, 128, "fallback", 1),
    BCase(300, 128, 128, "fallback", 1, dy_pad=1, tag="dypitch"),      # a dY pitch that is no multiple of 4
    BCase(777, 128, 128, "fallback", 1, dy_off=1, tag="dyoff"),        # a dY base pointer 4 bytes past a 16-byte boundary
    BCase(777, 128, 128, "fallback", 1, x_off=1, tag="xoff"),          # the same for X
    # ... and on its own shapes
    BCase(5000, 132, 96, "fallback", 4),            # rows_pad 5120; a ragged row tile of the layer kernel (132 = 128 + 4)
    BCase(131072, 36, 32, "fallback", 64, dy_pad=4),      # one tile: the 64-segment cap
)

# the fallback at the model's own shapes: reached only with the fast route switched off, one fresh process
CHILD_SETTINGS = {
    "TR0": (("SMK_LINEAR_WGRAD_TR", "0"), (
        BCase(2048, 512, 512, "fallback", 2),       # batch 2 of an attention projection
        BCase(1024, 2048, 512, "fallback", 1),      # batch 1 of the FFN's first layer
    )),
}


# ------------------------------------------------------------------------------------------------ the checks
SENT32 = 0x7FA5A5A5          # sentinel bits of an fp32 word (a NaN no kernel writes): output bands, the unwritten dW / db, the workspace
BAND = 256                   # sentinel words before and after dW, db and the workspace (a multiple of 4: dW / workspace stay 16-byte aligned)
TAIL = 64                    # poisoned rows after `rows` in both inputs


def within(name, what, y, ref, bound):
    """Asserts |y - ref| <= bound element by element (2-D; NaN counts as outside); returns the worst err / bound."""
    err = (y - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        rows, cols = torch.nonzero(bad, as_tuple=True)
        r, col = int(rows[0]), int(cols[0])
        ratio = (err / bound)[bad]
        rel = float(err.nan_to_num(1e30).max()) / max(float(ref.abs().max()), 1e-30)
        raise AssertionError(f"{name}: {what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at row {r} col {col}: "
                             f"got {float(y[r, col])!r} ref {float(ref[r, col])!r} bound {float(bound[r, col]):.3e}; rows {int(rows.min())}.."
                             f"{int(rows.max())}, cols {int(cols.min())}..{int(cols.max())}; worst err / bound "
                             f"{float(ratio.nan_to_num(1e30).max()):.3g}; global rel_err {rel:.3e}")
    return float((err / bound.clamp_min(1e-300)).max())


class Setup:
    """The poisoned inputs of one case: dY [rows][out] and X [rows][in] as views (pitch, offset) into NaN-filled buffers with TAIL NaN rows
    after them.  integer: values drawn from the integers of [-8, 8]."""

    def __init__(self, case: BCase, seed: int, integer: bool = False):
        self.case = c = case
        g = torch.Generator(device="cuda").manual_seed(seed)

        def operand(cols, pad, off):
            ld = cols + pad
            flat = torch.full(((c.rows + TAIL) * ld + 4,), float("nan"), device="cuda")
            assert flat.data_ptr() % 16 == 0
            view = flat[off:off + (c.rows + TAIL) * ld].view(c.rows + TAIL, ld)[:c.rows, :cols]
            if integer:
                view.copy_(torch.randint(-8, 9, (c.rows, cols), device="cuda", generator=g).float())
            else:
                view.copy_(torch.randn(c.rows, cols, device="cuda", generator=g))
            return flat, view

        self._dy_buf, self.dy = operand(c.out, c.dy_pad, c.dy_off)
        self._x_buf, self.x = operand(c.inf, c.x_pad, c.x_off)
        assert (self.dy.data_ptr() % 16 == 0) == (c.dy_off % 4 == 0) and (self.x.data_ptr() % 16 == 0) == (c.x_off % 4 == 0)
        assert self.dy.stride(0) == c.out + c.dy_pad and self.x.stride(0) == c.inf + c.x_pad

    def buffers(self, nbytes):
        """Fresh sentinel-filled storage: (out words, dW view, db view, workspace words) -- dW, db and a workspace of exactly nbytes, each with
        BAND sentinel words before and after it."""
        c = self.case
        n = c.out * c.inf
        assert nbytes % 4 == 0
        obuf = torch.full((BAND + n + BAND + c.out + BAND,), SENT32, device="cuda", dtype=torch.int32)
        wbuf = torch.full((BAND + nbytes // 4 + BAND,), SENT32, device="cuda", dtype=torch.int32)
        dw = obuf[BAND:BAND + n].view(torch.float32).view(c.out, c.inf)
        db = obuf[2 * BAND + n:2 * BAND + n + c.out].view(torch.float32)
        return obuf, dw, db, wbuf

    def call(self, dw, db, wbuf, nbytes):
        """smk_linear_wgrad through the C ABI; db None: the db == NULL form."""
        from smokephysai_amd import _lib
        c = self.case
        L = _lib.load()
        ws_ptr = wbuf.data_ptr() + 4 * BAND
        _lib.check(L.smk_linear_wgrad(self.dy.data_ptr(), self.dy.stride(0), self.x.data_ptr(), self.x.stride(0), c.rows, c.out, c.inf,
                                      dw.data_ptr(), None if db is None else db.data_ptr(), ws_ptr, nbytes, _lib.stream_ptr(dw.device)))

    def bands_intact(self, obuf, wbuf, nbytes, db_written: bool):
        c = self.case
        n = c.out * c.inf
        chk = obuf.clone()
        chk[BAND:BAND + n] = SENT32
        if db_written:
            chk[2 * BAND + n:2 * BAND + n + c.out] = SENT32
        touched = int((chk != SENT32).sum())
        assert touched == 0, f"{c.name}: {touched} words around dW / db overwritten (db {'written' if db_written else 'NULL'})"
        w = nbytes // 4
        before, after = int((wbuf[:BAND] != SENT32).sum()), int((wbuf[BAND + w:] != SENT32).sum())
        assert before == 0 and after == 0, f"{c.name}: workspace of exactly {nbytes} bytes overrun: {before} words before, {after} after"


def check_case(case: BCase, seed: int = 0, want_route: bool = True, tr_enabled: bool = True) -> dict:
    """Runs one case and asserts: (1) dW and db element by element within the derived bounds of fp64, and the global rel_err < 2e-5; (2) with
    integer operands dW and db EQUAL the integer product; (3) no NaN from the poisoned pitch padding / rows past `rows` (nor from the NaN-filled
    workspace: a stale or unwritten partial slab); (4) the sentinel bands around dW, db and a workspace of exactly
    smk_linear_wgrad_workspace bytes unchanged, and the db == NULL form leaves db alone and gives the same dW bits; (5) a repeated call and
    hip_linear_wgrad give the same bits; (6) want_route: the kernels the profiler saw are the ones the restated plan predicts, and the route
    and nseg are the table's.  Returns what the device took and the worst err / bound (recorded, never a threshold)."""
    from smokephysai_amd import _lib
    from smokephysai_amd.models.linear import hip_linear_wgrad
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    route = plan_route(case, cus, tr_enabled)
    L = _lib.load()
    nbytes = int(L.smk_linear_wgrad_workspace(case.rows, case.out, case.inf))
    assert nbytes == route["bytes"], f"{case.name}: the library asks for {nbytes} workspace bytes, the restated plan for {route['bytes']}"
    if want_route:
        assert (route["route"], route["nseg"]) == (case.route, case.nseg), f"{case.name}: the restated plan gives {route['route']} nseg {route['nseg']}"
    rec = {"name": case.name, "route": route["route"], "nseg": route["nseg"], "cus": cus}
    for integer in (False, True):
        s = Setup(case, seed + (7919 if integer else 0), integer)
        what = "integers" if integer else "randn"
        o1, dw1, db1, w1 = s.buffers(nbytes)
        if integer:                                             # (the route does not depend on the values: one profiled pair per case)
            s.call(dw1, db1, w1, nbytes)
        else:
            kernels = rec["kernels"] = sorted(launched_backward_kernels(lambda: s.call(dw1, db1, w1, nbytes)))
        if want_route and not integer:
            assert set(kernels) == expected_kernels(route, True), f"{case.name}: launched {sorted(kernels)}, the plan predicts {sorted(expected_kernels(route, True))}"
        s.bands_intact(o1, w1, nbytes, True)
        dyd, xd = s.dy.double(), s.x.double()
        ref, ref_b = dyd.t() @ xd, dyd.sum(0)
        if integer:
            ne = dw1.double() != ref
            if bool(ne.any()):
                r, col = (int(v[0]) for v in torch.nonzero(ne, as_tuple=True))
                rr, cc = torch.nonzero(ne, as_tuple=True)
                raise AssertionError(f"{case.name}: integer dW differs in {int(ne.sum())} of {ne.numel()} elements; first at [{r}][{col}]: got "
                                     f"{float(dw1[r, col])!r} want {float(ref[r, col])!r}; rows {int(rr.min())}..{int(rr.max())}, cols "
                                     f"{int(cc.min())}..{int(cc.max())}")
            nb = db1.double() != ref_b
            assert not bool(nb.any()), (f"{case.name}: integer db differs in {int(nb.sum())} of {case.out} columns; first at "
                                        f"{int(torch.nonzero(nb)[0])}: got {float(db1[nb][0])!r} want {float(ref_b[nb][0])!r}")
        else:
            c = 2.0 ** -14 + (case.rows + route["nseg"] + 16) * 2.0 ** -24
            rec["dw_err_over_bound"] = within(case.name, "dW", dw1.double(), ref, c * (dyd.abs().t() @ xd.abs()))
            rec["db_err_over_bound"] = within(case.name, "db", db1.double()[None], ref_b[None],
                                              ((case.rows + 16) * 2.0 ** -24 * dyd.abs().sum(0))[None])
            rec["rel_err"] = float((dw1.double() - ref).abs().max()) / float(ref.abs().max())
            assert rec["rel_err"] < 2e-5, f"{case.name}: global rel_err {rec['rel_err']:.3e}"
        # the db == NULL form: the same dW bits, db's words and every band untouched
        o2, dw2, db2, w2 = s.buffers(nbytes)
        if integer:
            s.call(dw2, None, w2, nbytes)
        else:
            k2 = launched_backward_kernels(lambda: s.call(dw2, None, w2, nbytes))
        if want_route and not integer:
            assert k2 == expected_kernels(route, False), f"{case.name}: db == NULL launched {sorted(k2)}"
        s.bands_intact(o2, w2, nbytes, False)
        assert torch.equal(dw2.view(torch.int32), dw1.view(torch.int32)), f"{case.name} ({what}): dW differs without db"
        # the same call again, and the Python wrapper: the same bits everywhere
        o3, dw3, db3, w3 = s.buffers(nbytes)
        s.call(dw3, db3, w3, nbytes)
        assert torch.equal(o3, o1), f"{case.name} ({what}): a second identical call differs in {int((o3 != o1).sum())} words"
        dw4, db4 = hip_linear_wgrad(s.dy, s.x, want_db=True)
        assert torch.equal(dw4.view(torch.int32), dw1.view(torch.int32)) and torch.equal(db4.view(torch.int32), db1.view(torch.int32)), \
            f"{case.name} ({what}): hip_linear_wgrad gives other bits than the C ABI call"
    return rec


def check_dx_handle(w_shape, rows, seed: int = 0) -> dict:
    """The input-gradient handle of a layer with weight W [out][in]: a HipLinear built from W.t().contiguous() and one refilled in place with
    update(W, None, transposed=True) give the same bits on the same dY -- also after an in-place change of W and a second update --
    and both lie within the forward table's elementwise bound of dY W in fp64 (K = out: c = 2^-14 + (out + 16) 2^-24, no bias)."""
    from smokephysai_amd.models.linear import HipLinear
    out_f, in_f = w_shape
    name = f"dX:{rows}x{out_f}->{in_f}"
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(out_f, in_f, device="cuda", generator=g) / out_f ** 0.5
    dy = torch.randn(rows, out_f, device="cuda", generator=g)
    stale = torch.randn(in_f, out_f, device="cuda", generator=g)            # what the refilled handle held before: nothing of it may survive
    refilled = HipLinear(stale, torch.randn(in_f, device="cuda", generator=g))      # (a bias too: update(.., None) must clear it)
    c = 2.0 ** -14 + (out_f + 16) * 2.0 ** -24
    worst = 0.0
    for rnd in range(2):
        refilled.update(w, None, transposed=True)
        fresh = HipLinear(w.t().contiguous(), None)
        a, b = fresh(dy), refilled(dy)
        assert a.shape == (rows, in_f)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} round {rnd}: {int((a != b).sum())} elements differ between the handles"
        ref = dy.double() @ w.double()
        worst = max(worst, within(name, f"round {rnd}", a.double(), ref, c * (dy.double().abs() @ w.double().abs())))
        rel = float((a.double() - ref).abs().max()) / float(ref.abs().max())
        assert rel < 2e-5, f"{name} round {rnd}: global rel_err {rel:.3e}"
        w.mul_(0.75).add_(0.05 * torch.randn(out_f, in_f, device="cuda", generator=g))       # "an optimizer step", in place
    return {"name": name, "err_over_bound": worst}


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
            out.append(check_case(c, seed=2000 + i, want_route=want, tr_enabled=False))
        except AssertionError as e:
            ok = False
            out.append({"name": c.name, "error": str(e)})
    print(json.dumps({"setting": setting, "ok": ok, "cus_checked": want, "cases": out}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1]))
