"""Every forward instantiation of the split-bf16 linear layer (launch_linear_x3, csrc/linear.hip), each from a case table row that names it
(tests/linear_variant_cases.py: shapes, flags and the derivation of the elementwise bound), checked element by element against fp64 with
poisoned input padding, a sentinel-filled output pitch and a repeated call; which kernel actually ran is read from the profiler.  Plus the
fused layer's row bound (smk_linear_ln_max_rows) at its edge."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from linear_variant_cases import (CHILD_SETTINGS, CUS, DEFAULT_CASES, EXPECTED, EXPECTED_BY_ENV_ONLY, b16, check_case, launched_kernels,
                                  linear_env, parse_kernel, x3, Setup)

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "linear_variant_cases.py")
_seen = {}          # case name -> kernels it launched (this process), child setting -> its JSON summary


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ no GPU needed
def test_kernel_names_parse_in_either_spelling():
    assert parse_kernel("void smk::k_linear_x3<4, 8, false, 1, 4, true>(smk::LinearArgs)") == x3(4, 8, lnf=True)
    assert parse_kernel("_ZN3smk11k_linear_x3ILi4ELi8ELb0ELi1ELi4ELb1EEEvNS_10LinearArgsE") == x3(4, 8, lnf=True)
    assert parse_kernel("void smk::k_linear_b16<8, 0, 4, false>(smk::LinearArgs)") == b16(8, 4)
    assert parse_kernel("_ZN3smk12k_linear_b16ILi4ELi0ELi2ELb1EEEvNS_10LinearArgsE") == b16(4, 2, True)
    assert parse_kernel("Memcpy DtoD") is None and parse_kernel("k_linear_wgrad_tr") is None


def test_case_table_names_every_forward_instantiation():
    assert len(EXPECTED) == 23
    by_default = {c.kernel for c in DEFAULT_CASES}
    by_env = {c.kernel for _, cases in CHILD_SETTINGS.values() for c in cases}
    assert by_default == EXPECTED - EXPECTED_BY_ENV_ONLY and len(by_default) == 22
    assert by_default | by_env == EXPECTED
    for c in DEFAULT_CASES + tuple(cc for _, cases in CHILD_SETTINGS.values() for cc in cases):
        assert c.K % 64 == 0 and c.N % 32 == 0 and (not c.rpg or c.M % c.rpg == 0), c.name
        assert ("k_linear_x3" in c.kernel and c.kernel.endswith("true>")) == (c.ln and "k_linear_x3" in c.kernel)
    assert len({c.name for c in DEFAULT_CASES}) == len(DEFAULT_CASES)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_no_linear_dispatch_override_is_set():
    """SMK_LINEAR_* change the dispatch and are read once per process (static locals): the table needs them all unset."""
    assert linear_env() == {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEFAULT_CASES, ids=lambda c: c.name)
def test_linear_variant(case):
    assert linear_env() == {}
    want = _cus() == CUS                 # (other CU counts: the shapes reach other tiles -- the numerical checks still hold)
    _seen[case.name] = check_case(case, seed=DEFAULT_CASES.index(case), want_kernel=want)


def _run_child(setting):
    if setting not in _seen:
        (var, val), _ = CHILD_SETTINGS[setting]
        env = {k: v for k, v in os.environ.items() if not k.startswith("SMK_LINEAR_")}
        env[var] = val
        p = subprocess.run([sys.executable, HELPER, setting], env=env, capture_output=True, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert p.returncode == 0 and lines, f"{setting}: exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        _seen[setting] = json.loads(lines[-1])
    return _seen[setting]


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(CHILD_SETTINGS))
def test_linear_variant_reached_only_through_env(setting):
    """The instantiations an SMK_LINEAR_* setting reaches, in a fresh child process (same checks; the child asserts its kernel too)."""
    summary = _run_child(setting)
    assert summary["ok"] and len(summary["cases"]) == len(CHILD_SETTINGS[setting][1]), summary
    if _cus() == CUS:
        assert summary["cus_checked"]
        for c, got in zip(CHILD_SETTINGS[setting][1], summary["cases"]):
            assert got["name"] == c.name and got["kernels"] == [c.kernel], got


@pytest.mark.gpu
def test_forward_instantiation_coverage():
    """The union of the kernels that ran equals the 23 forward instantiations: 22 by default, one only through SMK_LINEAR_KS=2."""
    if _cus() != CUS:
        pytest.skip(f"the table's shapes are derived for {CUS} CUs, this device has {_cus()}: which tile each reaches differs "
                    "(the numerical checks of every case still ran)")
    assert linear_env() == {}
    seen = set()
    for i, c in enumerate(DEFAULT_CASES):
        if c.name not in _seen:                      # (run on its own, e.g. under -k: launch the case here)
            s = Setup(c, seed=i)
            _seen[c.name] = launched_kernels(lambda: s.call(s.output_buffer()[1]))
        assert _seen[c.name] == {c.kernel}, (c.name, _seen[c.name])
        seen |= _seen[c.name]
    assert seen == EXPECTED - EXPECTED_BY_ENV_ONLY, sorted(seen ^ (EXPECTED - EXPECTED_BY_ENV_ONLY))
    for setting in CHILD_SETTINGS:
        seen |= {k for c in _run_child(setting)["cases"] for k in c["kernels"]}
    assert seen == EXPECTED, sorted(seen ^ EXPECTED)


# ------------------------------------------------------------------------------------------------ the fused layer's row bound
@pytest.mark.gpu
def test_fused_layer_row_bound_is_exact():
    """smk_linear_ln_max_rows is the largest row count smk_linear_forward_ln accepts, (rows + 256) K < 2^30 strictly: at K = 16,384 a call of
    exactly max_rows runs (first and last 256 rows against fp64), max_rows + 1 is refused -- by HipLinearLN (ValueError) and by the library
    itself -- and the unfused HipLinear serves those max_rows + 1 rows in 32-bit-offset chunks."""
    from smokephysai_amd import _lib
    from smokephysai_amd.models.linear import HipLinear, HipLinearLN
    K, N = 16384, 32
    g = torch.Generator(device="cuda").manual_seed(5)
    w = torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)
    b = torch.randn(N, device="cuda", generator=g)
    gamma = torch.rand(K, device="cuda", generator=g) + 0.5
    beta = torch.randn(K, device="cuda", generator=g) * 0.3
    lin = HipLinearLN(w, b, gamma, beta, 1e-5)
    R = lin.max_rows
    assert R == (2 ** 30 - 1) // K - 256 == 65279 and (R + 256) * K < 2 ** 30 <= (R + 257) * K
    x = torch.randn(R + 1, K, device="cuda", generator=g) + torch.randn(R + 1, 1, device="cuda", generator=g)    # 4.3 GB
    y = lin.forward_ln(x[:R])
    torch.cuda.synchronize()

    def ref(rows):
        xd = x[rows].double()
        return torch.nn.functional.layer_norm(xd, (K,), gamma.double(), beta.double(), 1e-5) @ w.double().t() + b.double()

    for rows in (slice(0, 256), slice(R - 256, R)):
        r = ref(rows)
        assert float((y[rows].double() - r).abs().max()) <= 2e-5 * float(r.abs().max()), rows
    with pytest.raises(ValueError):
        lin.forward_ln(x)
    # past the binding's own check: the library refuses the call as well (before any launch)
    del y
    yb = torch.empty(R + 1, N, device="cuda")
    for rows, ok in ((R + 1, False), (R, True)):
        rc = lin._L.smk_linear_forward_ln_split(lin._handle, x.data_ptr(), rows, K, yb.data_ptr(), N, lin.wsum.data_ptr(), 1e-5, None, 0, 1, 0, -1,
                                                _lib.stream_ptr(x.device))
        assert (rc == 0) == ok, (rows, rc, lin._L.smk_last_error())
    assert torch.equal(yb[:R], lin.forward_ln(x[:R]))
    del yb
    yf = HipLinear(w, b)(x)                                # R + 1 rows at K = 16,384: two chunks of whole 128-row blocks
    for rows in (slice(0, 256), slice(R + 1 - 256, R + 1)):
        r = x[rows].double() @ w.double().t() + b.double()
        assert float((yf[rows].double() - r).abs().max()) <= 2e-5 * float(r.abs().max()), rows
    # K > 2^22: no row fits -- 0, not a negative count
    del x, yf
    K2 = 2 ** 22 + 64
    big = HipLinearLN(torch.randn(32, K2, device="cuda") * 1e-3, None, torch.ones(K2, device="cuda"), torch.zeros(K2, device="cuda"), 1e-5)
    assert big.max_rows == 0 and not big.accepts(torch.zeros(1, K2, device="cuda"))


@pytest.mark.gpu
def test_pitched_rows_take_the_unfused_path_at_their_own_bound(golden):
    """HipLinearLN's bound holds at x's ACTUAL row pitch: 256 rows of a 128-feature layer fit max_rows by far, but with a row pitch of 2^21 + 128
    floats they do not fit (rows + 256) * ldx < 2^30.  forward_ln refuses them (ValueError) and HipBody.layer takes the unfused route for both
    LayerNorms -- bit for bit the output of the unfused layer on dense rows."""
    from smokephysai_amd.models import ChaosTransformerLayer
    from smokephysai_amd.models.hip_body import HipBody
    from conftest import rel_err
    gd = golden("transformer_layer.npz")
    layer = ChaosTransformerLayer(128, 2, chaos_strength=0.1)
    layer.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in gd.items() if k.startswith("w::")})
    layer = layer.cuda().eval()
    x = torch.from_numpy(gd["x"]).cuda()
    noise = torch.from_numpy(gd["noise"]).cuda()
    B, L, D = x.shape
    P = 2 ** 21 + 128
    buf = torch.zeros(B, L, P, device="cuda")                 # 2.1 GB
    xp = buf[..., :D]
    body = HipBody()
    assert body.fuse_layernorm
    with torch.no_grad():
        body.fuse_layernorm = False
        want = body.layer("t.", layer, x.clone(), noise)
        body.fuse_layernorm = True
        fused = body.layer("t.", layer, x.clone(), noise)
        ln = body.linear_ln("t.ffn.0", (layer.ffn[0],), layer.norm2)
        assert B * L <= ln.max_rows and ln.accepts(x) and not ln.accepts(xp)
        assert ln.rows_limit(P) == (2 ** 30 - 1) // P - 256 < B * L
        with pytest.raises(ValueError):
            ln.forward_ln(xp)
        xp.copy_(x)
        got = body.layer("t.", layer, xp, noise)
    assert got.data_ptr() == xp.data_ptr() and torch.equal(got, want)
    assert rel_err(fused.cpu().numpy(), gd["layer_out"]) < 1e-4 and rel_err(got.cpu().numpy(), gd["layer_out"]) < 1e-4
