"""Every instantiation of the attention and LayerNorm kernels (csrc/transformer.hip), each from a case table row that names it
(tests/attention_variant_cases.py: shapes, routes and the derivation of the elementwise bounds), checked element by element against fp64 with
NaN-poisoned input padding, sentinel-filled output padding and a repeated call; which kernel actually ran is read from the profiler.  Plus the
32-bit offset bound of smk_attention_kv at its edge, a workspace one step too small, and LayerNorm rows whose mean dwarfs their spread."""
import pytest
import torch

from attention_variant_cases import (BWD_CASES, BWD_KERNELS, COMBINE, CUS, DELTA, DELTA_CASES, EXPECTED, FWD_CASES, LN_BWD_CASES, LN_CASES,
                                     LN_FINISH, LN_OFFSET_DIMS, SCALE, att, att_bwd, attention_env, attention_reference, assert_within,
                                     check_backward, check_delta, check_forward, check_layernorm, check_layernorm_bwd, forward_route,
                                     launched_kernels, ln, ln_bwd, ln_nv, offset_row_errors, parse_kernel)

_seen = {}          # case name -> kernels it launched (this process)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ no GPU needed
def test_kernel_names_parse_in_either_spelling():
    assert parse_kernel("void smk::k_attention_x3<1, false, true>(smk::AttnArgs)") == att(1, kvs=True)
    assert parse_kernel("_ZN3smk14k_attention_x3ILi1ELb0ELb1EEEvNS_8AttnArgsE") == att(1, kvs=True)
    assert parse_kernel("_ZN3smk14k_attention_x3ILi2ELb0ELb0EEEvNS_8AttnArgsE") == att(2)
    assert parse_kernel("void smk::k_attention_bwd_x3<true>(smk::AttnBwdArgs)") == att_bwd(True)
    assert parse_kernel("_ZN3smk18k_attention_bwd_x3ILb0EEEvNS_11AttnBwdArgsE") == att_bwd(False)
    assert parse_kernel("smk::k_attention_combine(float const*, float*, float*, long long, int, int, int)") == COMBINE
    assert parse_kernel("_ZN3smk19k_attention_combineEPKfPfS2_xiii") == COMBINE
    assert parse_kernel("smk::k_attn_delta(float const*, float const*, long long, int, long long, long long, float*)") == DELTA
    assert parse_kernel("_ZN3smk12k_attn_deltaEPKfS1_xixxPf") == DELTA
    assert parse_kernel("void smk::k_layernorm<4>(smk::LayerNormArgs)") == ln(4)
    assert parse_kernel("_ZN3smk11k_layernormILi8EEEvNS_13LayerNormArgsE") == ln(8)
    assert parse_kernel("void smk::k_layernorm_bwd<2>(smk::LayerNormBwdArgs)") == ln_bwd(2)
    assert parse_kernel("_ZN3smk15k_layernorm_bwdILi1EEEvNS_16LayerNormBwdArgsE") == ln_bwd(1)
    assert parse_kernel("smk::k_layernorm_bwd_finish(smk::LayerNormBwdArgs, int)") == LN_FINISH
    assert parse_kernel("_ZN3smk22k_layernorm_bwd_finishENS_16LayerNormBwdArgsEi") == LN_FINISH
    assert parse_kernel("Memcpy DtoD") is None and parse_kernel("void smk::k_linear_x3<4, 8, false, 1, 4, true>(smk::LinearArgs)") is None


def test_case_tables_name_every_instantiation():
    assert len(EXPECTED) == 19
    named = set()
    for c in FWD_CASES:
        named |= {c.kernel} | c.ws_kernels
        assert c.L % 128 == 0 and c.L >= 128 and c.B >= 1 and c.H >= 1, c.name
        assert (c.nsplit, c.kernel) == forward_route(c.B, c.L, c.H, c.kvs), c.name       # the launcher's rule at 256 CUs
        assert c.nsplit == 1 or c.kernel == att(2, False, c.kvs), c.name
    shapes = {kvs: sorted((c.B, c.L, c.H, c.nsplit) for c in FWD_CASES if c.kvs == kvs) for kvs in (False, True)}
    assert shapes[False] == shapes[True]                                                  # every shape with both k | v formats
    for c in BWD_CASES:
        assert c.L % 128 == 0 and c.L >= 128, c.name
    named |= BWD_KERNELS | {DELTA}
    assert any(c.H > 8 for c in BWD_CASES + DELTA_CASES) and any(c.rows > CUS * 32 * 4 for c in DELTA_CASES)
    for c in LN_CASES + LN_BWD_CASES:
        assert c.D % 4 == 0 and 4 <= c.D <= 2048 and c.rows >= 1, c.name
        assert c.kernel in (ln(ln_nv(c.D)), ln_bwd(ln_nv(c.D))), c.name
        named.add(c.kernel)
    named.add(LN_FINISH)
    assert named == EXPECTED, sorted(named ^ EXPECTED)
    # pitches of the poisoned / sentinel buffers: multiples of 4 floats (the kernels' 16-byte accesses)
    from attention_variant_cases import K_PAD, O_PAD, Q_PAD, V_PAD
    assert all(p % 4 == 0 for p in (Q_PAD, K_PAD, V_PAD, O_PAD, 8, 12, 16, 20, 24))
    names = [c.name for c in FWD_CASES + BWD_CASES + DELTA_CASES + LN_CASES + LN_BWD_CASES]
    assert len(set(names)) == len(names)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_no_attention_dispatch_override_is_set():
    """SMK_ATTN_SPLIT / SMK_ATTN_KS / SMK_ATTN_SB change the dispatch and are read once per process: the table needs them all unset."""
    assert attention_env() == {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c.name)
def test_attention_forward_variant(case):
    assert attention_env() == {}
    _seen[case.name] = check_forward(case, want_kernel=_cus() == CUS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c.name)
def test_attention_backward_variant(case):
    _seen[case.name] = check_backward(case, want_kernel=_cus() == CUS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DELTA_CASES, ids=lambda c: c.name)
def test_attention_delta_variant(case):
    _seen[case.name] = check_delta(case, want_kernel=_cus() == CUS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: c.name)
def test_layernorm_variant(case):
    _seen[case.name] = check_layernorm(case, want_kernel=_cus() == CUS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_BWD_CASES, ids=lambda c: c.name)
def test_layernorm_backward_variant(case):
    _seen[case.name] = check_layernorm_bwd(case, want_kernel=_cus() == CUS)


@pytest.mark.gpu
def test_instantiation_coverage():
    """The union of the kernels that ran equals the 19 instantiations of the table."""
    if _cus() != CUS:
        pytest.skip(f"the table's shapes are derived for {CUS} CUs, this device has {_cus()}: which kernel each reaches differs "
                    "(the numerical checks of every case still ran)")
    assert attention_env() == {}
    checks = [(c, check_forward) for c in FWD_CASES] + [(c, check_backward) for c in BWD_CASES] + [(c, check_delta) for c in DELTA_CASES] \
        + [(c, check_layernorm) for c in LN_CASES] + [(c, check_layernorm_bwd) for c in LN_BWD_CASES]
    seen = set()
    for c, check in checks:
        if c.name not in _seen:                      # (run on its own, e.g. under -k: check the case here)
            _seen[c.name] = check(c)
        seen |= _seen[c.name]
    assert seen == EXPECTED, sorted(seen ^ EXPECTED)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.gpu
def test_attention_offset_bound_is_exact():
    """smk_attention_kv addresses k and v with 32-bit buffer offsets, B L ld < 2^29 floats: at L = 1,024 and ld = 512 it runs B = 1,023 and
    refuses B = 1,024 before any launch; hip_attention serves B = 1,024 in two batch chunks (1,023 + 1) -- the first bit for bit the direct
    call, the last query block of each chunk against fp64."""
    from smokephysai_amd import _lib
    from smokephysai_amd.models.attention import hip_attention
    Lh = _lib.load()
    B, L, H = 1024, 1024, 8
    D = 64 * H
    assert (B - 1) * L * D < 2 ** 29 <= B * L * D
    g = torch.Generator(device="cuda").manual_seed(3)
    q, k, v = (torch.randn(B, L, D, device="cuda", generator=g) for _ in range(3))            # 2 GiB each
    out = torch.full((B, L, D), float("nan"), device="cuda")
    st = _lib.stream_ptr(q.device)

    def call(nb):
        return Lh.smk_attention_kv(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), nb, L, H, 64, D, D, D, D, SCALE, _lib.SMK_FMT_F32,
                                   _lib.SMK_FMT_F32, None, 0, st)
    kernels, rc = launched_kernels(lambda: call(B))
    assert rc != 0 and not kernels, (rc, sorted(kernels))
    assert bool(out.isnan().all())
    _lib.check(call(B - 1))
    chunked = hip_attention(q, k, v, H, SCALE)
    assert torch.equal(chunked[:B - 1], out[:B - 1])
    for b in (B - 2, B - 1):
        for h in range(H):
            cols = slice(64 * h, 64 * h + 64)
            ref, bound, _, _ = attention_reference(q[b, L - 128:, cols], k[b, :, cols], v[b, :, cols])
            assert_within(chunked[b, L - 128:, cols], ref, bound, f"batch {b} head {h}")
            assert float((chunked[b, L - 128:, cols].double() - ref).abs().max()) < 2e-5 * float(ref.abs().max())


@pytest.mark.gpu
def test_workspace_one_step_short_runs_the_unsplit_kernel():
    """A workspace 16 bytes short of smk_attention_workspace_bytes is not used: the result is bit for bit the call without a workspace, from the
    unsplit kernel alone."""
    from smokephysai_amd import _lib
    Lh = _lib.load()
    B, L, H = 1, 1024, 8
    D = 64 * H
    need = int(Lh.smk_attention_workspace_bytes(B, L, H, 64))
    if _cus() == CUS:
        assert need == 4 * B * L * H * 66 * 4
    if need == 0:
        pytest.skip("no split on this device")
    g = torch.Generator(device="cuda").manual_seed(4)
    q, k, v = (torch.randn(B, L, D, device="cuda", generator=g) for _ in range(3))
    ws = torch.full((need,), 0xFF, device="cuda", dtype=torch.uint8)
    st = _lib.stream_ptr(q.device)

    def call(nbytes):
        out = torch.empty(B, L, D, device="cuda")
        _lib.check(Lh.smk_attention_kv(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, L, H, 64, D, D, D, D, SCALE, _lib.SMK_FMT_F32,
                                       _lib.SMK_FMT_F32, ws.data_ptr() if nbytes else None, nbytes, st))
        return out
    kernels, short = launched_kernels(lambda: call(need - 16))
    plain = call(0)
    assert torch.equal(short, plain)
    if _cus() == CUS:
        assert kernels == {att(2)}, sorted(kernels)
        k_full, _ = launched_kernels(lambda: call(need))
        assert k_full == {att(2), COMBINE}


@pytest.mark.gpu
@pytest.mark.parametrize("D", LN_OFFSET_DIMS)
def test_layernorm_rows_whose_mean_dwarfs_their_spread(D):
    """The fused LayerNorm test's rows (50 + 0.1 randn, every 7th -300 + 0.01 randn) through the standalone forward and backward: y, dx, dw
    and db within 1e-4 max-norm of fp64 -- the bar the fused LayerNorm + linear kernel holds on the same rows."""
    errs = offset_row_errors(D)
    assert max(errs.values()) < 1e-4, errs
