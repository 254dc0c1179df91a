"""Every plan of the linear layers' backward (smk_linear_wgrad on both routes, the bias gradient, the input-gradient handle refilled from W
read transposed), each from a row of tests/linear_backward_cases.py (shapes, the plans restated in Python, the derivation of the
elementwise bounds): against fp64 element by element, exactly on integer operands, with poisoned input padding, sentinel bands around dW, db
and an exactly sized workspace, the db == NULL form, a repeated call, and the launched kernels read from the profiler."""
import json
import os
import subprocess
import sys

import pytest
import torch

from linear_backward_cases import (BACKWARD_KERNELS, CHILD_SETTINGS, CUS, DEFAULT_CASES, BCase, check_case, check_dx_handle, expected_kernels,
                                   linear_env, parse_backward_kernel, plan_route, plan_wgrad_fallback, plan_wgrad_tr, workspace_bytes)

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "linear_backward_cases.py")
ALL_CASES = DEFAULT_CASES + tuple(c for _, cases in CHILD_SETTINGS.values() for c in cases)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ no GPU needed
def test_backward_kernel_names_parse_in_either_spelling():
    assert parse_backward_kernel("void smk::k_linear_wgrad_tr(smk::WgradTrArgs)") == "k_linear_wgrad_tr"
    assert parse_backward_kernel("smk::k_linear_wgrad_tr(smk::WgradTrArgs) [clone .kd]") == "k_linear_wgrad_tr"
    assert parse_backward_kernel("_ZN3smk17k_linear_wgrad_trENS_11WgradTrArgsE") == "k_linear_wgrad_tr"
    assert parse_backward_kernel("_ZN3smk17k_linear_wgrad_trENS_11WgradTrArgsE.kd") == "k_linear_wgrad_tr"
    assert parse_backward_kernel("void smk::k_transpose_pad(float const*, long long, int, int, float*, int, float*)") == "k_transpose_pad"
    assert parse_backward_kernel("_ZN3smk15k_transpose_padEPKfxiiPfiS2_") == "k_transpose_pad"
    assert parse_backward_kernel("_ZN3smk14k_sum_segmentsEPKfixPf") == "k_sum_segments"
    assert parse_backward_kernel("smk::k_sum_segments(float const*, int, long long, float*)") == "k_sum_segments"
    assert parse_backward_kernel("_ZN3smk12k_col_finishEPKfiiPf") == "k_col_finish"
    assert parse_backward_kernel("k_col_finish") == "k_col_finish"
    for other in ("void smk::k_linear_x3<4, 8, false, 1, 4, true>(smk::LinearArgs)", "_ZN3smk11k_linear_x3ILi4ELi8ELb0ELi1ELi4ELb1EEEvNS_10LinearArgsE",
                  "smk::k_col_finish_v2(float*)", "_ZN3smk15k_col_finish_v2EPf", "smk::k_conv2_wgrad_finish(float const*)", "Memcpy DtoD",
                  "smk::k_split_linear_weights_t16(float const*, smk::LinearDev, long long, int)", "xk_sum_segments"):
        assert parse_backward_kernel(other) is None, other
    assert len(set(BACKWARD_KERNELS)) == 4


def test_plan_restatement_on_known_plans():
    """The restated plans at the sizes whose plan can be read off csrc/linear.hip by hand (256 CUs: 512 slots / tiles, >= 256 rows a segment)."""
    t = plan_wgrad_tr(65536, 512, 512, 256)                 # 16 tiles: 32 segments of 2,048 rows
    assert (t["nseg"], t["rows_per_seg"], t["block_map"], t["bytes"]) == (32, 2048, "xcd", (32 * 512 * 512 + 32 * 512) * 4)
    t = plan_wgrad_tr(1024, 512, 512, 256)                  # batch 1: rows / 256 = 4 segments
    assert (t["nseg"], t["rows_per_seg"], t["block_map"], t["seg_rows"]) == (4, 256, "linear", [256] * 4)
    t = plan_wgrad_tr(70001, 256, 128, 256)                 # 2 tiles: 256 segments of 288 rows, the last ones ragged / empty
    assert (t["nseg"], t["rows_per_seg"]) == (256, 288) and t["seg_rows"][243] == 17 and set(t["seg_rows"][244:]) == {0}
    t = plan_wgrad_tr(777, 128, 384, 256)
    assert (t["nseg"], t["rows_per_seg"], t["seg_rows"]) == (3, 288, [288, 288, 201])
    t = plan_wgrad_tr(2051, 256, 384, 320)                  # another CU count: 640 / 6 = 106 -> 104, still capped by the rows
    assert t["nseg"] == 8
    t = plan_wgrad_tr(65536, 512, 512, 64)                  # 128 / 16 = 8
    assert t["nseg"] == 8 and t["rows_per_seg"] == 8192
    for refused in ((31, 128, 128, 256), (512, 64, 128, 256), (512, 128, 96, 256)):
        assert plan_wgrad_tr(*refused) is None
    assert plan_wgrad_tr(512, 128, 128, 256, ld_dy=129) is None and plan_wgrad_tr(512, 128, 128, 256, ldx=130) is None
    assert plan_wgrad_tr(512, 128, 128, 256, enabled=False) is None
    f = plan_wgrad_fallback(5000, 132, 96)
    assert (f["nseg"], f["rows_pad"]) == (4, 5120)
    assert f["off_wq"] == 132 * 5120 * 4 and f["off_part"] == f["off_wq"] + 5120 * 96 * 4 and f["off_col"] == f["off_part"] + 4 * 132 * 96 * 4
    assert f["bytes"] == f["off_col"] + 160 * 132 * 4
    f = plan_wgrad_fallback(300, 36, 32)
    assert (f["nseg"], f["rows_pad"], f["off_part"], f["off_col"]) == (1, 320, f["off_wq"] + 320 * 32 * 4, f["off_part"])
    assert plan_wgrad_fallback(131072, 36, 32)["nseg"] == 64 and plan_wgrad_fallback(1 << 20, 36, 32)["nseg"] == 64
    assert plan_wgrad_fallback(65536, 512, 512)["nseg"] == 32          # 16 tiles x 32 = 512 slots
    # the library's answer is the larger need of the two routes
    assert workspace_bytes(65536, 512, 512, 256) == max(plan_wgrad_fallback(65536, 512, 512)["bytes"], plan_wgrad_tr(65536, 512, 512, 256)["bytes"])
    assert workspace_bytes(32, 128, 128, 256) == plan_wgrad_fallback(32, 128, 128)["bytes"] > plan_wgrad_tr(32, 128, 128, 256)["bytes"]
    assert workspace_bytes(300, 36, 32, 256) == plan_wgrad_fallback(300, 36, 32)["bytes"]


def test_case_table_reaches_every_backward_plan():
    """At 256 CUs every row takes the route and nseg it names, and together the rows reach every branch the suite did not look at before."""
    assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
    routes = {}
    for c in ALL_CASES:
        child = c not in DEFAULT_CASES
        r = routes[c.name] = plan_route(c, CUS, tr_enabled=not child)
        assert (r["route"], r["nseg"]) == (c.route, c.nseg), (c.name, r["route"], r["nseg"])
        assert c.inf % 32 == 0 and c.out % 4 == 0 and c.rows <= 262144 and (c.out + 256) * (c.rows + 4096) < 2 ** 30, c.name     # the ABI's own limits
        assert expected_kernels(r, True) - expected_kernels(r, False) == {"k_col_finish"}
        if child:                                            # the model's shapes: the fast route would take them
            assert plan_route(c, CUS)["route"] == "tr"
    fast = [routes[c.name]["plan"] for c in DEFAULT_CASES if c.route == "tr"]
    assert {p["nseg"] for p in fast} == {1, 2, 3, 7, 8, 16, 24}
    assert {p["block_map"] for p in fast} == {"xcd", "linear"}
    assert {p["nseg"] for p in fast if p["block_map"] == "linear"} == {1, 2, 3, 7}
    assert any(0 < n < 32 for p in fast for n in p["seg_rows"])                      # a segment whose first chunk is its partial one
    assert any(n == 0 for p in fast for n in p["seg_rows"])                          # an empty segment
    assert any(p["nseg"] == 1 and p["seg_rows"][0] % 32 == 1 for p in fast)          # a 1-row partial chunk
    # the XCD slot map with several tiles, tiles_m != tiles_n, and more than one octet of segments
    assert any(p["block_map"] == "xcd" and p["nseg"] > 8 and p["tiles_m"] != p["tiles_n"] and min(p["tiles_m"], p["tiles_n"]) > 1 for p in fast)
    # ... and the plain map with tiles_m != tiles_n either way round
    assert {(p["tiles_m"] > p["tiles_n"]) for p in fast if p["block_map"] == "linear" and p["tiles_m"] != p["tiles_n"]} == {True, False}
    fb = [c for c in DEFAULT_CASES if c.route == "fallback"]
    assert {c.nseg for c in fb} == {1, 4, 64}
    # the fallback on shapes the fast route would take but for ONE condition each
    taken = lambda c, **kw: plan_route(BCase(**{**c.__dict__, **kw}), CUS)["route"] == "tr"       # noqa: E731
    rerouted = [c for c in fb if c.out % 128 == 0 and c.inf % 128 == 0]
    assert {c.rows for c in rerouted if c.rows < 32} == {1, 31}
    assert any(c.rows >= 32 and (c.out + c.dy_pad) % 4 and taken(c, dy_pad=8) for c in rerouted)
    assert any(c.dy_off % 4 and not c.x_off and taken(c, dy_off=0) for c in rerouted)
    assert any(c.x_off % 4 and not c.dy_off and taken(c, x_off=0) for c in rerouted)
    assert {c.nseg for _, cases in CHILD_SETTINGS.values() for c in cases} == {1, 2}


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_restated_workspace_equals_the_librarys():
    """smk_linear_wgrad_workspace(rows, out, in) == the restated byte count at this device's CU count, for every row of the table."""
    from smokephysai_amd import _lib
    assert linear_env() == {}
    L = _lib.load()
    torch.cuda.init()
    for c in ALL_CASES:
        assert int(L.smk_linear_wgrad_workspace(c.rows, c.out, c.inf)) == workspace_bytes(c.rows, c.out, c.inf, _cus()), c.name


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEFAULT_CASES, ids=lambda c: c.name)
def test_linear_backward_plan(case):
    assert linear_env() == {}
    want = _cus() == CUS                 # (other CU counts: other segment counts -- the numerical checks still hold)
    rec = check_case(case, seed=DEFAULT_CASES.index(case), want_route=want)
    print("linear-backward", json.dumps(rec))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(CHILD_SETTINGS))
def test_linear_backward_plan_reached_only_through_env(setting):
    """The fallback at the model's own shapes, in a fresh child process with the fast route switched off (same checks)."""
    (var, val), cases = CHILD_SETTINGS[setting]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SMK_LINEAR_")}
    env[var] = val
    p = subprocess.run([sys.executable, HELPER, setting], env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, f"{setting}: exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    summary = json.loads(lines[-1])
    print("linear-backward", json.dumps(summary))
    assert summary["ok"] and len(summary["cases"]) == len(cases), summary
    if _cus() == CUS:
        assert summary["cus_checked"]
        for c, got in zip(cases, summary["cases"]):
            assert (got["name"], got["route"], got["nseg"]) == (c.name, c.route, c.nseg), got
            assert "k_transpose_pad" in got["kernels"] and "k_linear_wgrad_tr" not in got["kernels"], got


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [96, 4096])
@pytest.mark.parametrize("w_shape", [(512, 512), (2048, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_input_gradient_handle_refilled_from_w_read_transposed(w_shape, rows):
    rec = check_dx_handle(w_shape, rows, seed=rows + w_shape[0])
    print("linear-backward", json.dumps(rec))
