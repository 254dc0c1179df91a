"""CPU-side checks of the optical-flow baselines: the numpy oracle (tests/optical_flow_oracle.py) against the properties the
specification promises, the new C-ABI symbols, and benchmark.evaluate_traditional_cv's result shape with a stubbed flow.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optical_flow_oracle as ofo  # noqa: E402

FLOW_SYMBOLS = ["smk_flow_levels", "smk_flow_farneback_workspace", "smk_flow_level_image", "smk_flow_poly_exp",
                "smk_flow_farneback_iteration", "smk_flow_farneback", "smk_warp_workspace", "smk_warp_frames", "smk_flow_lk_workspace",
                "smk_flow_min_eigen", "smk_good_features", "smk_flow_lk_track", "smk_flow_lk_scatter", "smk_flow_lucas_kanade"]


def test_header_binding_and_library_agree_on_the_flow_symbols():
    from smokephysai_amd import _lib
    L = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smokehip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr))
    for name in FLOW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/smokehip.h"
        assert name in _lib.EXPORTS, f"{name} missing from _lib.EXPORTS"
        assert hasattr(L, name), f"{name} not exported by the library"
    assert L.smk_abi_version() == 17                      # the additions are purely additive


def test_level_rule():
    from smokephysai_amd import _lib
    L = _lib.load()
    for (H, W), K in (((128, 128), 3), ((64, 64), 2), ((96, 160), 2), ((40, 72), 1), ((1024, 1024), 3), ((32, 32), 1)):
        assert ofo.level_count(H, W) == K
        assert L.smk_flow_levels(H, W) == K
    assert ofo.level_size(96, 160, 1) == (48, 80)
    for H, W in ((31, 64), (64, 1025), (0, 0)):           # bad shapes: no levels, no workspace
        assert L.smk_flow_levels(H, W) == 0
        assert L.smk_flow_farneback_workspace(1, H, W) == 0 and L.smk_flow_lk_workspace(1, H, W) == 0 and L.smk_warp_workspace(1, H, W) == 0


def test_bad_shapes_return_invalid():
    """The argument checks come before any launch, so they run without a GPU (the pointers are never dereferenced)."""
    from smokephysai_amd import _lib
    L = _lib.load()
    buf = torch.zeros(1 << 20, dtype=torch.uint8)
    p = buf.data_ptr()
    assert L.smk_flow_farneback(p, p, 1, 31, 64, p, p, buf.numel(), None) == _lib.SMK_ERR_INVALID
    assert L.smk_flow_farneback(p, p, 0, 64, 64, p, p, buf.numel(), None) == _lib.SMK_ERR_INVALID
    assert L.smk_flow_lucas_kanade(p, p, 1, 64, 2048, p, p, buf.numel(), None) == _lib.SMK_ERR_INVALID
    assert L.smk_warp_frames(p, p, None, 1, 16, 16, p, None, None, 0, None) == _lib.SMK_ERR_INVALID
    assert L.smk_flow_farneback(p, p, 1, 64, 64, p, p, 16, None) == _lib.SMK_ERR_INVALID        # workspace too small
    assert L.smk_flow_level_image(p, 1, 64, 64, 2, p, p, buf.numel(), None) == _lib.SMK_ERR_INVALID   # 64^2 has levels 0 and 1


def test_cpu_tensor_is_refused():
    from smokephysai_amd.evaluation import farneback_optical_flow, lucas_kanade_optical_flow, predict_next_frame
    f = torch.zeros(64, 64, dtype=torch.uint8)
    for call in (lambda: farneback_optical_flow(f, f), lambda: lucas_kanade_optical_flow(f, f),
                 lambda: predict_next_frame(f, torch.zeros(64, 64, 2))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_to_uint8_frames_truncates_and_saturates():
    from smokephysai_amd.evaluation import to_uint8_frames
    x = torch.tensor([0.0, 0.5, 0.999, 1.0, 0.0039, 1.7, -0.3, float("nan")])
    got = to_uint8_frames(x)
    assert got.dtype == torch.uint8
    assert got.tolist() == [0, 127, 254, 255, 0, 255, 0, 0]
    inside = torch.linspace(0, 1, 1001)
    np.testing.assert_array_equal(to_uint8_frames(inside).numpy(), (inside.numpy() * 255).astype(np.uint8))   # equal to the reference there


def test_farneback_recovers_a_shift():
    """Band-limited texture, 128^2, shifted by (2, -1): the float64 flow more than 20 pixels from the border has a mean endpoint error
    below a quarter of the shift's length (measured: 8.2e-5 pixels)."""
    prev, nxt = ofo.shifted_pair(128, 128, seed=1, shift=(2, -1))
    flow = ofo.farneback(prev[None], nxt[None], np.float64)[0]
    inner = flow[20:-20, 20:-20]
    epe = np.sqrt((inner[..., 0] - 2.0) ** 2 + (inner[..., 1] + 1.0) ** 2).mean()
    print(f"mean endpoint error {epe:.3e} px")
    assert epe < 0.25 * np.sqrt(5.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_frames_give_zero_flow_and_the_input_back(dtype):
    prev, _ = ofo.shifted_pair(64, 96, seed=2)
    flow = ofo.farneback(prev[None], prev[None], dtype)
    assert flow.dtype == dtype and flow.shape == (1, 64, 96, 2)
    assert np.all(flow == 0)
    np.testing.assert_array_equal(ofo.warp(prev[None], flow, dtype), prev[None])
    lk = ofo.lucas_kanade(prev, prev, dtype)
    assert np.all(lk == 0)
    assert ofo.mse_uint8(prev[None], prev[None])[0] == 0.0


def test_polynomial_expansion_is_exact_on_a_quadratic():
    """The weighted least-squares fit reproduces a quadratic's own coefficients away from the replicated border."""
    y, x = np.mgrid[0:48, 0:64].astype(np.float64)
    x0, y0 = 30.0, 20.0
    img = 3.0 + 0.5 * (x - x0) - 0.25 * (y - y0) + 0.02 * (x - x0) ** 2 - 0.01 * (y - y0) ** 2 + 0.03 * (x - x0) * (y - y0)
    c = ofo.poly_expansion(img[None], np.float64)[0]
    np.testing.assert_allclose(c[:, 20, 30], [0.5, -0.25, 0.02, -0.01, 0.03], atol=1e-10)


def test_warp_reads_zero_outside_and_rounds_half_to_even():
    prev = np.zeros((1, 32, 32), np.uint8)
    prev[0, 10, 10], prev[0, 10, 11] = 1, 4
    flow = np.zeros((1, 32, 32, 2), np.float32)
    flow[0, 10, 10] = (0.5, 0.0)          # (1 + 4) / 2 = 2.5 -> 2
    flow[0, 5, 5] = (5.5, 5.0)            # the same sample reached from another pixel
    flow[0, 0, 0] = (-0.5, 0.0)           # half outside: tap at x = -1 reads 0
    flow[0, 31, 31] = (1e30, -1e30)       # far outside
    flow[0, 3, 3] = (np.nan, 0.0)
    prev[0, 0, 0] = 201
    pred = ofo.warp(prev, flow, np.float32)[0]
    assert pred[10, 10] == 2 and pred[5, 5] == 2 and pred[0, 0] == 100 and pred[31, 31] == 0 and pred[3, 3] == 0


def test_corner_selection_order_ties_and_distance():
    eig = np.zeros((40, 48), np.float32)
    eig[10, 10] = 5.0
    eig[10, 14] = 5.0                     # tie with (10, 10), nearer than 7: the earlier (y, x) wins, this one is suppressed
    eig[10, 17] = 4.0                     # exactly 7 from (10, 10): distance 7 is allowed
    eig[30, 5] = 5.0                      # third of the tied maxima, later in (y, x)
    eig[30, 11] = 4.5                     # 6 from (30, 5): suppressed
    eig[20, 40] = 1.5                     # not above 0.3 x 5
    eig[20, 30] = 1.6                     # just above
    eig[0, 20] = 9.0                      # on the border: never a corner, but it sets the maximum
    eig[25, 25] = eig[25, 26] = 3.0       # a plateau: both equal their 3 x 3 maximum; (25, 25) first, (25, 26) suppressed
    got = ofo.select_corners(eig)
    assert 0.3 * 9.0 > 1.6                # with the border maximum the threshold is 2.7
    assert got == [(10, 10), (5, 30), (17, 10), (25, 25)]
    eig[0, 20] = 0.0                      # maximum 5: threshold 1.5, (30, 20) comes in, (40, 20) stays out (not strictly above)
    assert ofo.select_corners(eig) == [(10, 10), (5, 30), (17, 10), (25, 25), (30, 20)]
    assert ofo.select_corners(np.zeros((40, 48), np.float32)) == []


def test_lucas_kanade_tracks_a_shift():
    prev, nxt = ofo.shifted_pair(128, 128, seed=1, shift=(2, -1))
    pts = ofo.select_corners(ofo.min_eigen(prev[None], np.float64)[0])
    assert 10 <= len(pts) <= 100
    out, status = ofo.lk_track(prev, nxt, pts, np.float64)
    moved = (out - np.array(pts, np.float64))[status == 1]
    assert status.sum() >= len(pts) // 2
    np.testing.assert_allclose(np.median(moved, 0), [2.0, -1.0], atol=0.05)
    flow = ofo.lk_scatter(pts, out, status, 128, 128)
    assert np.count_nonzero(flow.any(-1)) == status.sum()


def test_evaluate_traditional_cv_keys_and_table_rows(monkeypatch, capsys):
    """benchmark.evaluate_traditional_cv with stubbed flow functions (no GPU): the reference's dict, per-pair means, and three rows."""
    import benchmark
    calls = []

    def stub_flow(name):
        def f(prev, nxt):
            assert prev.dtype == torch.uint8 and prev.dim() == 3          # one batched call per loader batch
            calls.append((name, prev.shape[0]))
            return torch.zeros(*prev.shape, 2)
        return f

    def stub_score(prev, flow, nxt):
        d = nxt.double() - prev.double()
        return prev, (d * d).mean(dim=(1, 2))

    monkeypatch.setattr(benchmark, "farneback_optical_flow", stub_flow("fb"))
    monkeypatch.setattr(benchmark, "lucas_kanade_optical_flow", stub_flow("lk"))
    monkeypatch.setattr(benchmark, "predict_and_score", stub_score)
    torch.manual_seed(0)
    data = [{"input": torch.rand(1, 32, 32), "target": torch.rand(1, 32, 32)} for _ in range(6)]
    loader = torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)
    res = benchmark.evaluate_traditional_cv(loader)
    assert list(res) == ["Farneback", "Lucas-Kanade"]
    assert calls == [("fb", 4), ("lk", 4), ("fb", 2), ("lk", 2)]
    want = np.mean([((np.floor(d["target"].numpy() * 255.0) - np.floor(d["input"].numpy() * 255.0)) ** 2).mean() for d in data])
    for r in res.values():
        assert set(r) == {"mse", "inference_time"}
        assert np.isfinite(r["mse"]) and r["inference_time"] >= 0
        assert abs(r["mse"] - want) < 1e-9 * want
    benchmark.print_results({"mse": 0.01, "physics_correlation": 0.5, "inference_time": 0.001}, res)
    out = capsys.readouterr().out
    rows = [ln for ln in out.splitlines() if ln.count("|") == 3 and not ln.startswith("Model")]
    assert [ln.split("|")[0].strip() for ln in rows] == ["SmokePhysAI", "Farneback", "Lucas-Kanade"]
    assert all("N/A" in ln for ln in rows[1:])
