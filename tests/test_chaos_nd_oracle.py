"""CPU checks of the n-axis chaos statistics' oracle (tests/chaos_nd_oracle.py; SPEC_3D.md section 9) and of the host-side pieces of the
3-D smoke product: the oracle's 2-axis instance reproduces the reference's recorded statistics, its 3-axis instance a literal triple loop,
the 3-D dataset draws its sources in the documented order, and the 3-D simulator refuses to run without a ROCm device."""
import numpy as np
import pytest
import torch

from chaos_nd_oracle import box_counts_nd, brute_box_counts_3d, diff_norm, hist256, history_features, mean_nd, stats_nd


def test_2d_instance_reproduces_the_reference_statistics(golden):
    g = golden("chaos_stats_64.npz")
    frame = g["frames"][-1]
    mean, counts, hist = stats_nd(frame)
    assert mean == np.float32(g["mean"])
    assert counts.tolist() == g["box_counts"].tolist() == [99, 30, 9, 5, 4]
    assert hist.tolist() == g["hist_counts"].tolist()


def test_histogram_equals_torch_histogram_on_every_fixture_frame(golden):
    for frame in golden("chaos_stats_64.npz")["frames"]:
        want = torch.histogram(torch.from_numpy(frame).flatten(), bins=256, range=(0.0, 1.0))[0].numpy()
        assert ((frame < 0) | (frame > 1)).sum() > 0                    # the fixture frames do leave [0, 1]
        assert hist256(frame).tolist() == want.astype(np.int64).tolist()


def test_distances_and_features_reproduce_the_reference(golden):
    g = golden("chaos_stats_64.npz")
    frames = list(g["frames"])
    d = [diff_norm(a, b) for a, b in zip(frames[-20:-1], frames[-19:])]
    np.testing.assert_allclose(d, g["lyap_dists"], rtol=1e-6)
    f = history_features(frames)
    np.testing.assert_allclose([f["lyapunov_exponent"], f["fractal_dimension"], f["entropy"]], g["feats"], rtol=1e-3, atol=1e-6)
    assert history_features(frames[:9]) == {}
    assert history_features(frames[:19])["lyapunov_exponent"] == 0.0


def test_3d_instance_equals_a_brute_force_loop_on_an_odd_shape():
    rng = np.random.default_rng(0)
    vol = (rng.random((13, 40, 70)) ** 8).astype(np.float32)
    mean = mean_nd(vol)
    counts = box_counts_nd(vol, mean)
    assert counts.tolist() == brute_box_counts_3d(vol, mean).tolist() == [3748, 510, 40, 0, 0]
    assert counts[3] == 0 and counts[4] == 0                            # D = 13: no whole box of edge 16 or 32
    assert hist256(vol).sum() == vol.size


def test_draw_source_configs3d_order():
    from smokephysai_amd.utils.data_loader import draw_source_configs3d
    D, H, W = 16, 64, 96
    np.random.seed(0)
    got = draw_source_configs3d(6, (D, H, W))
    np.random.seed(0)
    m = min(20, D // 4)
    for cfg in got:
        k = np.random.randint(1, 4)
        assert len(cfg["positions"]) == len(cfg["intensities"]) == k
        for (x, y, z), inten in zip(cfg["positions"], cfg["intensities"]):
            assert x == np.random.randint(20, W - 20)
            assert y == np.random.randint(20, H - 20)
            assert z == np.random.randint(m, D - m)
            assert inten == np.random.uniform(0.5, 2.0)
            assert 20 <= x < W - 20 and 20 <= y < H - 20 and m <= z < D - m
    # the depth margin is min(20, D // 4): 16 at D = 64, the full 20 cells from D = 80 on
    np.random.seed(1)
    assert all(16 <= z < 48 for c in draw_source_configs3d(40, (64, 64, 64)) for (_, _, z) in c["positions"])
    assert all(20 <= z < 108 for c in draw_source_configs3d(40, (128, 64, 64)) for (_, _, z) in c["positions"])


def test_smoke_simulator3d_has_no_cpu_fallback():
    from smokephysai_amd.physics import SmokeSimulator3D
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SmokeSimulator3D((16, 64, 64), device="cpu")
    from smokephysai_amd.utils.data_loader import SyntheticSmokeDataset3D
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SyntheticSmokeDataset3D(2, (16, 64, 64), device="cpu")
