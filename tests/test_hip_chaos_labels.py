"""GPU tests of the device route for the chaos labels (smk_chaos_features, chunk_chaos_labels_device, the dataset's labels="device",
get_chaos_features(as_tensor=True)).  Every comparison is against the host formulas (lyapunov_from_norms,
fractal_dimension_from_counts, entropy_from_hist, labels_from_stats / chunk_chaos_labels) on the same reduction results.

Tolerances (device fp64 against the host formulas):
  Lyapunov, fractal dimension: 1e-12 absolute.  Both routes are fp64 and differ by summation order (at most 18 terms), the closed-form
      slope against np.polyfit's SVD, and one or two ulp between the device and host logarithms (|log| <= 19): below 2e-14.
  entropy: 4e-6 absolute.  The host formula is fp32 (256 terms, pairwise depth 8, eps 6e-8, sum <= 8 -> 3.8e-6); the device is fp64
      on exact integer counts, so the gap is the fp32 formula's own rounding.
Against the reference's recorded labels: rtol 1e-3, atol 1e-6, the bar tests/test_hip_pipeline.py uses."""
import math
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smokephysai_amd.physics import SmokeSimulator                                                       # noqa: E402
from smokephysai_amd.physics.smoke_simulator import (chaos_features_device, entropy_from_hist,          # noqa: E402
                                                     fractal_dimension_from_counts, lyapunov_from_norms)
from smokephysai_amd.utils.data_loader import (HIST_TAIL, SyntheticSmokeDataset, chunk_chaos_labels,    # noqa: E402
                                               chunk_chaos_labels_device)

TOL = (1e-12, 1e-12, 4e-6)          # lyapunov, fractal dimension, entropy
NAMES = ("lyapunov_exponent", "fractal_dimension", "entropy")


def _host_rows(norms, box, hist, pos, hist_len):
    """The host formulas row by row, as get_chaos_features / labels_from_stats apply them."""
    out = np.empty((len(pos), 3))
    with np.errstate(all="ignore"):
        for k, (p, n) in enumerate(zip(pos, hist_len)):
            out[k, 0] = lyapunov_from_norms(norms[p - 19:p]) if n >= 20 else 0.0
            out[k, 1] = fractal_dimension_from_counts(box[p])
            out[k, 2] = entropy_from_hist(hist[p])
    return out


def _device_rows(norms, box, hist, pos, hist_len, groups=None):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()                         # noqa: E731
    return chaos_features_device(dev(norms, torch.float32), dev(box, torch.int32), dev(hist, torch.int32), dev(pos, torch.int32),
                                 dev(hist_len, torch.int32), groups=groups)


def _assert_close(got, want, what):
    """Column-wise absolute comparison at TOL; NaN must sit in the same places.  Prints the figures before asserting."""
    got, want = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(want, np.float64).reshape(-1, 3)
    assert got.shape == want.shape, what
    for c in range(3):
        a, b = got[:, c], want[:, c]
        nan_a, nan_b = np.isnan(a), np.isnan(b)
        err = float(np.abs(a[~nan_b & ~nan_a] - b[~nan_b & ~nan_a]).max()) if (~nan_b & ~nan_a).any() else 0.0
        print(f"{what}: {NAMES[c]} max |device - host| = {err:.3e} over {int((~nan_b).sum())} rows (bound {TOL[c]:.0e}), NaN rows {int(nan_b.sum())}")
        assert np.array_equal(nan_a, nan_b), (what, NAMES[c], "NaN in different rows")
        assert err <= TOL[c], (what, NAMES[c], err)


def test_golden_statistics_give_the_reference_features(golden):
    g = golden("chaos_stats_64.npz")
    S = 20                                                              # the 20 newest frames of the 25 the reference simulated
    norms = g["lyap_dists"].astype(np.float32)                          # what smk_frame_diff_norms writes is fp32
    box, hist = np.zeros((S, 5), np.int32), np.zeros((S, 256), np.int32)
    box[-1], hist[-1] = g["box_counts"], g["hist_counts"]
    pos, hist_len = np.array([S - 1], np.int32), np.array([len(g["frames"])], np.int32)
    got = _device_rows(norms, box, hist, pos, hist_len)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (1, 3)
    got = got.cpu().numpy()
    _assert_close(got, _host_rows(norms, box, hist, pos, hist_len), "golden statistics")
    print("golden statistics: device", got[0], "reference", g["feats"])
    np.testing.assert_allclose(got[0], g["feats"], rtol=1e-3, atol=1e-6)


def _random_stream(rows=2000, N=128, seed=11):
    """A stream of 19 + rows frames' worth of reduction results; row k reads frame 19 + k (so the Lyapunov windows overlap)."""
    rng = np.random.RandomState(seed)
    S = 19 + rows
    norms = (np.abs(rng.randn(S - 1)) * 10.0 ** rng.uniform(-6, 2, S - 1)).astype(np.float32)
    box = np.stack([rng.randint(0, (N >> (l + 1)) ** 2 + 1, S) for l in range(5)], axis=1).astype(np.int32)
    hist = np.zeros((S, 256), np.int32)
    for s in range(S):
        m = rng.randint(1, 257)                                         # occupied bins
        bins = rng.choice(256, m, replace=False)
        w = rng.rand(m) ** 3 + 1e-3
        total = rng.randint(m, 512 * 512 + 1)
        c = np.maximum(np.floor(w / w.sum() * (total - m)).astype(np.int64) + 1, 1)    # every chosen bin occupied, sum <= total
        hist[s, bins] = c
    pos = np.arange(19, S, dtype=np.int32)
    hist_len = rng.randint(10, 41, rows).astype(np.int32)
    # the edge rows
    norms[100:119] = 0.0                                                # row 100: every distance of the window is zero
    hist_len[100] = 20
    hist[19 + 5] = 0
    hist[19 + 5, 77] = 4096                                             # row 5: one occupied bin
    hist[19 + 6] = 0                                                    # row 6: no value in [0,1] -> NaN on both routes
    hist_len[7], hist_len[8] = 19, 20                                   # either side of the Lyapunov threshold
    box[19 + 9] = 0                                                     # row 9: no box set at any scale
    return norms, box, hist, pos, hist_len


def test_random_rows_match_the_host_formulas():
    norms, box, hist, pos, hist_len = _random_stream()
    assert hist.sum(axis=1).max() <= 512 * 512 and len(pos) == 2000
    want = _host_rows(norms, box, hist, pos, hist_len)
    assert np.isnan(want[6, 2]) and np.isnan(want[:, 2]).sum() == 1 and want[7, 0] == 0.0 and (want[:, 0] > 0).sum() > 100
    feats, means = _device_rows(norms, box, hist, pos, hist_len, groups=200)
    _assert_close(feats.cpu().numpy(), want, "random rows")
    with np.errstate(all="ignore"):
        _assert_close(means.cpu().numpy(), want.reshape(200, 10, 3).mean(axis=1), "group means of random rows")
    # rows that name no window or no frame get NaN and read nothing outside the arrays
    bad_pos = np.array([5, 18, len(norms) + 1, -1, 19], np.int32)
    bad_len = np.array([20, 25, 20, 20, 20], np.int32)
    bad = _device_rows(norms, box, hist, bad_pos, bad_len).cpu().numpy()
    assert np.isnan(bad[:2, 0]).all() and not np.isnan(bad[:2, 1:]).any()          # window before the stream: only Lyapunov is NaN
    assert np.isnan(bad[2:4]).all() and not np.isnan(bad[4]).any()


def test_repeated_calls_are_bit_identical():
    norms, box, hist, pos, hist_len = _random_stream(rows=400, seed=3)
    a, am = _device_rows(norms, box, hist, pos, hist_len, groups=40)
    b, bm = _device_rows(norms, box, hist, pos, hist_len, groups=40)
    c = _device_rows(norms, box, hist, pos, hist_len)                   # the ungrouped launch shape computes the same rows
    view = lambda t: t.cpu().numpy().view(np.int64)                     # noqa: E731  (bit patterns: NaN rows compare too)
    assert np.array_equal(view(a), view(b)) and np.array_equal(view(am), view(bm)) and np.array_equal(view(a), view(c))


@pytest.mark.parametrize("g", [1.05, 1.2])
@pytest.mark.parametrize("valid_head", [0, 5, 19])
def test_growing_stream_has_positive_lyapunov_on_both_routes(g, valid_head):
    """frame_k = (s_k / s_last) P with s_k = sum_{j<k} g^j: consecutive distances grow by g, so rows with 20 frames of history have
    Lyapunov ln g -- the unclamped branch no simulated fixture reaches (smoke decays)."""
    n, T = 3, 20
    K = HIST_TAIL + n * T
    P = np.random.RandomState(17).rand(64, 64)
    s = np.concatenate([[0.0], np.cumsum(g ** np.arange(K - 1, dtype=np.float64))])
    frames = ((s / s[-1])[:, None, None] * P).astype(np.float32)
    assert frames.min() >= 0.0 and frames.max() <= 1.0
    buf = torch.from_numpy(frames).cuda()
    host = chunk_chaos_labels(buf, n, T, valid_head)
    lyap = [avg["lyapunov_exponent"] for avg, _ in host]
    print(f"g={g} valid_head={valid_head}: host Lyapunov labels {lyap}, ln g = {math.log(g):.6f}")
    assert all(v > 0 for v in lyap)                                     # the condition of this test, on the HOST route
    assert all(abs(v - math.log(g)) <= 0.01 * math.log(g) for v in lyap[1:])
    got = chunk_chaos_labels_device(buf, n, T, valid_head)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (n, 3)
    _assert_close(got.cpu().numpy(), [[avg[k] for k in NAMES] for avg, _ in host], f"growing stream g={g} valid_head={valid_head}")


def test_chunk_labels_device_corners():
    buf = torch.rand(HIST_TAIL + 2 * 10, 64, 64, device="cuda")
    got = chunk_chaos_labels_device(buf, 2, 10, 0)                      # T <= start: no rows, the host route's defaults
    want = [[avg[k] for k in NAMES] for avg, _ in chunk_chaos_labels(buf, 2, 10, 0)]
    assert got.cpu().tolist() == want == [[0.0, 1.0, 0.0]] * 2
    with pytest.raises(ValueError):
        chunk_chaos_labels_device(buf, 1, 20, 0, start=8)
    buf = torch.rand(HIST_TAIL + 2 * 12, 64, 64, device="cuda")
    host = chunk_chaos_labels(buf, 2, 12, 3, start=9)
    _assert_close(chunk_chaos_labels_device(buf, 2, 12, 3, start=9).cpu().numpy(), [[avg[k] for k in NAMES] for avg, _ in host],
                  "start=9, T=12")


def _labels(data):
    return [[d["chaos_features"][k] for k in NAMES] for d in data]


def _assert_same_dataset(dev, host, what):
    assert len(dev) == len(host) > 0
    for a, b in zip(dev, host):
        assert torch.equal(a["sequence"], b["sequence"]) and a["sequence"].device == b["sequence"].device
        assert a["source_config"] == b["source_config"]
        assert set(a) == set(b) and all(type(a["chaos_features"][k]) is float for k in NAMES)
    _assert_close(_labels(dev), _labels(host), what)


@pytest.mark.parametrize("N,nsamp,kw", [(64, 5, dict(sim_batch=2)), (128, 3, dict())])
def test_device_label_dataset_equals_host_label_dataset(golden, tmp_path, N, nsamp, kw):
    def gen(labels, **extra):
        np.random.seed(0)
        return SyntheticSmokeDataset(num_samples=nsamp, grid_size=(N, N), device="cuda", labels=labels, **kw, **extra)
    host, dev = gen("host"), gen("device")
    _assert_same_dataset(dev.data, host.data, f"dataset {N}^2")
    g = golden(f"dataset_seed0_{N}.npz")
    for i in range(nsamp):
        if f"s{i}_chaos" in g:
            np.testing.assert_allclose(_labels(dev.data)[i], g[f"s{i}_chaos"], rtol=1e-3, atol=1e-6)
    assert "s0_chaos" in g
    np.random.seed(123)
    a = dev[0]
    np.random.seed(123)
    b = host[0]
    assert set(a) == set(b) and torch.equal(a["input"], b["input"]) and torch.equal(a["target"], b["target"])
    assert a["chaos_features"].dtype == torch.float32
    np.testing.assert_allclose(a["chaos_features"].numpy(), g["item0_seed123_chaos"], rtol=1e-3, atol=1e-6)
    # a cache written by one mode loads in the other
    for writer, reader in (("device", "host"), ("host", "device")):
        path = str(tmp_path / f"{writer}.pkl")
        written = gen(writer, cache_path=path)
        loaded = SyntheticSmokeDataset(num_samples=nsamp, grid_size=(N, N), device="cuda", cache_path=path, labels=reader)
        assert len(loaded) == nsamp
        for x, y in zip(loaded.data, written.data):
            assert torch.equal(x["sequence"], y["sequence"].cpu()) and x["source_config"] == y["source_config"]
            assert [float(x["chaos_features"][k]) for k in NAMES] == [float(y["chaos_features"][k]) for k in NAMES]
        with open(path, "rb") as f:
            assert set(pickle.load(f)[0]) == {"sequence", "chaos_features", "source_config"}
        np.random.seed(1)
        assert loaded[nsamp - 1]["chaos_features"].shape == (3,)


def test_device_label_dataset_rank_split_and_storage_device():
    def gen(labels, rank, world, **extra):
        np.random.seed(42)
        return SyntheticSmokeDataset(num_samples=5, grid_size=(64, 64), device="cuda", sim_batch=3, rank=rank, world=world,
                                     labels=labels, **extra).data
    full_host = gen("host", 0, 1)
    _assert_same_dataset(gen("device", 0, 1), full_host, "5 samples in chunks of 3")
    parts = gen("device", 0, 2) + gen("device", 1, 2)
    _assert_same_dataset(parts, full_host, "two-rank split")
    parts_host = gen("host", 0, 2) + gen("host", 1, 2)
    _assert_same_dataset(parts, parts_host, "two-rank split against the host split")
    # the device route's split equals its own single-process run bit for bit, as the host route's does
    assert _labels(parts) == _labels(gen("device", 0, 1))
    cpu = gen("device", 0, 1, storage_device="cpu")
    assert all(d["sequence"].device.type == "cpu" for d in cpu)
    _assert_same_dataset(cpu, gen("host", 0, 1, storage_device="cpu"), "storage_device=cpu")


def test_get_chaos_features_as_tensor():
    srcs = [[(30, 30)], [(20, 40), (44, 25)], [(25, 35)]]
    batched = SmokeSimulator((64, 64), batch_size=3)
    single = SmokeSimulator((64, 64))
    for b in range(3):
        batched.add_incense_source(srcs[b], [1.0 + b] * len(srcs[b]), grid=b)
    single.add_incense_source(srcs[1], [2.0] * 2)
    for step in range(1, 26):
        batched.simulate_step()
        single.simulate_step()
        if step == 9:
            assert batched.get_chaos_features(as_tensor=True) is None and single.get_chaos_features(as_tensor=True) is None
        if step in (10, 19, 20, 25):                                    # below and at the Lyapunov threshold, and the issue's 25
            got = batched.get_chaos_features(as_tensor=True)
            assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (3, 3)
            _assert_close(got.cpu().numpy(), [[d[k] for k in NAMES] for d in batched.get_chaos_features()], f"batched, {step} steps")
            one = single.get_chaos_features(as_tensor=True)
            assert one.dtype == torch.float64 and one.is_cuda and tuple(one.shape) == (3,)
            ref = single.get_chaos_features()
            _assert_close(one.cpu().numpy(), [ref[k] for k in NAMES], f"un-batched, {step} steps")
            assert torch.equal(one, got[1])                             # the same grid, alone or in a batch
    assert batched.get_chaos_features() == batched.get_chaos_features()  # the default call is untouched
