"""GPU tests of the 3-D smoke product's statistics path (SPEC_3D.md section 9): smk_volume_stats (csrc/chaos_nd.hip), the fractal emit of
the 3-D step (smk_sim3d_step_emit), SmokeSimulator3D and SyntheticSmokeDataset3D, against tests/chaos_nd_oracle.py -- the numpy form of the
n-axis rule whose 2-axis instance reproduces the reference's fixture (tests/test_chaos_nd_oracle.py).

Bounds:
  box counts, histogram: exact.  The counts are compared with the oracle EVALUATED AT THE DEVICE'S MEAN: the threshold is part of the input
      of the count, and the two means may differ by the one ulp below.
  means: within 1 fp32 ulp of float32(fp64 sum / cells) -- what two correctly rounded quotients of fp64 sums taken in different orders can
      differ by.  Against smk_chaos_stats (another summation order again) the same 1 ulp.
  norms: rtol 1e-6 of the fp64 value (fp64 accumulation, one rounding to fp32: 6e-8, plus the sum's own 1e-13).
  feature scalars of SmokeSimulator3D / the dataset labels: rtol 1e-3, atol 1e-6, the bar tests/test_hip_chaos_labels.py and
      tests/test_hip_pipeline.py use for these scalars.
  emit: bit for bit against smk_sim3d_step (no fractal), against smk_apply_fractal over the planes, and against the oracle's
      apply_fractal_perturbation evaluated with the device's fractal constant; 1e-6 relative (max-norm) against the oracle with its own
      constant, the bar of tests/test_config3_shapes.py (the Perlin constants differ by up to 2 ulp of sinf / cosf)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chaos_nd_oracle import diff_norm, history_features, mean_nd, stats_nd                               # noqa: E402
from conftest import rel_err                                                                             # noqa: E402
from smokephysai_amd import _lib                                                                         # noqa: E402
from smokephysai_amd.physics import FractalGenerator, NavierStokesSimulator3D, SmokeSimulator3D          # noqa: E402
from smokephysai_amd.physics.smoke_simulator import chaos_stats, frame_diff_norms, volume_stats          # noqa: E402
from smokephysai_amd.utils.data_loader import SyntheticSmokeDataset3D                                    # noqa: E402
from smokephysai_amd.utils.distributed import shard_range                                                # noqa: E402

NAMES = ("lyapunov_exponent", "fractal_dimension", "entropy")


def _ulps(a, b):
    """|a - b| in units of the fp32 spacing at b."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


def _check_against_oracle(vols, what, norms=True):
    """vols: a device tensor [n, ...] (3 or 4 dims).  Runs smk_volume_stats and compares every output with the oracle."""
    means, box, hist, d = volume_stats(vols, norms=norms)
    host = vols.cpu().numpy()
    means, box, hist = means.cpu().numpy(), box.cpu().numpy(), hist.cpu().numpy()
    n = host.shape[0]
    worst_ulp = 0.0
    for i in range(n):
        want_mean = mean_nd(host[i])
        u = float(_ulps(means[i], want_mean))
        worst_ulp = max(worst_ulp, u)
        _, counts, h = stats_nd(host[i], mean=means[i])
        assert u <= 1.0, (what, i, "mean", means[i], want_mean)
        assert box[i].tolist() == counts.tolist(), (what, i, "box counts", box[i], counts)
        assert np.array_equal(hist[i], h), (what, i, "histogram")
    worst_rel = 0.0
    if norms and n > 1:
        d = d.cpu().numpy()
        want = np.array([diff_norm(host[i], host[i + 1]) for i in range(n - 1)])
        worst_rel = float(np.max(np.abs(d - want) / np.maximum(want, 1e-300)))
        np.testing.assert_allclose(d, want, rtol=1e-6, atol=0, err_msg=what)
    else:
        assert d is None
    print(f"{what}: n={n} mean off by <= {worst_ulp:.2f} ulp, counts and histogram exact, norms rel err {worst_rel:.2e}")


def _values(shape, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.rand(*shape, device="cuda", generator=g)
    if kind == "sparse":
        return r ** 8 * 1.3                                              # mostly near zero, a few values above 1
    return r * 1.8                                                       # dense: every bin busy, 44 % above 1


# ---- 1. the 2-axis instance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(64, 64), (100, 76), (256, 256), (512, 512)])
def test_2d_instance_equals_smk_chaos_stats(hw):
    for kind in ("sparse", "dense"):
        f = _values((5, *hw), kind, 3)
        f[0, 0, :4] = torch.tensor([1.0, 1.5, -0.25, 0.0], device="cuda")   # exact 1.0 -> bin 255; above 1 and negative dropped
        f[1] = f[1] - 0.3                                                # many negatives
        m0, b0, h0 = chaos_stats(f)                                      # one workgroup per frame (csrc/chaos.hip)
        m1, b1, h1, d1 = volume_stats(f, norms=True)
        assert torch.equal(b0, b1) and torch.equal(h0, h1), (hw, kind)
        assert float(_ulps(m1.cpu().numpy(), m0.cpu().numpy()).max()) <= 1.0
        np.testing.assert_allclose(d1.cpu().numpy(), frame_diff_norms(f).cpu().numpy(), rtol=1e-6)
        _check_against_oracle(f, f"2-D {hw} {kind}")


def test_2d_instance_on_the_reference_fixture(golden):
    g = golden("chaos_stats_64.npz")
    f = torch.from_numpy(g["frames"]).cuda()
    m0, b0, h0 = chaos_stats(f)
    m1, b1, h1, d1 = volume_stats(f, norms=True)
    assert torch.equal(b0, b1) and torch.equal(h0, h1)
    assert float(_ulps(m1.cpu().numpy(), m0.cpu().numpy()).max()) <= 1.0
    assert b1[-1].tolist() == g["box_counts"].tolist() and h1[-1].tolist() == g["hist_counts"].tolist()
    assert float(_ulps(m1[-1].item(), np.float32(g["mean"]))) <= 1.0
    np.testing.assert_allclose(d1[-19:].cpu().numpy(), g["lyap_dists"], rtol=1e-6)


@pytest.mark.parametrize("hw", [(1024, 1024), (2048, 768)])
def test_2d_frames_above_the_old_ceiling(hw):
    for kind in ("sparse", "dense"):
        f = _values((3, *hw), kind, 5)
        _check_against_oracle(f, f"2-D {hw} {kind}")
        m, b, h = chaos_stats(f)                                         # raised before; now the public function routes it here
        m1, b1, h1, _ = volume_stats(f)
        assert torch.equal(m, m1) and torch.equal(b, b1) and torch.equal(h, h1)


# ---- 2. 3-D ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(13, 40, 70), (32, 32, 32), (33, 65, 129), (64, 128, 128)])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_3d_against_the_oracle(shape, n):
    for kind in ("sparse", "dense"):
        v = _values((n, *shape), kind, 7 + n)
        v[0, 0, 0, :2] = torch.tensor([1.0, -1.0], device="cuda")
        _check_against_oracle(v, f"3-D {shape} {kind}")
        _check_against_oracle(v, f"3-D {shape} {kind} (no norms)", norms=False)
    m, b, h = chaos_stats(v)                                             # the public 2-D functions accept volumes
    m1, b1, h1, d1 = volume_stats(v, norms=True)
    assert torch.equal(m, m1) and torch.equal(b, b1) and torch.equal(h, h1)
    if n > 1:
        assert torch.equal(frame_diff_norms(v), d1)


def test_3d_volumes_apart_and_misaligned():
    """A stride between volumes larger than a volume, and a base address that is not 16-byte aligned (the scalar-load form)."""
    big = _values((3, 2, 20, 40, 44), "sparse", 9)
    _check_against_oracle(big[:, 1], "3-D strided")                      # stride 2 volumes
    flat = _values((3 * 20 * 40 * 44 + 1,), "dense", 10)
    _check_against_oracle(flat[1:].view(3, 20, 40, 44), "3-D misaligned")


# ---- 3. full size ------------------------------------------------------------------------------------------------------------------------
def test_full_size_dense():
    v = _values((8, 64, 512, 512), "dense", 21)
    _check_against_oracle(v, "full size dense")


def test_full_size_stepper_volumes():
    sim = SmokeSimulator3D((64, 512, 512), batch_size=8)
    rng = np.random.RandomState(4)
    for b in range(8):
        for _ in range(1 + b % 3):
            sim.add_incense_source([(int(rng.randint(20, 492)), int(rng.randint(20, 492)), int(rng.randint(16, 48)))],
                                   [float(rng.uniform(0.5, 2.0))], grid=b)
    out = sim.simulate_sequence(3)                                       # [8, 3, 64, 512, 512]
    v = out[:, -1].contiguous()
    assert float(v.max()) > 0.1
    _check_against_oracle(v, "full size stepper")


# ---- 4. repeatability ----------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    for shape in [(6, 33, 65, 129), (4, 64, 256, 256), (4, 1024, 1024)]:
        v = _values(shape, "dense", 31)
        a = volume_stats(v, norms=True)
        for _ in range(3):
            b = volume_stats(v, norms=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), shape


# ---- 5. emit -----------------------------------------------------------------------------------------------------------------------------
def _sim_with_sources(shape, B):
    sim = NavierStokesSimulator3D(shape, batch_size=B)
    D, H, W = shape
    rng = np.random.RandomState(2)
    sim.add_smoke_sources([(b, int(rng.randint(8, W - 8)), int(rng.randint(8, H - 8)), int(rng.randint(2, D - 2)), 8, float(rng.uniform(0.5, 2.0)))
                           for b in range(B) for _ in range(1 + b)])
    return sim


def _emit(sim, frames, n_steps, add_fractal):
    fr = frames if frames.dim() == 5 else frames[:, None]
    _lib.check(_lib.load().smk_sim3d_step_emit(sim._handle, n_steps, fr.data_ptr(), fr.stride(0), fr.stride(1), int(add_fractal), 0.05,
                                               _lib.stream_ptr(sim._dev)))


def _state(sim):
    return [t.clone() for t in (sim._u, sim._v, sim._w, sim._p, sim._density)]


@pytest.mark.parametrize("shape", [(12, 64, 64), (9, 50, 50)])
def test_emit_without_fractal_is_the_plain_step(shape):
    B, T = 2, 3
    a, b = _sim_with_sources(shape, B), _sim_with_sources(shape, B)
    fa, fb = torch.empty(B, T, *shape, device="cuda"), torch.empty(B, T, *shape, device="cuda")
    a.step_into(fa, T)                                                   # smk_sim3d_step
    _emit(b, fb, T, add_fractal=False)
    assert torch.equal(fa, fb)
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))


@pytest.mark.parametrize("shape", [(12, 64, 64), (9, 50, 50)])
def test_emit_with_fractal(shape):
    from oracle import oracle
    B, T = 2, 3
    a, b = _sim_with_sources(shape, B), _sim_with_sources(shape, B)
    fa, fb = torch.empty(B, T, *shape, device="cuda"), torch.empty(B, T, *shape, device="cuda")
    a.step_into(fa, T)
    b.step_into(fb, T, add_fractal=True)
    assert float(fa.abs().max()) > 0.1
    want = FractalGenerator().apply_fractal_perturbation(fa, 0.05)       # smk_apply_fractal over the B * T * D slices
    assert torch.equal(fb, want) and not torch.equal(fb, fa)
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))  # the state keeps the unperturbed density
    # the oracle's apply_fractal_perturbation per depth plane.  Its arithmetic (three roundings) on the device's F: bit for bit.  With the
    # oracle's own F: the bar tests/test_config3_shapes.py holds the 2-D emitted frame to -- the device's Perlin constant differs from the
    # oracle's by up to 2 ulp (sinf / cosf), so no frame built on it can equal the oracle's in every bit, in 2-D or here.
    plain, got = fa.cpu().numpy(), fb.cpu().numpy()
    F_dev = FractalGenerator()._constants(shape[1:])[2].cpu().numpy()
    F = oracle.fractal_field(shape[1], shape[2])
    for idx in [(0, 0, 0), (1, T - 1, shape[0] // 2), (1, 1, shape[0] - 1)]:
        assert np.array_equal(got[idx], oracle.apply_fractal_perturbation(plain[idx], 0.05, F_dev)), idx
        err = rel_err(got[idx], oracle.apply_fractal_perturbation(plain[idx], 0.05, F))
        print(f"emit {shape} plane {idx}: rel err against the oracle with its own F {err:.2e}")
        assert err < 1e-6, idx


def test_emit_refuses_a_non_square_grid():
    sim = NavierStokesSimulator3D((8, 32, 48), batch_size=1)
    out = torch.empty(1, 8, 32, 48, device="cuda")
    with pytest.raises(_lib.SmokeHipError, match="square"):
        sim.step_into(out, 1, add_fractal=True)
    sim.step_into(out, 1)                                                # the plain step is fine


# ---- 6. SmokeSimulator3D -----------------------------------------------------------------------------------------------------------------
def _assert_features(got, want, what):
    assert set(got) == set(want) == set(NAMES), (what, got, want)
    g, w = [got[k] for k in NAMES], [want[k] for k in NAMES]
    print(f"{what}: device {g} oracle {w}")
    np.testing.assert_allclose(g, w, rtol=1e-3, atol=1e-6, err_msg=what)


def test_smoke_simulator3d_features_follow_the_history_oracle():
    shape, B = (16, 64, 64), 3
    sim = SmokeSimulator3D(shape, batch_size=B)
    sim.add_incense_source([(20, 24, 5)], [1.0], grid=0)
    sim.add_incense_source([(40, 30, 8), (25, 44, 10)], [1.7, 0.6], grid=1)
    sim.add_incense_source([(32, 32, 6), (22, 40, 11), (44, 21, 9)], [0.9, 1.2, 2.0], grid=2)
    hist = [[] for _ in range(B)]
    for step in range(1, 26):
        vol = sim.simulate_step()
        assert tuple(vol.shape) == (B, *shape)
        host = vol.cpu().numpy()
        for b in range(B):
            hist[b].append(host[b])
        if step == 9:
            assert sim.get_chaos_features() == [{} for _ in range(B)] and sim.get_chaos_features(as_tensor=True) is None
        if step in (10, 19, 20, 25):
            feats = sim.get_chaos_features()
            t = sim.get_chaos_features(as_tensor=True)
            assert t.dtype == torch.float64 and t.is_cuda and tuple(t.shape) == (B, 3)
            t = t.cpu().numpy()
            for b in range(B):
                want = history_features(hist[b])
                _assert_features(feats[b], want, f"step {step} grid {b}")
                _assert_features(dict(zip(NAMES, t[b])), feats[b], f"step {step} grid {b} as_tensor vs dict")
                if step < 20:
                    assert feats[b]["lyapunov_exponent"] == 0.0 and t[b, 0] == 0.0
    assert sim.history_len == 25
    # the three grids were given different sources: their features differ
    assert len({round(f["entropy"], 6) for f in sim.get_chaos_features()}) == B


def test_smoke_simulator3d_unbatched_returns_a_dict():
    shape = (16, 64, 64)
    sim = SmokeSimulator3D(shape)
    sim.add_incense_source([(30, 34, 7)], [1.5])
    vols = []
    assert sim.get_chaos_features() == {} and sim.compute_fractal_dimension() == 0.0 and sim.compute_entropy() == 0.0
    for _ in range(21):
        v = sim.simulate_step()
        assert tuple(v.shape) == shape
        vols.append(v.cpu().numpy())
    f = sim.get_chaos_features()
    assert isinstance(f, dict)
    _assert_features(f, history_features(vols), "un-batched")
    assert f == {"lyapunov_exponent": sim.compute_lyapunov_exponent(), "fractal_dimension": sim.compute_fractal_dimension(),
                 "entropy": sim.compute_entropy()}
    t = sim.get_chaos_features(as_tensor=True)
    assert tuple(t.shape) == (3,)
    _assert_features(dict(zip(NAMES, t.cpu().numpy())), f, "un-batched as_tensor")
    # the emitted volume is the perturbed one, the solver keeps the unperturbed density
    assert not np.array_equal(vols[-1], sim.ns_solver.density.cpu().numpy())
    plain = SmokeSimulator3D(shape)
    plain.add_incense_source([(30, 34, 7)], [1.5])
    v = plain.simulate_step(add_fractal=False)
    assert torch.equal(v, plain.ns_solver.density)


# ---- 7. SyntheticSmokeDataset3D --------------------------------------------------------------------------------------------------------
def _dataset(sim_batch, **kw):
    np.random.seed(0)
    return SyntheticSmokeDataset3D(5, (16, 64, 64), 20, sim_batch=sim_batch, **kw)


def test_dataset3d_chunking_labels_and_sharding():
    a, b = _dataset(2), _dataset(5)
    assert len(a) == len(b) == 5
    for x, y in zip(a.data, b.data):
        assert x["source_config"] == y["source_config"]
        assert torch.equal(x["sequence"], y["sequence"]) and tuple(x["sequence"].shape) == (20, 16, 64, 64)
        assert x["chaos_features"] == y["chaos_features"]
    # labels: the mean over t = 10..19 of the features the never-cleared history gives (sample i's window reaches into sample i-1)
    history = []
    for i, d in enumerate(a.data):
        seq = d["sequence"].cpu().numpy()
        feats = []
        for t in range(20):
            history.append(seq[t])
            history = history[-100:]
            if t >= 10:
                feats.append(history_features(history))
        want = {k: float(np.mean([f[k] for f in feats])) for k in NAMES}
        _assert_features(d["chaos_features"], want, f"sample {i}")
    assert a.data[1]["chaos_features"]["lyapunov_exponent"] != a.data[0]["chaos_features"]["lyapunov_exponent"]
    item = a[0]
    assert tuple(item["input"].shape) == tuple(item["target"].shape) == (1, 16, 64, 64)
    assert tuple(item["chaos_features"].shape) == (3,) and item["chaos_features"].dtype == torch.float32
    for rank in range(2):
        lo, hi = shard_range(5, rank, 2)
        part = _dataset(2, rank=rank, world=2)
        assert len(part) == hi - lo
        for x, y in zip(part.data, a.data[lo:hi]):
            assert torch.equal(x["sequence"], y["sequence"]) and x["chaos_features"] == y["chaos_features"]
            assert x["source_config"] == y["source_config"]
