"""smokephysai_amd.evaluation on the MI355X: the image-quality kernel (csrc/quality.hip) against a float64 numpy statement of the
reference's SSIM / MSE / PSNR formulas and against the reference's recorded numbers, and the batched perturbation tests against
serial loops written in the reference's order."""
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err
from smokephysai_amd.evaluation import PerturbationTester, RobustnessEvaluator
from smokephysai_amd.evaluation.perturbation_tests import draw_scenarios
from smokephysai_amd.evaluation.robustness_metrics import kernel_supported, plane_quality_sums

pytestmark = pytest.mark.gpu

C1, C2 = 0.01 ** 2, 0.03 ** 2
SHAPES = [(1, 1, 128, 128), (64, 1, 128, 128), (3, 2, 37, 53), (2, 1, 8, 8)]
WINDOWS = [1, 3, 7, 11, 31]


# ---- float64 oracle: the reference's formulas (robustness_metrics.py:76-105) -------------------------------------------
def _box_mean(a, k):
    """avg_pool2d(a, k, stride=1, padding=k//2) with count_include_pad (zeros outside, divisor k^2), odd k, in float64."""
    p = k // 2
    lead = [(0, 0)] * (a.ndim - 2)
    c = np.cumsum(np.cumsum(np.pad(a, lead + [(p, p), (p, p)]), -1), -2)
    c = np.pad(c, lead + [(1, 0), (1, 0)])
    H, W = a.shape[-2:]
    return (c[..., k:k + H, k:k + W] - c[..., :H, k:k + W] - c[..., k:k + H, :W] + c[..., :H, :W]) / (k * k)


def _oracle(x, y, k):
    x, y = x.astype(np.float64), y.astype(np.float64)
    m1, m2 = _box_mean(x, k), _box_mean(y, k)
    s11 = _box_mean(x * x, k) - m1 * m1
    s22 = _box_mean(y * y, k) - m2 * m2
    s12 = _box_mean(x * y, k) - m1 * m2
    ssim_map = ((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s11 + s22 + C2))
    mse = ((x - y) ** 2).mean()
    return ssim_map.mean(), mse, 20 * np.log10(1 / np.sqrt(mse))


def _pair(shape, seed):
    rng = np.random.RandomState(seed)
    x = rng.rand(*shape).astype(np.float32)
    y = np.clip(x + 0.1 * rng.randn(*shape), 0, 1).astype(np.float32)
    return x, y


# ---- image-quality kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_float64_formula(shape):
    x, y = _pair(shape, sum(shape))
    px, py = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ev = RobustnessEvaluator()
    for k in WINDOWS:
        assert kernel_supported(px, py, k)
        o_ssim, o_mse, o_psnr = _oracle(x, y, k)
        assert abs(ev.compute_ssim(px, py, window_size=k) - o_ssim) <= 2e-6, k
        r = ev.image_quality(px, py, window_size=k)
        assert abs(float(r["mse"].mean()) - o_mse) <= 1e-6 * o_mse, k
    assert abs(ev.compute_psnr(px, py) - o_psnr) <= 1e-4


@pytest.mark.parametrize("shape", [(2, 1, 8, 8), (3, 2, 37, 53)], ids=lambda s: "x".join(map(str, s)))
def test_identical_images_give_ssim_one_and_psnr_inf(shape):
    x = torch.rand(*shape, device="cuda")
    ev = RobustnessEvaluator()
    for k in (1, 11, 31):
        assert abs(ev.compute_ssim(x, x.clone(), window_size=k) - 1.0) <= 1e-6
    assert ev.compute_psnr(x, x.clone()) == float("inf")
    assert torch.isinf(ev.image_quality(x, x.clone())["psnr"]).all()


@pytest.mark.parametrize("case", ["a", "b"])
def test_kernel_matches_the_reference_recorded_numbers(golden, case):
    g = golden("evaluation_metrics_ref.npz")
    px, py = torch.from_numpy(g[f"{case}_pred"]).cuda(), torch.from_numpy(g[f"{case}_target"]).cuda()
    ev = RobustnessEvaluator()
    for k in (3, 11):
        assert abs(ev.compute_ssim(px, py, window_size=k) - float(g[f"{case}_ssim_k{k}"])) <= 2e-6, k
    assert abs(ev.compute_psnr(px, py) - float(g[f"{case}_psnr"])) <= 1e-4
    mse = float(ev.image_quality(px, py)["mse"].mean())
    assert abs(mse - float(g[f"{case}_mse"])) <= 1e-6 * float(g[f"{case}_mse"])
    # the even window is not the kernel's: it takes the torch formula (map (H+1) x (W+1)) and gives the reference's number
    assert not kernel_supported(px, py, 4)
    assert abs(ev.compute_ssim(px, py, window_size=4) - float(g[f"{case}_ssim_k4"])) <= 1e-6


def test_two_calls_are_bit_identical():
    x, y = _pair((64, 1, 128, 128), 7)
    px, py = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    a = plane_quality_sums(px, py, 11)
    b = plane_quality_sums(px, py, 11)
    assert a[0].shape == (64, 1) and a[0].dtype == torch.float64
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_image_quality_per_image_agrees_with_compute_ssim():
    x, y = _pair((5, 2, 64, 48), 11)
    px, py = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ev = RobustnessEvaluator()
    q = ev.image_quality(px, py, window_size=7)
    assert q["ssim"].shape == q["mse"].shape == q["psnr"].shape == (5,)
    for b in range(5):
        assert abs(float(q["ssim"][b]) - ev.compute_ssim(px[b:b + 1], py[b:b + 1], window_size=7)) <= 1e-12
        assert abs(float(q["psnr"][b]) - ev.compute_psnr(px[b:b + 1], py[b:b + 1])) <= 1e-9
    # evaluate_reconstruction_quality's numbers are the same launch's
    class _Recon(torch.nn.Module):
        def forward(self, t):
            return {"reconstructed": t}
    r = ev.evaluate_reconstruction_quality(_Recon(), px, py)
    assert set(r) == {"ssim", "psnr", "mse"} and all(isinstance(v, float) for v in r.values())
    assert abs(r["ssim"] - ev.compute_ssim(px, py)) <= 1e-12 and abs(r["psnr"] - ev.compute_psnr(px, py)) <= 1e-9


# ---- perturbation tests -----------------------------------------------------------------------------------------
def _model():
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    return SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()


def _serial_reference_loop(model, simulator, scenarios):
    """perturbation_tests.py:100-146 in the reference's order: one un-batched simulator, one scenario after another, batch-1
    forwards.  Returns frames [T, 20, H, W], features [T, 20, 3] and the per-scenario prediction variances."""
    frames, feats, variances = [], [], []
    with torch.no_grad():
        for sources in scenarios:
            simulator.ns_solver.setup_grid()
            for x, y, intensity in sources:
                simulator.add_incense_source([(x, y)], [intensity])
            seq = [simulator.simulate_step().clone() for _ in range(20)]
            preds = [model(f.unsqueeze(0).unsqueeze(0))["physics_features"] for f in seq]
            variances.append(torch.var(torch.stack(preds), dim=0).mean().item())
            frames.append(torch.stack(seq))
            feats.append(torch.cat(preds))
    return torch.stack(frames), torch.stack(feats), variances


def test_physics_perturbation_test_matches_the_serial_loop():
    from smokephysai_amd.physics import SmokeSimulator
    model = _model()
    tester = PerturbationTester()
    num_tests = 6
    np.random.seed(0)
    scenarios = draw_scenarios(num_tests, 128, 128)
    serial_sim = SmokeSimulator((128, 128), device="cuda")
    s_frames, s_feats, s_var = _serial_reference_loop(model, serial_sim, scenarios)

    rollout_sim = SmokeSimulator((128, 128), device="cuda")
    frames, feats = tester.perturbation_rollout(model, rollout_sim, scenarios)
    assert frames.shape == (num_tests, 20, 128, 128) and feats.shape == (num_tests, 20, 3)
    assert torch.equal(frames, s_frames), "batched frames differ from the serial loop's"
    assert rel_err(feats.cpu().numpy(), s_feats.cpu().numpy()) <= 1e-4

    caller = SmokeSimulator((128, 128), device="cuda")
    np.random.seed(0)
    res = tester.physics_perturbation_test(model, caller, num_tests=num_tests)
    assert set(res) == {"physics_prediction_stability", "num_tests"} and res["num_tests"] == num_tests
    assert abs(res["physics_prediction_stability"] - 1.0 / (1.0 + np.mean(s_var))) <= 1e-5
    for name in ("u", "v", "p", "density"):
        assert torch.equal(getattr(caller.ns_solver, name), getattr(serial_sim.ns_solver, name)), name
    assert len(caller.history) == len(serial_sim.history) == 100
    assert torch.equal(caller.history[-1], serial_sim.history[-1]) and torch.equal(caller.history[0], serial_sim.history[0])

    with pytest.raises(ValueError):
        tester.physics_perturbation_test(model, SmokeSimulator((128, 128), device="cuda", batch_size=2), num_tests=2)


def test_gaussian_noise_test_matches_a_serial_restatement():
    model = _model()
    x = torch.rand(4, 1, 128, 128, device="cuda")
    levels = [0.01, 0.05, 0.1, 0.2]
    torch.manual_seed(5)
    got = PerturbationTester().gaussian_noise_test(model, x, levels, batch_size=8)
    torch.manual_seed(5)                                   # the documented order: all draws first, in level order
    noisy = [torch.clamp(x + torch.randn_like(x) * lv, 0, 1) for lv in levels]
    with torch.no_grad():
        base = model(x)
        assert set(got) == {f"gaussian_{lv}" for lv in levels}
        for lv, nx in zip(levels, noisy):
            out = model(nx)
            fs = torch.nn.functional.cosine_similarity(base["latent_features"], out["latent_features"], dim=1).mean().item()
            mse = torch.nn.functional.mse_loss(out["reconstructed"], base["reconstructed"]).item()
            assert set(got[f"gaussian_{lv}"]) == {"feature_stability", "reconstruction_mse"}
            assert abs(got[f"gaussian_{lv}"]["feature_stability"] - fs) <= 1e-4, lv
            assert abs(got[f"gaussian_{lv}"]["reconstruction_mse"] - mse) <= 1e-4, lv


class _RecordInputs(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.inputs = []

    def forward(self, x):
        self.inputs.append(x.detach().clone())
        return self.inner(x)


def test_adversarial_test_keys_bounds_and_no_parameter_grads():
    model = _RecordInputs(_model())
    x = torch.rand(2, 1, 128, 128, device="cuda")
    eps = 0.1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = PerturbationTester().adversarial_test(model, x, epsilon=eps, num_steps=3)
    assert not any("eval forward with autograd" in str(m.message) for m in w)
    assert set(res) == {"adversarial_feature_stability", "adversarial_perturbation_norm"}
    # calls: 3 attack steps, then the baseline and the adversarial input clamp(x + delta, 0, 1)
    assert len(model.inputs) == 5 and torch.equal(model.inputs[3], x)
    moved = (model.inputs[4] - x).abs()
    assert float(moved.max()) <= eps + 1e-6 and float(moved.max()) > 0        # |clamp(x + delta) - x| <= |delta|_inf <= eps
    assert 0 < res["adversarial_perturbation_norm"] <= eps * np.sqrt(x.numel()) * (1 + 1e-6)
    assert np.isfinite(res["adversarial_feature_stability"])
    assert all(p.grad is None for p in model.parameters())
    assert all(p.requires_grad for p in model.parameters())
