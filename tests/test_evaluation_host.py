"""CPU checks of smokephysai_amd.evaluation: the public surface of the reference's src/evaluation package (names, parameters,
defaults), the scenario draws of physics_perturbation_test, and the torch-formula route of the metrics against the reference's
own recorded outputs (tests/golden/evaluation_*.npz, written by tests/golden/generate_evaluation_golden.py)."""
import inspect

import numpy as np
import pytest
import torch

from smokephysai_amd.evaluation import PerturbationTester, RobustnessEvaluator
from smokephysai_amd.evaluation.perturbation_tests import draw_scenarios

_EMPTY = inspect.Parameter.empty

# (method, [(parameter, default)]) of the reference's classes, positional-or-keyword parameters after self
REFERENCE_SURFACE = {
    RobustnessEvaluator: {
        "__init__": [("device", "cuda")],
        "evaluate_physics_consistency": [("model", _EMPTY), ("test_data", _EMPTY), ("physics_targets", _EMPTY)],
        "evaluate_reconstruction_quality": [("model", _EMPTY), ("test_data", _EMPTY), ("targets", _EMPTY)],
        "compute_ssim": [("pred", _EMPTY), ("target", _EMPTY), ("window_size", 11), ("sigma", 1.5)],
        "compute_psnr": [("pred", _EMPTY), ("target", _EMPTY)],
    },
    PerturbationTester: {
        "__init__": [("device", "cuda")],
        "gaussian_noise_test": [("model", _EMPTY), ("test_data", _EMPTY), ("noise_levels", [0.01, 0.05, 0.1, 0.2])],
        "adversarial_test": [("model", _EMPTY), ("test_data", _EMPTY), ("epsilon", 0.1), ("num_steps", 10)],
        "physics_perturbation_test": [("model", _EMPTY), ("simulator", _EMPTY), ("num_tests", 50)],
    },
}


@pytest.mark.parametrize("cls", list(REFERENCE_SURFACE), ids=lambda c: c.__name__)
def test_public_surface_matches_the_reference(cls):
    import smokephysai_amd.evaluation.perturbation_tests as pt
    import smokephysai_amd.evaluation.robustness_metrics as rm
    assert getattr({RobustnessEvaluator: rm, PerturbationTester: pt}[cls], cls.__name__) is cls
    for method, want in REFERENCE_SURFACE[cls].items():
        params = list(inspect.signature(getattr(cls, method)).parameters.values())[1:]
        positional = [(p.name, p.default) for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert positional == want, (method, positional)
        # additions are keyword-only and defaulted, so a reference call site binds identically
        assert all(p.kind == p.KEYWORD_ONLY and p.default is not _EMPTY for p in params if p.kind != p.POSITIONAL_OR_KEYWORD), method
    assert cls(device="cpu").device == "cpu" and cls().device == "cuda"


def test_new_batched_arguments_are_keyword_only():
    for method in ("gaussian_noise_test", "physics_perturbation_test"):
        p = inspect.signature(getattr(PerturbationTester, method)).parameters["batch_size"]
        assert p.kind == p.KEYWORD_ONLY and p.default == 64
    assert inspect.signature(RobustnessEvaluator.image_quality).parameters["window_size"].default == 11


def test_scenario_draws_reproduce_the_reference(golden):
    g = golden("evaluation_scenarios_seed0.npz")
    h, w = (int(v) for v in g["grid"])
    np.random.seed(0)
    scenarios = draw_scenarios(int(g["num_tests"]), h, w)
    assert len(scenarios) == int(g["num_tests"]) == 50
    flat = [(t, x, y, i) for t, s in enumerate(scenarios) for (x, y, i) in s]
    assert [r[0] for r in flat] == g["test"].tolist()
    assert [r[1] for r in flat] == g["x"].tolist()
    assert [r[2] for r in flat] == g["y"].tolist()
    assert [r[3] for r in flat] == g["intensity"].tolist()            # bit-identical doubles


@pytest.mark.parametrize("case", ["a", "b"])
def test_torch_route_reproduces_the_reference_metrics(golden, case):
    g = golden("evaluation_metrics_ref.npz")
    pred, target = torch.from_numpy(g[f"{case}_pred"]), torch.from_numpy(g[f"{case}_target"])
    ev = RobustnessEvaluator(device="cpu")
    for k in (3, 4, 11):
        got = ev.compute_ssim(pred, target, window_size=k)
        assert isinstance(got, float)
        assert abs(got - float(g[f"{case}_ssim_k{k}"])) <= 1e-7, k
    psnr = ev.compute_psnr(pred, target)
    assert isinstance(psnr, float) and abs(psnr - float(g[f"{case}_psnr"])) <= 1e-7 * max(1.0, abs(psnr))
    q = ev.image_quality(pred, target, window_size=11)
    assert set(q) == {"ssim", "mse", "psnr"} and q["ssim"].shape == (pred.shape[0],)
    assert abs(float(q["ssim"].mean()) - float(g[f"{case}_ssim_k11"])) <= 1e-6       # equal images: the mean of per-image means
    assert abs(float(q["mse"].mean()) - float(g[f"{case}_mse"])) <= 1e-7


def test_torch_route_psnr_of_identical_images_is_inf():
    x = torch.rand(2, 1, 16, 16)
    assert RobustnessEvaluator(device="cpu").compute_psnr(x, x.clone()) == float("inf")
