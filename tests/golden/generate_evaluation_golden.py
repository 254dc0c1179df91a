#!/usr/bin/env python3
"""Golden-vector generator for the evaluation package (developer tool; never collected by pytest, never run on a GPU).

Imports the upstream SmokePhysAI implementation (its `src` package, CPU only; its robustness_metrics module needs
scikit-learn) and records two small .npz fixtures next to this script:

  evaluation_metrics_ref.npz      seeded pred / target arrays and the upstream RobustnessEvaluator's own compute_ssim /
                                  compute_psnr and F.mse_loss outputs for windows 3, 4 (even: the map is (H+1) x (W+1)) and 11
  evaluation_scenarios_seed0.npz  the smoke sources upstream's PerturbationTester.physics_perturbation_test adds after
                                  np.random.seed(0) (num_tests=50, 128^2 grid), captured with a recording stub simulator and a
                                  stub model

Run:
    python tests/golden/generate_evaluation_golden.py --reference <path to an upstream SmokePhysAI checkout>
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
WINDOWS = (3, 4, 11)
CASES = {"a": (2, 1, 32, 32), "b": (3, 2, 19, 27)}


def metrics_fixture(RobustnessEvaluator):
    ev = RobustnessEvaluator(device="cpu")
    rng = np.random.RandomState(1234)
    out = {}
    for name, shape in CASES.items():
        pred = rng.rand(*shape).astype(np.float32)
        target = np.clip(pred + 0.1 * rng.randn(*shape), 0, 1).astype(np.float32)
        p, t = torch.from_numpy(pred), torch.from_numpy(target)
        out[f"{name}_pred"], out[f"{name}_target"] = pred, target
        for k in WINDOWS:
            out[f"{name}_ssim_k{k}"] = np.float64(ev.compute_ssim(p, t, window_size=k))
        out[f"{name}_psnr"] = np.float64(ev.compute_psnr(p, t))
        out[f"{name}_mse"] = np.float64(torch.nn.functional.mse_loss(p, t).item())
    np.savez_compressed(os.path.join(HERE, "evaluation_metrics_ref.npz"), **out)


class _RecordingSolver:
    def __init__(self, h, w):
        self.h, self.w = h, w
        self.resets = 0

    def setup_grid(self):
        self.resets += 1


class _RecordingSimulator:
    """Stands in for SmokeSimulator: records every add_incense_source call in the order it is made (per test)."""

    def __init__(self, h=128, w=128):
        self.ns_solver = _RecordingSolver(h, w)
        self.sources = []             # (test index, x, y, intensity)

    def add_incense_source(self, positions, intensities):
        for (x, y), inten in zip(positions, intensities):
            self.sources.append((self.ns_solver.resets - 1, x, y, inten))

    def simulate_step(self):
        return torch.zeros(self.ns_solver.h, self.ns_solver.w)


class _StubModel(torch.nn.Module):
    def forward(self, x):
        return {"physics_features": torch.zeros(x.shape[0], 3)}


def scenarios_fixture(PerturbationTester, num_tests=50):
    sim = _RecordingSimulator()
    np.random.seed(0)
    PerturbationTester(device="cpu").physics_perturbation_test(_StubModel(), sim, num_tests=num_tests)
    s = sim.sources
    np.savez_compressed(os.path.join(HERE, "evaluation_scenarios_seed0.npz"),
                        num_tests=np.int64(num_tests), grid=np.array([128, 128], np.int64),
                        test=np.array([r[0] for r in s], np.int64), x=np.array([r[1] for r in s], np.int64),
                        y=np.array([r[2] for r in s], np.int64), intensity=np.array([r[3] for r in s], np.float64))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of an upstream SmokePhysAI checkout (the directory holding src/)")
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.abspath(args.reference))
    from src.evaluation.perturbation_tests import PerturbationTester
    from src.evaluation.robustness_metrics import RobustnessEvaluator
    torch.set_num_threads(1)
    metrics_fixture(RobustnessEvaluator)
    scenarios_fixture(PerturbationTester)
    print("wrote evaluation_metrics_ref.npz, evaluation_scenarios_seed0.npz")


if __name__ == "__main__":
    main()
