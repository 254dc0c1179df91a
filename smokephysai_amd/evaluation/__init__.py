"""Evaluation utilities -- drop-in for the reference's src/evaluation package (RobustnessEvaluator, PerturbationTester)."""
from .perturbation_tests import PerturbationTester
from .robustness_metrics import RobustnessEvaluator

__all__ = ["PerturbationTester", "RobustnessEvaluator"]
