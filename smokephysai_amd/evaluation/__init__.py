"""Evaluation utilities -- drop-in for the reference's src/evaluation package (RobustnessEvaluator, PerturbationTester), and the optical-flow
baselines of its benchmark.py (optical_flow.py)."""
from .optical_flow import farneback_optical_flow, lucas_kanade_optical_flow, predict_next_frame, to_uint8_frames
from .perturbation_tests import PerturbationTester
from .robustness_metrics import RobustnessEvaluator, plane_ssim

__all__ = ["PerturbationTester", "RobustnessEvaluator", "farneback_optical_flow", "lucas_kanade_optical_flow", "plane_ssim",
           "predict_next_frame", "to_uint8_frames"]
