"""Evaluation-suite timings: the image-quality kernel against the reference's torch formula, and the batched
physics_perturbation_test against a serial loop written in the reference's order.  Device-event timing after warm-up; one JSON
line per measurement, all of them also written to the path given as argv[1] (default eval_probe.json)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from smokephysai_amd.evaluation import PerturbationTester, RobustnessEvaluator
from smokephysai_amd.evaluation.robustness_metrics import plane_quality_sums, ssim_torch
from smokephysai_amd.models import SmokePhysNet
from smokephysai_amd.physics import SmokeSimulator

dev = torch.device("cuda:0")
results = []


def timed(fn, warmup=3, reps=20):
    """ms per call: device events around `reps` calls after `warmup`, the median of 3 such windows."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        windows.append(a.elapsed_time(b) / reps)
    return float(np.median(windows))


def emit(rec):
    results.append(rec)
    print(json.dumps(rec), flush=True)


# ---- 1. metrics: one kernel launch (+ the per-plane sum) vs the reference's ~20 torch ops ----------------------------
for N in (128, 256):
    torch.manual_seed(0)
    x = torch.rand(64, 1, N, N, device=dev)
    y = (x + 0.1 * torch.randn_like(x)).clamp(0, 1)
    ev = RobustnessEvaluator()

    def torch_formula():                     # compute_ssim + compute_psnr + mse as the reference runs them, values left on the device
        return ssim_torch(x, y, 11).mean(), 20 * torch.log10(1.0 / torch.sqrt(F.mse_loss(x, y))), F.mse_loss(x, y)

    def kernel():
        return plane_quality_sums(x, y, 11)

    t_torch, t_kernel = timed(torch_formula), timed(kernel)
    t_api = timed(lambda: (ev.compute_ssim(x, y), ev.compute_psnr(x, y)), reps=10)        # public surface, host floats
    t_api_torch = timed(lambda: (ssim_torch(x, y, 11).mean().item(), (20 * torch.log10(1.0 / torch.sqrt(F.mse_loss(x, y)))).item()),
                        reps=10)
    s, e = kernel()
    ref = ssim_torch(x, y, 11).double().mean().item()
    emit({"probe": "image_quality", "shape": [64, 1, N, N], "window": 11, "torch_ms": t_torch, "kernel_ms": t_kernel,
          "speedup": t_torch / t_kernel, "api_ms": t_api, "api_torch_ms": t_api_torch, "api_speedup": t_api_torch / t_api,
          "ssim_kernel_minus_torch": s.sum().item() / x.numel() - ref,
          "bytes_read_MB": 2 * x.numel() * 4 / 1e6, "kernel_GBps": 2 * x.numel() * 4 / (t_kernel * 1e-3) / 1e9})

# ---- 2. physics_perturbation_test(num_tests=50) at 128^2: batched vs the reference's serial order ---------------------
torch.manual_seed(0)
model = SmokePhysNet().to(dev).eval()
tester = PerturbationTester()


def serial(num_tests):
    sim = SmokeSimulator((128, 128), device="cuda")
    res = []
    with torch.no_grad():
        for _ in range(num_tests):
            sim.ns_solver.setup_grid()
            for _ in range(np.random.randint(1, 4)):
                x = np.random.randint(20, sim.ns_solver.w - 20)
                y = np.random.randint(20, sim.ns_solver.h - 20)
                sim.add_incense_source([(x, y)], [np.random.uniform(0.5, 2.0)])
            seq = [sim.simulate_step().unsqueeze(0).unsqueeze(0) for _ in range(20)]
            preds = [model(f)["physics_features"] for f in seq]
            res.append(torch.var(torch.stack(preds), dim=0).mean().item())
    return 1.0 / (1.0 + np.mean(res))


def batched(num_tests):
    return tester.physics_perturbation_test(model, SmokeSimulator((128, 128), device="cuda"), num_tests=num_tests)[
        "physics_prediction_stability"]


np.random.seed(0)
serial(2)
np.random.seed(0)
batched(2)                                   # warm-up: code objects, the batch-64 / batch-1 forward shapes
for name, fn in (("serial", serial), ("batched", batched), ("serial", serial), ("batched", batched)):
    np.random.seed(0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    val = fn(50)
    b.record()
    b.synchronize()
    emit({"probe": "physics_perturbation_test", "num_tests": 50, "grid": 128, "route": name, "ms": a.elapsed_time(b),
          "stability": val})
t = {r["route"]: min(q["ms"] for q in results if q.get("route") == r["route"]) for r in results if "route" in r}
emit({"probe": "physics_perturbation_test_summary", "serial_ms": t["serial"], "batched_ms": t["batched"],
      "speedup": t["serial"] / t["batched"]})

out = sys.argv[1] if len(sys.argv) > 1 else "eval_probe.json"
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(results, f, indent=1)
