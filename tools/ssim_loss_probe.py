"""SSIM-loss timings (DESIGN.md 8.1 "Gradient"): `ssim_loss` forward + backward on csrc/quality.hip against the reference's torch formula
(`ssim_torch`) under torch's autograd, at 64 x 1 x 128^2 and 64 x 1 x 256^2, window 11, in one process with the two sides alternated.
Device-event timing after warm-up, five windows per side; one JSON line per measurement, all of them also written to the path given as
argv[1] (default profiles/r23/ssim_loss_probe.json).  Needs a ROCm GPU: there is no CPU timing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from smokephysai_amd.evaluation.robustness_metrics import ssim_torch
from smokephysai_amd.models.losses import ssim_loss

if not torch.cuda.is_available():
    raise SystemExit("ssim_loss_probe: no ROCm GPU; nothing is measured on the CPU")
dev = torch.device("cuda:0")
WINDOW, WARMUP, REPS, WINDOWS = 11, 5, 50, 5
results = []


def window_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


for N in (128, 256):
    torch.manual_seed(0)
    target = torch.rand(64, 1, N, N, device=dev)
    pred = (target + 0.1 * torch.randn_like(target)).clamp(0, 1).requires_grad_()

    def kernel_step():
        pred.grad = None
        ssim_loss(pred, target, WINDOW).backward()

    def torch_step():
        pred.grad = None
        (1 - ssim_torch(pred, target, WINDOW).mean((-2, -1)).mean()).backward()

    kernel_step()
    g_kernel = pred.grad.clone()
    torch_step()
    g_torch = pred.grad.clone()
    for _ in range(WARMUP):
        kernel_step()
        torch_step()
    torch.cuda.synchronize()
    t_kernel, t_torch = [], []
    for _ in range(WINDOWS):                                       # alternated: both sides see the same clock and neighbours
        t_kernel.append(window_ms(kernel_step))
        t_torch.append(window_ms(torch_step))
    rec = {"probe": "ssim_loss_forward_backward", "shape": [64, 1, N, N], "window": WINDOW, "reps_per_window": REPS,
           "kernel_ms": float(np.median(t_kernel)), "kernel_ms_windows": t_kernel,
           "torch_ms": float(np.median(t_torch)), "torch_ms_windows": t_torch,
           "speedup": float(np.median(t_torch) / np.median(t_kernel)),
           "grad_max_abs_diff_over_max": float((g_kernel - g_torch).abs().max() / g_torch.abs().max()),
           # pred and target read by both launches, three coefficient planes written and read, dpred written
           "kernel_min_bytes_MB": pred.numel() * 4 * (2 + 2 + 3 + 3 + 1) / 1e6}
    results.append(rec)
    print(json.dumps(rec), flush=True)

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23", "ssim_loss_probe.json")
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(results, f, indent=1)
