"""Eval-mode input gradients: what the 'hip_grad' route costs against the PyTorch-ROCm module route it replaces.
  1. wall time of PerturbationTester.adversarial_test(num_steps=10) at 8 x 128^2 on the default model, input_grad "hip" and "torch", each in a
     fresh child process started before this process touches the GPU, with MIOpen pointed at an empty private find-db (utils/miopen_db.py):
     the "torch" figure includes the find pass a new user meets.  This pair decides SmokePhysNet.INPUT_GRAD_DEFAULT.
  2. smk_conv1_train_dgrad against aten.convolution_backward (dX only) at 8 x 128^2 and 64 x 256^2, with the kernel's GB/s of dz against
     the measured copy rate and its two floors (bytes of dz at the copy rate, flops at the fp32 vector rate).
  3. one PGD step (forward + input gradient, default model) at the same two shapes, the two settings interleaved.
Device events, the median of 5 windows after warm-up, one GPU process at a time.  Writes the JSON given by --out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12              # B/s, measured device copy rate
FP32_VECTOR_RATE = 157e12        # flop/s


def child(route: str, steps: int) -> None:
    t0 = time.perf_counter()
    from smokephysai_amd.utils.miopen_db import use_private_find_db
    db = use_private_find_db("input_grad_probe")                    # the parent hands an empty directory over in MIOPEN_USER_DB_PATH
    import torch

    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(input_grad=route).cuda().eval()
    x = torch.rand(8, 1, 128, 128, device="cuda")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = PerturbationTester().adversarial_test(model, x, epsilon=0.1, num_steps=steps)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(json.dumps({"route": route, "steps": steps, "adversarial_test_s": round(t2 - t1, 3), "process_s": round(t2 - t0, 3),
                      "find_db": db, "find_db_entries": sorted(os.listdir(db)), "result": res}), flush=True)


def run_child(route: str, steps: int) -> dict:
    with tempfile.TemporaryDirectory(prefix="miopen_probe_") as db:
        env = dict(os.environ, MIOPEN_USER_DB_PATH=db)
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, "--steps", str(steps)], env=env, capture_output=True,
                           text=True, timeout=900)
        wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(f"child {route} failed ({p.returncode}): {p.stderr[-2000:]}")
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    rec["launch_to_exit_s"] = round(wall, 3)
    rec.pop("find_db")
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "input_grad_probe.json"))
    ap.add_argument("--child", choices=("hip", "torch"))
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps)

    # ---- 1. fresh processes first: this process has not touched the GPU yet
    wall = [run_child(route, args.steps) for route in ("hip", "torch")]
    for rec in wall:
        print(json.dumps(rec), flush=True)

    import numpy as np
    import torch
    import torch.nn.functional as F

    import bench
    from smokephysai_amd import _lib
    from smokephysai_amd.models import SmokePhysNet
    dev = torch.device("cuda:0")
    L = _lib.load()

    def timed(fn, warmup=3, reps=10, windows=5):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / reps)
        return float(np.median(ms)), [round(float(m), 4) for m in ms]

    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "copy_rate_Bps": COPY_RATE,
              "fp32_vector_rate_flops": FP32_VECTOR_RATE, "adversarial_test_fresh_process": wall, "kernel": [], "pgd_step": []}

    # ---- 2. the kernel against aten.convolution_backward (dX only)
    for B, N in ((8, 128), (64, 256)):
        torch.manual_seed(0)
        dz = torch.randn(B, 64, N, N, device=dev)
        x = torch.rand(B, 1, N, N, device=dev)
        w = torch.randn(64, 1, 7, 7, device=dev) * 0.1
        dx = torch.empty_like(x)
        st = _lib.stream_ptr(dev)
        hip = lambda: _lib.check(L.smk_conv1_train_dgrad(dz.data_ptr(), w.data_ptr(), B, N, N, dx.data_ptr(), st))
        aten = lambda: torch.ops.aten.convolution_backward(dz, x, w, None, [1, 1], [3, 3], [1, 1], False, [0, 0], 1, [True, False, False])[0]
        hip()
        agree = float((dx - aten()).abs().max() / aten().abs().max())
        ms_hip, win_hip = timed(hip)
        ms_aten, win_aten = timed(aten)
        nbytes, flops = dz.numel() * 4, 2.0 * 64 * 49 * B * N * N
        rec = {"B": B, "N": N, "hip_ms": round(ms_hip, 4), "hip_windows": win_hip, "aten_ms": round(ms_aten, 4), "aten_windows": win_aten,
               "max_rel_diff": agree, "dz_GBps": round(nbytes / (ms_hip * 1e-3) / 1e9, 1), "dz_share_of_copy_rate": round(nbytes / (ms_hip * 1e-3) / COPY_RATE, 3),
               "byte_floor_ms": round(nbytes / COPY_RATE * 1e3, 4), "flop_floor_ms": round(flops / FP32_VECTOR_RATE * 1e3, 4)}
        result["kernel"].append(rec)
        print(json.dumps(rec), flush=True)
        del dz, x, dx

    # ---- 3. one PGD step on the default model, the two settings interleaved
    torch.manual_seed(0)
    model = SmokePhysNet().to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    import warnings
    warnings.filterwarnings("ignore", message="SmokePhysNet: eval forward with autograd")
    for B, N in ((8, 128), (64, 256)):
        data = torch.rand(B, 1, N, N, device=dev)
        target = data if N == 128 else F.avg_pool2d(data, 2)
        delta = torch.zeros_like(data, requires_grad=True)

        def step():
            out = model(torch.clamp(data + delta, 0, 1))
            (grad,) = torch.autograd.grad(-F.mse_loss(out["reconstructed"], target), delta)
            return grad

        for route in ("hip", "torch", "hip", "torch"):
            model.input_grad = route
            ms, win = timed(step, warmup=3, reps=3 if N == 256 else 10)
            rec = {"B": B, "N": N, "input_grad": route, "ms": round(ms, 3), "windows": win}
            result["pgd_step"].append(rec)
            print(json.dumps(rec), flush=True)
        del data, delta
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
