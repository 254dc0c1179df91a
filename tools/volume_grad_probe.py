"""Input gradients for volumes: what Encoder3D's 'frozen' route costs against the PyTorch-ROCm module route it replaces.
  1. wall time of PerturbationTester.adversarial_test(num_steps=10) on a default SmokePhysNet3D at 8 x (16,128,128), input_grad "hip" and
     "torch", each in a fresh child process started before this process touches the GPU, with MIOpen pointed at an empty private find-db
     (utils/miopen_db.py): the "torch" figure includes the find pass a new user meets.  The child then repeats the call: the second
     figure is the warm cost, and the difference what the first pass (code loading, MIOpen's find) adds.
  2. smk_conv3d_s7_dgrad against aten.convolution_backward (dX only) of nn.Conv3d(1, 64, 7, padding 3) at the same shape and at
     2 x (8,64,64), the two alternated window by window, with the kernel's two floors: bytes of dz1 at the measured copy rate, and
     43,904 flop per voxel at the fp32 MFMA peak (the pipe the kernel uses; the vector ALUs have the same peak).
  3. one PGD step on the default model at 8 x (16,128,128), the two settings alternated.
Device events, the median of 5 windows after warm-up with the spread beside it, one GPU process at a time.  Writes the JSON given by --out."""
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
FP32_MFMA_RATE = 157e12          # flop/s: 256 CUs x 4 SIMDs x 64 flop per clock x 2.4 GHz
FLOP_PER_VOXEL = 2 * 343 * 64    # 43,904
SHAPE = (8, 16, 128, 128)


def child(route: str, steps: int) -> None:
    t0 = time.perf_counter()
    from smokephysai_amd.utils.miopen_db import use_private_find_db
    db = use_private_find_db("volume_grad_probe")                   # the parent hands an empty directory over in MIOPEN_USER_DB_PATH
    import torch

    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet3D
    torch.manual_seed(0)
    model = SmokePhysNet3D(input_grad=route).cuda().eval()
    B, D, H, W = SHAPE
    x = torch.rand(B, 1, D, H, W, device="cuda")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = PerturbationTester().adversarial_test(model, x, epsilon=0.1, num_steps=steps)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    # a second call in the same process: everything is warm (kernels loaded, MIOpen's choices made)
    res2 = PerturbationTester().adversarial_test(model, x, epsilon=0.1, num_steps=steps)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(json.dumps({"route": route, "steps": steps, "shape": list(SHAPE), "first_call_s": round(t2 - t1, 3), "second_call_s": round(t3 - t2, 3),
                      "process_s": round(t3 - t0, 3), "find_db": db, "find_db_entries": sorted(os.listdir(db)), "result": res,
                      "result_second": res2}), flush=True)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "volume_grad_probe.json"))
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
    from smokephysai_amd.models import SmokePhysNet3D
    from smokephysai_amd.models.encoder3d import hip_conv3d_s7_dgrad
    from smokephysai_amd.physics.render import render_volumes
    dev = torch.device("cuda:0")

    def window(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def alternated(fns: dict, warmup=3, reps=10, windows=5):
        """The candidates window by window in turn, so that a drift of the machine meets all of them alike."""
        for fn in fns.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(windows):
            for k, fn in fns.items():
                ms[k].append(window(fn, reps))
        return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                    "windows": [round(float(m), 4) for m in v]} for k, v in ms.items()}

    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "copy_rate_Bps": COPY_RATE,
              "fp32_mfma_rate_flops": FP32_MFMA_RATE, "adversarial_test_fresh_process": wall, "kernel": [], "pgd_step": []}

    # ---- 2. the kernel against aten.convolution_backward (dX only)
    for B, D, H, W in ((2, 8, 64, 64), SHAPE):
        torch.manual_seed(0)
        dz_cl = torch.randn(B, D, H, W, 64, device=dev) * (torch.rand(B, D, H, W, 64, device=dev) < 0.5)
        dz_nc = dz_cl.permute(0, 4, 1, 2, 3).contiguous()            # aten's layout, made outside the timed region
        x = torch.rand(B, 1, D, H, W, device=dev)
        w = torch.randn(64, 1, 7, 7, 7, device=dev) * 0.05
        hip = lambda: hip_conv3d_s7_dgrad(dz_cl, w)
        aten = lambda: torch.ops.aten.convolution_backward(dz_nc, x, w, None, [1, 1, 1], [3, 3, 3], [1, 1, 1], False, [0, 0, 0], 1,
                                                           [True, False, False])[0]
        ref = aten()[:, 0]
        agree = float((hip() - ref).abs().max() / ref.abs().max())
        t = alternated({"hip": hip, "aten": aten}, reps=10 if B * D * H * W < (1 << 20) else 3)
        voxels, nbytes = B * D * H * W, dz_cl.numel() * 4
        ms = t["hip"]["median_ms"]
        rec = {"shape": [B, D, H, W], "hip": t["hip"], "aten_dX": t["aten"], "max_rel_diff": agree,
               "byte_floor_ms": round(nbytes / COPY_RATE * 1e3, 4), "flop_floor_ms": round(voxels * FLOP_PER_VOXEL / FP32_MFMA_RATE * 1e3, 4),
               "counted_TFLOPs": round(voxels * FLOP_PER_VOXEL / (ms * 1e-3) / 1e12, 2),
               "share_of_floor": round(max(nbytes / COPY_RATE, voxels * FLOP_PER_VOXEL / FP32_MFMA_RATE) * 1e3 / ms, 3)}
        result["kernel"].append(rec)
        print(json.dumps(rec), flush=True)
        del dz_cl, dz_nc, x, ref
        torch.cuda.empty_cache()

    # ---- 3. one PGD step on the default model, the two settings alternated
    torch.manual_seed(0)
    model = SmokePhysNet3D().to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    B, D, H, W = SHAPE
    data = torch.rand(B, 1, D, H, W, device=dev)
    target = render_volumes(data[:, 0].contiguous())[:, None]        # 128 x 128: the head's size
    delta = torch.zeros_like(data, requires_grad=True)

    def step_on(route):
        def step():
            model.input_grad = route
            out = model(torch.clamp(data + delta, 0, 1))
            (grad,) = torch.autograd.grad(-F.mse_loss(out["reconstructed"], target), delta)
            return grad
        return step

    t = alternated({"hip": step_on("hip"), "torch": step_on("torch")}, warmup=2, reps=3)
    for route, rec in t.items():
        rec = dict({"shape": list(SHAPE), "input_grad": route}, **rec)
        result["pgd_step"].append(rec)
        print(json.dumps(rec), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
