"""Times of the 3-D chaos-statistics path (csrc/chaos_nd.hip, SmokeSimulator3D, SyntheticSmokeDataset3D) at BASELINE configs[4].

    python tools/chaos3d_probe.py [--batch 8] [--grid 64 512 512] [--reps 20] [--out profiles/r10/chaos3d_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and
max of the rounds are kept), the variants of one comparison alternating inside a round.  Reported per input kind (the stepper's own
volumes after ~20 steps with sources; dense U(0, 1.8)):
  * smk_volume_stats with and without the norms;
  * the same statistics written as torch ops (mean, >, amax over reshaped views for the five scales, histc, norm of the difference) --
    the baseline: it is not the code under test;
  * the byte floor: the bytes the kernel's passes read (3 reads of the batch with norms, 2 without) over the copy rate measured here
    (a device-to-device copy_ of the same batch: bytes read + bytes written over its time);
and once: SmokeSimulator3D.simulate_step against the bare step_into, the 2-axis instance against smk_chaos_stats at 64 x 256^2 and
64 x 512^2, and SyntheticSmokeDataset3D samples/s at (64, 128, 128).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smokephysai_amd.physics import NavierStokesSimulator3D, SmokeSimulator3D
from smokephysai_amd.physics.smoke_simulator import chaos_stats, frame_diff_norms, volume_stats, volume_stats_workspace
from smokephysai_amd.utils.data_loader import SyntheticSmokeDataset3D


def timed(fns, reps, warm, rounds):
    """ms per call of every function in `fns` (name -> callable): the functions alternate inside a round."""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            res[k].append(a.elapsed_time(b) / reps)
    return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in res.items()}


def torch_stats(v, norms):
    """The statistics as torch ops: what a user without the kernel would write (fp32 mean; counts, histogram and norms as torch defines them)."""
    n, D, H, W = v.shape
    mean = v.mean(dim=(1, 2, 3), keepdim=True)
    binary = (v > mean).view(torch.uint8)                                # amax has no bool form
    counts = []
    for s in (2, 4, 8, 16, 32):
        d, h, w = D // s, H // s, W // s
        b = binary[:, :d * s, :h * s, :w * s].reshape(n, d, s, h, s, w, s)
        counts.append(b.amax(dim=(2, 4, 6)).sum(dim=(1, 2, 3)))
    hist = torch.stack([torch.histc(v[i], bins=256, min=0.0, max=1.0) for i in range(n)])
    d = (v[1:] - v[:-1]).flatten(1).norm(dim=1) if norms else None
    return mean, counts, hist, d


def stepper_volumes(B, grid, steps):
    sim = NavierStokesSimulator3D(grid, batch_size=B)
    D, H, W = grid
    rng = np.random.RandomState(0)
    m = min(20, D // 4)
    sim.add_smoke_sources([(b, int(rng.randint(20, W - 20)), int(rng.randint(20, H - 20)), int(rng.randint(m, D - m)), 8,
                            float(rng.uniform(0.5, 2.0))) for b in range(B) for _ in range(1 + b % 3)])
    out = torch.empty(B, *grid, device="cuda")
    for _ in range(steps):
        sim.step_into(out, 1, add_fractal=(H == W))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", type=int, nargs=3, default=[64, 512, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dataset-samples", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chaos3d_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    B, grid = args.batch, tuple(args.grid)
    cells = grid[0] * grid[1] * grid[2]
    batch_bytes = B * cells * 4
    result = {"batch": B, "grid": list(grid), "batch_bytes": batch_bytes, "reps": args.reps, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp()}
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)

    # the copy rate of this device on this batch
    src = torch.rand(B, *grid, device="cuda")
    dst = torch.empty_like(src)
    cp = timed({"copy": lambda: dst.copy_(src)}, **kw)["copy"]
    rate = 2 * batch_bytes / (cp["ms_median"] * 1e-3)
    result["copy"] = dict(cp, bytes_per_s=rate)
    print(f"copy of {batch_bytes / 1e6:.0f} MB: {cp['ms_median']:.3f} ms = {rate / 1e12:.2f} TB/s (read + write)", flush=True)
    del dst

    ws = volume_stats_workspace(B, grid, "cuda")
    inputs = {"stepper_20_steps": stepper_volumes(B, grid, 20), "dense_u_0_1.8": src * 1.8}
    del src
    result["inputs"] = {}
    for name, v in inputs.items():
        zero_share = float((v == 0).float().mean())
        t = timed({"volume_stats_norms": lambda: volume_stats(v, norms=True, workspace=ws),
                   "volume_stats": lambda: volume_stats(v, workspace=ws),
                   "torch_norms": lambda: torch_stats(v, True),
                   "torch": lambda: torch_stats(v, False)}, **kw)
        floor = {"volume_stats_norms": 3 * batch_bytes / rate * 1e3, "volume_stats": 2 * batch_bytes / rate * 1e3}
        e = {"zero_share": zero_share, "times": t, "byte_floor_ms": floor,
             "torch_over_kernel_norms": t["torch_norms"]["ms_median"] / t["volume_stats_norms"]["ms_median"],
             "torch_over_kernel": t["torch"]["ms_median"] / t["volume_stats"]["ms_median"],
             "kernel_over_floor_norms": t["volume_stats_norms"]["ms_median"] / floor["volume_stats_norms"],
             "kernel_over_floor": t["volume_stats"]["ms_median"] / floor["volume_stats"]}
        result["inputs"][name] = e
        print(f"{name} ({zero_share * 100:.0f} % zeros): smk_volume_stats {t['volume_stats_norms']['ms_median']:.3f} ms with norms "
              f"({e['kernel_over_floor_norms']:.2f}x the byte floor {floor['volume_stats_norms']:.3f} ms), {t['volume_stats']['ms_median']:.3f} ms "
              f"without ({e['kernel_over_floor']:.2f}x {floor['volume_stats']:.3f} ms); torch ops {t['torch_norms']['ms_median']:.2f} / "
              f"{t['torch']['ms_median']:.2f} ms = {e['torch_over_kernel_norms']:.1f}x / {e['torch_over_kernel']:.1f}x the kernel", flush=True)
    del inputs, v

    # simulate_step (step + one statistics call over {previous, current} + the returned copy) against the bare step
    sim = SmokeSimulator3D(grid, batch_size=B)
    rng = np.random.RandomState(0)
    for b in range(B):
        sim.add_incense_source([(int(rng.randint(20, grid[2] - 20)), int(rng.randint(20, grid[1] - 20)), grid[0] // 2)], [1.0], grid=b)
    frame = torch.empty(B, *grid, device="cuda")
    square = grid[1] == grid[2]
    t = timed({"step_into": lambda: sim.ns_solver.step_into(frame, 1),
               "step_into_fractal": lambda: sim.ns_solver.step_into(frame, 1, add_fractal=square),
               "simulate_step": lambda: sim.simulate_step(add_fractal=square),
               "simulate_step_no_copy": lambda: sim.simulate_step(add_fractal=square, copy=False)}, reps=5, warm=3, rounds=args.rounds)
    result["simulate_step"] = dict(t, over_step_into=t["simulate_step"]["ms_median"] / t["step_into"]["ms_median"],
                                   fractal_emit_over_plain=t["step_into_fractal"]["ms_median"] / t["step_into"]["ms_median"])
    print("step: " + ", ".join(f"{k} {x['ms_median']:.3f} ms" for k, x in t.items()), flush=True)
    del sim, frame

    # the 2-axis instance against the one-workgroup-per-frame kernels
    result["frames_2d"] = {}
    for N in (256, 512):
        f = torch.rand(64, N, N, device="cuda") ** 8 * 1.3
        ws2 = volume_stats_workspace(64, (N, N), "cuda")
        t = timed({"smk_chaos_stats+diff_norms": lambda: (chaos_stats(f), frame_diff_norms(f)),
                   "smk_chaos_stats": lambda: chaos_stats(f),
                   "volume_stats_norms": lambda: volume_stats(f, norms=True, workspace=ws2),
                   "volume_stats": lambda: volume_stats(f, workspace=ws2)}, **kw)
        result["frames_2d"][f"64x{N}x{N}"] = t
        print(f"64 x {N}^2: " + ", ".join(f"{k} {x['ms_median']:.3f} ms" for k, x in t.items()), flush=True)

    # the dataset
    n = args.dataset_samples
    rates = []
    for rep in range(4):                                                  # the first generation is the warm-up
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = SyntheticSmokeDataset3D(n, (64, 128, 128), 20, sim_batch=8)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(ds) == n
        del ds
        if rep:
            rates.append(n / dt)
    result["dataset3d_64x128x128"] = {"samples": n, "volumes_per_sample": 20, "sim_batch": 8, "samples_per_s_median": statistics.median(rates),
                                      "samples_per_s_all": rates}
    print(f"SyntheticSmokeDataset3D (64,128,128): {statistics.median(rates):.1f} samples/s ({n} samples x 20 volumes, 3 generations)", flush=True)

    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
