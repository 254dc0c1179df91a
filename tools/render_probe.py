"""Times of the volume render (csrc/render.hip, smk_volume_render; SPEC_3D.md section 10) at BASELINE configs[4].

    python tools/render_probe.py [--batch 8] [--grid 64 512 512] [--reps 20] [--out profiles/r16/render_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and
max of the rounds are kept), the variants of one comparison alternating inside a round.  Per input kind (the stepper's own volumes after
~20 steps with sources; dense U(0, 1.8)) and per light:
  * render_volumes (image only, workspace reused): ms, the compulsory bytes (one read of the volumes + one write of the images) over that
    time, and the time beside ONE read of the volumes at the copy rate bench.py measures (bench.hbm_copy_gbs);
  * the same image written as torch ops (cumsum / exp / expm1 / sum) -- the baseline, not the code under test;
and once: SmokeSimulator3D.simulate_frames against the bare step_into of as many steps, and the share of RenderedSmokeDataset pixels in
[0.02, 0.98] under the default settings.  No figure is asserted.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smokephysai_amd.physics import NavierStokesSimulator3D, RenderSettings, SmokeSimulator3D, render_volumes, render_workspace
from smokephysai_amd.utils.data_loader import RenderedSmokeDataset

LIGHTS = ("none", "+z", "+y", "-y")


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


def torch_render(v, s):
    """The rule as torch ops, one volume of the batch at a time (the temporaries of the whole batch would be several GB)."""
    out = []
    for rho in v:
        tau = torch.cumsum(rho, 0) - rho
        if s.light == "none":
            L = 1.0
        else:
            if s.light == "+z":
                A = tau
            elif s.light == "+y":
                A = torch.cumsum(rho, 1) - rho
            else:
                A = torch.flip(torch.cumsum(torch.flip(rho, (1,)), 1), (1,)) - rho
            L = s.ambient + (1.0 - s.ambient) * torch.exp(-s.sigma_light * A)
        out.append(s.gain * (-torch.expm1(-s.sigma_view * rho) * L * torch.exp(-s.sigma_view * tau)).sum(0))
    return torch.stack(out)


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
    ap.add_argument("--frames-steps", type=int, default=4)
    ap.add_argument("--dataset-samples", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    B, grid = args.batch, tuple(args.grid)
    D, H, W = grid
    vol_bytes, img_bytes = B * D * H * W * 4, B * H * W * 4
    copy_gbs = bench.hbm_copy_gbs(torch.device("cuda", 0))
    one_read_ms = vol_bytes / (copy_gbs * 1e9) * 1e3
    result = {"batch": B, "grid": list(grid), "volume_bytes": vol_bytes, "image_bytes": img_bytes, "reps": args.reps, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "copy_GBs": copy_gbs, "one_volume_read_ms": one_read_ms}
    print(f"copy rate {copy_gbs / 1e3:.2f} TB/s: one read of the {vol_bytes / 1e6:.0f} MB of volumes = {one_read_ms:.3f} ms", flush=True)
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)

    inputs = {"stepper_20_steps": stepper_volumes(B, grid, 20), "dense_u_0_1.8": torch.rand(B, *grid, device="cuda") * 1.8}
    out = torch.empty(B, H, W, device="cuda")
    result["inputs"] = {}
    for name, v in inputs.items():
        e = {"zero_share": float((v == 0).float().mean()), "lights": {}}
        for light in LIGHTS:
            s = RenderSettings(light=light)
            ws = render_workspace(B, grid, light, "cuda")
            t = timed({"render_volumes": lambda: render_volumes(v, s, out=out, workspace=ws)}, **kw)["render_volumes"]
            tt = timed({"torch": lambda: torch_render(v, s)}, reps=2, warm=1, rounds=3)["torch"]
            err = float((render_volumes(v, s) - torch_render(v, s)).abs().max())
            r = {"render_volumes": t, "torch_ops": tt, "compulsory_GBs": (vol_bytes + img_bytes) / (t["ms_median"] * 1e-3) / 1e9,
                 "over_one_volume_read": t["ms_median"] / one_read_ms, "torch_over_kernel": tt["ms_median"] / t["ms_median"],
                 "max_abs_diff_to_torch": err, "workspace_bytes": 0 if ws is None else ws.numel() * 4}
            e["lights"][light] = r
            print(f"{name} light {light:>4}: {t['ms_median']:.3f} ms = {r['compulsory_GBs'] / 1e3:.2f} TB/s of compulsory bytes, "
                  f"{r['over_one_volume_read']:.2f}x one read of the volumes ({one_read_ms:.3f} ms); torch ops {tt['ms_median']:.1f} ms = "
                  f"{r['torch_over_kernel']:.0f}x; max |diff| to torch {err:.1e}", flush=True)
        result["inputs"][name] = e
    del inputs, v

    # simulate_frames (steps + renders, chunked) against the bare steps
    sim = SmokeSimulator3D(grid, batch_size=B)
    rng = np.random.RandomState(0)
    for b in range(B):
        sim.add_incense_source([(int(rng.randint(20, W - 20)), int(rng.randint(20, H - 20)), D // 2)], [1.0], grid=b)
    n = args.frames_steps
    vols = torch.empty(B, n, *grid, device="cuda")
    frames = torch.empty(B, n, H, W, device="cuda")
    square = H == W
    t = timed({"step_into": lambda: sim.ns_solver.step_into(vols, n, add_fractal=square),
               "simulate_frames": lambda: sim.simulate_frames(n, add_fractal=square, out=frames, chunk=n)}, reps=2, warm=1, rounds=args.rounds)
    result["simulate_frames"] = dict(t, steps=n, over_step_into=t["simulate_frames"]["ms_median"] / t["step_into"]["ms_median"])
    print(f"{n} steps: step_into {t['step_into']['ms_median']:.2f} ms, simulate_frames {t['simulate_frames']['ms_median']:.2f} ms "
          f"({result['simulate_frames']['over_step_into']:.3f}x)", flush=True)
    del sim, vols, frames

    # how much of the rendered dataset's pictures is neither black nor saturated
    np.random.seed(0)
    ds = RenderedSmokeDataset(args.dataset_samples, (16, 128, 128), 20, sim_batch=args.dataset_samples)
    px = torch.stack([d["sequence"] for d in ds.data])
    share = float(((px >= 0.02) & (px <= 0.98)).float().mean())
    result["dataset_16x128x128"] = {"samples": len(ds), "frames_per_sample": 20, "pixel_share_in_0.02_0.98": share, "max": float(px.max()),
                                    "share_above_0.98": float((px > 0.98).float().mean())}
    print(f"RenderedSmokeDataset (16,128,128), {len(ds)} samples x 20 frames: {share * 100:.1f} % of the pixels in [0.02, 0.98], "
          f"max {float(px.max()):.3f}", flush=True)

    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
