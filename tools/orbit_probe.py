"""Times of the orbit render (csrc/render_orbit.hip, smk_volume_render_orbit; SPEC_3D.md section 10 "Orbit views") at BASELINE configs[4].

    python tools/orbit_probe.py [--batch 8] [--grid 64 512 512] [--reps 5] [--out profiles/r20/orbit_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and
max of the rounds are kept).  Per input kind (the stepper's own volumes after ~20 steps with sources; dense U(0, 1.8)) and per light
("none", "-y"):
  * render_orbit with one view at azimuth 0, 30 and 90 (image only, workspace reused), beside
      - render_volumes on the same volumes: the floor, one read of the volumes ("none") or two ("-y");
      - ONE read of the volumes at the copy rate bench.py measures (bench.hbm_copy_gbs);
      - the same image written as torch ops (grid_sample over the (z, x) plane with the rows y as channels, then the cumsum form) -- the
        baseline, not the code under test -- and the largest difference to it;
  * render_orbit with the 12 views of a turntable (0, 30, ..., 330) in one call, per view and against 12 times the mean single view: whether
    a turntable reads the volumes once or twelve times shows here.
A new operator: there is no earlier time to compare with.  No figure is asserted.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from render_probe import stepper_volumes, timed
from smokephysai_amd.physics import RenderSettings, orbit_samples, orbit_workspace, render_orbit, render_volumes, render_workspace

LIGHTS = ("none", "-y")
SINGLE = (0.0, 30.0, 90.0)
RING = tuple(float(a) for a in range(0, 360, 30))


def torch_orbit(v, phi, s):
    """The rule as torch ops, one volume at a time: grid_sample (bilinear, zeros outside, align_corners) of [1, H, D, W] -- the rows y as
    channels -- at the S x W sample positions, then render_probe's cumsum form over the samples."""
    n, D, H, W = v.shape
    S = orbit_samples(D, W)
    c, sn = math.cos(math.radians(phi)), math.sin(math.radians(phi))
    a = torch.arange(W, device=v.device, dtype=torch.float32)[None, :] - (W - 1) / 2
    t = torch.arange(S, device=v.device, dtype=torch.float32)[:, None] - (S - 1) / 2
    x = (W - 1) / 2 + (a * c + t * sn)
    z = (D - 1) / 2 + (t * c - a * sn)
    grid = torch.stack([2 * x / max(W - 1, 1) - 1, 2 * z / max(D - 1, 1) - 1], dim=-1)[None]         # [1, S, W, (x, z)]
    out = []
    for rho in v:
        rs = F.grid_sample(rho.permute(1, 0, 2)[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]      # [H, S, W]
        tau = torch.cumsum(rs, 1) - rs
        if s.light == "none":
            L = 1.0
        else:
            A = torch.cumsum(rs, 0) - rs if s.light == "+y" else torch.flip(torch.cumsum(torch.flip(rs, (0,)), 0), (0,)) - rs
            L = s.ambient + (1.0 - s.ambient) * torch.exp(-s.sigma_light * A)
        out.append(s.gain * (-torch.expm1(-s.sigma_view * rs) * L * torch.exp(-s.sigma_view * tau)).sum(1))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", type=int, nargs=3, default=[64, 512, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/r20/orbit_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("orbit_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    B, grid = args.batch, tuple(args.grid)
    D, H, W = grid
    vol_bytes, img_bytes = B * D * H * W * 4, B * H * W * 4
    copy_gbs = bench.hbm_copy_gbs(torch.device("cuda", 0))
    one_read_ms = vol_bytes / (copy_gbs * 1e9) * 1e3
    result = {"batch": B, "grid": list(grid), "samples_per_ray": orbit_samples(D, W), "volume_bytes": vol_bytes, "image_bytes": img_bytes,
              "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(),
              "copy_GBs": copy_gbs, "one_volume_read_ms": one_read_ms, "inputs": {}}
    print(f"copy rate {copy_gbs / 1e3:.2f} TB/s: one read of the {vol_bytes / 1e6:.0f} MB of volumes = {one_read_ms:.3f} ms", flush=True)
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)
    inputs = {"stepper_20_steps": stepper_volumes(B, grid, 20), "dense_u_0_1.8": torch.rand(B, *grid, device="cuda") * 1.8}
    one = torch.empty(B, H, W, device="cuda")
    ring = torch.empty(B, len(RING), H, W, device="cuda")
    for name, v in inputs.items():
        e = {"zero_share": float((v == 0).float().mean()), "lights": {}}
        for light in LIGHTS:
            s = RenderSettings(light=light)
            ws, fws = orbit_workspace(B, grid, light, "cuda"), render_workspace(B, grid, light, "cuda")
            floor = timed({"render_volumes": lambda: render_volumes(v, s, out=one, workspace=fws)}, **kw)["render_volumes"]
            r = {"render_volumes": floor, "workspace_bytes": 0 if ws is None else ws.numel() * 4, "single_view": {}}
            for phi in SINGLE:
                t = timed({"orbit": lambda: render_orbit(v, phi, s, out=one, workspace=ws)}, **kw)["orbit"]
                tt = timed({"torch": lambda: torch_orbit(v, phi, s)}, reps=1, warm=1, rounds=2)["torch"]
                err = float((render_orbit(v, phi, s) - torch_orbit(v, phi, s)).abs().max())
                r["single_view"][str(phi)] = {"render_orbit": t, "torch_ops": tt, "over_render_volumes": t["ms_median"] / floor["ms_median"],
                                              "over_one_volume_read": t["ms_median"] / one_read_ms,
                                              "torch_over_kernel": tt["ms_median"] / t["ms_median"], "max_abs_diff_to_torch": err}
                print(f"{name} light {light:>4} azimuth {phi:5.1f}: {t['ms_median']:.3f} ms = {t['ms_median'] / floor['ms_median']:.2f}x "
                      f"render_volumes ({floor['ms_median']:.3f} ms) = {t['ms_median'] / one_read_ms:.2f}x one read of the volumes; torch ops "
                      f"{tt['ms_median']:.1f} ms; max |diff| to torch {err:.1e}", flush=True)
            t12 = timed({"ring": lambda: render_orbit(v, RING, s, out=ring, workspace=ws)}, **kw)["ring"]
            singles = timed({str(phi): (lambda phi=phi: render_orbit(v, phi, s, out=one, workspace=ws)) for phi in RING}, **kw)
            sum_singles = sum(x["ms_median"] for x in singles.values())
            r["turntable_12_views"] = {"render_orbit": t12, "ms_per_view": t12["ms_median"] / len(RING), "twelve_single_calls_ms": sum_singles,
                                       "over_twelve_single_calls": t12["ms_median"] / sum_singles,
                                       "over_one_volume_read": t12["ms_median"] / one_read_ms}
            print(f"{name} light {light:>4} turntable of 12: {t12['ms_median']:.3f} ms = {t12['ms_median'] / len(RING):.3f} ms per view = "
                  f"{t12['ms_median'] / sum_singles:.2f}x twelve single calls ({sum_singles:.3f} ms)", flush=True)
            e["lights"][light] = r
        result["inputs"][name] = e
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
