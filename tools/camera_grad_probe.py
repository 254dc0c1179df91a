"""Times of the free-camera render's gradient (csrc/render_camera_grad.hip, smk_volume_render_camera_backward; SPEC_3D.md section 10 "Free
camera -- Gradient") at BASELINE configs[4].

    python tools/camera_grad_probe.py [--batch 8] [--grid 64 512 512] [--reps 3] [--out profiles/r25/camera_grad_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and
max of the rounds are kept).  On the stepper's own volumes after ~20 steps with sources and on dense data (uniform random: no empty
chunk to skip), per light ("none", "-y"):
  * forward + backward of render_camera(..., differentiable=True) with one view at (azimuth, elevation) = (0,0), (30,30) and (-123,-60),
    and with a ring of 12 azimuths (0, 30, ..., 330) at elevation 30 in one call, beside
      - render_camera's own forward time for the same views (alternating in one round): how many forwards the gradient is worth;
      - one read and one write of the volumes at the copy rate bench.py measures (bench.hbm_copy_gbs): the floor of any gradient that
        reads rho and writes drho;
      - for the single views on the stepper's volumes, forward + backward of torch autograd over the torch-op form of the render that
        tools/camera_probe.py has (grid_sample + the cumsum form; its backward scatters with atomics) -- the baseline, not the code
        under test -- and the largest difference between the two gradients.
A new operator: there is no earlier time to compare with.  No figure is asserted.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from camera_probe import torch_camera
from render_probe import stepper_volumes, timed
from smokephysai_amd.physics import RenderSettings, camera_backward_workspace, camera_samples, camera_workspace, render_camera

LIGHTS = ("none", "-y")
SINGLE = ((0.0, 0.0), (30.0, 30.0), (-123.0, -60.0))
RING = tuple(float(a) for a in range(0, 360, 30))
RING_ELEVATION = 30.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", type=int, nargs=3, default=[64, 512, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-autograd baseline (several GB of temporaries per volume)")
    ap.add_argument("--no-dense", action="store_true", help="skip the dense data")
    ap.add_argument("--out", default="profiles/r25/camera_grad_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camera_grad_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    B, grid = args.batch, tuple(args.grid)
    D, H, W = grid
    vol_bytes = B * D * H * W * 4
    copy_gbs = bench.hbm_copy_gbs(torch.device("cuda", 0))
    floor_ms = 2 * vol_bytes / (copy_gbs * 1e9) * 1e3
    result = {"batch": B, "grid": list(grid), "samples_per_ray": camera_samples(D, H, W), "volume_bytes": vol_bytes, "reps": args.reps,
              "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "copy_GBs": copy_gbs,
              "read_plus_write_of_the_volumes_ms": floor_ms, "data": {}}
    print(f"copy rate {copy_gbs / 1e3:.2f} TB/s: one read and one write of the {vol_bytes / 1e6:.0f} MB of volumes = {floor_ms:.3f} ms", flush=True)
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)
    gen = torch.Generator(device="cuda").manual_seed(1)
    kinds = [("stepper", lambda: stepper_volumes(B, grid, 20))]
    if not args.no_dense:
        kinds.append(("dense", lambda: torch.rand(B, *grid, device="cuda", generator=gen)))
    for kind, make in kinds:
        vols = make()
        leaf = vols.clone().requires_grad_(True)
        result["data"][kind] = {"nonzero_share": float((vols != 0).float().mean()), "lights": {}}
        for light in LIGHTS:
            s = RenderSettings(light=light)
            ws = camera_workspace(B, grid, light, "cuda")
            bws = camera_backward_workspace(B, grid, light, "cuda")
            r = {"forward_workspace_bytes": 0 if ws is None else ws.numel() * 4, "backward_workspace_bytes": bws.numel() * 4, "views": {}}

            def measure(name, az, el, G, with_torch):
                def both():
                    leaf.grad = None
                    render_camera(leaf, az, el, s, workspace=ws, differentiable=True).backward(G)

                def forward():
                    with torch.no_grad():
                        render_camera(vols, az, el, s, workspace=ws)
                t = timed({"forward_backward": both, "forward": forward}, **kw)
                e = {"forward_backward": t["forward_backward"], "forward": t["forward"],
                     "forwards_worth": t["forward_backward"]["ms_median"] / t["forward"]["ms_median"],
                     "over_read_plus_write": t["forward_backward"]["ms_median"] / floor_ms,
                     "torch_autograd": "not measured", "torch_over_kernel": "not measured", "max_abs_diff_to_torch": "not measured"}
                line = (f"{kind:>7} light {light:>4} {name}: forward + backward {t['forward_backward']['ms_median']:.3f} ms, forward "
                        f"{t['forward']['ms_median']:.3f} ms = {e['forwards_worth']:.1f} forwards' worth, "
                        f"{e['over_read_plus_write']:.1f}x one read + one write of the volumes")
                if with_torch:
                    def torch_both():
                        leaf.grad = None
                        torch_camera(leaf, az, el, s).backward(G)
                    try:
                        tt = timed({"torch": torch_both}, reps=1, warm=1, rounds=2)["torch"]
                        want = leaf.grad.clone()
                        both()
                        e.update(torch_autograd=tt, torch_over_kernel=tt["ms_median"] / t["forward_backward"]["ms_median"],
                                 max_abs_diff_to_torch=float((leaf.grad - want).abs().max()))
                        line += (f"; torch autograd {tt['ms_median']:.1f} ms = {e['torch_over_kernel']:.1f}x; max |diff| "
                                 f"{e['max_abs_diff_to_torch']:.1e}")
                    except torch.cuda.OutOfMemoryError:           # its temporaries are [S, H, W] per volume and op: stays "not measured"
                        line += "; torch autograd: out of memory"
                leaf.grad = None
                print(line, flush=True)
                r["views"][name] = e
            for phi, theta in SINGLE:
                measure(f"view ({phi}, {theta})", phi, theta, torch.randn(B, H, W, device="cuda", generator=gen),
                        kind == "stepper" and not args.no_torch)
            measure(f"ring of 12 at elevation {RING_ELEVATION}", RING, RING_ELEVATION,
                    torch.randn(B, len(RING), H, W, device="cuda", generator=gen), False)
            result["data"][kind]["lights"][light] = r
        del vols, leaf
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
