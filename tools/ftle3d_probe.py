"""Times of the 3-D flow map and its FTLE field (physics.flow_map_step3d, ftle_field3d, flow_ftle3d; csrc/flow_map3d.hip; DESIGN.md
section 3.15), in the protocol of tools/ftle_probe.py.

    python tools/ftle3d_probe.py [--reps 5] [--rounds 3] [--out profiles/r33/ftle3d_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and max
of the rounds are kept); the variants of one shape alternate inside a round.  Per shape (8 x 64 x 512^2 and 8 x 16 x 128^2, J = 20), on the
stepper's own state after 10 steps with two sources per grid:
  * smk_flow_map3d_step in both directions on the stepper's padded velocity stores, from the displacement 8 steps of flow_ftle3d leave,
    beside a device-to-device copy of twelve volumes (six read, six written).  A call itself moves nine (u, v, w, three components in,
    three out) and gathers six of them through eight taps: the copy is the even count next above, a memory-bound yardstick;
  * smk_ftle3d_field on that displacement (three volumes in, one out, and the statistics);
  * 20 steps of flow_ftle3d in both directions against 20 bare steps of the stepper, with the mean and maximum FTLE the batch shows;
  * at the small shape only, route="torch" (the rule on the GPU: the baseline, not the code under test).
A new operator: there is no earlier time to compare with.  No figure is asserted.  Not measured: kernel times under a profiler, and the
torch route at the large shape."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from render_probe import timed
from smokephysai_amd import _lib
from smokephysai_amd.physics import flow_ftle3d
from step3d_grad_probe import DT, SHAPES, VISCOSITY, stepper_state

DIRECTIONS = ("backward", "forward")
STEPS = 20
TORCH_ROUTE_UP_TO = 8 * 16 * 128 * 128            # cells: the torch route is timed at the small shape only


def entry_point_times(sim, disp, kw):
    """The ABI calls as flow_ftle3d makes them: the map step on the stepper's stores, the FTLE on a dense displacement."""
    L = _lib.load()
    B, _, D, H, W = disp.shape
    dev = disp.device
    st = _lib.stream_ptr(dev)
    out = torch.empty_like(disp)
    ftle = torch.empty(B, D, H, W, device=dev)
    stats = torch.empty(B, 2, dtype=torch.float64, device=dev)
    nbytes = int(L.smk_ftle3d_workspace(B, D, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    fns = {}
    for code, direction in enumerate(DIRECTIONS):
        fns[f"smk_flow_map3d_step_{direction}"] = (lambda code=code: _lib.check(L.smk_flow_map3d_step(
            code, sim._u.data_ptr(), sim._v.data_ptr(), sim._w.data_ptr(), disp.data_ptr(), out.data_ptr(), B, D, H, W, sim._pc, sim._pv, W,
            DT, st)))
    fns["smk_ftle3d_field"] = lambda: _lib.check(L.smk_ftle3d_field(disp.data_ptr(), ftle.data_ptr(), stats.data_ptr(), B, D, H, W, W,
                                                                   STEPS * DT, ws.data_ptr(), nbytes, st))
    src = torch.empty(B * D * H * W * 6, device=dev).normal_()
    dst = torch.empty_like(src)
    fns["copy_of_twelve_volumes"] = lambda: dst.copy_(src)               # reads six volumes and writes six
    t = timed(fns, **kw)
    t["bytes_moved_by_a_map_step"] = 4 * B * D * H * W * 9
    t["bytes_moved_by_the_copy"] = 4 * B * D * H * W * 12
    t["map_step_over_copy"] = {d: t[f"smk_flow_map3d_step_{d}"]["ms_median"] / t["copy_of_twelve_volumes"]["ms_median"] for d in DIRECTIONS}
    return t


def measure_shape(B, D, H, W, J, kw):
    sim, state = stepper_state(B, D, H, W, J)
    settings = dict(dt=DT, viscosity=VISCOSITY, jacobi_iters=J)
    disp = flow_ftle3d(*state, 8, **settings).displacement
    r = {"batch": B, "grid": [D, H, W], "jacobi_iters": J, "entry_points": entry_point_times(sim, disp, kw)}
    e = r["entry_points"]
    print(f"{B} x {D}x{H}x{W}, J={J}: map step " + ", ".join(f"{d} {e[f'smk_flow_map3d_step_{d}']['ms_median']:.4f} ms" for d in DIRECTIONS) +
          f", copy of twelve volumes {e['copy_of_twelve_volumes']['ms_median']:.4f} ms; ftle field {e['smk_ftle3d_field']['ms_median']:.4f} ms",
          flush=True)
    kept = {}
    with_torch = B * D * H * W <= TORCH_ROUTE_UP_TO

    def run(direction, route):
        kept[direction, route] = flow_ftle3d(*state, STEPS, direction=direction, route=route, **settings)
    fns = {"bare_steps": lambda: sim.step_into(None, STEPS)}
    for direction in DIRECTIONS:
        fns[f"hip_{direction}"] = lambda direction=direction: run(direction, "hip")
    if with_torch:
        fns["torch_backward"] = lambda: run("backward", "torch")
    t = timed(fns, reps=1, warm=1, rounds=kw["rounds"])
    r["flow_ftle3d_20_steps"] = f = {
        **t, "hip_over_bare_steps": {d: t[f"hip_{d}"]["ms_median"] / t["bare_steps"]["ms_median"] for d in DIRECTIONS},
        "ftle": {d: {"mean_min": float(kept[d, "hip"].mean.min()), "mean_max": float(kept[d, "hip"].mean.max()),
                     "max_min": float(kept[d, "hip"].max.min()), "max_max": float(kept[d, "hip"].max.max())} for d in DIRECTIONS}}
    line = (f"    20 steps: bare {t['bare_steps']['ms_median']:.3f} ms; flow_ftle3d " +
            ", ".join(f"{d} {t[f'hip_{d}']['ms_median']:.3f} ms ({f['hip_over_bare_steps'][d]:.3f}x)" for d in DIRECTIONS))
    if with_torch:
        hip, ref = kept["backward", "hip"], kept["backward", "torch"]
        f["torch_over_hip_backward"] = t["torch_backward"]["ms_median"] / t["hip_backward"]["ms_median"]
        f["max_rel_diff_between_routes"] = float((hip.ftle - ref.ftle).abs().max() / ref.ftle.abs().max())
        line += (f"; torch backward {t['torch_backward']['ms_median']:.3f} ms = {f['torch_over_hip_backward']:.1f}x; routes differ by "
                 f"{f['max_rel_diff_between_routes']:.1e}")
    else:
        f["torch_route"] = "not measured at this shape"
    print(line + f"; backward ftle mean {f['ftle']['backward']['mean_min']:.2e} .. {f['ftle']['backward']['mean_max']:.2e}, max "
          f"{f['ftle']['backward']['max_min']:.2e} .. {f['ftle']['backward']['max_max']:.2e}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/r33/ftle3d_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ftle3d_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)
    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "reps": args.reps, "rounds": args.rounds,
              "kernel_times_under_a_profiler": "not measured",
              "shapes": [measure_shape(*shape, kw) for shape in SHAPES]}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
