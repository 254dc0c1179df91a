"""Times of the flow map and its FTLE field (physics.flow_map_step, ftle_field, flow_ftle; csrc/flow_map.hip).

    python tools/ftle_probe.py [--reps 5] [--rounds 3] [--out profiles/r32/ftle_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and max
of the rounds are kept); the variants of one shape alternate inside a round.  Per shape (64 x 256^2 with J = 100, 32 x 128^2 with J = 20),
on the stepper's own state after 10 steps with two sources per grid:
  * smk_flow_map_step in both directions on the stepper's padded velocity stores, from the displacement 8 steps of flow_ftle leave, beside
    a device-to-device copy of the bytes a call moves (u, v, two planes in, two planes out: six planes of H x W): which of the two the
    kernel is closer to;
  * smk_ftle_field on that displacement (two planes in, one out, and the statistics);
  * 20 steps of flow_ftle in both directions (host status check and synchronisation at the end included) against 20 bare steps of the
    stepper, and against route="torch" (the rule on the GPU: the baseline, not the code under test), with the mean and maximum FTLE
    the batch shows.
A new operator: there is no earlier time to compare with.  No figure is asserted.  Kernel times under a profiler: not measured."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from render_probe import timed
from smokephysai_amd import _lib
from smokephysai_amd.physics import flow_ftle
from step_grad_probe import DT, SHAPES, VISCOSITY, stepper_state

DIRECTIONS = ("backward", "forward")
STEPS = 20


def entry_point_times(sim, disp, kw):
    """The ABI calls as flow_ftle makes them: the map step on the stepper's stores, the FTLE on a dense displacement."""
    L = _lib.load()
    B, _, H, W = disp.shape
    dev = disp.device
    st = _lib.stream_ptr(dev)
    out = torch.empty_like(disp)
    ftle = torch.empty(B, H, W, device=dev)
    stats = torch.empty(B, 2, dtype=torch.float64, device=dev)
    nbytes = int(L.smk_ftle_workspace(B, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    fns = {}
    for code, direction in enumerate(DIRECTIONS):
        fns[f"smk_flow_map_step_{direction}"] = (lambda code=code: _lib.check(L.smk_flow_map_step(
            code, sim._u.data_ptr(), sim._v.data_ptr(), disp.data_ptr(), out.data_ptr(), B, H, W, sim._pc, sim._pv, W, DT, st)))
    fns["smk_ftle_field"] = lambda: _lib.check(L.smk_ftle_field(disp.data_ptr(), ftle.data_ptr(), stats.data_ptr(), B, H, W, W, STEPS * DT,
                                                               ws.data_ptr(), nbytes, st))
    src = torch.empty(B * H * W * 3, device=dev).normal_()
    dst = torch.empty_like(src)
    fns["copy_of_a_map_steps_bytes"] = lambda: dst.copy_(src)            # reads three planes and writes three: six in all
    t = timed(fns, **kw)
    t["bytes_moved_by_a_map_step"] = 4 * B * H * W * 6
    t["map_step_over_copy"] = {d: t[f"smk_flow_map_step_{d}"]["ms_median"] / t["copy_of_a_map_steps_bytes"]["ms_median"] for d in DIRECTIONS}
    return t


def measure_shape(B, H, W, J, kw):
    sim, state = stepper_state(B, H, W, J)
    settings = dict(dt=DT, viscosity=VISCOSITY, jacobi_iters=J)
    disp = flow_ftle(*state, 8, **settings).displacement
    r = {"batch": B, "grid": [H, W], "jacobi_iters": J, "entry_points": entry_point_times(sim, disp, kw)}
    e = r["entry_points"]
    print(f"{B} x {H}x{W}, J={J}: map step " + ", ".join(f"{d} {e[f'smk_flow_map_step_{d}']['ms_median']:.4f} ms" for d in DIRECTIONS) +
          f", copy of the same bytes {e['copy_of_a_map_steps_bytes']['ms_median']:.4f} ms; ftle field {e['smk_ftle_field']['ms_median']:.4f} ms",
          flush=True)
    kept = {}

    def run(direction, route):
        kept[direction, route] = flow_ftle(*state, STEPS, direction=direction, route=route, **settings)
    fns = {"bare_steps": lambda: sim.step_into(None, STEPS)}
    for direction in DIRECTIONS:
        fns[f"hip_{direction}"] = lambda direction=direction: run(direction, "hip")
    fns["torch_backward"] = lambda: run("backward", "torch")
    t = timed(fns, reps=1, warm=1, rounds=kw["rounds"])
    hip, ref = kept["backward", "hip"], kept["backward", "torch"]
    r["flow_ftle_20_steps"] = {
        **t, "hip_over_bare_steps": {d: t[f"hip_{d}"]["ms_median"] / t["bare_steps"]["ms_median"] for d in DIRECTIONS},
        "torch_over_hip_backward": t["torch_backward"]["ms_median"] / t["hip_backward"]["ms_median"],
        "max_rel_diff_between_routes": float((hip.ftle - ref.ftle).abs().max() / ref.ftle.abs().max()),
        "ftle": {d: {"mean_min": float(kept[d, "hip"].mean.min()), "mean_max": float(kept[d, "hip"].mean.max()),
                     "max_min": float(kept[d, "hip"].max.min()), "max_max": float(kept[d, "hip"].max.max())} for d in DIRECTIONS}}
    f = r["flow_ftle_20_steps"]
    print(f"    20 steps: bare {t['bare_steps']['ms_median']:.3f} ms; flow_ftle " +
          ", ".join(f"{d} {t[f'hip_{d}']['ms_median']:.3f} ms ({f['hip_over_bare_steps'][d]:.3f}x)" for d in DIRECTIONS) +
          f"; torch backward {t['torch_backward']['ms_median']:.3f} ms = {f['torch_over_hip_backward']:.1f}x; routes differ by "
          f"{f['max_rel_diff_between_routes']:.1e}; backward ftle mean {f['ftle']['backward']['mean_min']:.2e} .. "
          f"{f['ftle']['backward']['mean_max']:.2e}, max {f['ftle']['backward']['max_min']:.2e} .. {f['ftle']['backward']['max_max']:.2e}", flush=True)
    sim.close()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/r32/ftle_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ftle_probe: no ROCm device; this probe measures on the GPU only")
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
