"""Times of the tangent-linear 2-D fluid step (physics.fluid_step_jvp, lyapunov_exponents; csrc/fluid_tangent.hip).

    python tools/tangent_probe.py [--reps 5] [--rounds 3] [--out profiles/r28/tangent_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and max
of the rounds are kept); the variants of one shape alternate inside a round.  Per shape (64 x 256^2 with J = 100, 32 x 128^2 with J = 20),
on the stepper's own state after 10 steps with two sources per grid:
  * the bare NavierStokesSimulator.step(), fluid_step_jvp on route="hip" with T = 1, 4 and 8 tangents per grid, and on route="torch"
    (forward_ad over the rule on the GPU: the baseline, not the code under test) with T = 1: what a tangent costs in "steps' worth"
    ((jvp - bare step) / T / bare step) and the ratio to the torch route;
  * per T, the three smk_advect_tangent calls and smk_tangent_renorm on their own (device-event times around the ABI calls, not a
    profiler's kernel times), beside a device-to-device copy of the bytes an advect call moves by the plane count (3 + 4 T planes: three
    base fields read, three tangent fields read and one written per tangent): which of the two the kernel is closer to;
  * 20 steps of lyapunov_exponents (k = 1, renormalised every step; host status check and synchronisation at the end included), with the
    default tangent0 (drawn on the CPU and copied: a set-up cost) and with a tangent0 already on the device, and the exponents it returns.
A new operator: there is no earlier time to compare with.  No figure is asserted.  Kernel times under a profiler: not measured."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from render_probe import timed
from smokephysai_amd import _lib
from smokephysai_amd.physics import fluid_step_jvp, lyapunov_exponents
from step_grad_probe import DT, SHAPES, VISCOSITY, stepper_state

TS = (1, 4, 8)


def draw_tangents(state, T, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return tuple(torch.randn(s.shape[0], T, *s.shape[1:], device=s.device, generator=gen) for s in state)


def entry_point_times(state, T, kw):
    """The ABI calls on dense buffers of the state's shapes, and the copy that moves an advect call's bytes."""
    L = _lib.load()
    u, v, p, d = state
    B, H, W = d.shape
    dev = d.device
    st = _lib.stream_ptr(dev)
    tu, tv, tp, td = (t.flatten(0, 1).contiguous() for t in draw_tangents(state, T, 5))
    outs = [torch.empty_like(t) for t in (tu, tv, td)]
    nbytes = int(L.smk_tangent_renorm_workspace(B, T, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    norms = torch.empty(B * T, dtype=torch.float64, device=dev)
    fns = {}
    for which, (field, tfield, out) in enumerate(((u, tu, outs[0]), (v, tv, outs[1]), (d, td, outs[2]))):
        fns[f"smk_advect_tangent_which{which}"] = (lambda which=which, field=field, tfield=tfield, out=out: _lib.check(L.smk_advect_tangent(
            which, field.data_ptr(), u.data_ptr(), v.data_ptr(), tfield.data_ptr(), tu.data_ptr(), tv.data_ptr(), out.data_ptr(), B, T, H, W,
            W, W + 1, DT, st)))
    fns["smk_tangent_renorm"] = lambda: _lib.check(L.smk_tangent_renorm(tu.data_ptr(), tv.data_ptr(), tp.data_ptr(), td.data_ptr(),
                                                                        norms.data_ptr(), B, T, H, W, W, W + 1, ws.data_ptr(), nbytes, st))
    planes = 3 + 4 * T
    src = torch.empty(B * H * W * planes // 2, device=dev).normal_()
    dst = torch.empty_like(src)
    fns["copy_of_the_same_bytes"] = lambda: dst.copy_(src)           # reads half of (3 + 4T) planes and writes the other half
    out = timed(fns, **kw)
    out["planes_moved_by_an_advect_call"] = planes
    out["bytes_moved_by_an_advect_call"] = 4 * B * H * W * planes
    out["advect_over_copy"] = {f"which{w}": out[f"smk_advect_tangent_which{w}"]["ms_median"] / out["copy_of_the_same_bytes"]["ms_median"]
                               for w in range(3)}
    return out


def measure_shape(B, H, W, J, kw):
    sim, state = stepper_state(B, H, W, J)
    settings = dict(dt=DT, viscosity=VISCOSITY, jacobi_iters=J)
    tans = {T: draw_tangents(state, T, 1) for T in TS}
    fns = {"bare_step": lambda: sim.step_into(None, 1)}
    for T in TS:
        fns[f"hip_jvp_T{T}"] = lambda T=T: fluid_step_jvp(state, tans[T], **settings)
    fns["torch_jvp_T1"] = lambda: fluid_step_jvp(state, tans[1], route="torch", **settings)
    t = timed(fns, **kw)
    _, hip = fluid_step_jvp(state, tans[1], **settings)
    _, ref = fluid_step_jvp(state, tans[1], route="torch", **settings)
    diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(hip, ref))
    step_ms = t["bare_step"]["ms_median"]
    r = {"batch": B, "grid": [H, W], "jacobi_iters": J, "times": t,
         "jvp_steps_worth": {f"T{T}": t[f"hip_jvp_T{T}"]["ms_median"] / step_ms for T in TS},
         "steps_worth_per_tangent": {f"T{T}": (t[f"hip_jvp_T{T}"]["ms_median"] - step_ms) / T / step_ms for T in TS},
         "torch_over_hip_T1": t["torch_jvp_T1"]["ms_median"] / t["hip_jvp_T1"]["ms_median"],
         "max_rel_diff_between_routes": diff,
         "entry_points": {f"T{T}": entry_point_times(state, T, kw) for T in TS}}
    print(f"{B} x {H}x{W}, J={J}: bare step {step_ms:.3f} ms; hip jvp " +
          ", ".join(f"T={T} {t[f'hip_jvp_T{T}']['ms_median']:.3f} ms ({r['steps_worth_per_tangent'][f'T{T}']:.2f} steps' worth per tangent)" for T in TS) +
          f"; torch T=1 {t['torch_jvp_T1']['ms_median']:.3f} ms = {r['torch_over_hip_T1']:.1f}x; routes differ by {diff:.1e}", flush=True)
    for T in TS:
        e = r["entry_points"][f"T{T}"]
        print(f"    T={T}: advect tangent " + ", ".join(f"{e[f'smk_advect_tangent_which{w}']['ms_median']:.4f}" for w in range(3)) +
              f" ms, copy of the same bytes {e['copy_of_the_same_bytes']['ms_median']:.4f} ms, renorm {e['smk_tangent_renorm']['ms_median']:.4f} ms",
              flush=True)
    lyap = {}

    t0 = tuple(t.clone() for t in tans[1])

    def run_lyapunov():                                              # the default tangent0: drawn on the CPU from the seed and copied
        lyap["res"] = lyapunov_exponents(*state, 20, **settings)

    def run_lyapunov_given():                                        # tangent0 already on the device: the 20 steps themselves
        lyapunov_exponents(*state, 20, tangent0=t0, **settings)
    lt = timed({"default_tangent0": run_lyapunov, "tangent0_on_the_device": run_lyapunov_given}, reps=1, warm=1, rounds=kw["rounds"])
    ex = lyap["res"].exponents[:, 0]
    r["lyapunov_20_steps"] = {**lt, "exponent_min": float(ex.min()), "exponent_median": float(ex.median()), "exponent_max": float(ex.max()),
                              "steps_worth_per_step": lt["tangent0_on_the_device"]["ms_median"] / (20 * step_ms)}
    print(f"    20 steps of lyapunov_exponents: {lt['tangent0_on_the_device']['ms_median']:.3f} ms with tangent0 on the device = "
          f"{r['lyapunov_20_steps']['steps_worth_per_step']:.2f} steps' worth per step ({lt['default_tangent0']['ms_median']:.3f} ms with the default "
          f"draw on the CPU); exponents {float(ex.min()):.3f} .. {float(ex.max()):.3f}", flush=True)
    sim.close()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/r28/tangent_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tangent_probe: no ROCm device; this probe measures on the GPU only")
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
