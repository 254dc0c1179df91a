"""Times of the tangent-linear 3-D fluid step (physics.fluid_step3d_jvp, lyapunov_exponents3d; csrc/fluid_tangent3d.hip; DESIGN.md section
3.12): the twin of tools/tangent_probe.py.

    python tools/tangent3d_probe.py [--reps 5] [--rounds 3] [--out profiles/r30/tangent3d_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and max
of the rounds are kept); the variants of one shape alternate inside a round.  Per shape (8 x 64 x 512 x 512 and 8 x 16 x 128 x 128, J = 20),
on the stepper's own state after 10 steps with two sources per grid:
  * the bare NavierStokesSimulator3D.step() and fluid_step3d_jvp on route="hip" with T = 1, 2 and 4 tangents per grid: what a tangent
    costs in "steps' worth" ((jvp - bare step) / T / bare step);
  * per T, the four smk_advect3d_tangent calls and smk_tangent3d_renorm on their own (device-event times around the ABI calls, not a
    profiler's kernel times), beside a device-to-device copy of the bytes an advect call moves by the volume count (4 + 5 T volumes: four
    base fields read, four tangent fields read and one written per tangent): which of the two the kernel is closer to;
  * 20 steps of lyapunov_exponents3d (k = 1, renormalised every step; synchronisation at the end included) with a tangent0 already on the
    device, and the exponents it returns;
  * route="torch" (forward_ad over the rule on the GPU: the baseline, not the code under test) with T = 1 and the largest difference
    between the two routes' tangents, at the small shape only: the rule keeps the int64 index and several fp32 temporaries of each of its
    128 gathers alive under forward_ad, some 400 fields' worth -- about 215 GB at 8 x 64 x 512 x 512, more than half the device's memory -- so
    the large shape is reported as not run.
A new operator: there is no earlier time to compare with.  No figure is asserted.  Kernel times under a profiler: not measured."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from render_probe import timed
from smokephysai_amd import _lib
from smokephysai_amd.physics import fluid_step3d_jvp, lyapunov_exponents3d
from step3d_grad_probe import DT, SHAPES, VISCOSITY, stepper_state

TS = (1, 2, 4)


def draw_tangents(state, T, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return tuple(torch.randn(s.shape[0], T, *s.shape[1:], device=s.device, generator=gen) for s in state)


def entry_point_times(state, T, kw):
    """The ABI calls on dense buffers of the state's shapes, and the copy that moves an advect call's bytes."""
    L = _lib.load()
    u, v, w, p, d = state
    B, D, H, W = d.shape
    dev = d.device
    st = _lib.stream_ptr(dev)
    tu, tv, tw, tp, td = (t.flatten(0, 1).contiguous() for t in draw_tangents(state, T, 5))
    out = torch.empty(max(t.numel() for t in (tu, tv, tw, td)), device=dev)     # tout of any of the four shapes
    nbytes = int(L.smk_tangent3d_renorm_workspace(B, T, D, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    norms = torch.empty(B * T, dtype=torch.float64, device=dev)
    fns = {}
    for which, (field, tfield) in enumerate(((u, tu), (v, tv), (w, tw), (d, td))):
        fns[f"smk_advect3d_tangent_which{which}"] = (lambda which=which, field=field, tfield=tfield: _lib.check(L.smk_advect3d_tangent(
            which, field.data_ptr(), u.data_ptr(), v.data_ptr(), w.data_ptr(), tfield.data_ptr(), tu.data_ptr(), tv.data_ptr(), tw.data_ptr(),
            out.data_ptr(), B, T, D, H, W, W, W + 1, DT, st)))
    fns["smk_tangent3d_renorm"] = lambda: _lib.check(L.smk_tangent3d_renorm(
        tu.data_ptr(), tv.data_ptr(), tw.data_ptr(), tp.data_ptr(), td.data_ptr(), norms.data_ptr(), B, T, D, H, W, W, W + 1, ws.data_ptr(),
        nbytes, st))
    volumes = 4 + 5 * T
    src = torch.empty(B * D * H * W * volumes // 2, device=dev).normal_()
    dst = torch.empty_like(src)
    fns["copy_of_the_same_bytes"] = lambda: dst.copy_(src)           # reads half of (4 + 5T) volumes and writes the other half
    res = timed(fns, **kw)
    res["volumes_moved_by_an_advect_call"] = volumes
    res["bytes_moved_by_an_advect_call"] = 4 * B * D * H * W * volumes
    res["advect_over_copy"] = {f"which{k}": res[f"smk_advect3d_tangent_which{k}"]["ms_median"] / res["copy_of_the_same_bytes"]["ms_median"]
                               for k in range(4)}
    return res


def measure_shape(B, D, H, W, J, kw):
    sim, state = stepper_state(B, D, H, W, J)
    settings = dict(dt=DT, viscosity=VISCOSITY, jacobi_iters=J)
    tans = {T: draw_tangents(state, T, 1) for T in TS}
    fns = {"bare_step": lambda: sim.step_into(None, 1)}
    for T in TS:
        fns[f"hip_jvp_T{T}"] = lambda T=T: fluid_step3d_jvp(state, tans[T], **settings)
    t = timed(fns, **kw)
    step_ms = t["bare_step"]["ms_median"]
    r = {"batch": B, "grid": [D, H, W], "jacobi_iters": J, "times": t,
         "jvp_steps_worth": {f"T{T}": t[f"hip_jvp_T{T}"]["ms_median"] / step_ms for T in TS},
         "steps_worth_per_tangent": {f"T{T}": (t[f"hip_jvp_T{T}"]["ms_median"] - step_ms) / T / step_ms for T in TS}}
    # forward_ad over the rule keeps some 400 fields' worth of temporaries (module docstring): run only where that fits half the device
    need = 400 * 4 * B * D * H * W
    if need < torch.cuda.get_device_properties(0).total_memory // 2:
        _, hip = fluid_step3d_jvp(state, tans[1], **settings)
        _, ref = fluid_step3d_jvp(state, tans[1], route="torch", **settings)
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(hip, ref))
        del hip, ref
        tt = timed({"torch_jvp_T1": lambda: fluid_step3d_jvp(state, tans[1], route="torch", **settings)}, **kw)
        t.update(tt)
        r.update(torch_over_hip_T1=tt["torch_jvp_T1"]["ms_median"] / t["hip_jvp_T1"]["ms_median"], max_rel_diff_between_routes=diff)
    else:
        r["torch_route"] = f"not run: about {need / 1e9:.0f} GB of forward_ad temporaries at this shape"
    torch.cuda.empty_cache()
    print(f"{B} x {D}x{H}x{W}, J={J}: bare step {step_ms:.3f} ms; hip jvp " +
          ", ".join(f"T={T} {t[f'hip_jvp_T{T}']['ms_median']:.3f} ms ({r['steps_worth_per_tangent'][f'T{T}']:.2f} steps' worth per tangent)" for T in TS) +
          f"; torch T=1 {t.get('torch_jvp_T1', {}).get('ms_median', float('nan')):.3f} ms = {r.get('torch_over_hip_T1', float('nan')):.1f}x; "
          f"routes differ by {r.get('max_rel_diff_between_routes', float('nan')):.1e}", flush=True)
    r["entry_points"] = {}
    for T in TS:
        e = r["entry_points"][f"T{T}"] = entry_point_times(state, T, kw)
        torch.cuda.empty_cache()
        print(f"    T={T}: advect tangent " + ", ".join(f"{e[f'smk_advect3d_tangent_which{k}']['ms_median']:.4f}" for k in range(4)) +
              f" ms, copy of the same bytes {e['copy_of_the_same_bytes']['ms_median']:.4f} ms, renorm {e['smk_tangent3d_renorm']['ms_median']:.4f} ms",
              flush=True)
    lyap = {}
    t0 = tuple(x.clone() for x in tans[1])

    def run_lyapunov():                                              # tangent0 already on the device: the 20 steps themselves
        lyap["res"] = lyapunov_exponents3d(*state, 20, tangent0=t0, **settings)
    lt = timed({"tangent0_on_the_device": run_lyapunov}, reps=1, warm=1, rounds=kw["rounds"])
    ex = lyap["res"].exponents[:, 0]
    r["lyapunov_20_steps"] = {**lt, "exponent_min": float(ex.min()), "exponent_median": float(ex.median()), "exponent_max": float(ex.max()),
                              "steps_worth_per_step": lt["tangent0_on_the_device"]["ms_median"] / (20 * step_ms)}
    print(f"    20 steps of lyapunov_exponents3d: {lt['tangent0_on_the_device']['ms_median']:.3f} ms = "
          f"{r['lyapunov_20_steps']['steps_worth_per_step']:.2f} steps' worth per step; exponents {float(ex.min()):.3f} .. {float(ex.max()):.3f}",
          flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/r30/tangent3d_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tangent3d_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)
    shapes = []
    for shape in SHAPES[::-1]:                             # the small shape first: its figures are kept if the large one fails
        shapes.append(measure_shape(*shape, kw))
        from smokephysai_amd.physics import fluid_grad
        fluid_grad._SIMS.clear()                           # (the hip route's one stepper cache, 2-D and 3-D)
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "reps": args.reps, "rounds": args.rounds,
              "kernel_times_under_a_profiler": "not measured", "lyapunov_with_the_default_tangent0_drawn_on_the_cpu": "not measured",
              "shapes": shapes[::-1]}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
