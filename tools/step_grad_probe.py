"""Times of the differentiable 2-D fluid step (physics.fluid_step, csrc/fluid_grad.hip).

    python tools/step_grad_probe.py [--reps 5] [--rounds 3] [--out profiles/r26/step_grad_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and max
of the rounds are kept); the variants of one shape alternate inside a round.  Per shape (64 x 256^2 with J = 100, 32 x 128^2 with J = 20),
on the stepper's own state after 10 steps with two sources per grid:
  * forward + backward of one fluid_step on route="hip" and on route="torch" (the rule under torch autograd on the GPU: the baseline, not
    the code under test), beside the bare NavierStokesSimulator.step() and fluid_step's forward without a gradient request: what a
    differentiable step costs in "steps' worth";
  * each backward entry point on its own (smk_advect_backward for the three fields, smk_project_backward, smk_buoy_diffuse_backward):
    device-event times around the ABI calls, not a profiler's kernel times;
  * the largest difference between the two routes' gradients, relative to the largest gradient.
And ten PGD steps of PerturbationTester.adversarial_test(simulate=FluidRollout(steps=4)) on 128^2 frames on both routes (host clock around
the call, which ends in a synchronising .item()).
A new operator: there is no earlier time to compare with.  No figure is asserted."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from render_probe import timed
from smokephysai_amd import _lib
from smokephysai_amd.physics import FluidRollout, NavierStokesSimulator, fluid_step

SHAPES = ((64, 256, 256, 100), (32, 128, 128, 20))          # (B, H, W, jacobi_iters)
DT, VISCOSITY = 0.01, 0.001


def stepper_state(B, H, W, J, steps=10):
    sim = NavierStokesSimulator((H, W), dt=DT, viscosity=VISCOSITY, device="cuda", batch_size=B, jacobi_iters=J)
    sim.setup_grid()
    sim.add_smoke_sources([(b, W // 4 + (7 * b) % (W // 2), H // 2 + (5 * b) % (H // 4), max(4, H // 16), 1.0 + 0.05 * (b % 8)) for b in range(B)] +
                          [(b, W // 2 + (3 * b) % (W // 4), H // 4 + (11 * b) % (H // 4), max(3, H // 24), 1.5) for b in range(B)])
    sim.step_into(None, steps)
    sim.check()
    return sim, sim.state()


def entry_point_times(state, J, kw):
    """Device-event times of the backward entry points on dense buffers of the state's shapes."""
    L = _lib.load()
    u, v, p, d = state
    B, H, W = d.shape
    dev = d.device
    st = _lib.stream_ptr(dev)
    gen = torch.Generator(device="cuda").manual_seed(2)
    gu, gv, gd = (torch.randn(t.shape, device=dev, generator=gen) for t in (u, v, d))
    du, dv, dd, du2, dv2, far = (torch.empty_like(t) for t in (u, v, d, u, v, torch.empty(B, dtype=torch.int32, device=dev)))
    nbytes = int(L.smk_project_backward_workspace(B, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fns = {}
    for which, (field, gout, dfield) in enumerate(((u, gu, du2), (v, gv, dv2), (d, gd, dd))):
        fns[f"smk_advect_backward_which{which}"] = (lambda which=which, field=field, gout=gout, dfield=dfield: _lib.check(L.smk_advect_backward(
            which, field.data_ptr(), u.data_ptr(), v.data_ptr(), gout.data_ptr(), dfield.data_ptr(), du.data_ptr(), dv.data_ptr(),
            far.data_ptr(), B, H, W, W, W + 1, DT, st)))
    fns["smk_project_backward"] = lambda: _lib.check(L.smk_project_backward(
        gu.data_ptr(), gv.data_ptr(), gd.data_ptr(), du.data_ptr(), dv.data_ptr(), dd.data_ptr(), B, H, W, W, W + 1, J, DT, ws.data_ptr(),
        nbytes, st))
    fns["smk_buoy_diffuse_backward"] = lambda: _lib.check(L.smk_buoy_diffuse_backward(
        gu.data_ptr(), gv.data_ptr(), gd.data_ptr(), du.data_ptr(), dv.data_ptr(), dd.data_ptr(), B, H, W, W, W + 1, DT, VISCOSITY, st))
    out = timed(fns, **kw)
    out["smk_project_backward"]["launches"] = (J + 3) // 4 + 2
    return out


def measure_shape(B, H, W, J, kw):
    sim, state = stepper_state(B, H, W, J)
    gen = torch.Generator(device="cuda").manual_seed(1)
    ups = [torch.randn(t.shape, device="cuda", generator=gen) for t in state]
    leaves = [t.clone().requires_grad_(True) for t in state]
    settings = dict(dt=DT, viscosity=VISCOSITY, jacobi_iters=J)

    def both(route):
        def run():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(fluid_step(*leaves, route=route, **settings), ups)
        return run

    def forward_only():
        with torch.no_grad():
            fluid_step(*state, **settings)
    t = timed({"hip_forward_backward": both("hip"), "torch_forward_backward": both("torch"), "fluid_step_forward_no_grad": forward_only,
               "bare_step": lambda: sim.step_into(None, 1)}, **kw)
    both("torch")()
    want = [x.grad.clone() for x in leaves]
    both("hip")()
    diff = max(float((x.grad - w).abs().max() / w.abs().max()) for x, w in zip(leaves, want))
    finite = all(bool(torch.isfinite(x.grad).all()) for x in leaves)
    step_ms = t["bare_step"]["ms_median"]
    r = {"batch": B, "grid": [H, W], "jacobi_iters": J, "saved_bytes_per_step": 5 * 4 * B * H * W, "times": t,
         "hip_steps_worth": t["hip_forward_backward"]["ms_median"] / step_ms,
         "torch_steps_worth": t["torch_forward_backward"]["ms_median"] / step_ms,
         "torch_over_hip": t["torch_forward_backward"]["ms_median"] / t["hip_forward_backward"]["ms_median"],
         "max_rel_diff_between_routes": diff, "hip_gradients_finite": finite,
         "entry_points": entry_point_times(state, J, kw)}
    print(f"{B} x {H}x{W}, J={J}: forward + backward hip {t['hip_forward_backward']['ms_median']:.3f} ms = {r['hip_steps_worth']:.1f} steps' "
          f"worth (bare step {step_ms:.3f} ms, forward without a gradient {t['fluid_step_forward_no_grad']['ms_median']:.3f} ms); torch "
          f"{t['torch_forward_backward']['ms_median']:.3f} ms = {r['torch_over_hip']:.1f}x; routes differ by {diff:.1e}", flush=True)
    for name, e in r["entry_points"].items():
        print(f"    {name}: {e['ms_median']:.4f} ms", flush=True)
    sim.close()
    return r


def measure_pgd(batch, steps=4, num_steps=10, rounds=3):
    from smokephysai_amd.evaluation import PerturbationTester
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, chaos_strength=0.0).cuda().eval()
    frames = torch.rand(batch, 1, 128, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) ** 4
    r = {"batch": batch, "frame": [128, 128], "rollout_steps": steps, "pgd_steps": num_steps, "routes": {}}
    for route in ("hip", "torch"):
        sim = FluidRollout(steps=steps, route=route)
        times, res = [], None
        for k in range(rounds + 1):                        # (the first round warms up and is dropped)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = PerturbationTester().adversarial_test(model, frames, epsilon=0.1, num_steps=num_steps, simulate=sim)
            torch.cuda.synchronize()
            if k:
                times.append((time.perf_counter() - t0) * 1e3)
        r["routes"][route] = {"ms_median": sorted(times)[len(times) // 2], "ms_min": min(times), "ms_max": max(times), **res}
        print(f"PGD, {num_steps} steps through a {steps}-step rollout, {batch} x 128^2, route {route}: {r['routes'][route]['ms_median']:.1f} ms", flush=True)
    r["torch_over_hip"] = r["routes"]["torch"]["ms_median"] / r["routes"]["hip"]["ms_median"]
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pgd-batch", type=int, default=16)
    ap.add_argument("--out", default="profiles/r26/step_grad_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_grad_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)
    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "reps": args.reps, "rounds": args.rounds,
              "shapes": [measure_shape(*shape, kw) for shape in SHAPES], "pgd": measure_pgd(args.pgd_batch)}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
