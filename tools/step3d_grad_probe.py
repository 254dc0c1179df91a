"""Times of the differentiable 3-D fluid step (physics.fluid_step3d, csrc/fluid_grad3d.hip): the twin of
tools/step_grad_probe.py.

    python tools/step3d_grad_probe.py [--reps 3] [--rounds 3] [--out profiles/r27/step3d_grad_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and max
of the rounds are kept); the variants of one shape alternate inside a round.  Per shape (8 x 64 x 512 x 512 and 8 x 16 x 128 x 128, J = 20),
on the stepper's own state after 10 steps with two sources per grid:
  * forward + backward of one fluid_step3d on route="hip", beside the bare NavierStokesSimulator3D.step() and fluid_step3d's forward without a
    gradient request: what a differentiable step costs in "steps' worth";
  * the same on route="torch" (the rule under torch autograd on the GPU: the baseline, not the code under test) where its temporaries --
    some 400 fields' worth per step -- stay below half the device's memory; otherwise the shape is reported as not measured;
  * each backward entry point on its own (smk_advect3d_backward for the four fields, smk_project3d_backward,
    smk_buoy_diffuse3d_backward): device-event times around the ABI calls, not a profiler's kernel times;
  * the largest difference between the two routes' gradients, relative to the largest gradient, where both ran.
A new operator: there is no earlier time to compare with.  No figure is asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from render_probe import timed
from smokephysai_amd import _lib
from smokephysai_amd.physics import NavierStokesSimulator3D, fluid_step3d

SHAPES = ((8, 64, 512, 512, 20), (8, 16, 128, 128, 20))          # (B, D, H, W, jacobi_iters)
DT, VISCOSITY = 0.01, 0.001
PB_T = 2                                                           # csrc/fluid_grad3d.h FG3_PB_T


def stepper_state(B, D, H, W, J, steps=10):
    sim = NavierStokesSimulator3D((D, H, W), dt=DT, viscosity=VISCOSITY, device="cuda", batch_size=B, jacobi_iters=J)
    sim.setup_grid()
    sim.add_smoke_sources([(b, W // 4 + (7 * b) % (W // 2), H // 2 + (5 * b) % (H // 4), D // 2, max(4, D // 4), 1.0 + 0.05 * b) for b in range(B)] +
                          [(b, W // 2 + (3 * b) % (W // 4), H // 4 + (11 * b) % (H // 4), D // 3, max(3, D // 5), 1.5) for b in range(B)])
    sim.step_into(None, steps)
    return sim, sim.state()


def entry_point_times(state, J, kw):
    """Device-event times of the backward entry points on dense buffers of the state's shapes."""
    L = _lib.load()
    u, v, w, p, d = state
    B, D, H, W = d.shape
    dev = d.device
    st = _lib.stream_ptr(dev)
    gen = torch.Generator(device="cuda").manual_seed(2)
    gu, gv, gw, gd = (torch.randn(t.shape, device=dev, generator=gen) for t in (u, v, w, d))
    du, dv, dw, dd = (torch.empty_like(t) for t in (u, v, w, d))
    df = torch.empty(max(t.numel() for t in (u, v, w, d)), device=dev)          # dfield of any of the four shapes
    far = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = int(L.smk_project3d_backward_workspace(B, D, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fns = {}
    for which, (field, gout) in enumerate(((u, gu), (v, gv), (w, gw), (d, gd))):
        fns[f"smk_advect3d_backward_which{which}"] = (lambda which=which, field=field, gout=gout: _lib.check(L.smk_advect3d_backward(
            which, field.data_ptr(), u.data_ptr(), v.data_ptr(), w.data_ptr(), gout.data_ptr(), df.data_ptr(), du.data_ptr(), dv.data_ptr(),
            dw.data_ptr(), far.data_ptr(), B, D, H, W, W, W + 1, DT, st)))
    fns["smk_project3d_backward"] = lambda: _lib.check(L.smk_project3d_backward(
        gu.data_ptr(), gv.data_ptr(), gw.data_ptr(), gd.data_ptr(), du.data_ptr(), dv.data_ptr(), dw.data_ptr(), dd.data_ptr(), B, D, H, W, W,
        W + 1, J, DT, ws.data_ptr(), nbytes, st))
    fns["smk_buoy_diffuse3d_backward"] = lambda: _lib.check(L.smk_buoy_diffuse3d_backward(
        gu.data_ptr(), gv.data_ptr(), gw.data_ptr(), gd.data_ptr(), du.data_ptr(), dv.data_ptr(), dw.data_ptr(), dd.data_ptr(), B, D, H, W, W,
        W + 1, DT, VISCOSITY, st))
    out = timed(fns, **kw)
    out["smk_project3d_backward"]["launches"] = (J + PB_T - 1) // PB_T + 2
    return out


def measure_shape(B, D, H, W, J, kw):
    sim, state = stepper_state(B, D, H, W, J)
    gen = torch.Generator(device="cuda").manual_seed(1)
    ups = [torch.randn(t.shape, device="cuda", generator=gen) for t in state]
    leaves = [t.clone().requires_grad_(True) for t in state]
    settings = dict(dt=DT, viscosity=VISCOSITY, jacobi_iters=J)

    def both(route):
        def run():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(fluid_step3d(*leaves, route=route, **settings), ups)
        return run

    def forward_only():
        with torch.no_grad():
            fluid_step3d(*state, **settings)
    t = timed({"hip_forward_backward": both("hip"), "fluid_step3d_forward_no_grad": forward_only,
               "bare_step": lambda: sim.step_into(None, 1)}, **kw)
    both("hip")()
    got = [x.grad.clone() for x in leaves]
    finite = all(bool(torch.isfinite(g).all()) for g in got)
    step_ms = t["bare_step"]["ms_median"]
    r = {"batch": B, "grid": [D, H, W], "jacobi_iters": J, "saved_bytes_per_step": 7 * 4 * B * D * H * W, "times": t,
         "hip_steps_worth": t["hip_forward_backward"]["ms_median"] / step_ms, "hip_gradients_finite": finite}
    # The rule under torch autograd keeps, per step, the int64 index of each of its 128 gathers (4 advections x 4 interpolations x 8 taps)
    # and about as many fp32 temporaries again: some 400 fields' worth.  It is run only where that stays below half the device's memory.
    need = 400 * 4 * B * D * H * W
    if need < torch.cuda.get_device_properties(0).total_memory // 2:
        both("torch")()
        diff = max(float((x.grad - g).abs().max() / x.grad.abs().max()) for x, g in zip(leaves, got))
        tt = timed({"torch_forward_backward": both("torch")}, **kw)
        t.update(tt)
        r.update(torch_steps_worth=tt["torch_forward_backward"]["ms_median"] / step_ms,
                 torch_over_hip=tt["torch_forward_backward"]["ms_median"] / t["hip_forward_backward"]["ms_median"],
                 max_rel_diff_between_routes=diff)
    else:
        r["torch_route"] = f"not measured: about {need / 1e9:.0f} GB of autograd temporaries at this shape"
    for x in leaves:
        x.grad = None
    torch.cuda.empty_cache()
    r["entry_points"] = entry_point_times(state, J, kw)
    print(f"{B} x {D}x{H}x{W}, J={J}: forward + backward hip {t['hip_forward_backward']['ms_median']:.3f} ms = {r['hip_steps_worth']:.1f} steps' "
          f"worth (bare step {step_ms:.3f} ms, forward without a gradient {t['fluid_step3d_forward_no_grad']['ms_median']:.3f} ms); torch "
          f"{t.get('torch_forward_backward', {}).get('ms_median', float('nan')):.3f} ms; routes differ by "
          f"{r.get('max_rel_diff_between_routes', float('nan')):.1e}", flush=True)
    for name, e in r["entry_points"].items():
        print(f"    {name}: {e['ms_median']:.4f} ms", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/r27/step3d_grad_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step3d_grad_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)
    shapes = []
    for shape in SHAPES[::-1]:                             # the small shape first: its figures are kept if the large one fails
        shapes.append(measure_shape(*shape, kw))
        from smokephysai_amd.physics import fluid_grad
        fluid_grad._SIMS.clear()                           # (the hip route's one stepper cache, 2-D and 3-D)
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "reps": args.reps, "rounds": args.rounds,
              "shapes": shapes[::-1]}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
