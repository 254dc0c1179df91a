"""Times of the Lyapunov spectrum's orthonormalisation (smk_tangent_orthonormalize / smk_tangent3d_orthonormalize, csrc/tangent_qr.hip;
lyapunov_exponents(..., k > 1, gram_schmidt=)) beside the torch form it restates, which had never been measured.

    python tools/spectrum_probe.py [--reps 5] [--rounds 3] [--out profiles/r31/spectrum_probe.json]

Every time is a device-event time around `reps` back-to-back calls after `warm` untimed ones, repeated `rounds` times (median, min and max
of the rounds are kept); the variants of one (shape, k) alternate inside a round (tools/tangent_probe.py's method).  Shapes: 64 x 256 x 256
at J = 100 with k in {2, 4, 8}, 32 x 128 x 128 at J = 20 with k = 4, 8 x 64 x 512 x 512 at J = 20 with k in {2, 4}, 8 x 16 x 128 x 128 at
J = 20 with k in {2, 4, 8}; the state is the stepper's own after 10 steps with two sources per grid.  Per (shape, k):
  * one orthonormalisation of the same k unit-normal tangent states per grid with gram_schmidt="hip" (the entry point as
    lyapunov_exponents calls it, workspace allocated once, in place) and with "torch" (physics.fluid_tangent._gram_schmidt, the stack of
    its results included, as lyapunov_exponents runs it);
  * one tangent step at T = k (fluid_step_jvp / fluid_step3d_jvp, route="hip") beside them: what the spectrum pays per step anyway;
  * a device-to-device copy of k states: the byte yardstick (the rule reads and writes of the order of k^2 / 2 states);
  * 20 spectrum steps end to end (renormalised every step, tangent0 already on the device, the synchronisation at the end included) on
    both settings, and the largest difference between the two settings' exponents.
The torch form is run only where its temporaries fit the free device memory (estimated as 3 k + 3 states: the input, the finished list,
the stacked result and the fp64 temporaries of one field); otherwise the cell holds the reason and the figure.  No figure is asserted.
Kernel times under a profiler: not measured."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import step3d_grad_probe as P3
import step_grad_probe as P2
from render_probe import timed
from smokephysai_amd.physics import fluid_grad, fluid_step3d_jvp, fluid_step_jvp, lyapunov_exponents, lyapunov_exponents3d
from smokephysai_amd.physics.fluid_grad3d import HIP3
from smokephysai_amd.physics.fluid_tangent import _gram_schmidt, _HipRenorm

# (dimension record, stepper state, tangent step, spectrum, (B, *grid, J), the k to run), the small shape of each dimension first
JOBS = ((fluid_grad.HIP2, P2.stepper_state, fluid_step_jvp, lyapunov_exponents, P2.SHAPES[1], (4,)),
        (fluid_grad.HIP2, P2.stepper_state, fluid_step_jvp, lyapunov_exponents, P2.SHAPES[0], (2, 4, 8)),
        (HIP3, P3.stepper_state, fluid_step3d_jvp, lyapunov_exponents3d, P3.SHAPES[1], (2, 4, 8)),
        (HIP3, P3.stepper_state, fluid_step3d_jvp, lyapunov_exponents3d, P3.SHAPES[0], (2, 4)))


def draw_tangents(state, T, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return tuple(torch.randn(s.shape[0], T, *s.shape[1:], device=s.device, generator=gen) for s in state)


def measure(dim, state, jvp, spectrum, k, settings, kw):
    B, *grid = state[-1].shape
    dev = state[-1].device
    state_bytes = 4 * sum(s.numel() for s in state)
    tans = draw_tangents(state, k, 1)
    r = {"k": k, "bytes_of_k_states": k * state_bytes}
    need = (3 * k + 3) * state_bytes
    free = torch.cuda.mem_get_info()[0]
    run_torch = need < free
    if not run_torch:
        r["gram_schmidt_torch"] = f"not run: about {need / 1e9:.0f} GB of tensors and fp64 temporaries against {free / 1e9:.0f} GB free"
    work = tuple(t.clone() for t in tans)
    norms = torch.empty(B, k, dtype=torch.float64, device=dev)
    hip_gs = _HipRenorm(dim, B, k, grid, dev, dim.orthonormalize)
    src = torch.cat([t.reshape(-1) for t in tans])
    dst = torch.empty_like(src)
    fns = {"gram_schmidt_hip": lambda: hip_gs(work, norms)}
    if run_torch:
        fns["gram_schmidt_torch"] = lambda: _gram_schmidt(tans)
    fns["tangent_step"] = lambda: jvp(state, tans, **settings)
    fns["copy_of_k_states"] = lambda: dst.copy_(src)
    r.update(timed(fns, **kw))
    del src, dst, work
    torch.cuda.empty_cache()
    t0 = tuple(t.clone() for t in tans)
    got = {}

    def run(gs):
        got[gs] = spectrum(*state, 20, k=k, tangent0=t0, gram_schmidt=gs, **settings).exponents
    ends = {"spectrum_20_steps_hip": lambda: run("hip")}
    if run_torch:
        ends["spectrum_20_steps_torch"] = lambda: run("torch")
    r.update(timed(ends, reps=1, warm=1, rounds=kw["rounds"]))
    r["exponents_hip_grid0"] = got["hip"][0].tolist()
    if run_torch:
        r["torch_over_hip"] = r["gram_schmidt_torch"]["ms_median"] / r["gram_schmidt_hip"]["ms_median"]
        r["spectrum_torch_over_hip"] = r["spectrum_20_steps_torch"]["ms_median"] / r["spectrum_20_steps_hip"]["ms_median"]
        r["max_abs_diff_between_the_settings_exponents"] = float((got["hip"] - got["torch"]).abs().max())
    ms = lambda name: r[name]["ms_median"] if isinstance(r.get(name), dict) else float("nan")          # noqa: E731
    print(f"    k={k}: Gram-Schmidt hip {ms('gram_schmidt_hip'):.4f} ms, torch {ms('gram_schmidt_torch'):.4f} ms "
          f"({r.get('torch_over_hip', float('nan')):.1f}x); tangent step {ms('tangent_step'):.4f} ms; copy of k states "
          f"{ms('copy_of_k_states'):.4f} ms; 20 spectrum steps hip {ms('spectrum_20_steps_hip'):.2f} ms, torch "
          f"{ms('spectrum_20_steps_torch'):.2f} ms; exponents differ by {r.get('max_abs_diff_between_the_settings_exponents', float('nan')):.1e}",
          flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/r31/spectrum_probe.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_probe: no ROCm device; this probe measures on the GPU only")
    import bench
    kw = dict(reps=args.reps, warm=args.warm, rounds=args.rounds)
    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "reps": args.reps, "rounds": args.rounds,
              "kernel_times_under_a_profiler": "not measured", "shapes": []}
    for dim, stepper_state, jvp, spectrum, shape, ks in JOBS:
        *dims, J = shape
        sim, state = stepper_state(*dims, J)
        settings = dict(dt=P2.DT, viscosity=P2.VISCOSITY, jacobi_iters=J)
        print(f"{dims[0]} x {'x'.join(str(n) for n in dims[1:])}, J={J}", flush=True)
        rows = [measure(dim, state, jvp, spectrum, k, settings, kw) for k in ks]
        result["shapes"].append({"batch": dims[0], "grid": dims[1:], "jacobi_iters": J, "per_k": rows})
        del sim, state
        fluid_grad._SIMS.clear()                           # (the hip route's one stepper cache, 2-D and 3-D)
        torch.cuda.empty_cache()
        if args.out:                                       # written after every shape: the finished ones are kept if a later one fails
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
