"""Child of tests/test_hip_jacobi_prio_stairs.py (and the trajectory itself, which the test imports): `steps` time steps from rest with
two sources per grid; argv: H W B J steps out.npz.  The projection's switches are read once per process, so the form with
SMK_JACOBI_PERSIST=0 needs a process of its own.  Prints one line: RESULT <json of jacobi_plan()["projection"]>."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def trajectory(H, W, B, J, steps):
    """-> (dict of u, v, p, density and the last emitted frame as numpy arrays, the plan, sweep_forms() after every step)"""
    import torch

    from smokephysai_amd.physics import NavierStokesSimulator

    ns = NavierStokesSimulator((H, W), device="cuda:0", batch_size=B, jacobi_iters=J)
    ns.add_smoke_sources([(b, 40 + 3 * (b % 50), H - 50 - 2 * (b % 40), 8, 1.0 + 0.01 * b) for b in range(B)] +
                         [(b, W // 2 + (b % 7), 60 + (b % 30), 6, 0.7) for b in range(B)])
    frame = torch.empty(B, H, W, device="cuda:0")
    forms = []
    for _ in range(steps):
        ns.step_into(frame, 1)
        forms.append(ns.sweep_forms())
    ns.check()
    state = {k: getattr(ns, k).cpu().numpy() for k in ("u", "v", "p", "density")}
    state["frame"] = frame.cpu().numpy()
    return state, ns.jacobi_plan()["projection"], forms


if __name__ == "__main__":
    import numpy as np

    H, W, B, J, steps = (int(x) for x in sys.argv[1:6])
    state, plan, _ = trajectory(H, W, B, J, steps)
    np.savez(sys.argv[6], **state)
    print("RESULT " + json.dumps(plan))
