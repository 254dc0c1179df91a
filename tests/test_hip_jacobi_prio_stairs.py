"""The priority staircase of the pipelined Jacobi sweep (jb_prio_stairs, csrc/jacobi_plan.h; `sweep` in csrc/jacobi_band_tail.h): a
wave of the headline form lowers its issue priority as it moves from one barrier to the next.  Arithmetic, LDS traffic and
synchronisation are unchanged, so every word must be what the multi-launch form -- which has no staircase -- computes.

Shape: 256 x 256 at 52 grids and 22 sweeps, the smallest batch, and for it the smallest sweep count, for which the planner gives 4 cells
per lane, 6 rows per wave, the persistent launch with the folded prologue, both cell forms and the staircase (found with the host
planner: tests/test_jacobi_prio_stairs_host.py recomputes it; with fewer grids narrower bands of 2 rows per wave cost less, with fewer
sweeps the 6-row tile's halo does).  4 bands per grid.  24 steps from rest with two sources per grid: step 1 is fused in every band, the
steps behind it exact wherever the front's denormal divergence lies, so both sweep loops run -- asserted through sweep_forms().

Reference: the same trajectory in a fresh child process with SMK_JACOBI_PERSIST=0 (the switch is read once per process).  u, v, p,
density and the emitted frame are compared word for word.  `prio_stairs` appears in jacobi_plan()["projection"] only where it is true
(the recorded descriptions of tests/host/projection_plans_parent.txt stay byte-identical), so the child's plan must not have it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, B, J, STEPS = 256, 256, 52, 22, 24


def test_the_staircase_form_gives_the_words_of_the_multi_launch_form(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        from _prio_stairs_child import trajectory
    finally:
        sys.path.pop(0)
    assert os.environ.get("SMK_JACOBI_PERSIST", "1") == "1"
    state, plan, forms = trajectory(H, W, B, J, STEPS)
    assert plan["kernel"] == "k_jacobi_band<4,6>" and plan["persistent"] is True and plan["bands_per_grid"] >= 2, plan
    assert plan["cell_forms_of_a_step"] == 2 and plan["keep_rows_per_band"] > 0, plan            # two_forms; folds (the keep buffer)
    assert plan.get("prio_stairs") is True, plan
    # both sweep loops ran: all bands fused in some step, some band exact in another
    assert all(len(g) == plan["bands_per_grid"] for f in forms for g in f)
    assert any(all(w == 1 for g in f for w in g) for f in forms), forms[0]
    assert any(any(w == 0 for g in f for w in g) for f in forms)
    assert sum(w for f in forms for g in f for w in g) > 0 and any(w == 1 for g in forms[-1] for w in g)

    out = str(tmp_path / "multi_launch.npz")
    env = dict(os.environ)
    env["SMK_JACOBI_PERSIST"] = "0"
    env.pop("SMK_JACOBI_FAULT", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_prio_stairs_child.py")] + [str(x) for x in (H, W, B, J, STEPS)] + [out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ref_plan = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert ref_plan["persistent"] is False and ref_plan["kernel"].startswith("k_jacobi_band<4,"), ref_plan
    assert ref_plan.get("prio_stairs", False) is False and "prio_stairs" not in ref_plan, ref_plan
    ref = np.load(out)
    for k in ("u", "v", "p", "density", "frame"):
        a, b = state[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32, k
        differing = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        assert differing == 0, (k, differing)
    assert float(np.abs(state["p"]).max()) > 0 and float(state["frame"].max()) > 0        # (not a comparison of zeros)
