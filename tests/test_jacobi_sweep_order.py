"""The order of one Jacobi sweep inside k_jacobi_band (csrc/stencil.hip: edge rows first, their publish, interior rows around the barrier,
the neighbours' edge rows read one sweep ahead) against the CPU oracle, bit for bit.

The other bit-exactness tests of the projection compare mostly the persistent launch with the multi-launch form; both run the same
`sweep` / `run`, so a mistake in the order (a stale edge row, a buffer rewritten too early, a pipeline primed from the wrong rows after a
hand-off) would pass them.  Here every word of u, v, p and density after whole time steps is compared with oracle.OracleNS, the
bit-exact port of navier_stokes.py:151-173, over

* a table of shapes chosen so that every (cells per lane, rows per wave) pair the launchers dispatch is planned by some case,
  rows per wave 2, 3, 4, 6 and 8 among them (asserted: the plan comes from jacobi_plan(), not from this file),
* sweep counts J in {1, 2, 3, halo - 1, halo, halo + 1, 7, 100} (halo: the plan's at J = 100): the pipeline's priming, the odd sweep's
  copy, a chunk that is exactly / one short of / one more than the halo,
* the single persistent launch (the default) and the multi-launch form (SMK_JACOBI_PERSIST=0), each in a fresh process (the switch is
  read once per process),
* grids of 1, 2 and 3 or more bands.

No tolerance: the sweep's per-cell expression tree is the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, grids).  Rows per wave follow from H, the number of grids (bands x grids beyond the CU count cost a second round, which favours
# tall bands) and J; cells per lane = W / 64.  The plan of every case is recorded and the coverage asserted below.
SHAPES = [
    (32, 64, 2), (32, 128, 3), (32, 256, 2), (32, 512, 2),                 # one band of 2 rows per wave
    (40, 256, 5), (88, 128, 6),                                            # two bands
    (48, 64, 2), (48, 128, 3), (48, 256, 2), (48, 512, 200),               # one band of 3 (or bands of 2: J decides)
    (64, 64, 2), (64, 128, 2), (64, 256, 200), (64, 512, 200),             # one band of 4
    (96, 64, 200), (96, 128, 200), (96, 256, 200),                         # more grids than CUs: one band of 6 ...
    (128, 64, 200), (128, 128, 200), (128, 256, 200),                      # ... and of 8
    (128, 128, 32), (160, 256, 64), (192, 128, 13), (320, 64, 64),         # three and more bands
    (256, 256, 64),                                                        # the headline shape: four bands of 6
]
STEPS = 2                                              # the second step starts from a non-zero p
ODD_J = 7
# Pairs (cells per lane, rows per wave) the launchers can dispatch: rows per wave 2, 3, 4, 6, 8 at 1, 2 and 4 cells per lane, 2, 3, 4 at
# 8 cells per lane (8 x 6 and 8 x 8 exceed the register budget and are not instantiated).  None of them is beyond an admissible shape.
ALL_PAIRS = {(v, r) for v in (1, 2, 4) for r in (2, 3, 4, 6, 8)} | {(8, r) for r in (2, 3, 4)}


def sweep_counts(halo):
    js = {1, 2, 3, ODD_J, 100}
    if halo < 1000:                                    # (one band: no halo)
        js |= {halo - 1, halo, halo + 1}
    return sorted(j for j in js if j >= 1)


def checked_grids(B):
    return sorted({0, 1 % B, B // 2, max(B - 2, 0), B - 1})


def sources(H, W, B, J):
    rng = np.random.default_rng(1000 * H + 10 * W + B + J)
    return [(b, int(rng.integers(4, W - 4)), int(rng.integers(4, H - 4)), int(rng.integers(3, 12)), float(rng.uniform(0.5, 2.0)))
            for b in range(B) for _ in range(2)]


def oracle_state(H, W, J, density0):
    import oracle
    o = oracle.OracleNS((H, W), jacobi_iters=J)
    o.density = np.ascontiguousarray(density0, dtype=np.float32).copy()
    for _ in range(STEPS):
        o.step()
    return {k: getattr(o, k) for k in ("u", "v", "p", "density")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_table(shapes):
    """On the GPU, in this process: every case of the table; returns {case: {"plan": ..., "differs": [field@grid, ...]}}."""
    import torch
    sys.path.insert(0, ROOT)
    from smokephysai_amd.physics import NavierStokesSimulator
    out = {}
    for (H, W, B) in shapes:
        probe = NavierStokesSimulator((H, W), batch_size=B, jacobi_iters=100)
        halo = int(probe.jacobi_plan()["projection"].get("halo_rows", 1 << 20))
        probe.close()
        for J in sweep_counts(halo):
            ns = NavierStokesSimulator((H, W), batch_size=B, jacobi_iters=J)
            ns.add_smoke_sources(sources(H, W, B, J))
            d0 = ns.density.cpu().numpy().copy()
            ns.step_into(None, STEPS)
            ns.check()
            torch.cuda.synchronize()
            got = {k: getattr(ns, k).cpu().numpy() for k in ("u", "v", "p", "density")}
            differs = []
            for b in checked_grids(B):
                want = oracle_state(H, W, J, d0[b])
                differs += ["%s@%d" % (k, b) for k in want if not same_bits(got[k][b], want[k])]
            out["%dx%dxB%dxJ%d" % (H, W, B, J)] = {"plan": ns.jacobi_plan()["projection"], "differs": differs}
            ns.close()
    return out


def _child(persist):
    env = dict(os.environ)
    env["SMK_JACOBI_PERSIST"] = persist
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("TABLE ")][-1]
    return json.loads(line[len("TABLE "):])


@pytest.fixture(scope="module")
def persistent_form():
    return _child("1")


@pytest.fixture(scope="module")
def multi_launch_form():
    return _child("0")


def _pair(plan):
    """(cells per lane, rows per wave) of a band plan; None for the generic per-sweep kernel."""
    k = plan.get("kernel", "")
    if not k.startswith("k_jacobi_band<"):
        return None
    vec, rpw = (int(x) for x in k[len("k_jacobi_band<"):-1].split(","))
    assert plan["rows_per_workgroup"] == 16 * rpw, plan
    return vec, rpw


def _report(res):
    bad = {k: v["differs"] for k, v in res.items() if v["differs"]}
    for k, v in sorted(res.items()):
        print(k, _pair(v["plan"]), v["plan"].get("persistent"), v["plan"].get("bands_per_grid"), v["plan"].get("halo_rows"),
              v["plan"].get("sweeps_per_chunk"), "DIFFERS " + " ".join(v["differs"]) if v["differs"] else "ok")
    return bad


@pytest.mark.gpu
def test_persistent_launch_equals_the_oracle_in_every_word(persistent_form):
    bad = _report(persistent_form)
    assert not bad, bad
    assert sum(bool(v["plan"].get("persistent")) for v in persistent_form.values()) >= len(persistent_form) // 2   # the form under test ran


@pytest.mark.gpu
def test_multi_launch_form_equals_the_oracle_in_every_word(multi_launch_form):
    bad = _report(multi_launch_form)
    assert not bad, bad
    assert not any(v["plan"].get("persistent") for v in multi_launch_form.values())


@pytest.mark.gpu
def test_the_table_reaches_every_instantiation_and_band_count(persistent_form, multi_launch_form):
    for name, res in (("persistent", persistent_form), ("multi-launch", multi_launch_form)):
        pairs = {_pair(v["plan"]) for v in res.values()} - {None}
        assert pairs == ALL_PAIRS, (name, sorted(ALL_PAIRS - pairs), sorted(pairs - ALL_PAIRS))
        assert {r for _, r in pairs} == {2, 3, 4, 6, 8}, name
        bands = {v["plan"]["bands_per_grid"] for v in res.values() if _pair(v["plan"])}
        assert 1 in bands and 2 in bands and any(n >= 3 for n in bands), (name, sorted(bands))
    # sweeps per launch / chunk on both sides of the halo, and single sweeps
    assert any(k.endswith("xJ1") for k in multi_launch_form) and any(k.endswith("xJ100") for k in persistent_form)


def test_the_oracle_side_of_the_table_is_small():
    """No GPU: the table's sweep counts and checked grids stay within what the CPU oracle does in well under a minute."""
    cells = 0
    for (H, W, B) in SHAPES:
        assert W % 64 == 0 and W // 64 in (1, 2, 4, 8) and H >= 32
        for J in sweep_counts(21):
            cells += H * W * (J + 8) * STEPS * len(checked_grids(B)) * 2          # two forms
    assert cells < 4e9, cells                          # ~1e9 cell updates per 10 s of the C oracle on one core


if __name__ == "__main__":
    print("TABLE " + json.dumps(run_table(SHAPES)), flush=True)
