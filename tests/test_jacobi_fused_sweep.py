"""The two forms of the Jacobi cell in k_jacobi_band (csrc/stencil.h, stencil.hip): where every divergence value of a workgroup is +-0 or
has 2^-100 <= |div| <= 2^100 the sweeps take three adds and one fma with -div / 4 formed once per launch, elsewhere the reference's five
operations (navier_stokes.py:141-145).  Both must give the oracle's words, and sweep_forms() must say which one ran.

Every comparison is word for word (NaN = NaN) against the CPU oracle, never against another form of the kernel; it is made in a child
process (tests/_fused_sweep_child.py), one with SMK_JACOBI_PERSIST=1 and one with =0 -- the knob is read once per process.  Shapes:
64^2, 128^2, 256^2 x 3 grids (1, 2, 4 cells per lane; several bands), 320 x 64 x 100 (more bands x grids than one persistent launch holds),
J = 40; from rest 128^2 and 256^2 at J = 100; and 256^2 x 64, whose plan (4 cells per lane, 6 rows per wave, 4 bands, the keep buffer with
rows left on the HBM path) is the benchmark headline's.

Only that plan's one-launch step kernel has both forms (jb_two_forms: the one instantiation whose registers, scratch and occupancy the
second sweep loop leaves alone; `cell_forms_of_a_step` in jacobi_plan() says so).  There the verdict of every band of the compared
grids must be the one the ORACLE's divergence of that step implies -- fused in all bands for dense random states and for step 0 from
rest, exact in exactly the bands that hold a denormal, NaN or Inf value.  Every other kernel has the exact cell only: every band must
report 0, for the same states, and the words must be the oracle's all the same.  So the cases first specified as `fused` at
64^2, 128^2, 256^2 x 3, 320 x 64 and under SMK_JACOBI_PERSIST=0 are checked as `exact` here.  The crafted single values -- one cell of 2^-120,
the same cell at exactly 2^-100 -- run on the kernel with both forms through a whole step with viscosity 0 and no density, which leaves
the crafted velocities to the projection as they are; a NaN and an Inf go into a dense state of the same plan."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_results = {}


def _child(persist):
    if persist not in _results:
        env = dict(os.environ)
        env["SMK_JACOBI_PERSIST"] = persist
        env.pop("SMK_JACOBI_FAULT", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fused_sweep_child.py")], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
        _results[persist] = json.loads(line[len("RESULT "):])
    return _results[persist]


def _two_forms(case):
    return case["plan"].get("cell_forms_of_a_step") == 2


def _check_step(key, t, case, step):
    """the compared grids' verdicts are the ones the oracle's divergence implies; the others' are fused or exact as a whole kernel can be"""
    for b, want in step["expect"].items():
        assert step["forms"][int(b)] == want, (key, t, b, step["forms"][int(b)], want)
    if not _two_forms(case):
        assert all(w == 0 for g in step["forms"] for w in g), (key, t)
    assert step["mismatch"] == {}, (key, t, step["mismatch"])


PERSIST = pytest.mark.parametrize("persist", ["1", "0"])


@PERSIST
def test_the_cases_take_the_plans_they_are_meant_for(persist):
    res = _child(persist)
    cases = dict(res["dense"])
    cases.update({"rest:" + k: v for k, v in res["rest"].items()})
    plans = {k: v["plan"] for k, v in cases.items()}
    assert all(bool(p.get("persistent")) == (persist == "1") for p in plans.values()), plans
    assert {p["kernel"][len("k_jacobi_band<")] for p in plans.values()} == {"1", "2", "4"}, plans      # cells per lane
    assert max(p["bands_per_grid"] for p in plans.values()) >= 4
    for key in ("256x256xB64", "256x256xB64:naninf", "rest:256xB64"):
        assert plans[key]["kernel"] == "k_jacobi_band<4,6>", plans[key]
        assert _two_forms(cases[key]) == (persist == "1"), plans[key]       # the multi-launch kernels have the exact cell only
        assert [tuple(t) for t in cases[key]["tiles"]] == [(0, 96), (54, 150), (108, 204), (160, 256)], cases[key]["tiles"]
    assert sum(_two_forms(c) for c in cases.values()) == (3 if persist == "1" else 0), plans
    if persist == "1":
        assert plans["320x64xB100"]["launches"] >= 2, plans["320x64xB100"]
        assert plans["rest:256xB64"]["keep_overflow_rows_max"] > 0, plans["rest:256xB64"]


@PERSIST
def test_dense_random_states_equal_the_oracle_and_run_fused_where_the_kernel_has_both_forms(persist):
    res = _child(persist)
    for key, case in res["dense"].items():
        for t, step in enumerate(case["steps"]):
            _check_step(key, t, case, step)
    if persist == "1":
        for t, step in enumerate(res["dense"]["256x256xB64"]["steps"]):
            assert all(w == 1 for g in step["forms"] for w in g), (t, step["forms"])        # all 64 grids x 4 bands


@PERSIST
def test_a_nan_and_an_inf_turn_exactly_their_bands_exact(persist):
    case = _child(persist)["dense"]["256x256xB64:naninf"]
    step = case["steps"][0]
    assert step["oracle_nan_p"]["21"] > 0 and step["oracle_nan_p"]["0"] == 0
    if persist == "1":
        # v[5, 249] = NaN lies in band 0 alone, u[131, 85] = Inf in bands 1 and 2 (rows 54-149 and 108-203): band 3 stays fused
        assert step["expect"]["21"] == [0, 0, 0, 1], step["expect"]
        assert step["forms"][21] == [0, 0, 0, 1], step["forms"][21]
        assert all(g == [1, 1, 1, 1] for b, g in enumerate(step["forms"]) if b != 21)


@PERSIST
def test_from_rest_step_0_is_fused_the_front_steps_are_exact_and_all_equal_the_oracle(persist):
    for key, case in _child(persist)["rest"].items():
        steps = case["steps"]
        assert steps[0]["oracle_denormal_p"] > 0, key                   # the fused form is exercised on denormal results
        for t, step in enumerate(steps):
            _check_step(key, t, case, step)
        if _two_forms(case):
            assert all(w == 1 for g in steps[0]["forms"] for w in g), (key, steps[0]["forms"])
            for t in (1, 2, 3):
                assert any(w == 0 for g in steps[t]["forms"] for w in g), (key, t)
                assert any(0 in e for e in steps[t]["expect"].values()), (key, t)      # ... and the oracle's divergence says why


@PERSIST
@pytest.mark.parametrize("kind", ["tiny", "bound"])
def test_one_crafted_divergence_value_turns_exactly_its_two_bands_exact_and_the_bound_itself_stays_fused(persist, kind):
    """2^-120 in one cell of grid 1, on a row that bands 1 and 2 both hold: those two report exact, bands 0 and 3 and every band of the
    other 63 grids fused.  The same cell at exactly 2^-100: everything fused.  On the multi-launch kernels: everything exact."""
    case = _child(persist)["crafted"][kind]
    assert case["plan"]["kernel"] == "k_jacobi_band<4,6>" and [tuple(t) for t in case["tiles"]] == [(0, 96), (54, 150), (108, 204), (160, 256)]
    assert case["prologue_leaves_divergence"] is True
    assert case["guard_fails"]["0"] == [] and case["guard_fails"]["63"] == []         # the other grids: ordinary everywhere
    if kind == "tiny":
        assert case["cell_div"] == 2.0 ** -120 and case["guard_fails"]["1"] == [[128, 85]], (case["cell_div"], case["guard_fails"]["1"])
    else:
        assert case["cell_div"] == 2.0 ** -100 and case["guard_fails"]["1"] == [], (case["cell_div"], case["guard_fails"]["1"])
    if persist == "1":
        assert _two_forms(case)
        assert case["forms"][1] == ([1, 0, 0, 1] if kind == "tiny" else [1, 1, 1, 1]), case["forms"][1]
        assert all(g == [1, 1, 1, 1] for b, g in enumerate(case["forms"]) if b != 1), case["forms"]
    else:
        assert not _two_forms(case) and all(g == [0, 0, 0, 0] for g in case["forms"]), case["forms"]
    for b, want in case["expect"].items():
        assert case["forms"][int(b)] == want, (b, case["forms"][int(b)], want)
    assert case["mismatch"] == {}, case["mismatch"]
