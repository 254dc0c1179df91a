"""The priority staircase of the Jacobi sweep (jb_prio_stairs, smokephysai_amd/csrc/jacobi_plan.h), checked on the host: a stand-alone
program (tests/host/jacobi_prio_stairs_main.cpp, its own main) includes the header -- the text the kernel and its launchers compile -- and
prints the trait for every (cells per lane, rows per wave, persistent, folding) that has a kernel and the plans of the shapes below.
  * the trait is true exactly for the form listed here: 4 cells per lane, 6 rows per wave, persistent with the folded prologue;
  * it is false for every multi-launch form and for 4 x 8 (at the register cap, plain order);
  * plan_projection reports it for the headline step (256 x 256, 64 grids, 100 sweeps) and not for the multi-launch plan of the same
    shape, nor for the configs[1] and dataset shapes;
  * the smallest batch and sweep count at 256 x 256 with the staircase are those tests/test_hip_jacobi_prio_stairs.py states."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "jacobi_prio_stairs_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")

STAIRS_FORMS = {(4, 6, 1, 1)}                                 # (vec, rpw, persist, fold): the forms timed with the staircase (profiles/r34)
SMALLEST_256 = (52, 22)                                       # batch, sweeps: see tests/test_hip_jacobi_prio_stairs.py


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("priostairs") / "jacobi_prio_stairs")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    return run.stdout.splitlines()


def _traits(lines):
    t = {}
    for l in lines:
        if l.startswith("TRAIT "):
            key, val = l[6:].split(" | ")
            t[tuple(int(x) for x in key.split())] = int(val)
    assert len(t) == 4 * 5 * 2 * 2
    return t


def _plan(lines, tag, H, W, B, iters, allow):
    key = "%s %d %d %d %d %d | " % (tag, H, W, B, iters, allow)
    rows = [l[len(key):].split() for l in lines if l.startswith(key)]
    assert len(rows) == 1, key
    form, rest = rows[0][0], [int(x) for x in rows[0][1:]]
    return dict(zip(("form", "vec", "rpw", "nb", "folds", "two_forms", "pipelined", "prio_stairs"), [form] + rest))


def test_the_trait_is_true_exactly_for_the_listed_forms(lines):
    t = _traits(lines)
    assert {k for k, v in t.items() if v} == STAIRS_FORMS


def test_no_multi_launch_form_and_no_4x8_has_the_staircase(lines):
    t = _traits(lines)
    assert all(v == 0 for (vec, rpw, persist, fold), v in t.items() if not persist)
    assert all(v == 0 for (vec, rpw, persist, fold), v in t.items() if vec == 4 and rpw == 8)
    assert all(v == 0 for (vec, rpw, persist, fold), v in t.items() if not fold)


def test_the_headline_plan_reports_it(lines):
    p = _plan(lines, "PLAN", 256, 256, 64, 100, 1)
    assert p == dict(form="persistent", vec=4, rpw=6, nb=4, folds=1, two_forms=1, pipelined=1, prio_stairs=1)
    q = _plan(lines, "PLAN", 256, 256, 64, 100, 0)
    assert q["form"] == "bands" and (q["vec"], q["rpw"]) == (4, 6) and q["prio_stairs"] == 0
    for B in (32, 64):                                        # configs[1] and the dataset leg: not timed with it, so without it
        assert _plan(lines, "PLAN", 128, 128, B, 20, 1)["prio_stairs"] == 0


def test_the_smallest_256_shape_with_the_staircase(lines):
    p = _plan(lines, "SMALLEST", 256, 256, SMALLEST_256[0], SMALLEST_256[1], 1)
    assert p["prio_stairs"] == 1 and p["two_forms"] == 1 and p["folds"] == 1 and p["nb"] >= 2 and (p["vec"], p["rpw"]) == (4, 6)
