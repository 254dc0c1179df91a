"""The table of tests/stepper_layout_cases.py against the CPU plan code: every form string a case is listed for is the one the plan
headers (jacobi_plan.h, jacobi3d_plan.h, through the host programs of tests/host) select for the case's pitches and offsets, and the table
reaches every form the describe calls can report at these shapes.  The expected set comes from the plan code, not from a GPU run."""
import json
import os
import shutil
import subprocess

import pytest

import stepper_layout_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("layout_table")
    out = {}
    for name in ("projection_plan", "jacobi3d_plan"):
        out[name] = str(d / name)
        r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", INC, os.path.join(ROOT, "tests", "host", name + "_main.cpp"), "-o", out[name]],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip()


def test_2d_cases_list_the_forms_the_plan_selects_and_reach_all_of_them(exes):
    seen_kernels, seen_buoy = set(), set()
    for H, W, J in S.SHAPES_2D:
        for lay in S.LAYOUTS:
            in_off = lay.off[0] | lay.off[1] | lay.off[3]              # u, v, density: what a step reads (p is never read in rows)
            for persist in (True, False):
                kernel, how, buoy, _stage = _run(exes["projection_plan"], "forms", H, W, S.B2, lay.pc(W), lay.pv(W), in_off, 0, J, int(persist)).split("|")
                want = S.forms_2d(H, W, lay.name, persist)
                assert (kernel, buoy) == (want["kernel"], want["buoy_diffuse"]), (H, W, lay.name, persist)
                assert kernel == "k_jacobi_sweep" or (how == "persistent") == persist, (H, W, lay.name, persist)
                seen_kernels.add(kernel.split(",")[0])
                seen_buoy.add(buoy)
    # every cell count of the band kernel, the per-sweep kernel, and the three forms of the buoyancy / diffusion stage
    assert seen_kernels == {"k_jacobi_band<1", "k_jacobi_band<2", "k_jacobi_band<4", "k_jacobi_band<8", "k_jacobi_sweep"}
    assert seen_buoy == {"vec4", "scalar", "folded into the projection"}
    # each band shape is reached both on the vector path and, through an alignment gate, on the per-sweep kernel
    for H, W in ((96, 128), (256, 256), (64, 512)):
        kinds = {S.forms_2d(H, W, lay.name, True)["kernel"] == "k_jacobi_sweep" for lay in S.LAYOUTS}
        assert kinds == {True, False}, (H, W)


def test_3d_cases_list_the_forms_the_plan_selects_and_reach_all_of_them(exes):
    branches = set()
    for D, H, W, J in S.SHAPES_3D:
        for lay in S.LAYOUTS:
            d = json.loads(_run(exes["jacobi3d_plan"], "forms", S.B3, D, H, W, lay.pc(W), lay.off[2], J, 0))
            want = S.forms_3d(D, H, W, lay.name)
            assert (d["jacobi"], d["jacobi_sweep"], d["alignment"]["vec"], d["alignment"]["quad"]) == \
                (want["jacobi"], want["jacobi_sweep"], want["vec"], want["quad"]), (D, H, W, lay.name)
            branches.add((W % 4 == 0, want["vec"], want["quad"]))
    # quad; vec && !quad; !vec at W % 4 == 0; the generic width
    assert branches == {(True, True, True), (True, True, False), (True, False, False), (False, False, False)}
    sweeps = {S.forms_3d(D, H, W, lay.name)["jacobi_sweep"] for D, H, W, J in S.SHAPES_3D for lay in S.LAYOUTS}
    assert sweeps == {None, "quad per-sweep", "per-sweep"}
