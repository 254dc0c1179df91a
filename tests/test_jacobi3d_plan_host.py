"""The launch plan of the 3-D Jacobi sweeps (smokephysai_amd/csrc/jacobi3d_plan.h), checked on the host: a stand-alone program
(tests/host/jacobi3d_plan_main.cpp, its own main) includes the header -- the text launch3_jacobi compiles -- and
  * enumerates pitches W .. W+9, pointer offsets 0 / 4 / 8 / 12, odd and even D and H, three widths, nine sweep counts, with and without a
    third buffer: the launches add up to the sweeps, and where a four-cells-per-thread kernel is selected every float4 it makes of p, pn
    and div is 16-byte aligned (address arithmetic, not the gate's predicate); the enumeration reaches all three branches of the gate;
  * holds the simulator class's own layout to the plans launch3_jacobi made before the gate moved into the header."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "jacobi3d_plan_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("plan3d") / "jacobi3d_plan")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", out]
    # a plain host executable: address and undefined-behaviour checks where the toolchain has the runtimes, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_every_selected_quad_access_is_aligned_and_the_launches_add_up(exe):
    run = subprocess.run([exe, "alignment"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    m = re.search(r"^ALIGNMENT3D CASES (\d+) QUAD (\d+) VEC_NOT_QUAD (\d+) NARROW (\d+) VIOLATIONS (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    cases, quad, vec_only, narrow, violations = map(int, m.groups())
    assert cases == 2 * 2 * 3 * 10 * 4 * 3 * 9 * 2           # D x H x W x pitch x offset x B x sweeps x third buffer
    assert min(quad, vec_only, narrow) > 0
    assert violations == 0, run.stdout[:4000]


def test_the_simulator_layout_keeps_the_plans_it_had(exe):
    run = subprocess.run([exe, "wrapper"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    m = re.search(r"^WRAPPER3D (\d+) MISMATCH (\d+)$", run.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 10 and int(m.group(2)) == 0, run.stdout[:4000]
