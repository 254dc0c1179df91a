"""The staging plan of the orbit render (smokephysai_amd/csrc/orbit_plan.h), checked on the host: a stand-alone program
(tests/host/orbit_plan_main.cpp, its own main) includes the header -- the text the kernel compiles -- and walks, for 16 shapes (the
shapes of tests/test_hip_render_orbit.py, the limits D = 64 and W = 1024, single planes and single columns) and a grid of azimuths
(every 0.5 degrees from -360 to 720, every 7.5 to 22.5 for the widest shapes, and every quarter turn +- 1e-3 degrees), every strip, chunk and
sample as the kernel does: every neighbour of a sample that lies inside the volume lies inside the staged box, a skipped chunk has no
neighbour inside the volume, no box is larger than the LDS reserved for it, and no LDS index leaves the box.  An out-of-range LDS
index is the way this kernel goes wrong, and this needs no GPU.  Built with the host address and undefined-behaviour sanitizers where
the toolchain has their runtimes."""
import os
import re
import shutil
import subprocess

import pytest

from render_orbit_oracle import orbit_cos_sin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "orbit_plan_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("orbitplan") / "orbit_plan")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", INC, SRC, "-o", out]
    # a plain host executable: sanitizers where the toolchain has the runtimes, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_every_sample_finds_its_neighbours_in_the_staged_box(exe):
    run = subprocess.run([exe, "walk"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    m = re.search(r"^SHAPES (\d+) ANGLES (\d+) SAMPLES (\d+) BOXES (\d+) EMPTY (\d+) MAX_CELLS (\d+) MAX_SIDE (\d+) VIOLATIONS (\d+)$",
                  run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    shapes, angles, samples, boxes, empty, max_cells, max_side, violations = map(int, m.groups())
    print(run.stdout.strip())
    assert shapes == 16 and angles == 12 * (2161 + 26) + (145 + 26) + (73 + 26) + 2 * (49 + 26)
    assert samples > 10 ** 8 and boxes > 10 ** 5 and empty > 10 ** 4          # the walk reaches staged and skipped chunks alike
    assert 40 * 40 < max_cells <= 46 * 46 and 44 <= max_side <= 46            # the oblique angles fill the reserved box, none exceeds it
    assert violations == 0, run.stdout[:4000]


def test_the_angle_rule_of_the_library_is_the_oracles(exe):
    phis = [0, 90, -270, 450, 720.0, 180, -180, 270, -90, 90.001, 89.999, 37.5, -123, 200.25, 720.001, 1e6 + 0.25, -1e-3, 359.5]
    run = subprocess.run([exe, "angles"] + [repr(float(p)) for p in phis], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [line.split() for line in run.stdout.splitlines() if line.startswith("ANGLE ")]
    assert len(rows) == len(phis)
    for phi, (_, _, c, s) in zip(phis, rows):
        wc, ws = orbit_cos_sin(phi)
        assert float.fromhex(c) == float(wc) and float.fromhex(s) == float(ws), (phi, c, s, wc, ws)
