"""The gather plan of the orbit render's gradient (smokephysai_amd/csrc/orbit_grad_plan.h), checked on the host: a stand-alone program
(tests/host/orbit_grad_plan_main.cpp, its own main) includes the header -- the text the kernels compile -- and walks, for the 16 shapes
of tests/test_orbit_plan_host.py and a grid of azimuths (every 2.5 degrees from -360 to 720, every 22.5 or 45 off the quarter turns for
the widest shapes, and every quarter turn and its neighbours at +- 1e-3 degrees), every view, sample and tap as the ray pass does: every
sample one of whose in-volume taps is voxel (z, x) lies inside that voxel's candidate window and gets the forward's weight there, no
window exceeds the stated maximum of 4 x 4 candidates, and no LDS or scratch index leaves its buffer; the units into which a call cuts
its batch tile it exactly once.  An out-of-range scratch index is the way these kernels go wrong, and this needs no GPU.  Built with
the host address and undefined-behaviour sanitizers where the toolchain has their runtimes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "orbit_grad_plan_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("orbitgradplan") / "orbit_grad_plan")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", INC, SRC, "-o", out]
    # a plain host executable: sanitizers where the toolchain has the runtimes, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_every_tap_finds_its_sample_in_the_voxels_window(exe):
    run = subprocess.run([exe, "walk"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    m = re.search(r"^SHAPES (\d+) ANGLES (\d+) SAMPLES (\d+) TAPS (\d+) MAX_REACH ([0-9.]+) WINDOW (\d+) UNITS (\d+) CELLS (\d+) "
                  r"VIOLATIONS (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    print(run.stdout.strip())
    shapes, angles, samples, taps = (int(m.group(i)) for i in (1, 2, 3, 4))
    reach, window, units, cells, violations = float(m.group(5)), int(m.group(6)), int(m.group(7)), int(m.group(8)), int(m.group(9))
    assert shapes == 16 and angles == 12 * (433 + 39) + 2 * (49 + 39) + 2 * (25 + 39)
    assert samples > 10 ** 8 and taps > 10 ** 7                       # the walk reaches oblique and axis-aligned views alike
    assert window == 4 and 1.41 < reach < 1.42                         # sqrt(2) is reached, and the reach of 1.5 leaves 0.08 to spare
    assert units > 100 and cells > 10 ** 7                             # whole-volume units and row ranges, walked cell by cell
    assert violations == 0, run.stdout[:4000]
