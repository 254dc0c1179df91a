"""The march plan of the free-camera render (smokephysai_amd/csrc/camera_plan.h), checked on the host: a stand-alone program
(tests/host/camera_plan_main.cpp, its own main) includes the header -- the text the kernel compiles -- and walks, for 17 shapes (the
shapes of tests/test_hip_render_camera.py, single planes, rows and columns, the limits D = 64 and W = 1024 and a tall H = 1024) and a
grid of (azimuth, elevation) plus every exact quarter turn and right angle and 1e-3 degrees beside it (112 views, the same for every
shape), every tile, chunk and sample as the kernel does: a skipped chunk has no tap inside the volume (so no tap inside the volume is
missed), every position lies inside its brick's extremes, and every offset the kernel would read is the tap's own and inside the volume.  An out-of-range global offset is the
way this kernel goes wrong, and this needs no GPU.  Built with the host address and undefined-behaviour sanitizers where the toolchain
has their runtimes.  The same program prints the view coefficients of the library's angle rule, held equal to the oracle's."""
import os
import re
import shutil
import subprocess

import pytest

from render_camera_oracle import camera_coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "camera_plan_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("cameraplan") / "camera_plan")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", INC, SRC, "-o", out]
    # a plain host executable: sanitizers where the toolchain has the runtimes, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_every_tap_inside_the_volume_is_read_at_its_own_offset(exe):
    run = subprocess.run([exe, "walk"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    m = re.search(r"^SHAPES (\d+) VIEWS (\d+) SAMPLES (\d+) LIVE (\d+) SKIPPED (\d+) TAPS_INSIDE (\d+) VIOLATIONS (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    shapes, views, samples, live, skipped, taps_inside, violations = map(int, m.groups())
    print(run.stdout.strip())
    per_shape = 8 * 7 + 6 * 3 * 2 + 6 * 2 + 4 * 2               # the grid; quarter turns +- 1e-3; right angles and 1e-3 inside; exact pairs
    assert shapes == 17 and views == 17 * per_shape             # every shape, the limits included, walks every view
    # marched and skipped chunks alike (measured: 8.0e8 samples, 296165 marched and 7.7e6 skipped chunks, 3.2e8 taps inside a volume)
    assert samples > 5 * 10 ** 8 and live > 10 ** 5 and skipped > 10 ** 6 and taps_inside > 10 ** 8
    assert violations == 0, run.stdout[:4000]


def test_the_angle_rule_of_the_library_is_the_oracles(exe):
    views = [(0, 0), (90, 0), (0, 90), (0, -90), (180, 90), (270, -90), (37.5, 30), (-123, -60), (200.25, 12.5), (720.001, 45), (45, 0.001),
             (90.001, 89.999), (-1e-3, -89.999), (1e6 + 0.25, 1e-9), (450, 60), (-180, -30)]
    args = [repr(float(v)) for view in views for v in view]
    run = subprocess.run([exe, "angles"] + args + ["0.0", "90.5", "0.0", "nan", "inf", "0.0"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [line.split() for line in run.stdout.splitlines() if line.startswith("ANGLE ")]
    assert len(rows) == len(views) + 3 and all(r[3] == "INVALID" for r in rows[len(views):])
    for (phi, theta), row in zip(views, rows):
        (rx, ry, rz), (ex, ey, ez), (dx, dy, dz) = camera_coefficients(phi, theta)
        assert ry == 0.0
        got = [float.fromhex(h) for h in row[3:]]
        want = [float(v) for v in (rx, rz, ex, ey, ez, dx, dy, dz)]
        assert got == want, (phi, theta, row, want)
    for bad in ((0.0, 90.5), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(ValueError):
            camera_coefficients(*bad)
