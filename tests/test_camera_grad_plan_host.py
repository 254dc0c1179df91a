"""The gather plan of the free-camera render's gradient (smokephysai_amd/csrc/camera_grad_plan.h), checked on the host: a stand-alone
program (tests/host/camera_grad_plan_main.cpp, its own main) includes the header -- the text the kernels compile -- and walks the shapes
and views of the device test (render_camera_oracle.GPU_SHAPES x GPU_VIEWS): (a) every sample one of whose in-volume taps is voxel
(z, y, x) lies inside that voxel's 4 x 4 x 4 candidate window and gets the forward's weight there; (b) for every band height from 1 to H
every voxel is owned by exactly one band, lies in that band's slab, and every candidate of it with a weight lies in a row the band marches
and in a chunk the ray pass keeps; (c) no scratch offset leaves the scratch; (d) at the limit shapes and near-exact views the window still
holds and at least four marched rows fit the scratch.  A missed sample or an out-of-range scratch index is the way these kernels go
wrong, and this needs no GPU.  Built with the host address and undefined-behaviour sanitizers where the toolchain has their runtimes."""
import os
import re
import shutil
import subprocess

import pytest

from render_camera_oracle import GPU_SHAPES, GPU_VIEWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "camera_grad_plan_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("cameragradplan") / "camera_grad_plan")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", INC, SRC, "-o", out]
    # a plain host executable: sanitizers where the toolchain has the runtimes, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_the_program_walks_the_device_tests_cases():
    """The shape and view lists of the program are the device test's."""
    text = open(SRC).read()
    shapes = re.search(r"const int shapes\[\]\[3\] = \{(.*?)\};", text, flags=re.S).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", shapes)] == GPU_SHAPES
    views = re.search(r"const double views\[\]\[2\] = \{(.*?)\};", text, flags=re.S).group(1)
    assert tuple((float(a), float(b)) for a, b in re.findall(r"\{(-?[\d.]+), (-?[\d.]+)\}", views)) == GPU_VIEWS


def test_every_tap_finds_its_sample_and_every_voxel_its_band(exe):
    run = subprocess.run([exe, "walk"], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    m = re.search(r"^SHAPES (\d+) VIEWS (\d+) SAMPLES (\d+) TAPS (\d+) MAX_REACH ([0-9.]+) WINDOW (\d+) VOXELS (\d+) BANDS (\d+) "
                  r"CANDIDATES (\d+) LIMIT_TAPS (\d+) MIN_FIT (\d+) VIOLATIONS (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    print(run.stdout.strip())
    shapes, views, samples, taps = (int(m.group(i)) for i in (1, 2, 3, 4))
    reach, window = float(m.group(5)), int(m.group(6))
    voxels, bands, candidates, limit_taps, min_fit, violations = (int(m.group(i)) for i in range(7, 13))
    assert shapes == len(GPU_SHAPES) and views == len(GPU_SHAPES) * len(GPU_VIEWS)
    assert voxels == len(GPU_VIEWS) * sum(d * h * w for d, h, w in GPU_SHAPES)
    assert bands == 2 * len(GPU_VIEWS) * sum(sum(-(-h // r) for r in range(1, h + 1)) for _, h, _ in GPU_SHAPES)   # every height, lit and unlit
    assert samples > 10 ** 7 and taps > 10 ** 7 and candidates > 10 ** 7 and limit_taps > 10 ** 6
    assert window == 4 and 1.6 < reach < 3 ** 0.5 + 0.005              # near sqrt(3), and the reach of 1.75 has room to spare
    assert min_fit >= 4                                                # the scratch holds a band of one row and its three neighbours
    assert violations == 0, run.stdout[:4000]
