"""The row map and the group rule of smk_ftle3d_field (smokephysai_amd/csrc/flow_map3d.h), checked on the host in the pattern of
tests/test_tangent3d_rows_host.py: a stand-alone program (tests/host/ftle3d_rows_main.cpp, its own main) includes the header -- the text
the kernel, the launcher and the workspace query compile -- and walks the groups and rows of an FTLE call as the kernel does, over the
device tests' shapes and larger ones, dense and pitched.  Every cell is visited exactly once, no padding element is visited, no offset
leaves the volume, the groups tile the rows, and the workspace the walk needs is what smk_ftle3d_workspace returns.  One shape has
D * H > 4096, so that a run exceeds 16 rows.  Built with the host address and undefined-behaviour sanitizers where the toolchain has their
runtimes; the executable is run directly."""
import os
import re
import shutil
import subprocess

import pytest

from smokephysai_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ftle3d_rows_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")
# test_hip_flow_map3d.py's (flow_map3d_oracle.GRIDS, FAR, LONG_ROWS) and the ABI contract's
DEVICE_SHAPES = {(3, 3, 3), (4, 5, 7), (9, 19, 37), (12, 33, 40), (6, 12, 16), (16, 272, 8), (6, 19, 37)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("ftle3drows") / "ftle3d_rows")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", out]
    # a plain host executable: sanitizers where the toolchain has the runtimes, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _program_cases():
    text = open(SRC).read()
    shapes = re.search(r"const int shapes\[\]\[3\] = \{(.*?)\};", text, flags=re.S).group(1)
    pads = re.search(r"const int pads\[\] = \{(.*?)\};", text, flags=re.S).group(1)
    return [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", shapes)], [int(v) for v in re.findall(r"\d+", pads)]


def test_the_program_walks_the_device_tests_shapes_dense_and_pitched():
    import flow_map3d_oracle as F3
    from abi_contract_cases_flow_map3d import SHAPES
    shapes, pads = _program_cases()
    assert DEVICE_SHAPES == set(F3.GRIDS) | {F3.FAR[0], F3.LONG_ROWS} | set(SHAPES)
    assert DEVICE_SHAPES <= set(shapes)
    assert 0 in pads and any(p > 0 for p in pads)
    assert any(D * H > 4096 for D, H, _ in DEVICE_SHAPES)


def test_every_cell_is_visited_once_and_the_groups_tile_the_rows(exe):
    run = subprocess.run([exe, "walk"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    m = re.search(r"^CASES (\d+) ELEMENTS (\d+) ROWS (\d+) GROUPS (\d+) WORKSPACE (\d+) LONGEST (\d+) VIOLATIONS (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    print(run.stdout.strip())
    cases, elements, rows, groups, workspace, longest, violations = (int(v) for v in m.groups())
    shapes, pads = _program_cases()
    assert cases == len(shapes) * len(pads)
    assert elements == len(pads) * sum(D * H * W for D, H, W in shapes)
    assert rows == len(pads) * sum(D * H for D, H, W in shapes)
    L = _lib.load()
    assert workspace == len(pads) * sum(L.smk_ftle3d_workspace(2, D, H, W) for D, H, W in shapes)
    assert groups * 2 * 2 * 8 == workspace
    assert longest > 16                                        # a run longer than the minimum was walked
    assert violations == 0, run.stdout[:4000]
