"""The launch plan of the 2-D pressure projection (smokephysai_amd/csrc/jacobi_plan.h), checked on the host: a stand-alone program
(tests/host/projection_plan_main.cpp, its own main) includes the header -- the text the launchers compile -- and
  * checks what every plan must satisfy over a sweep of geometries (H 32 .. 1024 with non-multiples of 16, six widths, aligned and unaligned
    pitches, four batch sizes, seven sweep counts, 32 and 256 compute units, both values of allow_persist and with_gradient): the owned
    rows of the bands tile the grid, every tile lies in the grid and holds its owned rows and halo, the runs add up and fit the halo, a
    persistent plan fits the device, and the keep buffer's slots are used once;
  * recomputes tests/host/projection_plans_parent.txt, the plans and descriptions recorded from the planner as it was before it moved into
    the header, byte for byte;
(Both of these are about plan_projection, the plan worked out from the grid's shape; what a launch takes is plan_projection_on, that plan
held to the layout it runs on, which the next two are about.)
  * recomputes the plans of the simulator classes' own layout at every shape bench.py and tests/test_hip_physics.py step and holds them to
    the literals recorded before pointer and stride terms entered the gates (the alignment gates must not reroute that layout);
  * enumerates pitches W .. W+9, pointer offsets 0 / 4 / 8 / 12, odd and even H: every 8- or 16-byte access of the forms the gates select
    (DESIGN "Stepper state layouts") is naturally aligned, checked by address arithmetic and not by the gates' own predicate.
On the GPU a fresh simulator's jacobi_plan() must give the recorded description of its row (no kernel runs)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "projection_plan_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")
PARENT = os.path.join(ROOT, "tests", "host", "projection_plans_parent.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("projplan") / "projection_plan")
    base = [cxx, "-O2", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", out]
    # a plain host executable: undefined-behaviour checks where the toolchain has the runtime, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_every_plan_keeps_the_invariants(exe):
    run = subprocess.run([exe, "invariants"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    m = re.search(r"^PLANS (\d+) BAND_KERNEL (\d+) PERSISTENT (\d+) FOLDING (\d+) VIOLATIONS (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    plans, band, persistent, folding, violations = map(int, m.groups())
    assert plans == 20 * 6 * 3 * 4 * 7 * 2 * 2 * 2           # H x W x pitches x B x iters x num_cu x allow_persist x with_gradient
    assert band > plans // 4 and persistent > 1000 and folding > 1000     # the sweep reaches every form
    assert violations == 0, run.stdout[:4000]


def test_same_plans_as_before_the_move(exe):
    want = open(PARENT).read()
    assert len(want) < 64 * 1024 and want.count("\nPLAN ") >= 300 and want.count("\nDESC ") >= 12
    run = subprocess.run([exe, "table", PARENT], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    got_lines, want_lines = run.stdout.splitlines(), want.splitlines()
    differing = [(w, g) for w, g in zip(want_lines, got_lines) if w != g]
    assert not differing, differing[:5]
    assert run.stdout == want


def test_the_simulator_layout_keeps_the_plans_it_had(exe):
    """Rows padded to 32 floats, 16-byte aligned pointers: plan structs and the buoyancy/diffusion form equal to the recorded literals."""
    run = subprocess.run([exe, "wrapper"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    m = re.search(r"^WRAPPER (\d+) MISMATCH (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    assert int(m.group(1)) >= 60 and int(m.group(2)) == 0, run.stdout[:4000]


def test_every_selected_wide_access_is_naturally_aligned(exe):
    run = subprocess.run([exe, "alignment"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    m = re.search(r"^ALIGNMENT CASES (\d+) VEC4 (\d+) SCALAR (\d+) FOLD (\d+) BAND1 (\d+) BAND2 (\d+) BAND4 (\d+) BAND8 (\d+) SWEEPS (\d+) "
                  r"MISALIGNED (\d+)$", run.stdout, flags=re.M)
    assert m, run.stdout[-2000:]
    cases, vec4, scalar, fold, b1, b2, b4, b8, sweeps, bad = map(int, m.groups())
    assert cases == 7 * 7 * 10 * 10 * 4 * 4 * 2 * 2 * 2      # H x W x pitch_c x pitch_v x input offset x projected-uv offset x B x iters x allow_persist
    assert min(vec4, scalar, fold, b1, b2, b4, b8, sweeps) > 0          # the enumeration reaches every form
    assert bad == 0, run.stdout[:4000]


def _recorded_description(H, W, B, iters):
    """The DESC row of a simulator's geometry (its pitches: rows padded to 32 floats) on 256 compute units, persistent form allowed."""
    pc, pv = (W + 31) // 32 * 32, (W + 32) // 32 * 32
    key = "DESC %d %d %d %d %d %d 256 1 1 | " % (H, W, pc, pv, B, iters)
    rows = [line[len(key):] for line in open(PARENT).read().splitlines() if line.startswith(key)]
    assert len(rows) == 1, key
    return json.loads(rows[0])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,B,iters", [(64, 64, 2, 2), (128, 128, 2, 5), (256, 256, 2, 20), (96, 96, 2, 5)])
def test_a_simulator_reports_the_recorded_plan(H, W, B, iters):
    import torch

    from smokephysai_amd.physics import NavierStokesSimulator

    want = _recorded_description(H, W, B, iters)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip("the recorded plans are those of 256 compute units; this device has %d" % cus)
    ns = NavierStokesSimulator((H, W), device="cuda:0", batch_size=B, jacobi_iters=iters)
    assert ns.jacobi_plan()["projection"] == want
