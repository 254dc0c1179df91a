"""The two forms of the Jacobi cell and the guard between them (smokephysai_amd/csrc/stencil.h), checked on the host: a stand-alone
program (tests/host/jacobi_cell_forms_main.cpp, its own main) includes the header's inlines -- the text the kernel compiles -- and runs
1.5e8 operand pairs (S, d) the guard accepts through both: S over all finite bit patterns, d in {+-0} and [2^-100, 2^100], S within 16 ulp
of d and equal to it, S denormal, both signs of zero.  Not one word may differ.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "jacobi_cell_forms_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("cellforms") / "jacobi_cell_forms")
    base = [cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", INC, SRC, "-o", exe]
    # a plain host executable: undefined-behaviour checks where the toolchain has the runtime, without them otherwise
    r = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    return run.stdout


def test_no_word_differs_under_the_guard(report):
    m = re.search(r"PAIRS (\d+) DIFFERING (\d+) REJECTED_BY_GUARD (\d+)", report)
    assert m, report[-2000:]
    pairs, differing, rejected = map(int, m.groups())
    assert pairs >= 10 ** 8
    assert rejected == 0                                     # every d the program draws is one the guard accepts
    assert differing == 0, report[:2000]


def test_guard_edges(report):
    m = re.search(r"^GUARD (.*)$", report, flags=re.M)
    got = dict(kv.split("=") for kv in m.group(1).split())
    accepted = {"lo", "-lo", "hi", "-hi", "zero", "-zero"}   # 2^-100, 2^100 and both zeros; 1 ulp outside, NaN, Inf and denormals fail
    assert {k for k, v in got.items() if v == "1"} == accepted, got
    assert set(got) == accepted | {"nan", "-nan", "inf", "-inf", "below", "-below", "above", "-above", "denormal"}


def test_the_forms_differ_without_the_guard(report):
    """S = 2^-149, d = -2^-148: the exact cell gives 2^-149, the fused one 0 -- and the guard rejects this d."""
    m = re.search(r"COUNTEREXAMPLE guard=(\d) exact_bits=([0-9a-f]{8}) fused_bits=([0-9a-f]{8})", report)
    assert m.groups() == ("0", "00000001", "00000000"), report[-500:]
