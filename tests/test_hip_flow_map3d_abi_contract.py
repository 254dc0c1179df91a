"""smk_flow_map3d_step and smk_ftle3d_field held to what include/smokehip.h promises about memory and streams, in the harness of
tests/test_hip_abi_contract.py (tests/guarded_arena.py); the cases are tests/abi_contract_cases_flow_map3d.py: every field lies in one
arena the test owns with its rows pitched apart (pitches strictly larger than the rows), the fp32 pointers 4-byte aligned and no better,
the fp64 stats and the workspace 8-byte aligned and no better, the workspace exactly as large as smk_ftle3d_workspace says, every other
byte -- the padding of every row included -- a guard.

For every case: no guard word changes under a NaN fill or a zero fill; the outputs of the two runs are bit-equal, hold no fill word (every
element written) and are finite; the inputs come back unchanged; the outputs equal the dense, aligned call; and the call runs on the
caller's stream without waiting for it.  A workspace one byte short, and one that is 4-byte aligned only, are refused and leave the arena
as it was."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from abi_contract_cases_flow_map3d import ENTRY_POINTS, all_cases                                                      # noqa: E402
from guarded_arena import FILL_NAN, FILL_ZERO, Arena, Binder, bits, holds_fill, run_guarded                          # noqa: E402
from test_hip_abi_contract import DELAY_SECONDS, independent_side_stream, sleep_cycles_per_second                     # noqa: E402

CASES = all_cases()
case_param = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
_RUNS = {}


def _fills(case):
    """The two guarded runs of a case, shared by its tests and left unchanged."""
    if case.id not in _RUNS:
        _RUNS[case.id] = (run_guarded(case, FILL_NAN), run_guarded(case, FILL_ZERO))
    return _RUNS[case.id]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def test_the_table_reaches_every_entry_point():
    assert {c.entry for c in CASES} == set(ENTRY_POINTS)
    assert {c.id.split("-")[-1] for c in CASES if c.entry == "smk_flow_map3d_step"} == {"dir0", "dir1"}
    for entry in ENTRY_POINTS:                            # two shapes each
        assert len({c.id.split("-")[1] for c in CASES if c.entry == entry}) == 2, entry


@case_param
def test_keeps_to_its_buffers(case):
    nan, zero = _fills(case)
    assert nan.damage == 0, f"{case.id}, NaN fill: {nan.damage}"
    assert zero.damage == 0, f"{case.id}, zero fill: {zero.damage}"


@case_param
def test_reads_nothing_foreign_and_writes_every_element(case):
    nan, zero = _fills(case)
    assert set(nan.outputs) == {b.name for b in case.bufs if b.role in ("out", "inout")}
    for name, out in nan.outputs.items():
        assert _same_bits(out, zero.outputs[name]), f"{case.id}: {name} depends on the memory around the buffers"
        assert holds_fill(out, FILL_NAN) == 0, f"{case.id}: {holds_fill(out, FILL_NAN)} elements of {name} were never written"
        assert bool(torch.isfinite(out).all()), f"{case.id}: {name} is not finite"
    given = case.inputs()
    for run in (nan, zero):
        for name, after in run.inputs.items():
            assert _same_bits(after.reshape(-1).cpu(), given[name].reshape(-1)), f"{case.id}: the input '{name}' was written to"


@case_param
def test_same_values_as_the_dense_call(case):
    nan, _ = _fills(case)
    want = case.reference()
    assert set(want) == set(nan.outputs)
    for name, out in nan.outputs.items():
        differ = bits(out.reshape(-1)) != bits(want[name].reshape(-1))
        assert not bool(differ.any()), f"{case.id}: {name} differs from the dense, aligned call in {int(differ.sum())} of {differ.numel()} elements"


@case_param
def test_runs_on_the_callers_stream_without_waiting(case):
    nan, _ = _fills(case)                         # (also: every kernel of the call is loaded before the timed one)
    side = independent_side_stream()
    assert side is not None, "no side stream runs independently of the null stream here: the stream check could not tell anything"
    run = run_guarded(case, FILL_NAN, stream=side, delay_cycles=DELAY_SECONDS * sleep_cycles_per_second())
    print(f"{case.id}: host time of the call {run.host_seconds * 1e3:.3f} ms behind a delay of {DELAY_SECONDS * 1e3:.0f} ms")
    assert run.host_ahead, (f"{case.id}: the event behind the {DELAY_SECONDS} s delay had completed when the call returned after "
                            f"{run.host_seconds:.4f} s of host time: the call waited for the stream, or the delay is too short to tell")
    assert run.damage == 0, f"{case.id}, side stream: {run.damage}"
    for name, out in run.outputs.items():
        assert _same_bits(out, nan.outputs[name]), f"{case.id}: {name} differs on a side stream: part of the call left the caller's stream"


def _refused(case, buffers, fill, word):
    from smokephysai_amd import _lib
    lib = _lib.load()
    arena = Arena(buffers)
    arena.fill(fill)
    torch.cuda.synchronize()
    before = arena.buf.clone()
    rc = getattr(lib, case.entry)(*case.args(Binder(arena, _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device())))))
    torch.cuda.synchronize()
    assert rc == _lib.SMK_ERR_INVALID and word in lib.smk_last_error().decode()
    assert torch.equal(arena.buf, before), "a refused call wrote to the arena"


@pytest.mark.parametrize("fill", [FILL_NAN, FILL_ZERO], ids=["nan", "zero"])
def test_a_workspace_one_byte_short_is_refused(fill):
    from smokephysai_amd import _lib
    lib = _lib.load()
    case = next(c for c in CASES if c.entry == "smk_ftle3d_field")
    ws = next(b for b in case.buffers(lib) if b.role == "ws")
    _refused(case, [b for b in case.buffers(lib) if b.role != "ws"] + [dataclasses.replace(ws, elems=ws.elems - 1)], fill, "workspace")


def test_a_workspace_that_is_only_4_byte_aligned_is_refused():
    from smokephysai_amd import _lib
    lib = _lib.load()
    case = next(c for c in CASES if c.entry == "smk_ftle3d_field")
    ws = next(b for b in case.buffers(lib) if b.role == "ws")
    _refused(case, [b for b in case.buffers(lib) if b.role != "ws"] + [dataclasses.replace(ws, align=4, phase=4)], FILL_NAN, "8-byte")
