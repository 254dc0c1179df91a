"""The stateless C ABI (include/smokehip.h) held to what it promises about memory and streams -- "caller-owned memory", "the caller's
stream", "nothing allocated, no synchronisation", "workspace: at least smk_*_workspace(...) bytes", "every element written exactly once",
"planes *_stride floats apart" -- for the volume renders and their gradient, the SSIM forward and backward, the statistics, the
optical-flow methods, the train-step tail, the 3-D training convolutions (tests/abi_contract_cases.py) and the calls of a training step:
the 2-D training convolutions, the BatchNorm passes, the reconstruction head's convolutions, LayerNorm, the attention forward / backward /
delta, the linear weight gradient, the FFN's element-wise chain, the chaos term and the gradient exchange
(tests/abi_contract_cases_train.py).  The harness is tests/guarded_arena.py: every buffer of a call lies in one arena the test owns,
planes strided, pointers no better aligned than the header asks, the workspace exactly as large as its query says, and every other byte a
guard.

For every case:
  1. buffers         the call runs with the arena filled with 0xFFFFFFFF (NaN) and with 0: no guard byte changes under either -- the gaps
                     between planes and everything behind the workspace's stated size included;
  2. nothing foreign the outputs of the two runs are bit-equal, no output word of the NaN run still holds the fill (every element is
                     written; uint8 outputs, where 0xFF is a pixel value, are covered by the bit-equality), and the inputs are what was
                     copied in (with write_grad = 1 the gradients are outputs);
  3. same values     the outputs are bit-equal to reference(): the dense, aligned, wrapper-made call.  Strides, alignment and the
                     workspace's place must not change one bit;
  4. the stream      the call is repeated on a side stream behind a delay (torch.cuda._sleep), the copy of the inputs and an event: the
                     event is still pending when the call returns (the host did not wait, and the delay was long enough to tell), the
                     outputs equal step 1's and the guards are whole.  A kernel or memset of the call that went to the null stream would
                     run while the side stream sleeps, on NaN inputs or ahead of its predecessors.
What this cannot see: a stray read that lands on equal data under both fills (inside another buffer of the same call, say).

Where an entry point demands an alignment, a call with one pointer aligned half as well comes back with SMK_ERR_INVALID and leaves the
whole arena as it was, under both fills (test_a_weaker_alignment_is_refused).

Two controls use torch ops alone and show that the harness catches what it is for.

Out of scope here: the handle-owning objects (the steppers, the encoder, linear and decoder handles), the eval attention calls
(smk_attention / _ws / _kv / _received / _probs: their sentinel buffers are tests/attention_variant_cases.py), the eval 3-D convolutions with
smk_conv3d_im2col / smk_pool3d_accumulate, and the stateless 2-D physics helpers.  smk_decoder_forward and smk_pooled_head are held to the
same arena in tests/test_hip_decoder.py."""
import dataclasses
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from abi_contract_cases import ENTRY_POINTS, all_cases                                                      # noqa: E402
from abi_contract_cases_train import APPLY, BF16, BWD_DZ, BWD_SUMS, F32, REFUSED_ALIGNMENTS, STATS         # noqa: E402
from guarded_arena import FILL_NAN, FILL_ZERO, Arena, Binder, Buf, bits, holds_fill, run_guarded           # noqa: E402

pytestmark = pytest.mark.gpu

CASES = all_cases()
# The delay in front of the call on the side stream.  DESIGN.md "ABI contract tests" has the measurement behind it: at least 20 times the
# host time of the slowest call of the table, at most about 0.3 s.  A condition of the test, not a tolerance: too short a delay fails the
# event assertion below.
DELAY_SECONDS = 0.05
PROBE_DELAY_SECONDS = 0.02        # the delay while a candidate side stream is tried (independent_side_stream)
case_param = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])


@functools.lru_cache(maxsize=None)
def sleep_cycles_per_second() -> float:
    """torch.cuda._sleep counts device clock ticks: how many make a second on this device, from one timed sleep."""
    torch.cuda._sleep(1000)                      # (loads the kernel)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ticks = 4_000_000
    torch.cuda.synchronize()
    start.record()
    torch.cuda._sleep(ticks)
    end.record()
    torch.cuda.synchronize()
    return ticks / (start.elapsed_time(end) * 1e-3)


@functools.lru_cache(maxsize=None)
def _fills(case):
    """Step 1's two runs (shared by the tests of a case, left unchanged)."""
    return run_guarded(case, FILL_NAN), run_guarded(case, FILL_ZERO)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def test_the_table_reaches_every_entry_point():
    assert {c.entry for c in CASES} == set(ENTRY_POINTS)
    for entry, lights in (("smk_volume_render", ("none", "+y", "-y", "+z")), ("smk_volume_render_backward", ("none", "+y", "-y", "+z")),
                          ("smk_volume_render_orbit", ("none", "+y", "-y")), ("smk_volume_render_camera", ("none", "+y", "-y"))):
        for light in lights:
            assert sum(c.entry == entry and c.id.endswith("-" + light) for c in CASES) == 2, (entry, light)      # both shapes
    assert len(ENTRY_POINTS) == len(set(ENTRY_POINTS)) == 21 + 26

    def variants(entry, *keys):
        """The set of tag tuples the cases of an entry point carry (tests/abi_contract_cases_train.py gives every case its tags)."""
        return {tuple(c.tags[k] for k in keys) for c in CASES if c.entry == entry}
    phases = (STATS, APPLY, BWD_SUMS, BWD_DZ)
    for entry in ("smk_conv1_train_forward", "smk_conv2_train_forward", "smk_conv3_sigmoid_train_forward"):
        assert variants(entry, "bias") == {(True,), (False,)}, entry
    for entry in ("smk_conv1_train_wgrad", "smk_conv2_train_wgrad", "smk_linear_wgrad"):
        assert variants(entry, "db") == {(True,), (False,)}, entry
    for entry in ("smk_bn_relu_pool_forward", "smk_bn_relu_pool_backward"):
        assert variants(entry, "pool") == {(p,) for p in (1, 2, 4, 8, 16, 32)}, entry
    assert variants("smk_bn_relu_pool_phase", "pool", "phase", "frozen") == \
        {(p, ph, False) for p in (1, 2, 4, 8, 16, 32) for ph in phases} | {(1, APPLY, True), (1, BWD_DZ, True)}
    assert variants("smk_bn_cl_phase", "C", "pooled", "phase") == {(c, p, ph) for c in (64, 128) for p in (0, 1) for ph in phases}
    assert variants("smk_convt4s2_train_forward", "COUT", "tok") == variants("smk_convt4s2_train_dgrad", "COUT", "tok") == \
        variants("smk_convt4s2_train_wgrad", "COUT", "tok") == {(32, 0), (16, 0), (32, 1), (16, 1)}
    assert variants("smk_convt4s2_train_forward", "bias") == variants("smk_convt4s2_train_wgrad", "db") == {(True,), (False,)}
    assert variants("smk_conv3_sigmoid_train_backward", "grads") == {(True,), (False,)}
    assert variants("smk_layernorm", "split") == {(0,), (1,)}
    assert variants("smk_linear_wgrad", "form") == {("tr",), ("copy",)}
    assert variants("smk_ffn_elementwise", "op", "p") == {(op, p) for op in range(4) for p in (0.0, 0.25)}
    assert variants("smk_chaos_addend_batched", "layers") == {(2,)}
    assert variants("smk_reduce_shards", "world", "formats") >= {(w, f) for w in (1, 3) for f in ((F32, F32), (F32, BF16), (BF16, BF16))}
    assert (3, True) in variants("smk_reduce_shards", "world", "in_place")
    for entry in ENTRY_POINTS[21:]:                       # the training step's calls: two shapes or more each
        assert len({tuple(b.elems * b.planes for b in c.bufs if b.role != "out") for c in CASES if c.entry == entry}) >= 2, entry


@case_param
def test_keeps_to_its_buffers(case):
    nan, zero = _fills(case)
    assert nan.damage == 0, f"{case.id}, NaN fill: {nan.damage}"
    assert zero.damage == 0, f"{case.id}, zero fill: {zero.damage}"


@case_param
def test_reads_nothing_foreign_and_writes_every_element(case):
    nan, zero = _fills(case)
    assert nan.outputs, case.id
    for name, out in nan.outputs.items():
        assert _same_bits(out, zero.outputs[name]), f"{case.id}: '{name}' depends on the memory around the buffers"
        assert holds_fill(out, FILL_NAN) == 0, f"{case.id}: {holds_fill(out, FILL_NAN)} elements of '{name}' were never written"
        if out.is_floating_point():
            assert bool(torch.isfinite(out).all()), f"{case.id}: '{name}' is not finite"
    given = case.inputs()
    for run in (nan, zero):
        for name, after in run.inputs.items():
            assert _same_bits(after.reshape(-1).cpu(), given[name].reshape(-1)), f"{case.id}: the input '{name}' was written to"


@case_param
def test_same_values_as_the_ordinary_path(case):
    nan, _ = _fills(case)
    ref = case.reference()
    assert set(ref) == set(nan.outputs), (sorted(ref), sorted(nan.outputs))
    for name, out in nan.outputs.items():
        want = ref[name].detach()
        assert want.dtype == out.dtype and want.numel() == out.numel(), (case.id, name, want.shape, out.shape)
        differ = bits(out.reshape(-1)) != bits(want.reshape(-1))
        assert not bool(differ.any()), (f"{case.id}: '{name}' differs from the dense, aligned call in {int(differ.sum())} of {differ.numel()} "
                                        f"elements, first at {int(torch.nonzero(differ)[0])}")


def _two_op_chain(side, second_on_null_stream: bool, delay_seconds: float):
    """Step 4's protocol around two torch ops: b = 2 a on the side stream, then c = b + 1 on the side stream or -- the fault the stream check
    is for -- on the null stream, where it runs while the side stream still sleeps and reads b before it is written.
    -> (c, whether the delay was still running when the host had issued everything, the guard damage)"""
    n = 1 << 16
    arena = Arena([Buf("a", torch.float32, n), Buf("b", torch.float32, n, role="out"), Buf("c", torch.float32, n, role="out")])
    staged = torch.arange(n, dtype=torch.float32, device="cuda")
    arena.fill(FILL_NAN)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(delay_seconds * sleep_cycles_per_second()))
        arena.view("a").copy_(staged)
        ev = torch.cuda.Event()
        ev.record()
        torch.mul(arena.view("a"), 2.0, out=arena.view("b"))
        if not second_on_null_stream:
            torch.add(arena.view("b"), 1.0, out=arena.view("c"))
    if second_on_null_stream:
        torch.add(arena.view("b"), 1.0, out=arena.view("c"))
    ahead = not ev.query()
    torch.cuda.synchronize()
    return arena.view("c").clone(), ahead, arena.guard_damage(FILL_NAN)


def _chain_result():
    return torch.arange(1 << 16, dtype=torch.float32, device="cuda") * 2 + 1


@functools.lru_cache(maxsize=None)
def independent_side_stream():
    """A side stream whose pending work the null stream demonstrably does not wait for, or None.  Step 4 means something only on such a
    stream: the runtime spreads its streams over a few hardware queues, and two streams that share one run in the order of submission --
    there a launch that strayed to the null stream would still find its inputs ready.  So every candidate is tried with the two-op chain
    whose second op goes to the null stream, and the first one on which that changes the result is kept for every case."""
    tried = []
    for _ in range(12):
        side = torch.cuda.Stream()
        tried.append(side)
        c, ahead, _ = _two_op_chain(side, True, PROBE_DELAY_SECONDS)
        if ahead and not torch.equal(c, _chain_result()):
            return side
    return None


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
        assert _same_bits(out, nan.outputs[name]), f"{case.id}: '{name}' differs on a side stream: part of the call left the caller's stream"


BY_ID = {c.id: c for c in CASES}


@pytest.mark.parametrize("case_id,name", REFUSED_ALIGNMENTS, ids=[f"{c}-{n}" for c, n in REFUSED_ALIGNMENTS])
def test_a_weaker_alignment_is_refused(case_id, name):
    """The case's own call with `name` aligned half as well as the entry point demands (16 -> 8, 8 -> 4 bytes): the status comes back
    and no byte of the arena -- buffers, workspace and guards -- changes, under either fill.  Nothing is copied in: a refused call reads
    nothing."""
    from smokephysai_amd import _lib
    lib, case = _lib.load(), BY_ID[case_id]
    bufs = case.buffers(lib)
    (asked,) = [b.align for b in bufs if b.name == name]
    assert asked in (8, 16), (case_id, name, asked)
    bufs = [dataclasses.replace(b, align=asked // 2, phase=None) if b.name == name else b for b in bufs]
    arena = Arena(bufs)
    assert arena.ptr(name) % asked == asked // 2
    for fill in (FILL_NAN, FILL_ZERO):
        arena.fill(fill)
        torch.cuda.synchronize()
        rc = getattr(lib, case.entry)(*case.args(Binder(arena, _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device())))))
        torch.cuda.synchronize()
        assert rc == _lib.SMK_ERR_INVALID, f"{case_id}: '{name}' at {asked // 2}-byte alignment was not refused (status {rc})"
        damage = arena.guard_damage(fill, also=tuple(arena.bufs))
        assert damage == 0, f"{case_id}, refused for '{name}': {damage}"


# ------------------------------------------------------------------------------------------------ controls (torch ops only)
def test_control_a_store_one_word_past_a_buffer_is_reported():
    arena = Arena([Buf("first", torch.float32, 100, align=16), Buf("second", torch.float32, 37, 3, 40), Buf("third", torch.uint8, 10)])
    for fill in (FILL_NAN, FILL_ZERO):
        arena.fill(fill)
        assert arena.guard_damage(fill) == 0
        off, words = arena.span["second"]
        arena.buf[off + words] = 0x3F800000       # one word behind the last plane of 'second'; inside the arena's own allocation
        torch.cuda.synchronize()
        damage = arena.guard_damage(fill)
        assert damage == 1 and damage.first == off + words and damage.buffer == "second", str(damage)
        assert "second" in str(damage) and str(off + words) in str(damage)
        arena.fill(fill)
        arena.view("second")[1, 36] = 1.0         # the last element of a plane: the buffer's own
        assert arena.guard_damage(fill) == 0
        arena.buf[off + 37] = 5                   # the first word of the gap between two planes
        damage = arena.guard_damage(fill)
        assert damage == 1 and damage.first == off + 37 and damage.buffer == "second", str(damage)


def test_control_an_op_on_the_null_stream_changes_the_result():
    side = independent_side_stream()
    assert side is not None, "no side stream runs independently of the null stream here"
    right, ahead, damage = _two_op_chain(side, False, DELAY_SECONDS)
    assert ahead and damage == 0
    assert torch.equal(right, _chain_result())
    wrong, ahead, damage = _two_op_chain(side, True, DELAY_SECONDS)
    assert ahead and damage == 0
    assert not _same_bits(wrong, right)
