"""tests/guarded_arena.py and the case table of tests/abi_contract_cases.py on the CPU: the arena's layout rules (alignment and phase,
strided planes, uint8 tails, what counts as guard and how damage is reported), and that every case of the table builds its arena and its
ctypes argument list without a device.  The workspace sizes come from a stub here; on the device they are the library's own answers."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from abi_contract_cases import ENTRY_POINTS, all_cases                                                      # noqa: E402
from guarded_arena import (ALIGNMENTS, FILL_NAN, FILL_ZERO, GUARD, ITEMSIZE, Arena, Binder, Buf, build_arena, modulus,      # noqa: E402
                           weakest)
from smokephysai_amd import _lib                                                                            # noqa: E402

CASES = all_cases()
MIXED = [Buf("w4", torch.float32, 1027), Buf("w8", torch.float64, 3, align=8), Buf("w16", torch.float32, 5, align=16),
         Buf("w256", torch.uint8, 1001, align=256), Buf("even", torch.float32, 9, align=4, phase=8), Buf("i", torch.int32, 7, align=4, phase=12),
         Buf("planes", torch.float32, 37, 3, 40), Buf("bytes", torch.uint8, 10, 2, 13), Buf("empty", torch.float32, 0)]


class StubLib:
    """Answers every workspace query with `nbytes`."""

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def __getattr__(self, name):
        assert name.endswith("_workspace"), name
        return lambda *args: self.nbytes


def test_alignment_and_phase_of_every_buffer():
    arena = Arena(MIXED, device="cpu")
    for b in MIXED:
        addr, phase = arena.ptr(b.name), weakest(b.align) if b.phase is None else b.phase
        assert addr % modulus(b.align) == phase, (b.name, addr % 256)
        assert addr % b.align == 0
    assert arena.ptr("w4") % 16 == 4 and arena.ptr("w8") % 16 == 8                   # 4-byte but not 8-byte, 8-byte but not 16-byte aligned
    assert arena.ptr("w16") % 32 == 16 and arena.ptr("w256") % 256 == 0
    assert arena.ptr("missing") is None
    order = sorted(arena.span.values())
    assert order[0][0] >= GUARD and order[-1][0] + order[-1][1] + GUARD <= arena.buf.numel()
    for (off0, n0), (off1, _) in zip(order, order[1:]):
        assert off1 - (off0 + n0) >= GUARD


def test_the_older_triples_keep_their_meaning():
    arena = Arena([("a", 100, 0), ("b", 7, 2), ("c", 5, 1)], device="cpu")
    assert [arena.ptr(k) % 16 for k in "abc"] == [0, 8, 4]
    assert arena.view("b").dtype == torch.float32 and arena.view("b").shape == (7,)
    arena.fill(FILL_NAN)
    assert arena.guard_damage(FILL_NAN) == 0 and int(arena.guard_damage(FILL_NAN, also=("b",))) == 0
    arena.view("b")[3] = 1.0
    assert arena.guard_damage(FILL_NAN) == 0
    damage = arena.guard_damage(FILL_NAN, also=("b",))
    assert damage == 1 and damage.buffer == "b" and damage.first == arena.span["b"][0] + 3


def test_views_have_the_buffers_types_and_strides():
    arena = Arena(MIXED, device="cpu")
    arena.fill(FILL_ZERO)
    for b in MIXED:
        v = arena.view(b.name)
        assert v.dtype == b.dtype and v.data_ptr() == arena.ptr(b.name) or b.elems == 0
        assert tuple(v.shape) == ((b.elems,) if b.planes == 1 and b.stride is None else (b.planes, b.elems))
    assert arena.view("planes").stride() == (40, 1) and arena.view("bytes").stride() == (13, 1)
    arena.view("planes").fill_(1.0)
    arena.view("bytes").fill_(7)
    arena.view("w8").fill_(-2.5)
    assert arena.guard_damage(FILL_ZERO) == 0                                      # a buffer's own bytes are not guard
    words = arena.buf[arena.span["planes"][0]:][:3 * 40]
    assert int((words != 0).sum()) == 3 * 37 and int(words[37]) == 0 and int(words[40]) != 0


@pytest.mark.parametrize("fill", [FILL_NAN, FILL_ZERO])
def test_guard_damage_names_the_first_damaged_word(fill):
    arena = Arena(MIXED, device="cpu")
    first = min(arena.span.items(), key=lambda kv: kv[1][0])[0]
    last = max(arena.span.items(), key=lambda kv: kv[1][0])[0]
    off_p, _ = arena.span["planes"]
    off_b, n_b = arena.span["w8"]
    spots = {"before the first buffer": (arena.span[first][0] - 1, first),
             "in a stride gap": (off_p + 38, "planes"),
             "between two buffers": (off_b + n_b + 2, "w8"),
             "after the last buffer": (arena.buf.numel() - 1, last)}
    for what, (word, name) in spots.items():
        arena.fill(fill)
        assert arena.guard_damage(fill) == 0
        arena.buf[word] = 0x12345678
        damage = arena.guard_damage(fill)
        assert damage == 1 and damage.first == word and damage.buffer == name, (what, str(damage))
        assert f"arena word {word}" in str(damage) and f"'{name}'" in str(damage), (what, str(damage))
    arena.fill(fill)
    arena.buf[5], arena.buf[off_p + 39] = 1, 2
    damage = arena.guard_damage(fill)
    assert damage == 2 and damage.first == 5


@pytest.mark.parametrize("fill", [FILL_NAN, FILL_ZERO])
def test_the_tail_bytes_of_a_uint8_buffer_are_guard(fill):
    arena = Arena(MIXED, device="cpu")
    arena.fill(fill)
    raw = arena.buf.view(torch.uint8)
    start = 4 * arena.span["w256"][0]
    raw[start + 1000] = 0x5A                                                           # the buffer's last byte
    assert arena.guard_damage(fill) == 0
    raw[start + 1001] = 0x5A                                                           # the next byte of the same word
    damage = arena.guard_damage(fill)
    assert damage == 1 and damage.buffer == "w256" and damage.first == arena.span["w256"][0] + 250
    arena.fill(fill)
    start = 4 * arena.span["bytes"][0]
    raw[start + 9], raw[start + 13] = 0x5A, 0x5A                                      # last byte of plane 0, first of plane 1
    assert arena.guard_damage(fill) == 0
    raw[start + 10] = 0x5A                                                             # the gap between the planes, byte-granular
    assert arena.guard_damage(fill) == 1


def test_wrong_requests_are_refused():
    for bad in (Buf("x", torch.float64, 2, align=4), Buf("x", torch.float32, 2, align=4, phase=2), Buf("x", torch.float32, 2, align=16, phase=8),
                Buf("x", torch.float32, 8, 2, 7), Buf("x", torch.float32, 2, align=32)):
        with pytest.raises(AssertionError):
            Arena([bad], device="cpu")
    with pytest.raises(AssertionError):
        Arena([("a", 4, 0), ("a", 4, 0)], device="cpu")
    assert set(ALIGNMENTS) == {4, 8, 16, 256}


def test_the_table_has_every_entry_point_of_the_issue():
    assert {c.entry for c in CASES} == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert name in _lib._SIGNATURES, name


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_case_builds_its_arena_and_arguments_without_a_device(case):
    stub = StubLib(4096 + 8)
    arena = build_arena(case, stub, device="cpu")
    bufs = {b.name: b for b in case.buffers(stub)}
    assert set(arena.bufs) == set(bufs) and any(b.role in ("out", "inout") for b in bufs.values())
    for name, b in bufs.items():
        assert arena.ptr(name) % modulus(b.align) == (weakest(b.align) if b.phase is None else b.phase), name
        assert arena.span[name][1] == (b.span_bytes + 3) // 4
    if case.query is not None:
        assert bufs["workspace"].elems == 4096 + 8 and arena.span["workspace"][1] == (4096 + 8) // 4      # exactly the queried bytes
    stream = C.c_void_p(0x1000)
    args = case.args(Binder(arena, stream))
    argtypes = _lib._SIGNATURES[case.entry]
    assert len(args) == len(argtypes), (len(args), len(argtypes))
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + 4 * arena.buf.numel()
    for a, t in zip(args, argtypes):
        t.from_param(a)                                                                # ctypes takes it as this parameter
        if t is C.c_void_p and isinstance(a, int):
            assert lo <= a < hi                                                        # every device pointer lies in the arena
    assert args[-1] is stream
    if case.query is not None:                                                         # a query that returns 0: NULL, 0
        empty = build_arena(case, StubLib(0), device="cpu")
        assert "workspace" not in empty.bufs and Binder(empty, stream).workspace() == (None, 0)
        case.args(Binder(empty, stream))


def test_every_stride_of_the_table_is_larger_than_its_plane():
    strided = {}
    for case in CASES:
        for b in case.bufs:
            if b.stride is not None:
                assert b.stride > b.elems and b.planes > 1, (case.id, b)
                strided.setdefault(case.entry, set()).add(b.name)
    assert strided["smk_volume_render"] == {"vols", "image", "trans"}
    assert strided["smk_volume_render_backward"] == {"vols", "grad_image", "grad_trans", "grad_vols"}
    assert strided["smk_volume_render_orbit"] == strided["smk_volume_render_camera"] == {"vols", "image", "trans"}
    assert strided["smk_image_quality"] == {"pred", "target"} and strided["smk_image_quality_backward"] == {"pred", "target", "dpred"}
    assert strided["smk_chaos_stats"] == strided["smk_frame_diff_norms"] == {"frames"} and strided["smk_volume_stats"] == {"vols"}


def test_sizes_come_from_the_shapes():
    by_id = {c.id: c for c in CASES}
    b = {x.name: x for x in by_id["render_backward-5x37x70-+y"].bufs}
    assert (b["vols"].elems, b["vols"].stride, b["grad_vols"].stride, b["grad_image"].stride, b["grad_trans"].stride) == \
        (5 * 37 * 70, 5 * 37 * 70 + 3, 5 * 37 * 70 + 5, 37 * 70 + 1, 37 * 70 + 2)
    b = {x.name: x for x in by_id["render_camera-17x16x65-none"].bufs}
    assert b["image"].planes == 4 and b["image"].elems == 16 * 65
    b = {x.name: x for x in by_id["flow_farneback-64x96"].bufs}
    assert b["prev"].dtype == torch.uint8 and b["prev"].elems == 3 * 64 * 96 and b["flow"].elems == 3 * 64 * 96 * 2
    b = {x.name: x for x in by_id["adamw_step-keep_grad"].bufs}
    assert [b[f"param{i}"].elems for i in range(6)] == [1, 3, 5, 1027, 8193, 0]
    assert all(b[f"{f}3"].align == 4 for f in ("param", "grad", "exp_avg", "exp_avg_sq"))
    assert [b[f"{f}4"].align for f in ("param", "grad", "exp_avg", "exp_avg_sq")] == [16, 16, 4, 16]
    assert ITEMSIZE[torch.float64] == 8
