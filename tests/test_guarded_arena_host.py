"""tests/guarded_arena.py and the case table of tests/abi_contract_cases.py on the CPU: the arena's layout rules (alignment and phase,
strided planes, uint8 tails, what counts as guard and how damage is reported), and that every case of the table builds its arena and its
ctypes argument list without a device.  The workspace sizes are the library's own answers where the query is a function of the shape
alone (DEVICE_FREE_QUERIES: libsmokehip.so loads and answers them without a GPU); the queries that ask the device for its compute units --
the renders', the metrics', the 2-D and 3-D weight gradients', smk_linear_wgrad's -- are answered by a stub here, and by the library on
the device."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from abi_contract_cases import ENTRY_POINTS, all_cases                                                      # noqa: E402
from guarded_arena import (ALIGNMENTS, FILL_NAN, FILL_ZERO, GUARD, ITEMSIZE, Arena, Binder, Buf, bits, build_arena,        # noqa: E402
                           holds_fill, modulus, weakest)
from smokephysai_amd import _lib                                                                            # noqa: E402

CASES = all_cases()
MIXED = [Buf("w4", torch.float32, 1027), Buf("w8", torch.float64, 3, align=8), Buf("w16", torch.float32, 5, align=16),
         Buf("w256", torch.uint8, 1001, align=256), Buf("even", torch.float32, 9, align=4, phase=8), Buf("i", torch.int32, 7, align=4, phase=12),
         Buf("planes", torch.float32, 37, 3, 40), Buf("bytes", torch.uint8, 10, 2, 13), Buf("empty", torch.float32, 0),
         Buf("halves", torch.bfloat16, 1031, align=8), Buf("half_planes", torch.bfloat16, 5, 3, 8, align=8)]


# the workspace queries of the training step's calls that depend on the shape alone (api.hip: no device_num_cu() behind them)
DEVICE_FREE_QUERIES = ("smk_layernorm_bwd_workspace", "smk_conv3_sigmoid_train_workspace", "smk_convt4s2_train_wgrad_workspace",
                       "smk_bn_train_workspace", "smk_bn_cl_workspace")


class StubLib:
    """Answers the workspace queries: the DEVICE_FREE_QUERIES through the library itself (real=True), every other one with `nbytes`."""

    def __init__(self, nbytes, real=False):
        self.nbytes, self.real, self.asked = nbytes, real, []

    def __getattr__(self, name):
        assert name.endswith("_workspace"), name
        self.asked.append(name)
        if self.real and name in DEVICE_FREE_QUERIES:
            return getattr(_lib.load(), name)
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
    assert arena.view("planes").stride() == (40, 1) and arena.view("bytes").stride() == (13, 1) and arena.view("half_planes").stride() == (8, 1)
    arena.view("halves").fill_(1.5)
    arena.view("half_planes").fill_(-3.0)
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


@pytest.mark.parametrize("fill", [FILL_NAN, FILL_ZERO])
def test_the_tail_and_the_gaps_of_a_bfloat16_buffer_are_guard(fill):
    arena = Arena(MIXED, device="cpu")
    assert arena.ptr("halves") % 16 == 8 and arena.span["halves"][1] == 516             # 1031 halves: 515 words and one half of the 516th
    arena.fill(fill)
    raw = arena.buf.view(torch.int16)
    start = 2 * arena.span["halves"][0]
    raw[start + 1030] = 0x3FC0                                                         # the buffer's last element
    assert arena.guard_damage(fill) == 0
    raw[start + 1031] = 0x3FC0                                                         # the other half of the same word
    damage = arena.guard_damage(fill)
    assert damage == 1 and damage.buffer == "halves" and damage.first == arena.span["halves"][0] + 515
    arena.fill(fill)
    start = 2 * arena.span["half_planes"][0]
    raw[start + 4], raw[start + 8] = 0x3FC0, 0x3FC0                                    # last element of plane 0, first of plane 1
    assert arena.guard_damage(fill) == 0
    raw[start + 5] = 0x3FC0                                                            # the gap between the planes, in the word of plane 0's end
    damage = arena.guard_damage(fill)
    assert damage == 1 and damage.first == arena.span["half_planes"][0] + 2
    assert holds_fill(arena.view("halves"), fill) == 1031 and bits(arena.view("halves")).dtype == torch.int16
    arena.view("halves").fill_(2.0)
    assert holds_fill(arena.view("halves"), fill) == 0


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
    stub = StubLib(4096 + 8, real=True)
    arena = build_arena(case, stub, device="cpu")
    bufs = {b.name: b for b in case.buffers(stub)}
    own = case.query is not None and stub.asked[0] in DEVICE_FREE_QUERIES          # the library's own answer, not the stub's
    assert set(arena.bufs) == set(bufs) and any(b.role in ("out", "inout") for b in bufs.values())
    for name, b in bufs.items():
        assert arena.ptr(name) % modulus(b.align) == (weakest(b.align) if b.phase is None else b.phase), name
        assert arena.span[name][1] == (b.span_bytes + 3) // 4
    if own:
        assert bufs["workspace"].elems == int(case.query(_lib.load())) > 0 and bufs["workspace"].elems % 4 == 0, case.id
        assert arena.span["workspace"][1] == bufs["workspace"].elems // 4                                  # exactly the queried bytes
    elif case.query is not None:
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


def test_the_shape_only_queries_are_the_restated_sizes():
    """The five queries the host can ask, against the sizes include/smokehip.h and the launchers state."""
    L = _lib.load()
    assert L.smk_layernorm_bwd_workspace(256) == 1024 * 2 * 256 * 4 and L.smk_layernorm_bwd_workspace(0) == 0
    assert L.smk_bn_train_workspace(2, 16, 64, 256, 8) == 2 * 16 * 2 * 1 * 4            # one float2 per 16,384-float chunk and channel
    assert L.smk_bn_train_workspace(2, 16, 32, 512, 16) == 2 * 16 * 2 * 2 * 4           # two 8,192-float chunks per plane
    assert L.smk_bn_cl_workspace(1, 1, 8, 16, 64) == 8 * 2 * 64 * 8                     # 128 rows in groups of 16: fp64 pairs per channel
    assert L.smk_bn_cl_workspace(1, 2, 96, 96, 64) == 1024 * 2 * 64 * 8 and L.smk_bn_cl_workspace(1, 1, 8, 16, 96) == -1
    assert L.smk_conv3_sigmoid_train_workspace(2, 16, 64) == (2 * 16 * 64 + 8 * 145) * 4 and L.smk_conv3_sigmoid_train_workspace(1, 8, 16) == 0
    assert L.smk_convt4s2_train_wgrad_workspace(1, 16, 32, 16, 16) == 8 * (16 * 32 * 16 + 32) * 4
    assert L.smk_convt4s2_train_wgrad_workspace(1, 16, 32, 16, 8) == 0                  # an unsupported shape: NULL, 0
    asked = set()
    for case in CASES:
        if case.query is not None:
            stub = StubLib(16, real=True)
            case.buffers(stub)
            asked.update(stub.asked)
    assert set(DEVICE_FREE_QUERIES) <= asked


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
    # the 19 pitch arguments of the training step's calls: each has a case whose pitch is larger than its row
    assert strided["smk_layernorm"] == {"x", "y"} and strided["smk_layernorm_backward"] == {"x", "dy", "dx"}
    assert strided["smk_attention_forward_lse"] == {"q", "k", "v", "out"}
    assert strided["smk_attention_backward"] == {"q", "k", "v", "dout", "dq", "dk", "dv"} and strided["smk_attention_delta"] == {"dout", "out"}
    assert strided["smk_linear_wgrad"] == {"dy", "x"} and strided["smk_chaos_addend"] == {"addend"}
    assert strided["smk_chaos_addend_batched"] == {"addend0", "addend1"} and strided["smk_reduce_shards"] == {"shards"}
    pitches = {}
    for case in CASES:
        pitches.setdefault(case.entry, set()).update((b.name, b.stride - b.elems) for b in case.bufs if b.stride is not None)
    for entry in ("smk_layernorm_backward", "smk_attention_forward_lse", "smk_attention_backward", "smk_attention_delta", "smk_linear_wgrad"):
        pads = [pad for _, pad in pitches[entry]]
        assert len(set(pads)) == len(pads) or entry == "smk_linear_wgrad", (entry, pitches[entry])      # every pitch of a call differs


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
    assert ITEMSIZE[torch.float64] == 8 and ITEMSIZE[torch.bfloat16] == 2
    b = {x.name: x for x in by_id["reduce_shards-w3-f32_bf16-1030"].bufs}
    assert (b["shards"].planes, b["shards"].elems, b["shards"].stride, b["shards"].align) == (3, 1030, 1036, 16)
    assert (b["out"].dtype, b["out"].elems, b["out"].align, b["out"].span_bytes) == (torch.bfloat16, 1030, 8, 2060)
    b = {x.name: x for x in by_id["reduce_shards-w3-bf16_bf16-1030-inplace"].bufs}
    assert list(b) == ["shards"] and b["shards"].role == "inout" and b["shards"].align == 8
    b = {x.name: x for x in by_id["bn_relu_pool_phase-2x16x6x10-pool1-frozen-bwd_dz"].bufs}
    assert b["z"].elems == b["dz"].elems == 2 * 16 * 60 and b["z"].align == b["dz"].align == b["dout"].align == 16 and b["gamma"].align == 4
    b = {x.name: x for x in by_id["chaos_addend_batched-3x256-2layers"].bufs}
    assert (b["addend0"].planes, b["addend0"].stride, b["addend1"].stride) == (15, 257, 259)
    b = {x.name: x for x in by_id["linear_wgrad-512x128x128-db-copying"].bufs}
    assert (b["dy"].stride, b["x"].stride, b["dy"].align, b["x"].align) == (131, 133, 4, 4)
    b = {x.name: x for x in by_id["linear_wgrad-512x1024x512-db"].bufs}
    assert (b["dy"].stride, b["x"].stride, b["dy"].align, b["x"].align) == (1028, 520, 16, 16)
    for cid in ("reduce_shards-w1-f32_f32-4", "reduce_shards-w1-f32_bf16-1028"):            # one shard: the stride argument is larger than n all the same
        args = by_id[cid].args(Binder(build_arena(by_id[cid], StubLib(0), device="cpu"), C.c_void_p(0x1000)))
        assert args[4] == args[3] + 4 and args[2] == 1, (cid, args[2:5])
    b = {x.name: x for x in by_id["linear_wgrad-300x68x96-db"].bufs}
    assert (b["dy"].stride, b["x"].stride, b["dy"].align, b["dw"].align) == (71, 101, 4, 16)
