"""The guarded arena: one allocation the test owns, holding every buffer of one call of the stateless C ABI (include/smokehip.h) with
guard words before, between and behind them, and run_guarded, which makes that one call.  A plain helper module (imported the way
render_oracle and optical_flow_oracle are); tests/test_hip_decoder.py and tests/test_hip_abi_contract.py use it on the device,
tests/test_guarded_arena_host.py holds the arena itself to its layout rules on the CPU.

What the arena is for.  The header promises, for almost every stateless entry point, "caller-owned memory", "the caller's stream",
"nothing allocated, no synchronisation", "workspace: at least smk_*_workspace(...) bytes", "every element written exactly once" and
"planes *_stride floats apart".  Exactly sized, 16-byte aligned, contiguous torch tensors on the null stream cannot show a breach of any
of them: a store a few words past an output lands in the allocator's slack, a read past an input finds zeros.  Here every byte around a
buffer -- the gaps between strided planes, the tail of a uint8 buffer's last word and everything behind the workspace's stated size
included -- holds a fill word that the test chose, is checked afterwards, and is changed between two runs."""
import contextlib
import ctypes as C
import time
from dataclasses import dataclass
from typing import Optional

import torch

GUARD = 4096                      # words of guard on both sides of every arena buffer
FILL_NAN, FILL_ZERO = -1, 0       # int32 fill words: 0xFFFFFFFF (a NaN as float32; 0xFF bytes) and 0x00000000

ITEMSIZE = {torch.float32: 4, torch.int32: 4, torch.uint8: 1, torch.float64: 8, torch.bfloat16: 2}
ALIGNMENTS = (4, 8, 16, 256)      # bytes


def modulus(align: int) -> int:
    """The modulus a buffer's phase is counted in: 16 bytes for the alignments below 16, 256 bytes from there."""
    return 16 if align < 16 else 256


def weakest(align: int) -> int:
    """The phase that gives a pointer `align`-byte alignment and nothing more: 4 -> 4 (mod 16), 8 -> 8 (mod 16), 16 -> 16 (mod 256),
    256 -> 0."""
    return {4: 4, 8: 8, 16: 16, 256: 0}[align]


@dataclass(frozen=True)
class Buf:
    """One buffer of a call.  `planes` planes of `elems` elements, `stride` elements apart (None: dense); its address is congruent to
    `phase` bytes modulo modulus(align) (phase a multiple of align; None: weakest(align)).  role: "in" (copied in, must come back
    unchanged), "out" (every element written), "inout" (copied in and written), "ws" (a workspace: elems is its size in bytes, dtype
    uint8; 0 bytes means the call passes NULL, 0)."""
    name: str
    dtype: torch.dtype
    elems: int
    planes: int = 1
    stride: Optional[int] = None
    align: int = 4
    phase: Optional[int] = None
    role: str = "in"

    def checked(self):
        assert self.dtype in ITEMSIZE and self.align in ALIGNMENTS and self.role in ("in", "out", "inout", "ws"), self
        item = ITEMSIZE[self.dtype]
        assert self.align % min(item, 4) == 0 and self.align >= min(item, 8), f"{self.name}: {self.dtype} cannot be {self.align}-byte aligned"
        phase = weakest(self.align) if self.phase is None else self.phase
        assert 0 <= phase < modulus(self.align) and phase % self.align == 0, f"{self.name}: phase {phase} of alignment {self.align}"
        assert self.elems >= 0 and self.planes >= 1 and (self.stride is None or self.stride >= self.elems), self
        return phase

    @property
    def pitch(self) -> int:
        return self.elems if self.stride is None else self.stride

    @property
    def span_bytes(self) -> int:
        """From the first byte of plane 0 to the last byte of the last plane."""
        return ((self.planes - 1) * self.pitch + self.elems) * ITEMSIZE[self.dtype]


class GuardDamage(int):
    """The number of damaged guard words (an int: `== 0` is the test), with `first`, the arena word offset of the first one, `buffer`, the
    name of the nearest buffer, and `where`, a sentence for failure messages."""

    def __new__(cls, count, first=None, buffer=None, where="no guard word damaged"):
        self = super().__new__(cls, count)
        self.first, self.buffer, self.where = first, buffer, where
        return self

    def __str__(self):
        return f"{int(self)} damaged guard words; {self.where}"


class Arena:
    """One int32 allocation holding named buffers, at least GUARD words of guard before, between and behind them.  `buffers`: Buf
    entries, or the older (name, float32 elements, phase) triples, where `phase` is the buffer's word offset modulo 4 (0 = 16-byte
    aligned, 2 = 8-byte but not 16-byte aligned, 1 = 4-byte aligned only).  Every buffer occupies whole 32-bit words; bytes of those
    words that are not the buffer's (a uint8 or bfloat16 buffer's tail, the gaps between strided planes) are guard like the words between
    buffers."""

    def __init__(self, buffers, device="cuda"):
        bufs = [b if isinstance(b, Buf) else Buf(b[0], torch.float32, b[1], align=4, phase=4 * (b[2] % 4), role="inout") for b in buffers]
        bufs = [b for b in bufs if not (b.role == "ws" and b.elems == 0)]          # a workspace of 0 bytes: NULL, no place in the arena
        assert len({b.name for b in bufs}) == len(bufs), "buffer names repeat"
        words = [(b.span_bytes + 3) // 4 for b in bufs]
        total = sum(words) + (len(bufs) + 1) * (GUARD + 64) + 64
        self.buf = torch.empty(total, dtype=torch.int32, device=device)
        base = self.buf.data_ptr()
        assert base % 4 == 0
        self.bufs, self.span, cur = {}, {}, 0
        for b, nw in zip(bufs, words):
            phase, mod = b.checked(), modulus(b.align)
            off = cur + GUARD
            off += ((phase - (base + 4 * off)) % mod) // 4
            assert (base + 4 * off) % mod == phase and off + nw + GUARD <= total, b
            self.bufs[b.name], self.span[b.name] = b, (off, nw)
            cur = off + nw
        self.owned = torch.zeros(4 * total, dtype=torch.bool, device=device)       # the bytes that belong to a buffer; all others are guard
        for name in self.bufs:
            self._bytes_of(self.owned, name).fill_(True)

    def _bytes_of(self, flat, name):
        """The bytes of buffer `name` in `flat` (a byte-per-byte tensor over the arena), as a [planes, bytes of a plane] view."""
        b, item = self.bufs[name], ITEMSIZE[self.bufs[name].dtype]
        first = 4 * self.span[name][0]
        return flat[first:first + b.span_bytes].as_strided((b.planes, b.elems * item), (b.pitch * item, 1)) if b.span_bytes else flat[first:first]

    def fill(self, word):
        self.buf.fill_(word)

    def view(self, name):
        """The buffer in its dtype: 1-D for one dense plane, [planes, elems] (rows `stride` apart) otherwise."""
        b = self.bufs[name]
        off, nw = self.span[name]
        typed = self.buf[off:off + nw].view(b.dtype)
        if b.planes == 1 and b.stride is None:
            return typed[:b.elems]
        return typed.as_strided((b.planes, b.elems), (b.pitch, 1))

    def ptr(self, name):
        """The buffer's address; None for a name the arena does not hold (a workspace of 0 bytes)."""
        return self.buf.data_ptr() + 4 * self.span[name][0] if name in self.span else None

    def nearest(self, word_offset):
        """The name of the buffer whose words lie nearest to `word_offset`."""
        def distance(kv):
            off, nw = kv[1]
            return max(off - word_offset, word_offset - (off + nw - 1), 0)
        return min(self.span.items(), key=distance)[0]

    def guard_damage(self, word, also=()) -> GuardDamage:
        """The words with a byte outside every buffer (and inside the buffers named in `also`) that no longer holds the fill: their
        number, with the offset of the first and the nearest buffer's name."""
        guard = ~self.owned
        for name in also:
            self._bytes_of(guard, name).fill_(True)
        pattern = torch.tensor([word], dtype=torch.int32).view(torch.uint8).to(self.buf.device)
        bad = ((self.buf.view(torch.uint8).view(-1, 4) != pattern) & guard.view(-1, 4)).any(dim=1)
        count = int(bad.sum())
        if count == 0:
            return GuardDamage(0)
        first = int(torch.nonzero(bad)[0])
        name = self.nearest(first)
        off, nw = self.span[name]
        rel = f"{off - first} words before its start" if first < off else (f"{first - (off + nw - 1)} words behind its last word" if first >= off + nw
                                                                           else f"word {first - off} of its span (a gap or tail that is not the buffer's)")
        return GuardDamage(count, first, name, f"first at arena word {first}: buffer '{name}', {rel}; now {int(self.buf[first]) & 0xFFFFFFFF:#010x}")


# ------------------------------------------------------------------------------------------------ one guarded call
class Binder:
    """What a case's args() sees of the arena: pointers, strides, the workspace and the stream."""

    def __init__(self, arena, stream):
        self.arena, self.stream = arena, stream

    def ptr(self, name):
        return self.arena.ptr(name)

    def stride(self, name):
        return self.arena.bufs[name].pitch

    def workspace(self, name="workspace"):
        """(pointer, bytes): (None, 0) where the query returned 0."""
        b = self.arena.bufs.get(name)
        return (self.arena.ptr(name), b.elems) if b is not None else (None, 0)


@dataclass
class Run:
    outputs: dict           # name -> clone of every "out" / "inout" buffer, [planes, elems] or 1-D
    inputs: dict            # name -> clone of every "in" buffer after the call
    damage: GuardDamage
    host_seconds: float     # the host time of the ABI call itself
    host_ahead: Optional[bool]      # side stream only: the delay in front of the call was still running when the call returned


def build_arena(case, lib, device="cuda"):
    """The case's arena: its buffers with the workspace sized by the library's own query (exactly that many bytes)."""
    return Arena(case.buffers(lib), device=device)


def run_guarded(case, fill, stream=None, delay_cycles=0) -> Run:
    """Build the arena from the case's buffer list, fill every word with `fill`, copy the inputs in, make the one ABI call through ctypes
    with _lib.stream_ptr, synchronise; return clones of the outputs and the guard damage.  With `stream`: the fill happens on the null
    stream and is waited for; then a delay of `delay_cycles` (torch.cuda._sleep), the copy of the inputs from staging tensors, an event
    and the call are enqueued on `stream`, and host_ahead says whether the event was still pending when the call returned."""
    from smokephysai_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    arena = build_arena(case, lib)
    staging = {k: v.to(dev) for k, v in case.inputs().items()}
    assert set(staging) == {n for n, b in arena.bufs.items() if b.role in ("in", "inout")}, (sorted(staging), sorted(arena.bufs))
    arena.fill(fill)
    torch.cuda.synchronize()
    ahead = None
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        if stream is not None:
            torch.cuda._sleep(int(delay_cycles))
        for name, t in staging.items():
            view = arena.view(name)
            view.copy_(t.reshape(view.shape))
        if stream is not None:
            ev = torch.cuda.Event()
            ev.record()
        fn = getattr(lib, case.entry)
        t0 = time.perf_counter()
        args = case.args(Binder(arena, _lib.stream_ptr(dev)))
        rc = fn(*args)
        host = time.perf_counter() - t0
        if stream is not None:
            ahead = not ev.query()
    torch.cuda.synchronize()
    _lib.check(rc)
    outs = {n: arena.view(n).clone() for n, b in arena.bufs.items() if b.role in ("out", "inout")}
    ins = {n: arena.view(n).clone() for n, b in arena.bufs.items() if b.role == "in"}
    return Run(outs, ins, arena.guard_damage(fill), host, ahead)


def bits(t: torch.Tensor) -> torch.Tensor:
    """A tensor's bits for exact comparison: int32 words for 4-byte types, int64 for float64, int16 for bfloat16, the bytes of uint8."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def holds_fill(t: torch.Tensor, fill: int) -> int:
    """How many elements of an output still hold the fill word (float64: both of its words; bfloat16: its half of one, 0xFFFF being a
    NaN no finite sum rounds to).  uint8 outputs have no recognisable fill -- 0xFF and 0x00 are pixel values -- and answer 0: an unwritten
    byte of theirs differs between the two fills instead."""
    if t.dtype == torch.uint8:
        return 0
    return int((bits(t) == fill).sum())
