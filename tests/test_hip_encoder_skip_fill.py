"""What tests/test_hip_encoder_skip.py cannot see of the encoder's tile skip (csrc/encoder.hip, "tile skip"), now that the main kernels
find their tiles from the band masks themselves and copy the empty tiles' cells:

* every output word is written: the features go into buffers pre-filled with two different sentinel words (HipEncoder's own
  torch.empty buffer usually still holds the previous call's correct features, which hides a tile that is neither run nor filled);
* band counts beyond the other file's 32-80: the headline's 512 and a call of 2,048 bands;
* ranks at the edges of the walk k = blockIdx.x, += gridDim.x: 1, grid - 1, grid, grid + 1 and about half of all tiles non-empty.

The last two compare bitwise (SHA-256 of the bytes) against a child process with SMK_ENC_SKIP=0, in the manner of the other file, and
hold tiles_run to the numpy rule's count on every call."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_encoder_skip import BATCH, DTYPES, simulated_frames, tiles_with_nonzero_window  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINELS = (0xFFFFFFFF, 0x7FC12345)
LAYOUTS = ("nchw", "tokens")


def make_encoder():
    from smokephysai_amd.models.encoder import HipEncoder
    w = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests/golden/encoder_weights.npz")).items()}
    return HipEncoder(w)


def forward_into(enc, x, layout, dtype, word):
    """smk_encoder_forward / smk_encoder_forward_tokens through ctypes on a buffer whose every 32-bit word is `word` -> int32 view."""
    from smokephysai_amd import _lib
    B, H, W = x.shape
    out = torch.full((B * 128 * 1024,), word - (1 << 32) if word >= 1 << 31 else word, dtype=torch.int32, device="cuda")
    fn = enc._L.smk_encoder_forward if layout == "nchw" else enc._L.smk_encoder_forward_tokens
    _lib.check(fn(enc._handle, x.data_ptr(), x.stride(0), B, H, W, 128, out.data_ptr(), _lib.DTYPES[dtype], _lib.stream_ptr(x.device)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N", [64, 128, 256])
def test_every_output_word_is_written(N):
    """Three dtypes x both layouts x (simulated, all-zero, dense) at each size: the results in a 0xFFFFFFFF-filled and in a
    0x7FC12345-filled buffer are bytewise equal to each other and to enc(...) / enc.tokens(...) on the same input."""
    B = BATCH[N]
    rng = np.random.RandomState(2000 + N)
    inputs = {"simulated": simulated_frames(B, N), "zero": torch.zeros(B, N, N, device="cuda"),
              "dense": torch.from_numpy((rng.rand(B, N, N) * 1.8).astype(np.float32)).cuda()}
    enc = make_encoder()
    bad = []
    for name, x in inputs.items():
        for dtype in DTYPES:
            for layout in LAYOUTS:
                a, b = (forward_into(enc, x, layout, dtype, w) for w in SENTINELS)
                ref = enc(x, input_dim=128, dtype=dtype) if layout == "nchw" else enc.tokens(x, input_dim=128, dtype=dtype)
                ref = ref.reshape(-1).view(torch.int32)
                left = [int((a == (s - (1 << 32) if s >= 1 << 31 else s)).sum()) for s in SENTINELS]
                print(f"N={N} {name} {dtype} {layout}: words equal to sentinel 0 in buffer 0: {left[0]}, a==b {torch.equal(a, b)}, a==ref {torch.equal(a, ref)}")
                if not (torch.equal(a, b) and torch.equal(a, ref)):
                    bad.append((name, dtype, layout, int((a != b).sum()), int((a != ref).sum())))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- against the direct path
def grid_size():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def unit_pixels():
    """Isolated pixels of a 64^2 frame and the tiles (ty, tx) each one marks under the rule: rows 1 and 62 (top / bottom four rows of
    the frame) mark one tile, rows 20 and 36 (interior, tile columns 4..11) two vertically adjacent ones.  All 24 tiles are distinct."""
    units = []
    for tx in range(4):
        c = 16 * tx + 8
        units += [((1, c), [(0, tx)]), ((62, c), [(7, tx)]), ((20, c), [(2, tx), (3, tx)]), ((36, c), [(4, tx), (5, tx)])]
    return units


def frames_with_tiles(B, want, seed):
    """[B][64][64] of isolated pixels with exactly `want` non-empty tiles (seeded choice of frames and positions)."""
    rng = np.random.RandomState(seed)
    units = unit_pixels()
    order = [(b, u) for b in range(B) for u in range(len(units))]
    rng.shuffle(order)
    x = np.zeros((B, 64, 64), np.float32)
    left = want
    for b, u in order:
        (r, c), tiles = units[u]
        if len(tiles) <= left:
            x[b, r, c] = rng.uniform(0.25, 2.0)
            left -= len(tiles)
        if left == 0:
            break
    assert left == 0, (B, want)
    return x


def edge_cases():
    G = grid_size()
    B = max(40, (G + 2 + 23) // 24 + 1)                      # 32 B tiles > G (skip path), 24 B markable tiles >= G + 1
    cases = {}
    last = np.zeros((B, 64, 64), np.float32)
    last[B - 1, 62, 56] = 1.0
    cases["one_last"] = (last, 1)
    for name, want in (("grid-1", G - 1), ("grid", G), ("grid+1", G + 1), ("half", 16 * B)):
        cases[name] = (frames_with_tiles(B, want, 3000 + want), want)
    return cases


def band_cases(which):
    if which == "bands512":                                   # the headline: 64 frames of 256^2 = 512 bands of 64 tiles
        x = simulated_frames(64, 256)
        return {"bands512": (x, None)}
    rng = np.random.RandomState(4000)                         # 1,024 frames of 64^2 = 2,048 bands of 16 tiles, about half of the tiles run
    x = np.where(rng.rand(1024, 64, 64) < 0.0018, rng.uniform(0.25, 2.0, (1024, 64, 64)), 0.0).astype(np.float32)
    return {"bands2048": (x, None)}


BIG_COMBOS = (("bf16x3", "nchw"), ("bf16x3", "tokens"), ("bf16", "nchw"), ("i8x3", "tokens"))


def run_cases(which, expect_skip):
    enc = make_encoder()
    cases = edge_cases() if which == "edges" else band_cases(which)
    combos = BIG_COMBOS if which == "bands2048" else [(d, l) for d in DTYPES for l in LAYOUTS]
    digests = {}
    for name, (x, want) in cases.items():
        xn = x.cpu().numpy() if torch.is_tensor(x) else x
        flags = tiles_with_nonzero_window(xn)
        if want is not None:                                  # the case is what it claims, on any CU count, before anything is launched
            assert int(flags.sum()) == want, (name, int(flags.sum()), want)
        if name == "one_last":
            assert flags[-1, -1, -1] and flags.sum() == 1
        want = int(flags.sum())
        if which == "bands2048":
            assert flags.size == 2048 * 16 and want > 16 * grid_size() and want < flags.size
        xg = x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
        for dtype, layout in combos:
            out = enc(xg, input_dim=128, dtype=dtype) if layout == "nchw" else enc.tokens(xg, input_dim=128, dtype=dtype)
            total, run = enc.skip_stats()
            print(f"{which} {name} {dtype} {layout}: tiles_run {run} of {total}, rule {want}")
            assert total == flags.size, (name, dtype, layout, total)
            assert run == (want if expect_skip else total), (name, dtype, layout, run, want, total)
            digests[f"{name}/{dtype}/{layout}"] = hashlib.sha256(out.cpu().numpy().tobytes()).digest()
            del out
    return digests


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, "tests")
import test_hip_encoder_skip_fill as T
d = T.run_cases(sys.argv[2], expect_skip=False)
keys = sorted(d)
np.save(f"{sys.argv[1]}/keys.npy", np.array(keys))
np.save(f"{sys.argv[1]}/digests.npy", np.stack([np.frombuffer(d[k], np.uint8) for k in keys]))
print("direct-ok")
'''


def against_direct_path(tmp_path, which, ncases):
    env = dict(os.environ, SMK_ENC_SKIP="0")
    out = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path), which], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and "direct-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    direct = dict(zip([str(k) for k in np.load(tmp_path / "keys.npy")], np.load(tmp_path / "digests.npy")))
    got = run_cases(which, expect_skip=True)
    assert sorted(got) == sorted(direct) and len(got) == ncases
    bad = [k for k in sorted(got) if got[k] != direct[k].tobytes()]
    assert not bad, f"skip path differs from the direct path in {len(bad)} of {len(got)} cases: {bad}"


def test_headline_band_count_equals_direct_path_bitwise(tmp_path):
    """64 simulated frames of 256^2: 512 bands (two per chunk of the in-kernel sums), three dtypes x both layouts."""
    against_direct_path(tmp_path, "bands512", 6)


def test_band_count_beyond_the_lookup_structures_equals_direct_path_bitwise(tmp_path):
    """1,024 frames of 64^2 = 2,048 bands and 32,768 tiles, about half of them non-empty.  That is more bands than the
    SKIP_CHUNKS = 256 chunk sums a workgroup keeps in LDS (8 bands per chunk: the walk inside a chunk runs), and more rounds per
    workgroup (> 16 on a grid of 2 x CUs, asserted) than the SKIP_SLATE = 16 looked-up tiles it holds at a time (the slate is
    refilled inside the tile loop).  bf16x3 in both layouts, bf16 NCHW, i8x3 tokens."""
    against_direct_path(tmp_path, "bands2048", 4)


def test_ranks_at_the_edges_of_the_walk_equal_direct_path_bitwise(tmp_path):
    """Isolated-pixel batches of 64^2 frames whose number of non-empty tiles is 1 (the call's very last tile), grid - 1, grid,
    grid + 1 and half of all tiles, grid = 2 x CUs; the counts are asserted with the numpy rule before any launch."""
    against_direct_path(tmp_path, "edges", 5 * 6)


def test_isolated_pixels_mark_the_tiles_the_cases_rely_on():
    """Pixel (62, 56) of a 64^2 frame marks tile (7, 3) alone, (20, 24) marks (2, 1) and (3, 1); every unit of unit_pixels() marks
    exactly the tiles it lists.  (Needs no device; kept beside the cases it guards.)"""
    for (r, c), tiles in [((62, 56), [(7, 3)]), ((20, 24), [(2, 1), (3, 1)])] + unit_pixels():
        x = np.zeros((1, 64, 64), np.float32)
        x[0, r, c] = 1.0
        assert sorted(zip(*np.nonzero(tiles_with_nonzero_window(x)[0]))) == sorted(tiles), (r, c)
