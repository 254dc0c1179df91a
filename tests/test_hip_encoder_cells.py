"""The encoder's tile skip per pooled cell (csrc/encoder.hip, "per pooled cell"; csrc/encoder_cells.h): at 256^2 a tile whose left or
right 8 x 8 cell has an all-zero 16 x 16 window runs a body of half the size, and the work list is two segments (two-cell tiles, then
one-cell tiles).  None of it may show in the results.  Batches of 2 and 3 frames of 256^2 (1,024 and 1,536 tiles: more than the 512
workgroups of a 256-CU device, so the list path engages), bf16x3, token-major and planar; every case is compared bitwise against

* a child process with SMK_ENC_CELLS=0 (whole tiles from the same list),
* a child process with SMK_ENC_SKIP=0 (every tile runs), and
* itself in two buffers pre-filled with different sentinel words (every word is written),

and tiles_run has to equal the numpy tile rule's count on every call.  The children run every case once (module fixture)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_encoder_cells_host import cells_live, tiles_live  # noqa: E402
from test_hip_encoder_skip import simulated_frames  # noqa: E402
from test_hip_encoder_skip_fill import SENTINELS, forward_into, make_encoder  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 256
LAYOUTS = ("tokens", "nchw")
SPECIAL = np.array([1e-45, -0.0, np.nan, np.inf], np.float32)
LISTS = [(two, one) for two in (0, 600) for one in (0, 1, 511, 512, 513)]


def counts(x):
    """(live tiles, two-cell tiles, one-cell tiles) of frames [B][256][256] by the numpy rule."""
    c = cells_live(x).reshape(len(x), N // 8, N // 16, 2)
    return int(c.any(axis=3).sum()), int((c[..., 0] & c[..., 1]).sum()), int((c[..., 0] ^ c[..., 1]).sum())


def list_frames(two, one):
    """3 frames of isolated pixels with exactly `two` two-cell tiles and `one` one-cell tiles.  A pixel at row 16 q + 9 marks tile rows
    2q and 2q + 1 and no other; at row 1 tile row 0 alone.  Column 16 tx + 6 marks both cells of tile column tx alone; column 16 tx + 1
    marks the left cell of tx and the right cell of tx - 1 (4 one-cell tiles per pixel; 2 at tx = 0, 1 at tx = 0 and row 1).  Two-cell
    pixels go to tile columns 6 .. 15, one-cell pixels to 0 .. 5, the last pair rows of the walk (q = 0) stay free for the small units."""
    x = np.zeros((3, N, N), np.float32)
    assert two % 2 == 0
    slots = [(b, q, tx) for q in range(15, -1, -1) for b in range(3) for tx in range(6, 16)]
    for b, q, tx in slots[:two // 2]:
        x[b, 16 * q + 9, 16 * tx + 6] = 1.0 + 0.001 * tx
    fours, rest = divmod(one, 4)
    slots = [(b, q, tx) for q in range(15, 0, -1) for b in range(3) for tx in (1, 3, 5)]
    assert fours <= len(slots)
    for b, q, tx in slots[:fours]:
        x[b, 16 * q + 9, 16 * tx + 1] = 0.5 + 0.001 * q
    if rest & 2:
        x[0, 9, 1] = 0.75                                      # tile rows 0, 1 of tile column 0: left cells
    if rest & 1:
        x[1, 1, 1] = 1.25                                      # tile (0, 0): left cell
    return x


def pixel_cases():
    """Single non-zero pixels, one per frame: every column class of an interior tile (c0 + 0..3 left only, c0 + 4..11 both,
    c0 + 12..15 right only), and rows x columns 0 / 3 / 4 / 251 / 252 / 255 (the corners among them); values cycle through 1.0 and the
    special words 1e-45, -0.0, NaN, Inf."""
    pixels = [(100, 80 + c) for c in range(16)] + [(r, c) for r in (0, 3, 4, 251, 252, 255) for c in (0, 3, 4, 251, 252, 255)]
    values = [1.0] + list(SPECIAL)
    cases = {}
    for k in range(0, len(pixels), 3):
        x = np.zeros((3, N, N), np.float32)
        for i, (r, c) in enumerate(pixels[k:k + 3]):
            x[i, r, c] = values[(k + i) % 5]
        if k + 3 > len(pixels):
            x = x[:len(pixels) - k + 1]                       # a batch of 2: one pixel frame and one zero frame
        cases[f"pixels{k // 3}"] = x
    return cases


def host_cases():
    rng = np.random.RandomState(256)
    cases = {"zero2": np.zeros((2, N, N), np.float32), "dense3": (rng.rand(3, N, N) * 1.8).astype(np.float32)}
    cases.update(pixel_cases())
    special = np.zeros((2, N, N), np.float32)
    for i, (r, c) in enumerate([(33, 33), (41, 78), (120, 13), (200, 255), (255, 129), (77, 200), (8, 131), (150, 150)]):
        special[i % 2, r, c] = SPECIAL[i % 4]
    cases["special"] = special
    for two, one in LISTS:
        cases[f"list{two}+{one}"] = list_frames(two, one)
    return cases


def device_cases():
    cases = {k: torch.from_numpy(v).cuda() for k, v in host_cases().items()}
    sim = simulated_frames(3, N, steps=30)
    cases["stepper3"] = sim
    cases["stepper2"] = sim[1:].contiguous()
    buf = torch.full((3, N * N + 24), 7.5, device="cuda")      # frame_stride > H * W, the gap full of garbage
    buf[:, :N * N] = (sim * torch.tensor([1.0, 0.0, 1.0], device="cuda")[:, None, None]).reshape(3, N * N)
    cases["pitched"] = buf[:, :N * N].view(3, N, N)
    assert cases["pitched"].stride(0) == N * N + 24
    return cases


def run_cases(expect_skip):
    """Every case x layout on one handle, into sentinel-filled buffers -> {key: sha256 of the output bytes}.  Checks the tile counts of
    each call and that the two sentinel runs agree."""
    enc = make_encoder()
    digests = {}
    for name, x in device_cases().items():
        want = int(tiles_live(x.cpu().numpy()).sum())
        for layout in LAYOUTS:
            a = forward_into(enc, x, layout, "bf16x3", SENTINELS[0])
            total, run = enc.skip_stats()
            b = forward_into(enc, x, layout, "bf16x3", SENTINELS[1])
            print(f"{name} {layout}: tiles_run {run} of {total}, rule {want}, cells (live, two, one) {counts(x.cpu().numpy())}")
            assert total == len(x) * 512 and total > 2 * torch.cuda.get_device_properties(0).multi_processor_count
            assert run == (want if expect_skip else total), (name, layout, run, want, total)
            assert torch.equal(a, b), (name, layout, int((a != b).sum()))      # a word left unwritten keeps its sentinel in one of them
            digests[f"{name}/{layout}"] = hashlib.sha256(a.cpu().numpy().tobytes()).digest()
    return digests


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, "tests")
import test_hip_encoder_cells as T
d = T.run_cases(expect_skip=sys.argv[2] == "skip")
keys = sorted(d)
np.save(f"{sys.argv[1]}/keys.npy", np.array(keys))
np.save(f"{sys.argv[1]}/digests.npy", np.stack([np.frombuffer(d[k], np.uint8) for k in keys]))
print("child-ok")
'''


def child(tmp, env, expect):
    tmp.mkdir()
    out = subprocess.run([sys.executable, "-c", CHILD, str(tmp), expect], cwd=ROOT, env=dict(os.environ, **env), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "child-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    return dict(zip([str(k) for k in np.load(tmp / "keys.npy")], [d.tobytes() for d in np.load(tmp / "digests.npy")]))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cells")
    return {"cells": run_cases(expect_skip=True),
            "whole_tiles": child(tmp / "whole", {"SMK_ENC_CELLS": "0"}, "skip"),
            "direct": child(tmp / "direct", {"SMK_ENC_SKIP": "0"}, "direct")}


def test_cases_are_what_they_claim():
    """The lists hold exactly the two-cell and one-cell tile counts they name; the column classes of a pixel mark the cells the issue
    lists (and the neighbour tile's facing cell); the stepper frames have one-cell tiles."""
    for two, one in LISTS:
        live, n2, n1 = counts(list_frames(two, one))
        assert (live, n2, n1) == (two + one, two, one)
    for c in range(16):
        x = np.zeros((1, N, N), np.float32)
        x[0, 100, 80 + c] = 1.0
        cl = cells_live(x)[0, 12]                            # cell row of pixel row 100; tile column 5 = cells 10, 11
        want = {10} if c < 4 else {10, 11} if c < 12 else {11}
        want |= {9} if c < 4 else {12} if c >= 12 else set()   # the neighbour tile's facing cell
        assert set(np.flatnonzero(cl)) == want, c
    live, n2, n1 = counts(simulated_frames(3, N, steps=30).cpu().numpy())
    assert n1 > 0 and n2 > 0 and live < 3 * 512


@pytest.mark.parametrize("reference", ["whole_tiles", "direct"])
def test_cells_equal_reference_bitwise(results, reference):
    got, ref = results["cells"], results[reference]
    assert sorted(got) == sorted(ref) and len(got) == 2 * (2 + 18 + 1 + len(LISTS) + 3)
    bad = [k for k in sorted(got) if got[k] != ref[k]]
    assert not bad, f"the cell path differs from {reference} in {len(bad)} of {len(got)} cases: {bad[:12]}"
