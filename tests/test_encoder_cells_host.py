"""The cell rule of the encoder's tile skip (smokephysai_amd/csrc/encoder_cells.h), checked on the host: a stand-alone program
(tests/host/encoder_cells_main.cpp, its own main) includes the header's inlines -- the text the kernels compile -- and applies them to
frames this test writes; numpy applies the rule as the issue states it (a cell is live iff a word != 0x00000000 lies inside the image
within the cell +- 4 pixels).  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "encoder_cells_main.cpp")
INC = os.path.join(ROOT, "smokephysai_amd", "csrc")
N = 256


def cells_live(frames):
    """[B][32][32] bool: cell (row, col) of 8 x 8 pixels has a non-zero word within +- 4 pixels, clipped to the image."""
    bits = np.ascontiguousarray(frames, dtype=np.float32).view(np.uint32) != 0
    B = bits.shape[0]
    padded = np.zeros((B, N + 8, N + 8), bool)
    padded[:, 4:-4, 4:-4] = bits
    out = np.zeros((B, N // 8, N // 8), bool)
    for cy in range(N // 8):
        for cx in range(N // 8):
            out[:, cy, cx] = padded[:, 8 * cy:8 * cy + 16, 8 * cx:8 * cx + 16].any(axis=(1, 2))
    return out


def tiles_live(frames):
    """The tile rule of tests/test_hip_encoder_skip.py: 8 x 16 tile + 4 pixels each way."""
    bits = np.ascontiguousarray(frames, dtype=np.float32).view(np.uint32) != 0
    B = bits.shape[0]
    padded = np.zeros((B, N + 8, N + 8), bool)
    padded[:, 4:-4, 4:-4] = bits
    out = np.zeros((B, N // 8, N // 16), bool)
    for ty in range(N // 8):
        for tx in range(N // 16):
            out[:, ty, tx] = padded[:, 8 * ty:8 * ty + 16, 16 * tx:16 * tx + 24].any(axis=(1, 2))
    return out


def host_frames():
    """Frame 0: the stepper's frame of the golden trajectory.  Then single pixels at every column class of a tile and at the image's
    edges and corners, special values, one zero and one dense frame, and random sparse frames."""
    golden = np.load(os.path.join(ROOT, "tests", "golden", "physics_traj_256_2src_200.npz"))["final_frame_fractal"].astype(np.float32)
    frames = [golden]
    special = np.array([1e-45, -0.0, np.nan, np.inf], np.float32)
    k = 0
    for row in (0, 3, 4, 100, 251, 252, 255):
        for col in list(range(32, 48)) + [0, 3, 4, 11, 12, 243, 244, 251, 252, 255]:
            x = np.zeros((N, N), np.float32)
            x[row, col] = special[k % 4] if k % 3 == 0 else 1.0
            k += 1
            frames.append(x)
    frames.append(np.zeros((N, N), np.float32))
    rng = np.random.RandomState(7)
    frames.append((rng.rand(N, N) * 1.8).astype(np.float32))
    for density in (1e-4, 1e-3, 1e-2):
        frames.append(np.where(rng.rand(N, N) < density, rng.rand(N, N), 0).astype(np.float32))
    return np.stack(frames)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("enccells")
    exe = str(tmp / "encoder_cells")
    base = [cxx, "-O2", "-std=c++17", "-I", INC, SRC, "-o", exe]
    # a plain host executable: undefined-behaviour and address checks where the toolchain has the runtimes, without them otherwise
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    frames = host_frames()
    frames.tofile(tmp / "frames.f32")
    run = subprocess.run([exe, str(tmp / "frames.f32"), str(len(frames)), str(tmp / "cells.u8")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    got = np.fromfile(tmp / "cells.u8", np.uint8).reshape(len(frames), N // 8, N // 16, 2).astype(bool)
    return frames, got, run.stdout


def test_cell_words_equal_the_numpy_rule(host):
    frames, got, out = host
    want = cells_live(frames).reshape(len(frames), N // 8, N // 16, 2)
    assert np.array_equal(got, want)
    assert "BLOCK_RULE_MISMATCHES 0\n" in out            # the scan's 4 x 4 flag blocks give the same bits as the pixel windows
    assert np.array_equal(got.any(axis=3), tiles_live(frames))   # tile live == left or right: the tile counts keep their meaning
    assert "A1_PIXELS_OK" in out


def test_golden_frame_counts(host):
    """The stepper frame of the issue: 44 live tiles, 70 live cells, 18 one-cell tiles."""
    frames, got, _ = host
    g = got[0]
    assert int(g.any(axis=2).sum()) == 44
    assert int(g.sum()) == 70
    assert int((g[..., 0] ^ g[..., 1]).sum()) == 18
    assert abs(float((frames[0] != 0).mean()) - 0.030) < 0.001


def test_work_list_is_two_ascending_segments(host):
    frames, got, out = host
    line = [l for l in out.splitlines() if l.startswith("ENTRIES")][0].split()[1:]
    entries = [tuple(map(int, e.split(":"))) for e in line]
    flat = got.reshape(-1, 2)
    both = [(t, 0) for t in np.flatnonzero(flat[:, 0] & flat[:, 1])]
    one = [(t, 2 if flat[t, 0] else 3) for t in np.flatnonzero(flat[:, 0] ^ flat[:, 1])]
    assert entries == both + one
    assert f"TILES {len(both) + len(one)} BOTH {len(both)} ONE {len(one)}" in out
