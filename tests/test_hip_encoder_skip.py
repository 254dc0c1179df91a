"""The encoder's tile skip (csrc/encoder.hip, "tile skip"): tiles whose 16 x 24 input window is all-zero words are filled from the
handle's zero-response table instead of being computed.  Skipping must be invisible in the results -- every comparison here is
bitwise against the direct path (a child process with SMK_ENC_SKIP=0; the switch is read once per process) -- and must actually
happen: after each call smk_encoder_skip_stats has to equal, exactly, the tile count a numpy implementation of the rule gives.

Outputs are handed over as SHA-256 digests of their bytes (the features of one case are up to 21 MB, there are 200 cases): equal
digests = equal bits, which is stricter than torch.equal where an Inf/NaN input puts NaN into the features."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("bf16x3", "bf16", "i8x3")
BATCH = {64: 40, 128: 12, 256: 4}            # 1280 / 1536 / 2048 tiles: more than 3 workgroups on each of 256 CUs (768)


def tiles_with_nonzero_window(frames):
    """The rule, in numpy: flags [B][N/8][N/16], True where any 32-bit word of the tile's window (8 x 16 tile + 4 pixels each way,
    clipped to the image) is not 0x00000000."""
    bits = np.ascontiguousarray(frames, dtype=np.float32).view(np.uint32) != 0
    B, N, _ = bits.shape
    padded = np.zeros((B, N + 8, N + 8), bool)
    padded[:, 4:-4, 4:-4] = bits
    flags = np.zeros((B, N // 8, N // 16), bool)
    for ty in range(N // 8):
        for tx in range(N // 16):
            flags[:, ty, tx] = padded[:, 8 * ty:8 * ty + 16, 16 * tx:16 * tx + 24].any(axis=(1, 2))
    return flags


def simulated_frames(B, N, steps=30, jacobi=20, seed=0):
    import bench
    from smokephysai_amd.physics import SmokeSimulator
    sim = SmokeSimulator((N, N), device="cuda", batch_size=B, jacobi_iters=jacobi)
    sim.ns_solver.add_smoke_sources(bench.draw_sources(B, N, seed))
    frame = torch.empty(B, N, N, device="cuda")
    for _ in range(steps):
        sim.ns_solver.step_into(frame, 1, add_fractal=True, fractal_intensity=0.05)
    return frame


def probe_pixels(N):
    """(row, col) of single pixels around tile (ty, tx) = (2, 1) -- rows 16..23, cols 16..31 -- at distance 4 (inside the window: the tile
    must run) and 5 (outside: it must not) on each side and diagonal, and the same at the image's corner and edge tiles."""
    r0, c0, r1, c1 = 16, 16, 23, 31
    near = [(r0 - 4, c0 + 3), (r1 + 4, c0 + 3), (r0 + 2, c0 - 4), (r0 + 2, c1 + 4),
            (r0 - 4, c0 - 4), (r0 - 4, c1 + 4), (r1 + 4, c0 - 4), (r1 + 4, c1 + 4)]
    far = [(r0 - 5, c0 + 3), (r1 + 5, c0 + 3), (r0 + 2, c0 - 5), (r0 + 2, c1 + 5),
           (r0 - 5, c0 - 5), (r0 - 5, c1 + 5), (r1 + 5, c0 - 5), (r1 + 5, c1 + 5)]
    # corner tile (0, 0) is rows 0..7, cols 0..15: its window ends at row 11 / col 19; the last tile's window starts at N-12 / N-20
    border = [(0, 0), (11, 19), (12, 20), (11, 20), (12, 19), (N - 1, N - 1), (N - 12, N - 20), (N - 13, N - 21), (N - 12, N - 21),
              (0, N - 1), (N - 1, 0), (0, N // 2), (N // 2, 0), (N - 1, N // 2 + 3), (N // 2 + 5, N - 1)]
    return near, far, border


def one_pixel_batch(B, N, pixels, values=(1.0,)):
    x = np.zeros((B, N, N), np.float32)
    for k, (r, c) in enumerate(pixels):
        x[k % B, r, c] = values[k % len(values)]
    return x


def input_cases(N):
    """name -> (frames tensor on the GPU [B][N][N], possibly pitched).  Seeded: the child process builds the same bits."""
    B = BATCH[N]
    rng = np.random.RandomState(1000 + N)
    near, far, border = probe_pixels(N)
    cases = {}
    sim = simulated_frames(B, N)
    cases["simulated"] = sim
    cases["zero"] = torch.zeros(B, N, N, device="cuda")
    cases["dense"] = torch.from_numpy((rng.rand(B, N, N) * 1.8).astype(np.float32)).cuda()
    # one pixel per frame while frames last, so that the probes do not hide each other
    cases["near4"] = torch.from_numpy(one_pixel_batch(B, N, near[:B])).cuda()
    cases["near4b"] = torch.from_numpy(one_pixel_batch(B, N, near[-min(B, 4):])).cuda()
    cases["far5"] = torch.from_numpy(one_pixel_batch(B, N, far[:B])).cuda()
    cases["far5b"] = torch.from_numpy(one_pixel_batch(B, N, far[-min(B, 4):])).cuda()
    for k in range(0, len(border), B):
        cases[f"border{k // B}"] = torch.from_numpy(one_pixel_batch(B, N, border[k:k + B])).cuda()
    special = np.array([1e-45, -0.0, np.nan, np.inf], np.float32)
    assert special.view(np.uint32).tolist() == [1, 0x80000000, 0x7FC00000, 0x7F800000]
    cases["special"] = torch.from_numpy(one_pixel_batch(B, N, [(33, 37), (41, 9), (20, 50), (57, 30)], special)).cuda()
    for pad in (24, 3):              # frame_stride > H*W, gap full of garbage; 24 keeps frames 16-byte aligned, 3 does not
        buf = torch.full((B, N * N + pad), 7.5, device="cuda")
        buf[:, :N * N] = (sim * (torch.arange(B, device="cuda") % 2 == 0)[:, None, None].float()).reshape(B, N * N)
        cases[f"pitched{pad}"] = buf[:, :N * N].view(B, N, N)
        assert cases[f"pitched{pad}"].stride(0) == N * N + pad
    return cases


def run_cases(N, expect_skip):
    """Every (input, dtype, layout) at size N on one handle -> {key: sha256 of the output bytes}; checks the tile counts of each call."""
    from smokephysai_amd.models.encoder import HipEncoder
    w = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests/golden/encoder_weights.npz")).items()}
    enc = HipEncoder(w)
    digests = {}
    for name, x in input_cases(N).items():
        flags = tiles_with_nonzero_window(x.cpu().numpy())
        want = int(flags.sum())
        if name.startswith("near4"):
            assert flags[:, 2, 1].sum() == min(flags.shape[0], 8 if name == "near4" else 4), name      # distance 4 runs the tile
        if name.startswith("far5"):
            assert not flags[:, 2, 1].any(), name                                                      # distance 5 does not
        if name == "special":
            assert want >= 4 and flags.any(axis=(1, 2))[:4].all()                                      # each special value counts
        if name == "dense":
            assert want == flags.size
        for dtype in DTYPES:
            for layout in ("nchw", "tokens"):
                out = enc(x, input_dim=128, dtype=dtype) if layout == "nchw" else enc.tokens(x, input_dim=128, dtype=dtype)
                total, run = enc.skip_stats()
                print(f"N={N} {name} {dtype} {layout}: tiles_run {run} of {total}, rule {want}")
                assert total == flags.size, (name, dtype, layout, total)
                assert run == (want if expect_skip else total), (name, dtype, layout, run, want, total)
                digests[f"{N}/{name}/{dtype}/{layout}"] = hashlib.sha256(out.cpu().numpy().tobytes()).digest()
    return digests


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, "tests")
import test_hip_encoder_skip as T
N = int(sys.argv[2])
d = T.run_cases(N, expect_skip=False)
keys = sorted(d)
np.save(f"{sys.argv[1]}/direct_keys_{N}.npy", np.array(keys))
np.save(f"{sys.argv[1]}/direct_digests_{N}.npy", np.stack([np.frombuffer(d[k], np.uint8) for k in keys]))
print("direct-ok")
'''


@pytest.mark.parametrize("N", [64, 128, 256])
def test_skip_path_equals_direct_path_bitwise(tmp_path, N):
    """bf16x3, bf16, i8x3 x both layouts on simulated, zero, dense, single-pixel (distance 4 / 5, corners, edges; 1e-45, -0.0, NaN,
    Inf) and pitched batches: same bits as the SMK_ENC_SKIP=0 child, and tiles_run == the numpy rule's count on every call (==
    tiles_total for the dense batch and everywhere in the child)."""
    env = dict(os.environ, SMK_ENC_SKIP="0")
    out = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path), str(N)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and "direct-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    keys = [str(k) for k in np.load(tmp_path / f"direct_keys_{N}.npy")]
    direct = dict(zip(keys, np.load(tmp_path / f"direct_digests_{N}.npy")))
    got = run_cases(N, expect_skip=True)
    assert sorted(got) == sorted(direct) and len(got) >= 11 * 6
    bad = [k for k in sorted(got) if got[k] != direct[k].tobytes()]
    assert not bad, f"skip path differs from the direct path in {len(bad)} of {len(got)} cases: {bad[:12]}"


def test_bench_frames_leave_under_a_tenth_of_the_tiles():
    """The bench's configuration (64 grids of 256^2, bench.draw_sources(64, 256, 0), Jacobi-100, fractal 0.05) after 75 steps:
    tiles_run <= 0.10 * tiles_total (the CPU oracle gives 0.0735 and the stepper is bit-exact to it).  A condition on the input."""
    import bench
    from smokephysai_amd.models.encoder import HipEncoder
    frame = simulated_frames(64, 256, steps=75, jacobi=100, seed=0)
    enc = HipEncoder(bench.encoder_weights(0))
    enc.tokens(frame, input_dim=128, dtype="bf16x3")
    total, run = enc.skip_stats()
    want = int(tiles_with_nonzero_window(frame.cpu().numpy()).sum())
    print(f"bench frames after 75 steps: tiles_run {run} of {total} ({run / total:.4f}), rule {want}")
    assert total == 64 * 512 and run == want
    assert run <= 0.10 * total


def test_batch_sizes_change_and_graph_replays_follow_the_input():
    """Two forwards on one handle with different batch sizes (the workspace grows; the first result is reproduced afterwards), then a
    GraphedSmokePhysNet capture and three replays with the input changed between them (zero -> simulated -> dense): each replay equals
    the eager forward bitwise, and the captured forward went through the skip path."""
    from smokephysai_amd.models import GraphedSmokePhysNet, SmokePhysNet
    from smokephysai_amd.models.encoder import HipEncoder
    N = 128
    sim = simulated_frames(16, N)
    w = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests/golden/encoder_weights.npz")).items()}
    enc = HipEncoder(w)
    a8 = enc.tokens(sim[:8], input_dim=128)
    t8 = enc.skip_stats()
    a16 = enc.tokens(sim, input_dim=128)
    t16 = enc.skip_stats()
    assert t8[0] == 8 * 128 and t16[0] == 16 * 128
    assert t8[1] == int(tiles_with_nonzero_window(sim[:8].cpu().numpy()).sum())
    assert t16[1] == int(tiles_with_nonzero_window(sim.cpu().numpy()).sum())
    assert torch.equal(a16[:8], a8) and torch.equal(enc.tokens(sim[:8], input_dim=128), a8)
    assert enc.skip_stats() == t8

    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=64, num_layers=2, num_heads=4, chaos_strength=0.1).cuda().eval()
    graphed = GraphedSmokePhysNet(model, clone=True)
    B = 8
    noise = torch.randn(2, 3, B, 1, device="cuda")
    rng = np.random.RandomState(5)
    inputs = [torch.zeros(B, 1, N, N, device="cuda"), sim[:B, None].contiguous(),
              torch.from_numpy((rng.rand(B, 1, N, N) * 1.8).astype(np.float32)).cuda()]
    with torch.no_grad():
        for i, xin in enumerate(inputs):
            out = graphed(xin, chaos_noise=noise)
            total, run = model.hip_encoder().skip_stats()
            want = int(tiles_with_nonzero_window(xin[:, 0].cpu().numpy()).sum())
            print(f"replay {i}: tiles_run {run} of {total}, rule {want}")
            assert (total, run) == (B * 128, want), i
            ref = model(xin, chaos_noise=noise)
            for k in ref:
                assert torch.equal(ref[k], out[k]), (i, k)
    assert graphed.captures == 1
