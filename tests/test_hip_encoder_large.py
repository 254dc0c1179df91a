"""The fused encoder on frames beyond 256^2 (csrc/encoder.hip, "frames beyond 256^2"): at 512^2 and 1024^2 a pooled cell spans 2 and 8 of
the kernels' 8 x 16 tiles, so the main kernels write per-tile partial sums and k_encoder_pool_partials adds them.

Shapes are the smallest that reach every new branch: 512^2 with B = 2 (4,096 tiles: several rounds of the persistent walk) and
1024^2 with B = 1.  The reference is torch on the CPU in fp64 (conv2d / batch_norm / relu / the two adaptive_avg_pool2d) with the
random weights of test_hip_encoder.test_vs_oracle_random_weights_and_batch; it agrees with oracle.encoder_features to 6.5e-8, which
takes 47 s (512^2) and 171 s (1024^2) per frame and is therefore not used here.  The bars are conftest.rel_err < 2e-5 (f32), 1e-4
(bf16x3, i8x3) and 2e-2 (bf16), the project's own.

Skip-path comparisons are bitwise (SHA-256 of the bytes) against one child process per size with SMK_ENC_SKIP=0 (the switch is read
once per process), and smk_encoder_skip_stats has to equal the numpy rule's count exactly."""
import hashlib
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err  # noqa: E402
from test_hip_encoder_skip import simulated_frames, tiles_with_nonzero_window  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (512, 1024)
PARITY_BATCH = {512: 2, 1024: 1}
SKIP_BATCH = {512: 4, 1024: 2}               # 8,192 / 16,384 tiles: well beyond the 768 resident workgroups
MFMA_DTYPES = ("bf16x3", "bf16", "i8x3")
BARS = {"f32": 2e-5, "bf16x3": 1e-4, "i8x3": 1e-4, "bf16": 2e-2}


def random_weights():
    rng = np.random.RandomState(0)
    w = dict(conv1_w=rng.randn(64, 1, 7, 7) * 0.2, conv1_b=rng.randn(64) * 0.1, bn1_w=rng.rand(64) + 0.5,
             bn1_b=rng.randn(64) * 0.1, bn1_mean=rng.randn(64) * 0.2, bn1_var=rng.rand(64) + 0.3,
             conv2_w=rng.randn(128, 64, 3, 3) * 0.05, conv2_b=rng.randn(128) * 0.1, bn2_w=rng.rand(128) + 0.5,
             bn2_b=rng.randn(128) * 0.1, bn2_mean=rng.randn(128) * 0.2, bn2_var=rng.rand(128) + 0.3)
    return {k: v.astype(np.float32) for k, v in w.items()}


def torch_reference(frames, w, input_dims=(128,)):
    """fp64 on the CPU, frame by frame: {input_dim: [B,128,32,32]}."""
    t = {k: torch.from_numpy(v).double() for k, v in w.items()}
    out = {d: [] for d in input_dims}
    for f in np.asarray(frames):
        x = torch.from_numpy(f).double()[None, None]
        a = F.relu(F.batch_norm(F.conv2d(x, t["conv1_w"], t["conv1_b"], padding=3), t["bn1_mean"], t["bn1_var"], t["bn1_w"], t["bn1_b"],
                                False, 0.0, 1e-5))
        a = F.relu(F.batch_norm(F.conv2d(a, t["conv2_w"], t["conv2_b"], padding=1), t["bn2_mean"], t["bn2_var"], t["bn2_w"], t["bn2_b"],
                                False, 0.0, 1e-5))
        for d in input_dims:
            out[d].append(F.adaptive_avg_pool2d(F.adaptive_avg_pool2d(a, d), 32)[0].numpy())
    return {d: np.stack(v) for d, v in out.items()}


def make_encoder(w=None):
    from smokephysai_amd.models.encoder import HipEncoder
    return HipEncoder({k: torch.from_numpy(v) for k, v in (w or random_weights()).items()})


@pytest.fixture(scope="module")
def parity():
    """Dense U(0, 1.8) frames of both sizes and their references, computed once."""
    w = random_weights()
    data = {}
    for N in SIZES:
        rng = np.random.RandomState(3000 + N)
        frames = (rng.rand(PARITY_BATCH[N], N, N) * 1.8).astype(np.float32)
        data[N] = (frames, torch_reference(frames, w, (128, 32) if N == 512 else (128,)))
    return w, data


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "i8x3", "bf16"])
def test_parity_with_the_fp64_reference(parity, N, dtype):
    w, data = parity
    frames, ref = data[N]
    enc = make_encoder(w)
    got = enc(torch.from_numpy(frames).cuda(), input_dim=128, dtype=dtype).cpu().numpy()
    errs = [rel_err(got[b], ref[128][b]) for b in range(len(frames))] + [rel_err(got, ref[128])]
    print(f"{N}^2 {dtype}: rel err per frame and over the batch {errs}")
    assert max(errs) < BARS[dtype]
    if N == 512 and dtype == "bf16x3":
        got32 = enc(torch.from_numpy(frames).cuda(), input_dim=32, dtype=dtype).cpu().numpy()
        errs32 = [rel_err(got32[b], ref[32][b]) for b in range(len(frames))] + [rel_err(got32, ref[32])]
        print(f"512^2 bf16x3 input_dim=32: {errs32}")
        assert max(errs32) < BARS[dtype]


def test_bf16x3_on_the_32x32x16_shape(parity, tmp_path):
    """SMK_ENC_SHAPE=32 (read once per process, hence a child): k_encoder_bf16<X3> at both sizes against the same references."""
    w, data = parity
    np.savez(tmp_path / "in.npz", **{f"frames{N}": data[N][0] for N in SIZES}, **{f"ref{N}": data[N][1][128] for N in SIZES})
    child = r'''
import sys, numpy as np, torch
sys.path.insert(0, "tests")
import test_hip_encoder_large as T
d = np.load(sys.argv[1])
enc = T.make_encoder()
for N in T.SIZES:
    x = torch.from_numpy(d[f"frames{N}"]).cuda()
    got = enc(x, input_dim=128, dtype="bf16x3")
    tok = enc.tokens(x, input_dim=128, dtype="bf16x3")
    assert torch.equal(tok, got.flatten(2).transpose(1, 2)), N
    err = T.rel_err(got.cpu().numpy(), d[f"ref{N}"])
    print(N, "rel err", err)
    assert err < 1e-4, (N, err)
print("shape32-ok")
'''
    out = subprocess.run([sys.executable, "-c", child, str(tmp_path / "in.npz")], cwd=ROOT, env=dict(os.environ, SMK_ENC_SHAPE="32"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "shape32-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("N", SIZES)
def test_tokens_equal_the_transposed_features(parity, N):
    w, data = parity
    x = torch.from_numpy(data[N][0]).cuda()
    enc = make_encoder(w)
    for dtype in MFMA_DTYPES:
        feats = enc(x, input_dim=128, dtype=dtype)
        tok = enc.tokens(x, input_dim=128, dtype=dtype)
        assert tok.shape == (x.shape[0], 1024, 128)
        assert torch.equal(tok, feats.flatten(2).transpose(1, 2)), (N, dtype)


# ---------------------------------------------------------------------------------------------------------------- 3./4. the skip path
def probe_pixels(N):
    """Single pixels around tile (ty, tx) = (2, 1) -- rows 16..23, cols 16..31 -- at distance 4 (inside its window: the tile runs) and 5
    (outside: it does not), and the four corners of the image."""
    r0, c0, r1, c1 = 16, 16, 23, 31
    near = [(r0 - 4, c0 + 3), (r1 + 4, c0 + 3), (r0 + 2, c0 - 4), (r0 + 2, c1 + 4),
            (r0 - 4, c0 - 4), (r0 - 4, c1 + 4), (r1 + 4, c0 - 4), (r1 + 4, c1 + 4)]
    far = [(r0 - 5, c0 + 3), (r1 + 5, c0 + 3), (r0 + 2, c0 - 5), (r0 + 2, c1 + 5),
           (r0 - 5, c0 - 5), (r0 - 5, c1 + 5), (r1 + 5, c0 - 5), (r1 + 5, c1 + 5)]
    corners = [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)]
    return near, far, corners


def one_pixel_batch(B, N, pixels):
    x = np.zeros((B, N, N), np.float32)
    for k, (r, c) in enumerate(pixels):
        x[k, r, c] = 1.0
    return x


def mostly_full_frames(N=1024, B=2, seed=77):
    """Dense frames with the windows of a seeded tenth of the tiles zeroed: about 90 % of the tiles stay non-empty, more than 16 rounds
    of 768 workgroups, so every workgroup refills its slate of looked-up tiles at the 1024^2 band geometry (one tile row per band)."""
    rng = np.random.RandomState(seed)
    x = (rng.rand(B, N, N) * 1.8).astype(np.float32)
    for b in range(B):
        for t in rng.choice((N // 8) * (N // 16), (N // 8) * (N // 16) // 10, replace=False):
            ty, tx = divmod(int(t), N // 16)
            x[b, max(8 * ty - 4, 0):8 * ty + 12, max(16 * tx - 4, 0):16 * tx + 20] = 0.0
    return x


def input_cases(N):
    """name -> frames on the GPU [B][N][N] (possibly pitched).  Seeded: the child process builds the same bits."""
    B = SKIP_BATCH[N]
    rng = np.random.RandomState(4000 + N)
    near, far, corners = probe_pixels(N)
    sim = simulated_frames(B, N)
    cases = {"simulated": sim, "zero": torch.zeros(B, N, N, device="cuda"),
             "dense": torch.from_numpy((rng.rand(B, N, N) * 1.8).astype(np.float32)).cuda()}
    for name, pixels in (("near4", near), ("far5", far), ("corners", corners)):     # one pixel per frame: probes do not hide each other
        for k in range(0, len(pixels), B):
            cases[f"{name}_{k // B}"] = torch.from_numpy(one_pixel_batch(B, N, pixels[k:k + B])).cuda()
    buf = torch.full((B, N * N + 24), 7.5, device="cuda")                            # frame_stride = H*W + 24, the gap full of garbage
    buf[:, :N * N] = (sim * (torch.arange(B, device="cuda") % 2 == 0)[:, None, None].float()).reshape(B, N * N)
    cases["pitched24"] = buf[:, :N * N].view(B, N, N)
    assert cases["pitched24"].stride(0) == N * N + 24
    if N == 1024:
        cases["mostly_full"] = torch.from_numpy(mostly_full_frames()).cuda()
    return cases


def run_cases(N, expect_skip):
    """Every (input, dtype, layout) at size N on one handle -> {key: sha256 of the output bytes}; checks the tile counts of each call."""
    enc = make_encoder()
    digests = {}
    for name, x in input_cases(N).items():
        flags = tiles_with_nonzero_window(x.cpu().numpy())
        want = int(flags.sum())
        if name.startswith("near4"):
            assert flags[:, 2, 1].all(), name                                        # distance 4 runs the tile
        if name.startswith("far5"):
            assert not flags[:, 2, 1].any(), name                                    # distance 5 does not
        if name.startswith("corners"):
            assert want == flags.shape[0], name                                      # a corner pixel marks its corner tile alone
        if name == "dense":
            assert want == flags.size
        if name == "zero":
            assert want == 0
        if name == "simulated":
            assert 0 < want < flags.size // 2
        if name == "mostly_full":
            assert 16 * 768 < want < 16384, want
        for dtype in MFMA_DTYPES:
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
import test_hip_encoder_large as T
N = int(sys.argv[2])
d = T.run_cases(N, expect_skip=False)
keys = sorted(d)
np.save(f"{sys.argv[1]}/direct_keys_{N}.npy", np.array(keys))
np.save(f"{sys.argv[1]}/direct_digests_{N}.npy", np.stack([np.frombuffer(d[k], np.uint8) for k in keys]))
print("direct-ok")
'''


_PATHS = {}


def both_paths(N):
    """(digests of this process = skip path, digests of the SMK_ENC_SKIP=0 child = direct path) for size N; one child per size, its exit
    status checked before anything else runs.  Computed once: a failure is kept and raised again, never run a second time."""
    if N not in _PATHS:
        try:
            _PATHS[N] = _both_paths(N)
        except BaseException as e:                           # noqa: BLE001
            _PATHS[N] = e
    if isinstance(_PATHS[N], BaseException):
        raise _PATHS[N]
    return _PATHS[N]


def _both_paths(N):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([sys.executable, "-c", CHILD, tmp, str(N)], cwd=ROOT, env=dict(os.environ, SMK_ENC_SKIP="0"),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "direct-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
        keys = [str(k) for k in np.load(os.path.join(tmp, f"direct_keys_{N}.npy"))]
        direct = dict(zip(keys, (d.tobytes() for d in np.load(os.path.join(tmp, f"direct_digests_{N}.npy")))))
    return run_cases(N, expect_skip=True), direct


@pytest.mark.parametrize("N", SIZES)
def test_skip_path_equals_direct_path_bitwise(N):
    """bf16x3, bf16, i8x3 x both layouts on simulated, all-zero, dense, one-pixel (distance 4 / 5 from tile (2, 1), image corners) and
    pitched batches: the same bits as the direct path, and tiles_run == the numpy rule's count on every call."""
    got, direct = both_paths(N)
    assert sorted(got) == sorted(direct) and len(got) >= 9 * 6
    bad = [k for k in sorted(got) if got[k] != direct[k] and "/mostly_full/" not in k]
    assert not bad, f"skip path differs from the direct path in {len(bad)} of {len(got)} cases: {bad[:12]}"


def test_slate_refill_at_one_tile_row_per_band():
    """1024^2, B = 2, about 90 % of the 16,384 tiles non-empty (more than 16 x 768): bitwise against the direct path; the exact tile
    counts were asserted call by call in run_cases."""
    got, direct = both_paths(1024)
    keys = [k for k in sorted(got) if "/mostly_full/" in k]
    assert len(keys) == 6
    bad = [k for k in keys if got[k] != direct[k]]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- 5. seams inside a cell
@pytest.mark.parametrize("N, rows, cols, cell", [(512, (40, 48), (0, 512), None), (1024, (112, 120), (176, 192), (3, 5))])
def test_one_tile_of_a_cell(N, rows, cols, cell):
    """512^2: a frame that is non-zero only in rows 8-15 of the 16-row cell band 32..47 (the lower tile row of every cell of pooled row 2).
    1024^2: only tile (2, 1) of the 4 x 2 tiles of cell (3, 5).  The cells must equal the reference (bf16x3 < 1e-4, over the frame and over
    the cells alone)."""
    rng = np.random.RandomState(5000 + N)
    frames = np.zeros((1, N, N), np.float32)
    frames[0, rows[0]:rows[1], cols[0]:cols[1]] = (rng.rand(rows[1] - rows[0], cols[1] - cols[0]) * 1.8 + 0.1).astype(np.float32)
    w = random_weights()
    ref = torch_reference(frames, w)[128]
    enc = make_encoder(w)
    x = torch.from_numpy(frames).cuda()
    got = enc(x, input_dim=128, dtype="bf16x3").cpu().numpy()
    total, run = enc.skip_stats()
    assert run == int(tiles_with_nonzero_window(frames).sum()) < total
    pi = rows[0] * 32 // N
    sel = (slice(None), slice(None), pi, slice(None)) if cell is None else (slice(None), slice(None), cell[0], cell[1])
    assert cell is None or cell == (rows[0] * 32 // N, cols[0] * 32 // N)
    errs = (rel_err(got, ref), rel_err(got[sel], ref[sel]))
    print(f"{N}^2 seam: rel err frame {errs[0]:.3e}, cells {errs[1]:.3e}")
    assert max(errs) < 1e-4
    tok = enc.tokens(x, input_dim=128, dtype="bf16x3")
    assert torch.equal(tok.cpu(), torch.from_numpy(got).flatten(2).transpose(1, 2))


# ---------------------------------------------------------------------------------------------------------------- 6. the model
def test_model_takes_the_fused_route_at_512():
    from smokephysai_amd.models import GraphedSmokePhysNet, SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(input_dim=32, hidden_dim=128, num_layers=1, num_heads=2, output_channels=16).cuda().eval()
    B, N = 2, 512
    rng = np.random.RandomState(6)
    x = torch.from_numpy((rng.rand(B, 1, N, N) * 1.8).astype(np.float32)).cuda()
    x2 = torch.from_numpy((rng.rand(B, 1, N, N) * 1.8).astype(np.float32)).cuda()
    noise = torch.randn(1, 3, B, 1, device="cuda")
    with torch.no_grad():
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            assert model._encoder_route(x) == "hip"
            out = model(x, chaos_noise=noise)
        assert not [c for c in caught if "outside the fused HIP encoder" in str(c.message)], [str(c.message) for c in caught]
        assert model.hip_encoder().skip_stats()[0] == B * 2048
        out = {k: v.clone() for k, v in out.items()}
        model._encoder_route = lambda frames: "modules"        # the same model, input_encoder on the PyTorch-ROCm modules
        try:
            ref = {k: v.clone() for k, v in model(x, chaos_noise=noise).items()}
        finally:
            del model._encoder_route
        for k in ref:
            err = rel_err(out[k].cpu().numpy(), ref[k].cpu().numpy())
            print(f"model output {k}: fused vs modules rel err {err:.3e}")
            assert err < 1e-4, (k, err)
        graphed = GraphedSmokePhysNet(model, clone=True)
        for xin in (x, x2):
            got = graphed(xin, chaos_noise=noise)
            eager = model(xin, chaos_noise=noise)
            for k in eager:
                assert torch.equal(eager[k], got[k]), k
        assert graphed.captures == 1


# ---------------------------------------------------------------------------------------------------------------- 7. still refused
def test_unsupported_shapes_still_raise():
    from smokephysai_amd._lib import SmokeHipError
    enc = make_encoder()
    for shape in ((1, 1, 2048, 2048), (1, 1, 512, 256)):
        for call in (enc, enc.tokens):
            with pytest.raises(SmokeHipError):
                call(torch.zeros(*shape, device="cuda"), input_dim=128, dtype="bf16x3")
    with pytest.raises(SmokeHipError):
        enc(torch.zeros(1, 1, 512, 512, device="cuda"), input_dim=48)
