"""Optical-flow baselines of the reference's benchmark.py (benchmark.py:21-94) on HIP: Farneback dense flow, Lucas-Kanade sparse flow
and the bilinear warp, batched over frame pairs (csrc/flow.hip; DESIGN.md "Optical-flow baselines" is the specification).

The reference calls OpenCV on one uint8 numpy pair at a time.  cv2 is not a dependency here: the kernels implement the published
algorithms with the reference's call parameters, and equality with cv2's own output is unmeasured.  Frames are uint8 tensors on a ROCm
device, [H, W], [H, W, 1] or batched [N, H, W] with 32 <= H, W <= 1024; results stay on the device.  A CPU tensor is an error: there is
no CPU fallback.

`to_uint8_frames(x)` stands in for the reference's `(x * 255).astype(np.uint8)`: x * 255 is clamped to 0..255 and truncated toward zero.
Wherever the frames lie in [0, 1] the bytes equal the reference's; a density outside that range saturates here, where numpy's cast
wraps modulo 256.
"""
import torch

from .. import _lib

MIN_DIM, MAX_DIM = 32, 1024              # csrc/flow.h FLOW_MIN_DIM / FLOW_MAX_DIM
MAX_CORNERS = 100                        # csrc/flow.h LK_MAX_CORNERS
_MAX_PAIRS = 65535                       # frame pairs per library call


def to_uint8_frames(x: torch.Tensor) -> torch.Tensor:
    """(x * 255) clamped to 0..255 and truncated toward zero, as uint8 (NaN becomes 0)."""
    return torch.nan_to_num(x.float() * 255.0, nan=0.0).clamp_(0.0, 255.0).to(torch.uint8)


def _frames(t: torch.Tensor, what: str):
    """-> (device, contiguous [N, H, W] uint8, function restoring the caller's leading shape)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    dev = _lib.require_cuda(t.device, what)
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: frames must be uint8 (see to_uint8_frames), got {t.dtype}")
    single = False
    if t.dim() == 3 and t.shape[2] == 1 and t.shape[1] != 1:
        t, single = t[:, :, 0], True
    elif t.dim() == 2:
        single = True
    elif t.dim() != 3:
        raise ValueError(f"{what}: frames must be [H, W], [H, W, 1] or [N, H, W], got {tuple(t.shape)}")
    t = t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()
    n, H, W = t.shape
    if n < 1 or not (MIN_DIM <= H <= MAX_DIM and MIN_DIM <= W <= MAX_DIM):
        raise ValueError(f"{what}: needs at least one frame with {MIN_DIM} <= H, W <= {MAX_DIM}, got {tuple(t.shape)}")
    return dev, t, (lambda r: r[0]) if single else (lambda r: r)


def _pair(prev, nxt, what):
    dev, a, restore = _frames(prev, what)
    _, b, _ = _frames(nxt, what)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"{what}: prev {tuple(prev.shape)} on {prev.device} and next {tuple(nxt.shape)} on {nxt.device} differ")
    return dev, a, b, restore


def _workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)     # the caching allocator aligns to 512 bytes


def _chunks(n):
    return [(s, min(_MAX_PAIRS, n - s)) for s in range(0, n, _MAX_PAIRS)]


def level_count(H: int, W: int) -> int:
    """Farneback pyramid depth K: the largest K <= 3 with min(H, W) * 0.5^(K-1) >= 32 (0 for an unsupported shape)."""
    return int(_lib.load().smk_flow_levels(H, W))


def level_size(H: int, W: int, level: int):
    """(round(H * 0.5^level), round(W * 0.5^level)), half to even."""
    return round(H * 0.5 ** level), round(W * 0.5 ** level)


def farneback_optical_flow(prev: torch.Tensor, next: torch.Tensor) -> torch.Tensor:
    """benchmark.py:21-39: dense flow [..., H, W, 2] fp32 (dx, dy) with the reference's parameters (0.5, 3, 15, 3, 5, 1.2, 0)."""
    dev, a, b, restore = _pair(prev, next, "farneback_optical_flow")
    n, H, W = a.shape
    L = _lib.load()
    flow = torch.empty(n, H, W, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for s, m in _chunks(n):
            nbytes = L.smk_flow_farneback_workspace(m, H, W)
            ws = _workspace(nbytes, dev)
            _lib.check(L.smk_flow_farneback(a[s].data_ptr(), b[s].data_ptr(), m, H, W, flow[s].data_ptr(), ws.data_ptr(), nbytes,
                                            _lib.stream_ptr(dev)))
    return restore(flow)


def lucas_kanade_optical_flow(prev: torch.Tensor, next: torch.Tensor) -> torch.Tensor:
    """benchmark.py:41-78: Shi-Tomasi corners of prev tracked into next; the field [..., H, W, 2] is zero except
    flow[int(y0), int(x0)] = (x1 - x0, y1 - y0) at the tracked corners (all zero for a frame without corners)."""
    dev, a, b, restore = _pair(prev, next, "lucas_kanade_optical_flow")
    n, H, W = a.shape
    L = _lib.load()
    flow = torch.empty(n, H, W, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for s, m in _chunks(n):
            nbytes = L.smk_flow_lk_workspace(m, H, W)
            ws = _workspace(nbytes, dev)
            _lib.check(L.smk_flow_lucas_kanade(a[s].data_ptr(), b[s].data_ptr(), m, H, W, flow[s].data_ptr(), ws.data_ptr(), nbytes,
                                               _lib.stream_ptr(dev)))
    return restore(flow)


def _warp(prev, flow, nxt, what):
    dev, a, restore = _frames(prev, what)
    n, H, W = a.shape
    if not isinstance(flow, torch.Tensor) or flow.device != a.device or flow.dtype != torch.float32:
        raise ValueError(f"{what}: flow must be an fp32 tensor on the frames' device")
    f = flow.reshape(-1, H, W, 2).contiguous() if flow.numel() == n * H * W * 2 else None
    if f is None:
        raise ValueError(f"{what}: flow {tuple(flow.shape)} does not match frames {tuple(prev.shape)}")
    b = None
    if nxt is not None:
        _, b, _ = _frames(nxt, what)
        if b.shape != a.shape:
            raise ValueError(f"{what}: next {tuple(nxt.shape)} does not match prev {tuple(prev.shape)}")
    L = _lib.load()
    pred = torch.empty_like(a)
    mse = torch.empty(n, dtype=torch.float64, device=dev) if b is not None else None
    with torch.cuda.device(dev):
        for s, m in _chunks(n):
            nbytes = L.smk_warp_workspace(m, H, W)
            ws = _workspace(nbytes, dev)
            _lib.check(L.smk_warp_frames(a[s].data_ptr(), f[s].data_ptr(), b[s].data_ptr() if b is not None else None, m, H, W,
                                         pred[s].data_ptr(), mse[s].data_ptr() if b is not None else None, ws.data_ptr(), nbytes,
                                         _lib.stream_ptr(dev)))
    return restore(pred), (mse if mse is None else restore(mse))


def predict_next_frame(prev: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """benchmark.py:80-94: pred(y, x) = bilinear sample of prev at (x + dx, y + dy), zero outside, rounded half to even; uint8, [H, W]
    or [N, H, W] (an [H, W, 1] frame gives [H, W], as cv2.remap does)."""
    return _warp(prev, flow, None, "predict_next_frame")[0]


def predict_and_score(prev: torch.Tensor, flow: torch.Tensor, next: torch.Tensor):
    """predict_next_frame plus the reference's per-pair sklearn mean_squared_error(next, pred) on the 0..255 scale, as fp64 on the
    device: (pred uint8, mse float64 [N] -- a 0-d tensor for a single pair).  Exact integer sums: bit-identical from call to call."""
    return _warp(prev, flow, next, "predict_and_score")


# ---------------------------------------------------------------- the stages, one library call each (tests/test_hip_optical_flow.py,
# tools/flow_probe.py); all take and return contiguous device tensors
def _fb_ws(L, n, h, w, dev):
    nbytes = L.smk_flow_farneback_workspace(n, h, w)
    return _workspace(nbytes, dev), nbytes


def level_image(frames: torch.Tensor, level: int) -> torch.Tensor:
    dev, a, _ = _frames(frames, "level_image")
    n, H, W = a.shape
    h, w = level_size(H, W, level)
    L = _lib.load()
    out = torch.empty(n, h, w, dtype=torch.float32, device=dev)
    ws, nbytes = _fb_ws(L, n, H, W, dev)
    with torch.cuda.device(dev):
        _lib.check(L.smk_flow_level_image(a.data_ptr(), n, H, W, level, out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(dev)))
    return out


def poly_expansion(img: torch.Tensor) -> torch.Tensor:
    """img [n, h, w] fp32 -> [n, 5, h, w] = (bx, by, axx, ayy, axy)"""
    dev = _lib.require_cuda(img.device, "poly_expansion")
    img = img.contiguous()
    n, h, w = img.shape
    coef = torch.empty(n, 5, h, w, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().smk_flow_poly_exp(img.data_ptr(), n, h, w, coef.data_ptr(), _lib.stream_ptr(dev)))
    return coef


def farneback_iteration(coef0: torch.Tensor, coef1: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """One matrix update + box mean + solve from flow [n, h, w, 2]; returns the new flow (the input is left alone)."""
    dev = _lib.require_cuda(flow.device, "farneback_iteration")
    n, h, w, _ = flow.shape
    out = flow.contiguous().clone()
    L = _lib.load()
    ws, nbytes = _fb_ws(L, n, h, w, dev)
    with torch.cuda.device(dev):
        _lib.check(L.smk_flow_farneback_iteration(coef0.contiguous().data_ptr(), coef1.contiguous().data_ptr(), out.data_ptr(), n, h, w,
                                                  ws.data_ptr(), nbytes, _lib.stream_ptr(dev)))
    return out


def min_eigen_map(frames: torch.Tensor) -> torch.Tensor:
    dev, a, _ = _frames(frames, "min_eigen_map")
    n, H, W = a.shape
    eig = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().smk_flow_min_eigen(a.data_ptr(), n, H, W, eig.data_ptr(), _lib.stream_ptr(dev)))
    return eig


def good_features(eig: torch.Tensor):
    """eig [n, H, W] fp32 -> (pts [n, 100, 2] fp32 (x, y) in order of selection, counts [n] int32)"""
    dev = _lib.require_cuda(eig.device, "good_features")
    eig = eig.contiguous()
    n, H, W = eig.shape
    L = _lib.load()
    pts = torch.empty(n, MAX_CORNERS, 2, dtype=torch.float32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    nbytes = L.smk_flow_lk_workspace(n, H, W)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(L.smk_good_features(eig.data_ptr(), n, H, W, pts.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                                       _lib.stream_ptr(dev)))
    return pts, counts


def lk_track(prev: torch.Tensor, next: torch.Tensor, pts: torch.Tensor, counts: torch.Tensor):
    """-> (out_pts [n, 100, 2] fp32, status [n, 100] uint8)"""
    dev, a, b, _ = _pair(prev, next, "lk_track")
    n, H, W = a.shape
    L = _lib.load()
    pts = pts.contiguous()
    counts = counts.contiguous()
    out = torch.empty(n, MAX_CORNERS, 2, dtype=torch.float32, device=dev)
    status = torch.empty(n, MAX_CORNERS, dtype=torch.uint8, device=dev)
    nbytes = L.smk_flow_lk_workspace(n, H, W)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(L.smk_flow_lk_track(a.data_ptr(), b.data_ptr(), n, H, W, pts.data_ptr(), counts.data_ptr(), out.data_ptr(),
                                       status.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(dev)))
    return out, status


def lk_scatter(pts, out_pts, status, counts, H: int, W: int) -> torch.Tensor:
    dev = _lib.require_cuda(pts.device, "lk_scatter")
    n = pts.shape[0]
    flow = torch.empty(n, H, W, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().smk_flow_lk_scatter(pts.contiguous().data_ptr(), out_pts.contiguous().data_ptr(),
                                                   status.contiguous().data_ptr(), counts.contiguous().data_ptr(), n, H, W,
                                                   flow.data_ptr(), _lib.stream_ptr(dev)))
    return flow
