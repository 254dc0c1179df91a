"""numpy oracle of the optical-flow baselines, written from the rules in DESIGN.md "Optical-flow baselines" (not from the kernels).

Every function takes a `dtype`: float64 is the truth, float32 is the yardstick for rounding (each operation is rounded to `dtype`, in the
order the specification fixes).  Frames are uint8 arrays [n, H, W]; flows are [n, H, W, 2] (dx, dy).  Reads nothing under oracle/, and
nothing under smokephysai_amd/ imports it.
"""
import numpy as np

POLY_N, POLY_SIGMA = 5, 1.2              # the reference's call: calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0)
FB_WIN, FB_ITERS, FB_MAX_LEVELS, FB_MIN_DIM = 15, 3, 3, 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
MAX_CORNERS, QUALITY, MIN_DISTANCE, EIG_BLOCK = 100, 0.3, 7, 7
LK_WIN, LK_MAX_LEVEL, LK_ITERS, LK_EPS, LK_MIN_EIG = 15, 2, 30, 0.01, 1e-4


def _T(dtype):
    return np.dtype(dtype).type


# ------------------------------------------------------------------ Farneback
def level_count(H, W):
    K = 1
    while K < FB_MAX_LEVELS and min(H, W) * 0.5 ** K >= FB_MIN_DIM:
        K += 1
    return K


def level_size(H, W, k):
    return int(np.rint(H * 0.5 ** k)), int(np.rint(W * 0.5 ** k))


def blur_taps(k, dtype):
    if k == 0:
        return np.array([0.25, 0.5, 0.25], dtype)
    sigma, r = (0.5, 1) if k == 1 else (1.5, 4)
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(dtype)


def _taps_along(P, taps, axis, size):
    """sum_t taps[t] * P[t : t + size] along `axis`, left to right"""
    sl = [slice(None)] * P.ndim
    acc = None
    for t in range(len(taps)):
        sl[axis] = slice(t, t + size)
        term = taps[t] * P[tuple(sl)]
        acc = term if acc is None else acc + term
    return acc


def resize_bilinear(src, hd, wd, inv, mul, dtype):
    """src [n, hs, ws] or [n, hs, ws, c]; src coordinate = (dst + 0.5) * inv - 0.5 clamped to the source; result * mul"""
    T = _T(dtype)
    hs, ws = src.shape[1:3]

    def axis(nd, ns):
        s = (np.arange(nd).astype(dtype) + T(0.5)) * T(inv) - T(0.5)
        s = np.minimum(np.maximum(s, T(0)), T(ns - 1))
        f0 = np.floor(s)
        i0 = f0.astype(np.int64)
        return i0, np.minimum(i0 + 1, ns - 1), s - f0

    y0, y1, fy = axis(hd, hs)
    x0, x1, fx = axis(wd, ws)
    if src.ndim == 4:
        fx = fx[:, None]
    fyb = fy[:, None, None] if src.ndim == 4 else fy[:, None]
    one = T(1)
    top = src[:, y0][:, :, x0] * (one - fx) + src[:, y0][:, :, x1] * fx
    bot = src[:, y1][:, :, x0] * (one - fx) + src[:, y1][:, :, x1] * fx
    return ((top * (one - fyb) + bot * fyb) * T(mul)).astype(dtype)


def level_image(frames, k, dtype):
    n, H, W = frames.shape
    taps = blur_taps(k, dtype)
    r = len(taps) // 2
    P = np.pad(frames.astype(dtype), ((0, 0), (r, r), (r, r)), mode="reflect")
    hpass = _taps_along(P, taps, 2, W)
    blur = _taps_along(hpass, taps, 1, H)
    if k == 0:
        return blur
    h, w = level_size(H, W, k)
    return resize_bilinear(blur, h, w, float(2 ** k), 1.0, dtype)


def poly_constants(dtype):
    """(g, xg, xxg for k = 0..5; ig11, ig03, ig33, ig55) from the inverse of the 6 x 6 moment matrix of the basis (1, x, y, x^2, y^2, xy)"""
    x = np.arange(-POLY_N, POLY_N + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * POLY_SIGMA ** 2))
    g /= g.sum()
    X, Y = np.meshgrid(x, x)
    basis = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y], 0).reshape(6, -1)
    wgt = np.outer(g, g).reshape(-1)
    G = (basis * wgt) @ basis.T
    inv = np.linalg.inv(G)
    k = np.arange(0, POLY_N + 1, dtype=np.float64)
    gk = g[POLY_N:]
    return ((gk).astype(dtype), (gk * k).astype(dtype), (gk * k * k).astype(dtype),
            _T(dtype)(inv[1, 1]), _T(dtype)(inv[0, 3]), _T(dtype)(inv[3, 3]), _T(dtype)(inv[5, 5]))


def poly_expansion(img, dtype):
    """img [n, h, w] -> [n, 5, h, w] = (bx, by, axx, ayy, axy)"""
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_constants(dtype)
    n, h, w = img.shape
    N = POLY_N
    P = np.pad(img.astype(dtype), ((0, 0), (N, N), (N, N)), mode="edge")
    c = P[:, N:N + h, :]
    r0 = g[0] * c
    r1 = np.zeros_like(c)
    r2 = np.zeros_like(c)
    for k in range(1, N + 1):
        a, b = P[:, N + k:N + k + h, :], P[:, N - k:N - k + h, :]
        s, d = a + b, a - b
        r0 = r0 + g[k] * s
        r1 = r1 + xg[k] * d
        r2 = r2 + xxg[k] * s
    b1, b3, b6 = g[0] * r0[:, :, N:N + w], g[0] * r1[:, :, N:N + w], g[0] * r2[:, :, N:N + w]
    b2, b4, b5 = np.zeros_like(b1), np.zeros_like(b1), np.zeros_like(b1)
    for k in range(1, N + 1):
        p, m = slice(N + k, N + k + w), slice(N - k, N - k + w)
        s0, d0 = r0[:, :, p] + r0[:, :, m], r0[:, :, p] - r0[:, :, m]
        s1, d1 = r1[:, :, p] + r1[:, :, m], r1[:, :, p] - r1[:, :, m]
        s2 = r2[:, :, p] + r2[:, :, m]
        b1 = b1 + g[k] * s0
        b2 = b2 + xg[k] * d0
        b4 = b4 + xxg[k] * s0
        b3 = b3 + g[k] * s1
        b5 = b5 + xg[k] * d1
        b6 = b6 + g[k] * s2
    return np.stack([b2 * ig11, b3 * ig11, b1 * ig03 + b4 * ig33, b1 * ig03 + b6 * ig33, b5 * ig55], 1).astype(dtype)


def _border_scale(n, dtype):
    s = np.ones(n, dtype)
    tab = np.array(BORDER, dtype)
    for i in range(n):
        if i < 5:
            s[i] = tab[i]
        if i >= n - 5:
            s[i] = s[i] * tab[n - 1 - i]
    return s


def update_matrices(c0, c1, flow, dtype):
    """c0, c1 [n, 5, h, w], flow [n, h, w, 2] -> [n, 5, h, w] = (g11, g12, g22, h1, h2)"""
    T = _T(dtype)
    n, _, h, w = c0.shape
    c0, c1, flow = c0.astype(dtype), c1.astype(dtype), flow.astype(dtype)
    dx, dy = flow[..., 0], flow[..., 1]
    xs = np.arange(w).astype(dtype)[None, None, :]
    ys = np.arange(h).astype(dtype)[None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        fxp, fyp = xs + dx, ys + dy
        inside = (fxp >= 0) & (fxp < w - 1) & (fyp >= 0) & (fyp < h - 1)
        x0f, y0f = np.floor(np.where(inside, fxp, T(0))), np.floor(np.where(inside, fyp, T(0)))
        fx, fy = np.where(inside, fxp, T(0)) - x0f, np.where(inside, fyp, T(0)) - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)       # only reached where `inside` is false
        one = T(1)
        a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
        bi = np.arange(n)[:, None, None]
        s = [((a00 * c1[:, k][bi, y0, x0] + a01 * c1[:, k][bi, y0, x1]) + a10 * c1[:, k][bi, y1, x0]) + a11 * c1[:, k][bi, y1, x1]
             for k in range(5)]
        half, quarter = T(0.5), T(0.25)
        dbx = np.where(inside, (c0[:, 0] - s[0]) * half, T(0))
        dby = np.where(inside, (c0[:, 1] - s[1]) * half, T(0))
        axx = np.where(inside, (c0[:, 2] + s[2]) * half, c0[:, 2])
        ayy = np.where(inside, (c0[:, 3] + s[3]) * half, c0[:, 3])
        axyh = np.where(inside, (c0[:, 4] + s[4]) * quarter, c0[:, 4] * half)
        dbx = (dbx + axx * dx) + axyh * dy
        dby = (dby + axyh * dx) + ayy * dy
        sc = _border_scale(w, dtype)[None, None, :] * _border_scale(h, dtype)[None, :, None]
        axx, ayy, axyh, dbx, dby = axx * sc, ayy * sc, axyh * sc, dbx * sc, dby * sc
        return np.stack([axx * axx + axyh * axyh, axyh * (axx + ayy), ayy * ayy + axyh * axyh, axx * dbx + axyh * dby,
                         axyh * dbx + ayy * dby], 1).astype(dtype)


def box_solve(M, dtype):
    """15 x 15 box mean (border replicate; 15 terms left to right, then 15 top down, then * 1/225) and d = G^-1 h"""
    T = _T(dtype)
    n, _, h, w = M.shape
    r = FB_WIN // 2
    with np.errstate(invalid="ignore", over="ignore"):
        P = np.pad(M.astype(dtype), ((0, 0), (0, 0), (r, r), (r, r)), mode="edge")
        ones = np.ones(FB_WIN, dtype)
        m = _taps_along(_taps_along(P, ones, 3, w), ones, 2, h) * T(1.0 / (FB_WIN * FB_WIN))
        g11, g12, g22, h1, h2 = (m[:, k] for k in range(5))
        idet = T(1) / ((g11 * g22 - g12 * g12) + T(1e-3))
        return np.stack([(g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet], -1).astype(dtype)


def farneback_iteration(c0, c1, flow, dtype):
    return box_solve(update_matrices(c0, c1, flow, dtype), dtype)


def farneback(prev, nxt, dtype):
    n, H, W = prev.shape
    K = level_count(H, W)
    flow = None
    for k in range(K - 1, -1, -1):
        h, w = level_size(H, W, k)
        flow = np.zeros((n, h, w, 2), dtype) if flow is None else resize_bilinear(flow, h, w, 0.5, 2.0, dtype)
        c0 = poly_expansion(level_image(prev, k, dtype), dtype)
        c1 = poly_expansion(level_image(nxt, k, dtype), dtype)
        for _ in range(FB_ITERS):
            flow = farneback_iteration(c0, c1, flow, dtype)
    return flow


# ------------------------------------------------------------------ warp and error
def warp(prev, flow, dtype):
    """pred(y, x) = bilinear sample of prev at (x + dx, y + dy); taps outside read 0; round half to even; saturate to uint8"""
    T = _T(dtype)
    n, H, W = prev.shape
    flow = flow.astype(dtype)
    img = prev.astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        sx = np.arange(W).astype(dtype)[None, None, :] + flow[..., 0]
        sy = np.arange(H).astype(dtype)[None, :, None] + flow[..., 1]
        ok = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
        sx, sy = np.where(ok, sx, T(0)), np.where(ok, sy, T(0))
        x0f, y0f = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0f, sy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        bi = np.arange(n)[:, None, None]

        def tap(y, x):
            valid = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            return np.where(valid, img[bi, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], T(0))

        one = T(1)
        top = tap(y0, x0) * (one - fx) + tap(y0, x0 + 1) * fx
        bot = tap(y0 + 1, x0) * (one - fx) + tap(y0 + 1, x0 + 1) * fx
        v = np.where(ok, top * (one - fy) + bot * fy, T(0))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def mse_uint8(nxt, pred):
    """per-pair fp64 mean of (next - pred)^2 on the 0..255 scale (exact integer sums)"""
    d = nxt.astype(np.int64) - pred.astype(np.int64)
    return (d * d).reshape(d.shape[0], -1).sum(1).astype(np.float64) / float(d.shape[1] * d.shape[2])


# ------------------------------------------------------------------ Shi-Tomasi corners
def min_eigen(frames, dtype):
    """Sobel 3 x 3 (reflect-101), 7 x 7 box sums of the products (reflect-101 on the derivative maps), all exact integers; then
    lambda_min = (a + c) - sqrt((a - c)^2 + b^2) with a = Sxx / 2, b = Sxy, c = Syy / 2 in `dtype`"""
    T = _T(dtype)
    n, H, W = frames.shape
    P = np.pad(frames.astype(np.int64), ((0, 0), (1, 1), (1, 1)), mode="reflect")

    def at(dy, dx):
        return P[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    ix = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    iy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    r = EIG_BLOCK // 2

    def box(a):
        Q = np.pad(a, ((0, 0), (r, r), (r, r)), mode="reflect")
        ones = np.ones(EIG_BLOCK, np.int64)
        return _taps_along(_taps_along(Q, ones, 2, W), ones, 1, H)

    a = box(ix * ix).astype(dtype) * T(0.5)
    b = box(ix * iy).astype(dtype)
    c = box(iy * iy).astype(dtype) * T(0.5)
    d = a - c
    return ((a + c) - np.sqrt(d * d + b * b)).astype(dtype)


def select_corners(eig):
    """eig [H, W] -> list of (x, y): value strictly above 0.3 x the maximum (in eig's dtype), equal to the 3 x 3 maximum, off the 1-pixel
    border; by value descending, ties by (y, x) ascending; accepted if no accepted corner is nearer than 7; at most 100"""
    H, W = eig.shape
    T = eig.dtype.type
    thr = T(max(eig.max(), 0)) * T(QUALITY)
    P = np.pad(eig, 1, mode="constant", constant_values=-np.inf)
    local = np.max(np.stack([P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0), 0)
    cand = (eig > thr) & (eig == local)
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    ys, xs = np.nonzero(cand)
    order = sorted(range(len(ys)), key=lambda i: (-float(eig[ys[i], xs[i]]), int(ys[i]), int(xs[i])))
    out = []
    for i in order:
        x, y = int(xs[i]), int(ys[i])
        if all((x - px) ** 2 + (y - py) ** 2 >= MIN_DISTANCE ** 2 for px, py in out):
            out.append((x, y))
            if len(out) == MAX_CORNERS:
                break
    return out


# ------------------------------------------------------------------ pyramidal Lucas-Kanade
def pyr_down(img, dtype):
    """(1, 4, 6, 4, 1) / 16 along rows then columns, reflect-101, even samples; [h, w] -> [(h + 1) / 2, (w + 1) / 2]"""
    h, w = img.shape
    taps = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], dtype)
    P = np.pad(img.astype(dtype), 2, mode="reflect")
    rows = _taps_along(P, taps, 1, w)[:, ::2]
    return _taps_along(rows, taps, 0, h)[::2, :]


def _scharr(img, dtype):
    T = _T(dtype)
    h, w = img.shape
    P = np.pad(img, 1, mode="edge")

    def at(dy, dx):
        return P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    gx = ((T(3) * (at(-1, 1) - at(-1, -1)) + T(10) * (at(0, 1) - at(0, -1))) + T(3) * (at(1, 1) - at(1, -1))) * T(0.03125)
    gy = ((T(3) * (at(1, -1) - at(-1, -1)) + T(10) * (at(1, 0) - at(-1, 0))) + T(3) * (at(1, 1) - at(-1, 1))) * T(0.03125)
    return gx, gy


def _bil_setup(x, y, w, h, T):
    x = np.minimum(np.maximum(x, T(0)), T(w - 1))
    y = np.minimum(np.maximum(y, T(0)), T(h - 1))
    x0f, y0f = np.floor(x), np.floor(y)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    return x0, y0, np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1), x - x0f, y - y0f


def _bil(img, s, T):
    x0, y0, x1, y1, fx, fy = s
    one = T(1)
    top = img[y0, x0] * (one - fx) + img[y0, x1] * fx
    bot = img[y1, x0] * (one - fx) + img[y1, x1] * fx
    return top * (one - fy) + bot * fy


def _inside(x, y, w, h):
    return bool(x >= 0 and x <= w - 1 and y >= 0 and y <= h - 1)


def lk_track(prev, nxt, pts, dtype):
    """prev, nxt [H, W] uint8, pts list of (x, y) -> (out [len, 2], status [len]).  A level is skipped when the point or its guess lies
    outside that level's image, or G's smaller eigenvalue / 225 is below 1e-4; a point is lost when that happens at level 0 or the
    iteration leaves the image."""
    T = _T(dtype)
    I, J = [prev.astype(dtype)], [nxt.astype(dtype)]
    for _ in range(LK_MAX_LEVEL):
        I.append(pyr_down(I[-1], dtype))
        J.append(pyr_down(J[-1], dtype))
    grads = [_scharr(im, dtype) for im in I]
    r = LK_WIN // 2
    wy, wx = np.divmod(np.arange(LK_WIN * LK_WIN), LK_WIN)
    ox, oy = (wx - r).astype(dtype), (wy - r).astype(dtype)
    out = np.zeros((len(pts), 2), dtype)
    status = np.zeros(len(pts), np.uint8)
    for i, (x0, y0) in enumerate(pts):
        px0, py0 = T(x0), T(y0)
        vx, vy = T(0), T(0)
        ok = True
        for L in range(LK_MAX_LEVEL, -1, -1):
            h, w = I[L].shape
            sc = T(0.5 ** L)
            px, py = px0 * sc, py0 * sc
            level_ok = _inside(px, py, w, h) and _inside(px + vx, py + vy, w, h)
            if level_ok:
                s = _bil_setup(px + ox, py + oy, w, h, T)
                iv, gx, gy = _bil(I[L], s, T), _bil(grads[L][0], s, T), _bil(grads[L][1], s, T)
                gxx, gxy, gyy = (gx * gx).sum(dtype=dtype), (gx * gy).sum(dtype=dtype), (gy * gy).sum(dtype=dtype)
                det = gxx * gyy - gxy * gxy
                dd = gxx - gyy
                min_eig = ((gyy + gxx) - np.sqrt(dd * dd + T(4) * gxy * gxy)) / (T(2) * T(LK_WIN * LK_WIN))
                level_ok = bool(min_eig >= T(LK_MIN_EIG) and det > 0)
                if level_ok:
                    for _ in range(LK_ITERS):
                        sj = _bil_setup((px + vx) + ox, (py + vy) + oy, w, h, T)
                        diff = iv - _bil(J[L], sj, T)
                        b1, b2 = (diff * gx).sum(dtype=dtype), (diff * gy).sum(dtype=dtype)
                        ddx, ddy = (gyy * b1 - gxy * b2) / det, (gxx * b2 - gxy * b1) / det
                        vx, vy = vx + ddx, vy + ddy
                        if not _inside(px + vx, py + vy, w, h):
                            level_ok = False
                            break
                        if ddx * ddx + ddy * ddy < T(LK_EPS * LK_EPS):
                            break
            if L == 0:
                ok = level_ok
            else:
                vx, vy = vx * T(2), vy * T(2)
        out[i] = (px0 + vx, py0 + vy)
        status[i] = 1 if ok else 0
    return out, status


def lk_scatter(pts, out, status, H, W, dtype=np.float32):
    flow = np.zeros((H, W, 2), dtype)
    for (x0, y0), (x1, y1), st in zip(pts, out, status):
        if st:
            flow[int(y0), int(x0)] = (dtype(x1) - dtype(x0), dtype(y1) - dtype(y0))
    return flow


def lucas_kanade(prev, nxt, dtype):
    """prev, nxt [H, W] uint8 -> flow [H, W, 2]"""
    pts = select_corners(min_eigen(prev[None], dtype)[0])
    out, status = lk_track(prev, nxt, pts, dtype)
    return lk_scatter(pts, out, status, prev.shape[0], prev.shape[1], _T(dtype))


# ------------------------------------------------------------------ test inputs
def texture(H, W, seed, sigma=2.0):
    """band-limited texture: Gaussian-blurred uniform noise (periodic), stretched to 0..255, float64"""
    rng = np.random.RandomState(seed)
    a = rng.rand(H, W)
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    a = np.real(np.fft.ifft2(np.fft.fft2(a) * np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))))
    a = (a - a.min()) / (a.max() - a.min())
    return a * 255.0


def shifted_pair(H, W, seed, shift=(2, -1), sigma=2.0):
    """(prev, next) uint8 with next(y, x) = prev(y - sy, x - sx) for shift = (sx, sy), cut from one larger texture"""
    sx, sy = shift
    m = 8
    big = texture(H + 2 * m, W + 2 * m, seed, sigma)
    prev = big[m:m + H, m:m + W]
    nxt = big[m - sy:m - sy + H, m - sx:m - sx + W]
    return prev.astype(np.uint8), nxt.astype(np.uint8)
