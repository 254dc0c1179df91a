"""Oracle of the gradient of the orbit render, written from the rule of SPEC_3D.md section 10 "Orbit views -- Gradient" (not from the
kernels, and not by differentiating anything: tests/test_render_orbit_grad_host.py holds it against torch's fp64 autograd of the forward
rule).

orbit_grad_fp64       : d(loss)/d(rho) in float64: render_grad_fp64 (tests/render_grad_oracle.py) over the samples of every view
                        (orbit_samples_fp64), scattered back with the four bilinear weights, summed over the views.
err                   : max|d - ref| / max(max|ref|, V * s), s = render_grad_oracle.term_scale, V the views of the volume.
render_orbit_torch    : the forward rule as torch ops in the tensor's own dtype (gathers of the four taps, then render_torch): what
                        autograd replays.  In float64 it is the rule; in float32, with the positions formed in fp32 exactly as the rule
                        writes them, its autograd is the "fp32 replay": what fp32 alone costs, whatever the device does.
orbit_grad_view_cases_fp64 : orbit_grad_fp64 of one view for all the sigma pairs and lights at once, G alone and Gt alone (the gradient is
                        linear in the pair; "both" is their sum), sharing tau, alpha and the light prefixes -- what the case list calls.
reference             : per group of the shared case list (a shape, a density kind, a light), computed once and left unchanged: the
                        volumes, the upstream gradients, the float64 gradients of every case and the replay's error on each.
The shared case list: GPU_SHAPES x DENSITIES x 2 volumes x the 8 GPU_AZIMUTHS in one call x SIGMAS x ORBIT_LIGHTS x COMBOS.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from render_grad_oracle import GAIN, render_grad_fp64, render_torch, term_scale
from render_oracle import DENSITIES
from render_orbit_oracle import (AMBIENT, GPU_AZIMUTHS, GPU_SHAPES, HOST_AZIMUTHS, HOST_SHAPES, ORBIT_LIGHTS, SIGMAS,  # noqa: F401
                                 _positions, orbit_samples_fp64, volumes)

COMBOS = ("both", "image", "trans")        # which upstream gradients a call is given
BOUND = 1e-4                               # device against orbit_grad_fp64 in `err`


def upstream(shape, n, V, seed=1):
    """G and Gt for n volumes of `shape` seen from V views: standard normal float32 [n, V, H, W]."""
    rng = np.random.default_rng(seed)
    img = (n, V) + tuple(shape[-2:])
    return rng.standard_normal(img).astype(np.float32), rng.standard_normal(img).astype(np.float32)


def _taps(D, W, phi, dtype):
    """The four taps of every sample: [(voxel z [S,W], voxel x [S,W], weight [S,W], inside the volume [S,W])], all in `dtype`."""
    z, x = _positions(D, W, phi, dtype)
    z0, x0 = np.floor(z), np.floor(x)
    fz, fx = z - z0, x - x0
    zi, xi = z0.astype(np.int64), x0.astype(np.int64)
    one = dtype(1)
    taps = []
    for dz in (0, 1):
        for dx in (0, 1):
            w = (fz if dz else one - fz) * (fx if dx else one - fx)
            inside = (zi + dz >= 0) & (zi + dz < D) & (xi + dx >= 0) & (xi + dx < W)
            taps.append((zi + dz, xi + dx, w, inside))
    return taps


def scatter_fp64(d_s, D, phi):
    """B^T: d_s [S,H,W'] (a gradient per sample) -> [D,H,W], every sample's value added to its in-volume taps with their weights."""
    S, H, W = d_s.shape
    out = np.zeros((D, W, H))
    cols = np.moveaxis(np.asarray(d_s, np.float64), 1, 2)                      # [S, W', H]
    for zi, xi, w, inside in _taps(D, W, phi, np.float64):
        np.add.at(out, (zi[inside], xi[inside]), w[inside][:, None] * cols[inside])
    return np.moveaxis(out, 2, 1)


def orbit_grad_fp64(rho, azimuths, G=None, Gt=None, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [D,H,W]; azimuths: V numbers; G / Gt [V,H,W] or None (= zero) -> d(sum(image * G) + sum(transmittance * Gt)) / d(rho)."""
    rho = np.asarray(rho, np.float64)
    if light not in ORBIT_LIGHTS:
        raise ValueError(light)
    d = np.zeros_like(rho)
    for k, phi in enumerate(azimuths):
        d_s = render_grad_fp64(orbit_samples_fp64(rho, phi), None if G is None else G[k], None if Gt is None else Gt[k], sigma_view,
                               sigma_light, ambient, gain, light)
        d += scatter_fp64(d_s, rho.shape[0], phi)
    return d


def err(d, ref, V, G, Gt, sigma_view, sigma_light, ambient, gain, light):
    ref = np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), V * term_scale(G, Gt, sigma_view, sigma_light, ambient, gain, light))
    return float(np.abs(np.asarray(d, np.float64) - ref).max()) / scale


# ---- the forward rule as torch ops ----------------------------------------------------------------------------------------------------
def orbit_samples_torch(rho, phi):
    """rho [..., D, H, W] (float32: positions and weights in fp32 as the rule writes them; float64: in float64) -> rho_s [..., S, H, W]."""
    import torch
    import torch.nn.functional as F
    D, H, W = rho.shape[-3:]
    dtype = np.float32 if rho.dtype == torch.float32 else np.float64
    padded = F.pad(rho.transpose(-1, -2), (0, 0, 1, 1, 1, 1))                   # [..., D+2, W+2, H]: a border of zeros
    v = [padded[..., torch.from_numpy(np.clip(zi, -1, D) + 1).to(rho.device), torch.from_numpy(np.clip(xi, -1, W) + 1).to(rho.device), :]
         for zi, xi, _, _ in _taps(D, W, phi, dtype)]                           # [..., S, W, H] each
    z, x = _positions(D, W, phi, dtype)
    fz = torch.from_numpy(z - np.floor(z)).to(rho.device)[..., None]
    fx = torch.from_numpy(x - np.floor(x)).to(rho.device)[..., None]
    out = (1 - fz) * ((1 - fx) * v[0] + fx * v[1]) + fz * ((1 - fx) * v[2] + fx * v[3])      # the rule's order
    return out.transpose(-1, -2)


def render_orbit_torch(rho, phi, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """The orbit render of rho [..., D, H, W] from one azimuth as torch ops in rho's dtype -> (image, transmittance) [..., H, W]."""
    return render_torch(orbit_samples_torch(rho, phi), sigma_view, sigma_light, ambient, gain, light)


def orbit_grad_autograd(rho, azimuths, G, Gt, sigma_view, sigma_light, ambient, gain, light, dtype):
    """torch autograd of render_orbit_torch in `dtype` (torch.float64: the rule; torch.float32: the replay) -> numpy [D,H,W]."""
    import torch
    r = torch.tensor(np.asarray(rho), dtype=dtype, requires_grad=True)
    loss = 0
    for k, phi in enumerate(azimuths):
        img, tr = render_orbit_torch(r, phi, sigma_view, sigma_light, ambient, gain, light)
        if G is not None:
            loss = loss + (img * torch.tensor(np.asarray(G[k]), dtype=dtype)).sum()
        if Gt is not None:
            loss = loss + (tr * torch.tensor(np.asarray(Gt[k]), dtype=dtype)).sum()
    loss.backward()
    return r.grad.numpy()


# ---- the shared case list -------------------------------------------------------------------------------------------------------------
def _excl(x, axis, reverse=False):
    r = np.flip(x, axis) if reverse else x
    c = np.cumsum(r, axis=axis) - r
    return np.flip(c, axis) if reverse else c


def orbit_grad_view_cases_fp64(rho, phi, G, Gt, sigmas=SIGMAS, lights=ORBIT_LIGHTS, ambient=AMBIENT, gain=GAIN):
    """One view.  rho [D,H,W], G / Gt [H,W] -> {(sv, sl, light): (gradient with G alone, gradient with Gt alone)} [D,H,W] float64: the
    rule's formulas with everything a sigma pair or a light does not change formed once, and one scatter for all of them."""
    rho = np.asarray(rho, np.float64)
    D = rho.shape[0]
    rs = orbit_samples_fp64(rho, phi)
    gG, Gt = gain * np.asarray(G, np.float64), np.asarray(Gt, np.float64)
    inc = np.cumsum(rs, axis=0)
    tau = inc - rs
    A = {"+y": _excl(rs, 1), "-y": _excl(rs, 1, reverse=True)}
    keys, parts = [], []
    for sv, sl in sigmas:
        T, E0, alpha = np.exp(-sv * tau), np.exp(-sv * rs), -np.expm1(-sv * rs)
        dt = np.broadcast_to(-sv * Gt * np.exp(-sv * inc[-1]), rs.shape)
        for light in lights:
            if light == "none":
                L, shadow = 1.0, 0.0
            else:
                X = np.exp(-sl * A[light])
                L = ambient + (1.0 - ambient) * X
                Sm = gG * alpha * T * (-sl * (1.0 - ambient) * X)
                shadow = _excl(Sm, 1, reverse=(light == "+y"))
            LT = L * T
            keys.append((sv, sl, light))
            parts += [gG * sv * (E0 * LT - _excl(alpha * LT, 0, reverse=True)) + shadow, dt]
    out = scatter_fp64(np.concatenate(parts, axis=1), D, phi)                  # stacked along H: the scatter does not look at y
    H = rho.shape[1]
    return {key: (out[:, 2 * i * H:(2 * i + 1) * H], out[:, (2 * i + 1) * H:(2 * i + 2) * H]) for i, key in enumerate(keys)}


def orbit_replay_view_cases(rho, phi, G, Gt, sigmas=SIGMAS, lights=ORBIT_LIGHTS, ambient=AMBIENT, gain=GAIN):
    """One view of the fp32 replay: {(sv, sl, light, combo): gradient [D,H,W] float32} by torch's fp32 autograd of render_orbit_torch."""
    import torch
    r = torch.tensor(np.asarray(rho, np.float32), requires_grad=True)
    rs = orbit_samples_torch(r, phi)
    Gi, Gr = torch.tensor(np.asarray(G, np.float32)), torch.tensor(np.asarray(Gt, np.float32))
    res = {}
    for sv, sl in sigmas:
        for light in lights:
            img, tr = render_torch(rs, sv, sl, ambient, gain, light)
            li, lt = (img * Gi).sum(), (tr * Gr).sum()
            for combo, loss in (("both", li + lt), ("image", li), ("trans", lt)):
                res[sv, sl, light, combo] = torch.autograd.grad(loss, r, retain_graph=True)[0].numpy()
    return res


def combo_grads(combo, G, Gt):
    """The (G, Gt) a call of `combo` is given."""
    return (G if combo != "trans" else None), (Gt if combo != "image" else None)


_REFERENCE = {}
CASE_GROUPS = [(shape, kind, light) for shape in GPU_SHAPES for kind in DENSITIES for light in ORBIT_LIGHTS]


def reference(shape, kind, light):
    """One group of the case list -- a shape, a density kind, a light; its 2 volumes x 8 azimuths x 4 sigma pairs x 3 combos -- computed
    once and left unchanged.  "vols": [2,D,H,W] float32; "G", "Gt": [2,V,H,W] float32 (the same for every group of a shape); "ref":
    {(sv, sl, combo): [2,D,H,W] float64, the views summed}; "replay": {the same key: the replay's err, the worse of the two volumes};
    "replay_worst": (err, key).  The 16 (volume, azimuth) pairs are independent: 16 threads share them, each with
    single-threaded torch ops."""
    group = (tuple(shape), kind, light)
    if group not in _REFERENCE:
        V = len(GPU_AZIMUTHS)
        vols = volumes(kind, shape)
        G, Gt = upstream(shape, 2, V)
        jobs = [(i, k) for i in range(2) for k in range(V)]

        def job(j):
            torch.set_num_threads(1)           # the pairs are the parallelism, not the ops: 16 threads of 16-thread ops only contend
            i, k = j
            return (orbit_grad_view_cases_fp64(vols[i], GPU_AZIMUTHS[k], G[i, k], Gt[i, k], lights=(light,)),
                    orbit_replay_view_cases(vols[i], GPU_AZIMUTHS[k], G[i, k], Gt[i, k], lights=(light,)))
        import torch
        threads = torch.get_num_threads()
        try:
            with ThreadPoolExecutor(max_workers=16) as pool:
                done = list(pool.map(job, jobs))
        finally:
            torch.set_num_threads(threads)     # (the workers' setting reaches the calling thread's)
        ref, rep = {}, {}
        for (i, k), (r64, r32) in zip(jobs, done):
            for (sv, sl, _), (dg, dt) in r64.items():
                for combo, d in (("both", dg + dt), ("image", dg), ("trans", dt)):
                    key = (sv, sl, combo)
                    ref.setdefault(key, np.zeros((2,) + tuple(shape)))[i] += d
                    rep.setdefault(key, np.zeros((2,) + tuple(shape)))[i] += r32[sv, sl, light, combo].astype(np.float64)
        replay, worst = {}, (0.0, None)
        for key, want in ref.items():
            sv, sl, combo = key
            e = 0.0
            for i in range(2):
                g, gt = combo_grads(combo, G[i], Gt[i])
                e = max(e, err(rep[key][i], want[i], V, g, gt, sv, sl, AMBIENT, GAIN, light))
            replay[key] = e
            if e > worst[0]:
                worst = (e, key)
        _REFERENCE[group] = {"vols": vols, "G": G, "Gt": Gt, "ref": ref, "replay": replay, "replay_worst": worst}
    return _REFERENCE[group]
