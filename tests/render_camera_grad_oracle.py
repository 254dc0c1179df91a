"""Oracle of the gradient of the free-camera render, written from the rule of SPEC_3D.md section 10 "Free camera -- Gradient" (not from
the kernels, and not by differentiating anything: tests/test_render_camera_grad_host.py holds it against torch's fp64 autograd of the
forward rule).

camera_sample_grads_fp64 : Q = d(loss)/d(rho_s) and R = d(loss)/d(A_s) [S,H,W] of one view, from the samples rho_s and A_s: the front
                        view's gradient rule (render_grad_fp64's) with s in the role of z, the shadow term kept apart as R because A_s
                        is no prefix of the samples.
scatter_fp64          : B^T, the transpose of the trilinear interpolation: every sample's value added to its in-volume taps with the
                        forward's eight weights.
camera_grad_fp64      : d(loss)/d(rho) in float64: B^T Q + P_y^T (B^T R), P_y^T on the voxel grid, summed over the views.
err                   : max|d - ref| / max(max|ref|, V * s), the orbit gradient's metric (render_orbit_grad_oracle.err).
render_camera_torch   : the forward rule as torch ops in the tensor's own dtype (a gather of the eight taps combined in the rule's order,
                        the voxel-grid prefix by cumsum, interpolated like rho): what autograd replays.  In float64 it is the rule; in
                        float32, with the positions formed in fp32 exactly as the rule writes them, its autograd is the "fp32 replay".
camera_grad_view_cases_fp64 / camera_replay_view_cases : one view for all the sigma pairs and combos of the case list at once.
reference             : per group of the shared case list (a shape, a density kind, a light), computed once and left unchanged.
The shared case list: GPU_SHAPES x DENSITIES x 2 volumes x the 8 GPU_VIEWS in one call x SIGMAS x CAMERA_LIGHTS x COMBOS.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from render_camera_oracle import (AMBIENT, CAMERA_LIGHTS, GPU_SHAPES, GPU_VIEWS, HOST_SHAPES, HOST_VIEWS, SIGMAS,  # noqa: F401
                                  camera_grid, camera_samples_count, volumes)
from render_grad_oracle import GAIN
from render_oracle import DENSITIES, light_prefix
from render_orbit_grad_oracle import COMBOS, combo_grads, err, upstream  # noqa: F401  (re-exported to the tests)

BOUND = 1e-4                               # device against camera_grad_fp64 in `err`


def _excl(x, axis, reverse=False):
    r = np.flip(x, axis) if reverse else x
    c = np.cumsum(r, axis=axis) - r
    return np.flip(c, axis) if reverse else c


def _tap_list(grid):
    """The eight taps of every sample of a CameraGrid: [(offset into the padded flat volume [S,H,W], weight [S,H,W])], tap
    (dz, dy, dx) with the weight (fz | 1 - fz) (fy | 1 - fy) (fx | 1 - fx)."""
    D, H, W = grid.shape
    sy, sz = W + 4, (H + 4) * (W + 4)
    one = grid.dtype(1)
    taps = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (grid.fz if dz else one - grid.fz) * ((grid.fy if dy else one - grid.fy) * (grid.fx if dx else one - grid.fx))
                taps.append((grid.base + (dz * sz + dy * sy + dx), w))
    return taps


def scatter_fp64(d_s, grid):
    """B^T: d_s [..., S,H,W] (a gradient per sample; leading dimensions: several at once) -> [..., D,H,W].  The padding of the grid
    takes what falls outside the volume."""
    D, H, W = grid.shape
    d_s = np.asarray(d_s, np.float64)
    lead = d_s.shape[:-3]
    flat = d_s.reshape((-1,) + d_s.shape[-3:])
    cells = (D + 4) * (H + 4) * (W + 4)
    out = np.zeros((flat.shape[0], cells))
    for at, w in _tap_list(grid):
        at = at.reshape(-1)
        for i in range(flat.shape[0]):
            out[i] += np.bincount(at, weights=(w * flat[i]).reshape(-1), minlength=cells)
    return out.reshape(lead + (D + 4, H + 4, W + 4))[..., 2:-2, 2:-2, 2:-2]


def camera_sample_grads_fp64(rho_s, A_s, G, Gt, sigma_view, sigma_light, ambient, gain, light):
    """(Q, R) [S,H,W] of one view; G / Gt [H,W] or None (= zero); A_s is not looked at under "none" (R = 0)."""
    rho_s = np.asarray(rho_s, np.float64)
    gG = np.zeros(rho_s.shape[1:]) if G is None else gain * np.asarray(G, np.float64)
    gt = np.zeros(rho_s.shape[1:]) if Gt is None else np.asarray(Gt, np.float64)
    inc = np.cumsum(rho_s, axis=0)
    T, E0, alpha = np.exp(-sigma_view * (inc - rho_s)), np.exp(-sigma_view * rho_s), -np.expm1(-sigma_view * rho_s)
    if light == "none":
        L, R = 1.0, np.zeros_like(rho_s)
    else:
        X = np.exp(-sigma_light * np.asarray(A_s, np.float64))
        L = ambient + (1.0 - ambient) * X
        R = gG * alpha * T * (-sigma_light * (1.0 - ambient) * X)
    LT = L * T
    Q = gG * sigma_view * (E0 * LT - _excl(alpha * LT, 0, reverse=True)) - sigma_view * gt * np.exp(-sigma_view * inc[-1])
    return Q, R


def shadow_transpose(U, light):
    """P_y^T on the voxel grid: the sum of U over the rows y' that y shadows ("+y": y' > y, "-y": y' < y)."""
    return np.zeros_like(U) if light == "none" else _excl(U, -2, reverse=(light == "+y"))


def camera_grad_fp64(rho, views, G=None, Gt=None, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [D,H,W]; views: V (azimuth, elevation) pairs; G / Gt [V,H,W] or None (= zero) -> d(sum(image * G) + sum(transmittance * Gt)) /
    d(rho)."""
    rho = np.asarray(rho, np.float64)
    if light not in CAMERA_LIGHTS:
        raise ValueError(light)
    d = np.zeros_like(rho)
    A = np.ascontiguousarray(light_prefix(rho, light))
    for k, (phi, theta) in enumerate(views):
        grid = camera_grid(rho.shape, phi, theta)
        Q, R = camera_sample_grads_fp64(grid.interpolate(rho), grid.interpolate(A), None if G is None else G[k],
                                        None if Gt is None else Gt[k], sigma_view, sigma_light, ambient, gain, light)
        both = scatter_fp64(np.stack([Q, R]), grid)
        d += both[0] + shadow_transpose(both[1], light)
    return d


# ---- the forward rule as torch ops ----------------------------------------------------------------------------------------------------
class TorchGrid:
    """The taps and fractions of one (shape, view) as torch tensors in the dtype of the volumes they will sample (float32: positions and
    fractions formed in fp32 as the rule writes them)."""

    def __init__(self, shape, phi, theta, dtype, device="cpu"):
        import torch
        np_dtype = np.float32 if dtype == torch.float32 else np.float64
        g = camera_grid(tuple(shape), phi, theta, np_dtype)
        D, H, W = g.shape
        sy, sz = W + 4, (H + 4) * (W + 4)
        offs = np.array([dz * sz + dy * sy + dx for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], np.int64)
        self.index = torch.from_numpy((g.base[None] + offs[:, None, None, None]).reshape(-1)).to(device)     # [8 * S*H*W]
        self.f = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (g.fz, g.fy, g.fx))
        self.samples = g.fz.shape

    def interpolate(self, field):
        """field [..., D,H,W] -> its trilinear samples [..., S,H,W] in the rule's order; taps outside the field count as 0."""
        import torch.nn.functional as F
        padded = F.pad(field, (2, 2, 2, 2, 2, 2)).reshape(field.shape[:-3] + (-1,))
        v = padded.index_select(-1, self.index).reshape(field.shape[:-3] + (8,) + tuple(self.samples))
        fz, fy, fx = self.f
        gx, gy = 1 - fx, 1 - fy

        def plane(n):
            return gy * (gx * v[..., n, :, :, :] + fx * v[..., n + 1, :, :, :]) + fy * (gx * v[..., n + 2, :, :, :] + fx * v[..., n + 3, :, :, :])
        return (1 - fz) * plane(0) + fz * plane(4)


def march_torch(rho_s, A_s, sigma_view, sigma_light, ambient, gain, light):
    """Section 10's rule over samples [..., S,H,W] (A_s: the sampled prefix, not looked at under "none") -> (image, transmittance)."""
    import torch
    tau = torch.cumsum(rho_s, -3) - rho_s
    alpha = -torch.expm1(-sigma_view * rho_s)
    L = 1.0 if light == "none" else ambient + (1.0 - ambient) * torch.exp(-sigma_light * A_s)
    return gain * (alpha * L * torch.exp(-sigma_view * tau)).sum(-3), torch.exp(-sigma_view * rho_s.sum(-3))


def prefix_torch(rho, light):
    """The voxel-grid exclusive prefix along y in the light's direction of travel, [..., D,H,W]."""
    import torch
    r = torch.flip(rho, (-2,)) if light == "-y" else rho
    c = torch.cumsum(r, -2) - r
    return torch.flip(c, (-2,)) if light == "-y" else c


def render_camera_torch(rho, phi, theta, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y", grid=None):
    """The free-camera render of rho [..., D, H, W] from one view as torch ops in rho's dtype -> (image, transmittance) [..., H, W]."""
    grid = grid or TorchGrid(rho.shape[-3:], phi, theta, rho.dtype, rho.device)
    A_s = None if light == "none" else grid.interpolate(prefix_torch(rho, light))
    return march_torch(grid.interpolate(rho), A_s, sigma_view, sigma_light, ambient, gain, light)


def camera_grad_autograd(rho, views, G, Gt, sigma_view, sigma_light, ambient, gain, light, dtype):
    """torch autograd of render_camera_torch in `dtype` (torch.float64: the rule; torch.float32: the replay) -> numpy [D,H,W]."""
    import torch
    r = torch.tensor(np.asarray(rho), dtype=dtype, requires_grad=True)
    loss = 0
    for k, (phi, theta) in enumerate(views):
        img, tr = render_camera_torch(r, phi, theta, sigma_view, sigma_light, ambient, gain, light)
        if G is not None:
            loss = loss + (img * torch.tensor(np.asarray(G[k]), dtype=dtype)).sum()
        if Gt is not None:
            loss = loss + (tr * torch.tensor(np.asarray(Gt[k]), dtype=dtype)).sum()
    loss.backward()
    return r.grad.numpy()


# ---- the shared case list -------------------------------------------------------------------------------------------------------------
def camera_grad_view_cases_fp64(rho, phi, theta, G, Gt, sigmas=SIGMAS, lights=CAMERA_LIGHTS, ambient=AMBIENT, gain=GAIN):
    """One view.  rho [D,H,W], G / Gt [H,W] -> {(sv, sl, light): (gradient with G alone, gradient with Gt alone)} [D,H,W] float64: the
    samples formed once, and one scatter for everything."""
    rho = np.asarray(rho, np.float64)
    grid = camera_grid(rho.shape, phi, theta)
    rs = grid.interpolate(rho)
    As = {light: grid.interpolate(np.ascontiguousarray(light_prefix(rho, light))) for light in lights if light != "none"}
    keys, parts = [], []
    for sv, sl in sigmas:
        for light in lights:
            Qg, R = camera_sample_grads_fp64(rs, As.get(light), G, None, sv, sl, ambient, gain, light)
            Qt, _ = camera_sample_grads_fp64(rs, As.get(light), None, Gt, sv, sl, ambient, gain, light)
            keys.append((sv, sl, light))
            parts += [Qg, R, Qt]
    out = scatter_fp64(np.stack(parts), grid)
    return {key: (out[3 * i] + shadow_transpose(out[3 * i + 1], key[2]), out[3 * i + 2]) for i, key in enumerate(keys)}


def camera_replay_view_cases(rho, phi, theta, G, Gt, sigmas=SIGMAS, lights=CAMERA_LIGHTS, ambient=AMBIENT, gain=GAIN):
    """One view of the fp32 replay: {(sv, sl, light, combo): gradient [D,H,W] float32} by torch's fp32 autograd of render_camera_torch."""
    import torch
    r = torch.tensor(np.asarray(rho, np.float32), requires_grad=True)
    grid = TorchGrid(r.shape, phi, theta, torch.float32)
    rs = grid.interpolate(r)
    Gi, Gr = torch.tensor(np.asarray(G, np.float32)), torch.tensor(np.asarray(Gt, np.float32))
    res = {}
    for light in lights:
        As = None if light == "none" else grid.interpolate(prefix_torch(r, light))
        for sv, sl in sigmas:
            img, tr = march_torch(rs, As, sv, sl, ambient, gain, light)
            li, lt = (img * Gi).sum(), (tr * Gr).sum()
            for combo, loss in (("both", li + lt), ("image", li), ("trans", lt)):
                res[sv, sl, light, combo] = torch.autograd.grad(loss, r, retain_graph=True)[0].numpy()
    return res


_REFERENCE = {}
CASE_GROUPS = [(shape, kind, light) for shape in GPU_SHAPES for kind in DENSITIES for light in CAMERA_LIGHTS]


def reference(shape, kind, light):
    """One group of the case list -- a shape, a density kind, a light; its 2 volumes x 8 views x 4 sigma pairs x 3 combos -- computed
    once and left unchanged.  "vols": [2,D,H,W] float32; "G", "Gt": [2,V,H,W] float32 (the same for every group of a shape); "ref":
    {(sv, sl, combo): [2,D,H,W] float64, the views summed}; "replay": {the same key: the replay's err, the worse of the two volumes};
    "replay_worst": (err, key).  The 16 (volume, view) pairs are independent: 16 threads share them, each with single-threaded torch
    ops."""
    group = (tuple(shape), kind, light)
    if group not in _REFERENCE:
        import torch
        V = len(GPU_VIEWS)
        vols = volumes(kind, shape)
        G, Gt = upstream(shape, 2, V)
        jobs = [(i, k) for i in range(2) for k in range(V)]

        def job(j):
            torch.set_num_threads(1)           # the pairs are the parallelism, not the ops: 16 threads of 16-thread ops only contend
            i, k = j
            phi, theta = GPU_VIEWS[k]
            return (camera_grad_view_cases_fp64(vols[i], phi, theta, G[i, k], Gt[i, k], lights=(light,)),
                    camera_replay_view_cases(vols[i], phi, theta, G[i, k], Gt[i, k], lights=(light,)))
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
