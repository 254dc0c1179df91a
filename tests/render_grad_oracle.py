"""numpy oracle of the gradient of the front-view volume render, written from the "Gradient" rule of SPEC_3D.md section 10 (not from the
kernels, and not by differentiating anything: tests/test_render_grad_host.py holds it against torch's fp64 autograd of the forward rule).

render_grad_fp64 : d(loss)/d(rho) in float64 from the upstream gradients G (image) and Gt (transmittance) -- the reference of every test.
err              : the error metric of the section: max|d - ref| over max(max|ref|, s), s the size of one term of the sum.  In opaque
                   volumes the true gradient is a difference of O(1) terms that cancels to almost nothing; max|ref| alone would then
                   measure the noise of the reference.
render_torch     : the forward rule as torch ops (cumsum / flip), differentiable in any dtype: what autograd replays, and what the render
                   looks like without the kernel.
Also the shapes, settings and upstream gradients shared by tests/test_render_grad_host.py and tests/test_hip_render_grad.py.
"""
import numpy as np

from render_oracle import AMBIENT, DENSITIES, LIGHTS, SIGMAS, _exclusive, density, light_prefix        # noqa: F401  (shared case list)

# (D, H, W): the smallest at which the segment tail, the column tail, each DMAX instance and the segment scan can each go wrong
SHAPES = [(1, 8, 8), (2, 8, 8), (5, 33, 36), (24, 70, 64), (64, 64, 64), (64, 32, 130), (16, 300, 40)]
GAIN = 1.5
BOUND = 1e-5               # device against render_grad_fp64 in `err`: SPEC_3D.md section 10


def upstream(shape, seed=1):
    """G and Gt for volumes of `shape` = (..., D, H, W): standard normal float32 [..., H, W]."""
    rng = np.random.default_rng(seed)
    img = tuple(shape[:-3]) + tuple(shape[-2:])
    return rng.standard_normal(img).astype(np.float32), rng.standard_normal(img).astype(np.float32)


def render_grad_fp64(rho, G=None, Gt=None, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [..., D, H, W], G / Gt [..., H, W] or None (= zero) -> d(sum(image * G) + sum(transmittance * Gt)) / d(rho), float64."""
    rho = np.asarray(rho, np.float64)
    zero = np.zeros(rho.shape[:-3] + rho.shape[-2:])
    G = zero if G is None else np.asarray(G, np.float64)
    Gt = zero if Gt is None else np.asarray(Gt, np.float64)
    sv, sl, a, g = float(sigma_view), float(sigma_light), float(ambient), float(gain)
    gG = (g * G)[..., None, :, :]
    tau = _exclusive(rho, -3)
    T = np.exp(-sv * tau)
    A = light_prefix(rho, light)
    lit = light != "none"
    X = np.exp(-sl * A) if lit else np.zeros_like(rho)
    L = a + (1.0 - a) * X if lit else np.ones_like(rho)
    alpha = -np.expm1(-sv * rho)
    c = alpha * L * T
    trans = np.exp(-sv * rho.sum(axis=-3))
    d = gG * sv * (np.exp(-sv * rho) * L * T - _exclusive(c, -3, reverse=True))            # own absorption, and dimming of all behind
    d = d - sv * (Gt * trans)[..., None, :, :]
    if lit:
        S = gG * alpha * T * (-sl * (1.0 - a) * X)
        if light == "+z":
            d = d + _exclusive(S, -3, reverse=True)           # the voxels behind on the ray
        elif light == "+y":
            d = d + _exclusive(S, -2, reverse=True)           # the voxels at larger y
        else:
            d = d + _exclusive(S, -2)                         # "-y": the voxels at smaller y
    return d


def term_scale(G, Gt, sigma_view, sigma_light, ambient, gain, light):
    """s: the size of one term of the sum."""
    mg = 0.0 if G is None else float(np.abs(G).max())
    mt = 0.0 if Gt is None else float(np.abs(Gt).max())
    s = sigma_view * (gain * mg + mt)
    if light != "none":
        s += sigma_light * (1.0 - ambient) * gain * mg
    return s


def err(d, ref, G, Gt, sigma_view, sigma_light, ambient, gain, light):
    ref = np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), term_scale(G, Gt, sigma_view, sigma_light, ambient, gain, light))
    return float(np.abs(np.asarray(d, np.float64) - ref).max()) / scale


def render_torch(rho, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """The forward rule on a torch tensor [..., D, H, W] in its own dtype -> (image, transmittance), as cumsum / flip / exp ops."""
    import torch

    def exclusive(x, dim, reverse=False):
        r = torch.flip(x, (dim,)) if reverse else x
        c = torch.cumsum(r, dim) - r
        return torch.flip(c, (dim,)) if reverse else c
    tau = exclusive(rho, -3)
    if light == "none":
        L = torch.ones_like(rho)
    else:
        A = tau if light == "+z" else exclusive(rho, -2, reverse=(light == "-y"))
        L = ambient + (1.0 - ambient) * torch.exp(-sigma_light * A)
    alpha = -torch.expm1(-sigma_view * rho)
    image = gain * (alpha * L * torch.exp(-sigma_view * tau)).sum(-3)
    return image, torch.exp(-sigma_view * rho.sum(-3))
