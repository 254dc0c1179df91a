"""Executable form of DESIGN.md section 8.1 "Gradient": the closed-form gradient of a plane's mean SSIM with respect to the prediction,
the reference's SSIM map (robustness_metrics.py:79-99) in whatever precision its inputs have, and the seeded inputs the SSIM-loss tests
share.  Everything runs on the CPU; planes are [n, H, W], the upstream gradient is one value per plane."""
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
SHAPES = [(1, 1), (5, 7), (16, 64), (17, 65), (37, 53), (33, 130)]
WINDOWS = [1, 3, 11, 31]
KINDS = ["uniform", "smoke", "near"]


def box(z, k):
    """avg_pool2d(z, k, stride=1, padding=k//2): zeros outside the plane, divisor always k^2 (its own transpose for odd k)."""
    return F.avg_pool2d(z[:, None], k, stride=1, padding=k // 2)[:, 0]


def ssim_map(p, t, k):
    """The reference's SSIM map of planes [n, H, W]."""
    m1, m2 = box(p, k), box(t, k)
    s11 = box(p * p, k) - m1 * m1
    s22 = box(t * t, k) - m2 * m2
    s12 = box(p * t, k) - m1 * m2
    return ((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s11 + s22 + C2))


def plane_means(p, t, k):
    """Mean SSIM of every plane, in the inputs' precision."""
    return ssim_map(p, t, k).mean((-2, -1))


def closed_form_grad(p, t, k, upstream):
    """d/dp of sum_i upstream[i] * mean(ssim_map(p, t, k)[i]) by the closed form, in the inputs' precision (float64 in the tests)."""
    H, W = p.shape[-2:]
    g = (upstream / (H * W))[:, None, None]
    mx, my = box(p, k), box(t, k)
    sxx = box(p * p, k) - mx * mx
    syy = box(t * t, k) - my * my
    sxy = box(p * t, k) - mx * my
    A1, A2 = 2 * mx * my + C1, 2 * sxy + C2
    B1, B2 = mx * mx + my * my + C1, sxx + syy + C2
    S = A1 * A2 / (B1 * B2)
    b = g * (-S / B2)                                                    # dS/dExx
    c = g * (2 * A1 / (B1 * B2))                                         # dS/dExy
    a = g * (2 * my * A2 / (B1 * B2) - 2 * mx * S / B1) - my * c - 2 * mx * b     # total dS/dmu_x
    return box(a, k) + 2 * p * box(b, k) + t * box(c, k)


def autograd_grad(p, t, k, upstream):
    """The same gradient from torch's autograd of the reference's formula, in the inputs' precision."""
    q = p.detach().clone().requires_grad_()
    (plane_means(q, t, k) * upstream.to(p.dtype)).sum().backward()
    return q.grad


def make_case(kind, n, H, W, seed):
    """(pred, target) as float32 [n, H, W], seeded."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        p = torch.rand(n, H, W, dtype=torch.float64, generator=gen)
        t = torch.rand(n, H, W, dtype=torch.float64, generator=gen)
    elif kind == "smoke":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        blob = 1.5 * torch.exp(-((yy - H / 2) ** 2 + (xx - W / 3) ** 2) / (2 * (min(H, W) / 5) ** 2))
        t = blob.expand(n, H, W).clone()
        t[t < 0.05] = 0
        p = torch.sigmoid(4 * (t - 0.5) + 0.3 * torch.randn(n, H, W, dtype=torch.float64, generator=gen))
    elif kind == "near":
        t = torch.rand(n, H, W, dtype=torch.float64, generator=gen)
        p = t + 1e-3 * torch.randn(n, H, W, dtype=torch.float64, generator=gen)
    else:
        raise ValueError(kind)
    return p.float(), t.float()


def make_upstream(n, seed):
    """Standard-normal upstream gradients [n] float32; with n >= 3 plane 1 gets an exact 0 and plane 2 a negative value."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(1000 + seed)).float()
    if n >= 3:
        g[1] = 0.0
        g[2] = -g[2].abs() - 0.25
    return g


def grad_error(d, d64):
    """max|d - d64| / max|d64|."""
    return float((d.double() - d64).abs().max() / d64.abs().max())
