"""numpy oracle of the front-view volume render, written from the rule in SPEC_3D.md section 10 (not from the kernels).

render_fp64        : the rule in float64 -- the reference of every test.
render_fp32_replay : the rule in float32 with the freedoms the spec leaves an implementation (a fixed summation order; the light prefix
                     along y formed per row segment: segment totals, an exclusive scan of them, a running sum inside the segment).  It
                     shows what fp32 arithmetic alone costs against the fp64 rule, which is what the device tolerance is derived from.
Also the shapes, densities and settings shared by tests/test_render_host.py and tests/test_hip_render.py.
"""
import numpy as np

LIGHTS = ("none", "+y", "-y", "+z")
SHAPES = [(1, 8, 8), (2, 8, 8), (5, 33, 36), (24, 70, 64), (64, 128, 128), (16, 300, 40)]          # (D, H, W)
SIGMAS = [(0.02, 0.05), (0.1, 0.1), (0.5, 1.0), (4.0, 8.0)]                                        # (sigma_view, sigma_light)
DENSITIES = ("sparse", "dense")
AMBIENT = 0.25


def density(kind, shape, seed=0):
    """sparse: rng.random()**8 * 1.3 (mostly near zero, as smoke); dense: rng.random() * 1.8.  float32."""
    rng = np.random.default_rng(seed)
    r = rng.random(shape)
    return ((r ** 8) * 1.3 if kind == "sparse" else r * 1.8).astype(np.float32)


def _exclusive(rho, axis, reverse=False):
    """Exclusive prefix sum along `axis`; reverse: the sum of everything AFTER the element."""
    r = np.flip(rho, axis) if reverse else rho
    c = np.cumsum(r, axis=axis) - r
    return np.flip(c, axis) if reverse else c


def light_prefix(rho, light):
    """A[z,y,x] of the rule: the density the light has crossed before it reaches the voxel."""
    if light == "none":
        return np.zeros_like(rho)
    if light == "+z":
        return _exclusive(rho, -3)
    if light == "+y":
        return _exclusive(rho, -2)
    if light == "-y":
        return _exclusive(rho, -2, reverse=True)
    raise ValueError(light)


def render_fp64(rho, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [..., D, H, W] -> (image [..., H, W], transmittance [..., H, W]) in float64."""
    rho = np.asarray(rho, np.float64)
    tau = _exclusive(rho, -3)
    A = light_prefix(rho, light)
    L = ambient + (1.0 - ambient) * np.exp(-sigma_light * A) if light != "none" else np.ones_like(rho)
    alpha = -np.expm1(-sigma_view * rho)
    image = gain * np.sum(alpha * L * np.exp(-sigma_view * tau), axis=-3)
    return image, np.exp(-sigma_view * rho.sum(axis=-3))


def render_fp32_replay(rho, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y", segment=16, expm1=True):
    """The rule in float32: every product, sum, exp one fp32 operation; z ascending; the +-y prefix per segment of `segment` rows.
    expm1=False forms alpha as 1 - exp(-x) instead (the form the spec rules out)."""
    f = np.float32
    rho = np.asarray(rho, f)
    D, H, W = rho.shape
    nsv, nsl, a, oma, g = f(-sigma_view), f(-sigma_light), f(ambient), f(1.0 - ambient), f(gain)
    A = np.zeros((D, H, W), f)
    if light in ("+y", "-y"):
        order = list(range(H)) if light == "+y" else list(range(H - 1, -1, -1))
        segs = [order[i:i + segment] for i in range(0, H, segment)]
        run = np.zeros((D, W), f)
        for rows in segs:
            acc = run.copy()                       # the scanned total of the segments before this one
            tot = np.zeros((D, W), f)
            for y in rows:
                A[:, y] = acc
                acc = acc + rho[:, y]
                tot = tot + rho[:, y]
            run = run + tot
    tau = np.zeros((H, W), f)
    img = np.zeros((H, W), f)
    for z in range(D):
        r = rho[z]
        x = nsv * r
        alpha = -np.expm1(x) if expm1 else f(1) - np.exp(x)
        Az = tau if light == "+z" else A[z]
        L = a + oma * np.exp(nsl * Az) if light != "none" else f(1)
        img = img + (alpha * L) * np.exp(nsv * tau)
        tau = tau + r
    return (g * img).astype(f), np.exp(nsv * tau).astype(f)
