"""numpy oracle of the orbit render, written from the rule in SPEC_3D.md section 10 "Orbit views" (not from the kernel).

orbit_cos_sin          : the angle rule (remainder in double, exact quarter turns, one cast to fp32).
orbit_samples_fp64     : rho_s[s,y,x'], the S bilinear samples of every ray, positions and weights in float64.
render_orbit_fp64      : render_fp64 (tests/render_oracle.py) over those samples -- the reference of every test.
render_orbit_lights_fp64 : the same images for several lights at once, sharing tau and alpha (what the GPU test calls: 8 azimuths x
                         4 sigma pairs x 3 lights per volume); tests/test_render_orbit_host.py holds it equal to render_orbit_fp64.
render_orbit_fp32_replay : the rule in float32 as the spec words it -- positions c + (a cos + t sin) with one rounding per operation, the
                         four-tap interpolation in the stated order, the light prefix formed on the voxel grid by a running fp32 sum
                         and interpolated with the samples' weights, s ascending.  What fp32 alone costs against the fp64 rule.
Also the shapes, azimuths and volumes shared by tests/test_render_orbit_host.py and tests/test_hip_render_orbit.py.
"""
import math

import numpy as np

from render_oracle import SIGMAS, density, render_fp64  # noqa: F401  (SIGMAS, density: re-exported to the tests)

ORBIT_LIGHTS = ("none", "+y", "-y")
HOST_SHAPES = [(3, 5, 7), (5, 33, 36), (24, 70, 64), (64, 40, 48)]                                   # (D, H, W): the replay's cases
HOST_AZIMUTHS = (0.0, 90.0, 37.5, -123.0, 200.25)
GPU_SHAPES = [(1, 1, 1), (3, 5, 7), (6, 5, 8), (5, 33, 36), (24, 70, 64), (64, 40, 48), (16, 64, 130)]
GPU_AZIMUTHS = (0.0, 90.0, 180.0, 270.0, 37.5, -123.0, 200.25, 720.001)
AMBIENT = 0.25


def orbit_samples_count(D, W):
    """S: the smallest integer >= hypot(D, W) with the parity of D."""
    q = D * D + W * W
    s = math.isqrt(q)
    if s * s < q:
        s += 1
    return s + ((s - D) % 2)


def orbit_cos_sin(phi):
    """(cos, sin) as float32: r = remainder(phi, 360) in double; a multiple of 90 is exact, anything else cos / sin of radians(r)."""
    r = math.remainder(float(phi), 360.0)
    if r % 90.0 == 0.0:
        c, s = {-2: (-1.0, 0.0), -1: (0.0, -1.0), 0: (1.0, 0.0), 1: (0.0, 1.0), 2: (-1.0, 0.0)}[int(r // 90.0)]
    else:
        c, s = math.cos(math.radians(r)), math.sin(math.radians(r))
    return np.float32(c), np.float32(s)


def _positions(D, W, phi, dtype):
    """(z, x) [S, W] of every sample of every image column, every operation in `dtype`."""
    S = orbit_samples_count(D, W)
    c, s = (dtype(v) for v in orbit_cos_sin(phi))
    cz, cx, tc = dtype((D - 1) / 2), dtype((W - 1) / 2), dtype((S - 1) / 2)
    a = (np.arange(W).astype(dtype) - cx)[None, :]
    t = (np.arange(S).astype(dtype) - tc)[:, None]
    x = cx + (a * c + t * s)
    z = cz + (t * c - a * s)
    assert x.dtype == dtype and z.dtype == dtype
    return z, x


def _interpolate(field, z, x):
    """field [D,H,W] at the positions (z, x) [S,W] -> [S,H,W]; neighbours outside the field count as 0.  In field's dtype."""
    D, H, W = field.shape
    dtype = field.dtype.type
    z0, x0 = np.floor(z), np.floor(x)
    fz, fx = (z - z0)[..., None], (x - x0)[..., None]
    zi, xi = z0.astype(np.int64), x0.astype(np.int64)
    padded = np.zeros((D + 2, W + 2, H), field.dtype)                                             # a border of zeros: what lies outside
    padded[1:-1, 1:-1] = np.moveaxis(field, 1, 2)

    def tap(dz, dx):
        return padded[np.clip(zi + dz, -1, D) + 1, np.clip(xi + dx, -1, W) + 1]                   # [S, W, H]

    one = dtype(1)
    gx = one - fx
    out = (one - fz) * (gx * tap(0, 0) + fx * tap(0, 1)) + fz * (gx * tap(1, 0) + fx * tap(1, 1))
    assert out.dtype == field.dtype
    return np.moveaxis(out, 2, 1)


def orbit_samples_fp64(rho, phi):
    """rho [D,H,W] -> rho_s [S,H,W] in float64."""
    rho = np.asarray(rho, np.float64)
    z, x = _positions(rho.shape[0], rho.shape[2], phi, np.float64)
    return _interpolate(rho, z, x)


def render_orbit_fp64(rho, phi, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [D,H,W] -> (image [H,W], transmittance [H,W]) in float64: section 10's rule over the samples, s in the role of z."""
    if light not in ORBIT_LIGHTS:
        raise ValueError(light)
    return render_fp64(orbit_samples_fp64(rho, phi), sigma_view, sigma_light, ambient, gain, light)


def render_orbit_lights_fp64(rho_s, sigma_view, sigma_light, ambient=0.25, gain=1.0, lights=ORBIT_LIGHTS):
    """({light: image}, transmittance) from the samples rho_s [S,H,W]: render_fp64's formulas with tau and alpha formed once."""
    rho_s = np.asarray(rho_s, np.float64)
    inc = np.cumsum(rho_s, axis=0)
    base = -np.expm1(-sigma_view * rho_s) * np.exp(-sigma_view * (inc - rho_s))
    images = {}
    for light in lights:
        if light == "none":
            images[light] = gain * base.sum(axis=0)
            continue
        r = rho_s if light == "+y" else rho_s[:, ::-1]
        A = np.cumsum(r, axis=1) - r
        A = A if light == "+y" else A[:, ::-1]
        images[light] = gain * (base * (ambient + (1.0 - ambient) * np.exp(-sigma_light * A))).sum(axis=0)
    return images, np.exp(-sigma_view * inc[-1])


def _running(x, axis):
    """The exclusive running sum of a float32 array along `axis`, formed by one sequential fp32 addition per element."""
    inc = np.add.accumulate(x, axis=axis, dtype=np.float32)
    out = np.zeros_like(x)
    dst = [slice(None)] * x.ndim
    src = [slice(None)] * x.ndim
    dst[axis], src[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = inc[tuple(src)]
    return out, inc


def orbit_replay_samples(rho, phi, lights=ORBIT_LIGHTS):
    """(rho_s, {light: A_s}) in float32: what render_orbit_fp32_replay marches over (independent of the sigmas)."""
    rho = np.ascontiguousarray(rho, np.float32)
    z, x = _positions(rho.shape[0], rho.shape[2], phi, np.float32)
    A = {}
    for light in lights:
        if light == "none":
            continue
        r = rho if light == "+y" else rho[:, ::-1]
        pre = _running(np.ascontiguousarray(r), 1)[0]
        A[light] = _interpolate(np.ascontiguousarray(pre if light == "+y" else pre[:, ::-1]), z, x)
    return _interpolate(rho, z, x), A


def replay_lights_from_samples(rho_s, A_s, sigma_view, sigma_light, ambient=0.25, gain=1.0):
    """The march in float32, s ascending: every product, sum and exp one fp32 operation.  A_s: {light: samples of the prefix}
    (orbit_replay_samples); "none" is always formed.  -> ({light: image}, transmittance)."""
    f = np.float32
    nsv, nsl, a, oma, g = f(-sigma_view), f(-sigma_light), f(ambient), f(1.0 - ambient), f(gain)
    tau, total = _running(rho_s, 0)
    alpha = -np.expm1(nsv * rho_s)
    T = np.exp(nsv * tau)
    images = {}
    for light in ("none",) + tuple(A_s):
        L = a + oma * np.exp(nsl * A_s[light]) if light != "none" else f(1)
        term = (alpha * L) * T
        assert term.dtype == np.float32
        images[light] = (g * np.add.accumulate(term, axis=0, dtype=np.float32)[-1]).astype(f)
    return images, np.exp(nsv * total[-1]).astype(f)


def replay_from_samples(rho_s, A_s, sigma_view, sigma_light, ambient=0.25, gain=1.0, light="none"):
    """One light of replay_lights_from_samples; A_s None: unlit."""
    images, T = replay_lights_from_samples(rho_s, {} if A_s is None else {light: A_s}, sigma_view, sigma_light, ambient, gain)
    return images["none" if A_s is None else light], T


def render_orbit_fp32_replay(rho, phi, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [D,H,W] -> (image, transmittance) in float32 by the rule's own arithmetic."""
    if light not in ORBIT_LIGHTS:
        raise ValueError(light)
    rho_s, A = orbit_replay_samples(rho, phi, lights=(light,))
    return replay_from_samples(rho_s, A.get(light), sigma_view, sigma_light, ambient, gain, light)


def volumes(kind, shape, n=2):
    """n different volumes [n,D,H,W] of one density kind (seeds 0, 1, ...)."""
    return np.stack([density(kind, shape, seed=i) for i in range(n)])
