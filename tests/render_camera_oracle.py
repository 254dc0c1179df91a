"""numpy oracle of the free-camera render, written from the rule in SPEC_3D.md section 10 "Free camera" (not from the kernel).

camera_samples_count   : S, the samples on a ray.
camera_coefficients    : the angle rule -> the nine view coefficients (right, up, view) as float32.
camera_grid            : the positions of every sample of every pixel in one dtype, as tap indices and weights; it depends on the shape and
                         the view only, so one grid serves every volume and every field (rho, the light prefixes) seen from that view.
camera_samples_fp64    : rho_s[s,y',x'], the S trilinear samples of every ray, positions and weights in float64.
camera_lights_fp64     : section 10's rule over samples rho_s and sampled prefixes A_s, for several lights at once, sharing tau and alpha.
render_camera_fp64     : the reference of every test: image and transmittance of one volume, view, setting and light in float64.
camera_replay_samples  : the rule in float32 as the spec words it -- positions with one rounding per operation, the eight-tap interpolation in
                         the stated order, the light prefix formed on the voxel grid by a running fp32 sum and interpolated like rho; the march
                         over them is replay_lights_from_samples of tests/render_orbit_oracle.py (s ascending).
reference_of_view      : everything the tests need of one view of several volumes, the samples formed once and shared by the sigma pairs
                         and the lights.
Also the shapes, views and volumes shared by tests/test_render_camera_host.py and tests/test_hip_render_camera.py.
"""
import math

import numpy as np

from conftest import rel_err
from render_oracle import SIGMAS, density, light_prefix  # noqa: F401  (SIGMAS, density: re-exported to the tests)
from render_orbit_oracle import _running, orbit_cos_sin, replay_lights_from_samples, volumes  # noqa: F401

CAMERA_LIGHTS = ("none", "+y", "-y")
AMBIENT = 0.25
# (D, H, W) and (azimuth, elevation) of the device test and of the replay's error budget
GPU_SHAPES = [(1, 1, 1), (3, 5, 7), (6, 5, 8), (5, 33, 36), (24, 70, 64), (64, 40, 48), (16, 64, 130)]
GPU_VIEWS = ((0.0, 0.0), (37.5, 30.0), (-123.0, -60.0), (200.25, 12.5), (90.0, 90.0), (0.0, -90.0), (720.001, 45.0), (45.0, 0.001))
# the smaller list the host test also walks
HOST_SHAPES = [(3, 5, 7), (6, 5, 8), (5, 33, 36), (4, 40, 6)]
HOST_VIEWS = ((0.0, 0.0), (90.0, 0.0), (37.5, 30.0), (-123.0, -60.0), (200.25, 89.999), (0.0, 90.0), (180.0, -90.0))


def camera_samples_count(D, H, W):
    """S: the smallest integer >= sqrt(D^2 + H^2 + W^2) with the parity of D."""
    q = D * D + H * H + W * W
    s = math.isqrt(q)
    if s * s < q:
        s += 1
    return s + ((s - D) % 2)


def camera_coefficients(phi, theta):
    """(r, e, d), each an (x, y, z) triple of float32: right, up (increasing image row) and view direction.  (c, s): the orbit's angle
    rule, fp32 read back as doubles; (ce, se): exact at 0, 90, -90, otherwise cos / sin of radians(theta) in double; products in double,
    one cast each."""
    theta = float(theta)
    if not math.isfinite(float(phi)) or not math.isfinite(theta) or not -90.0 <= theta <= 90.0:
        raise ValueError(f"camera angles ({phi}, {theta}): finite, elevation in [-90, 90]")
    c, s = (float(v) for v in orbit_cos_sin(phi))
    if theta == 0.0:
        ce, se = 1.0, 0.0
    elif abs(theta) == 90.0:
        ce, se = 0.0, math.copysign(1.0, theta)
    else:
        ce, se = math.cos(math.radians(theta)), math.sin(math.radians(theta))
    f = np.float32
    return (f(c), f(0.0), f(-s)), (f(s * se), f(ce), f(c * se)), (f(s * ce), f(-se), f(c * ce))


class CameraGrid:
    """Tap indices and weights of every sample [S,H,W] of one (shape, view) in one dtype.  The volume is thought padded with two planes
    of zeros on every side: a floor is clipped to [-2, N], so that both its taps are zeros whenever they lie outside the volume."""

    def __init__(self, shape, phi, theta, dtype):
        D, H, W = shape
        S = camera_samples_count(D, H, W)
        (rx, _, rz), (ex, ey, ez), (dx, dy, dz) = (tuple(dtype(v) for v in t) for t in camera_coefficients(phi, theta))
        cz, cy, cx, tc = dtype((D - 1) / 2), dtype((H - 1) / 2), dtype((W - 1) / 2), dtype((S - 1) / 2)
        a = (np.arange(W).astype(dtype) - cx)[None, None, :]
        b = (np.arange(H).astype(dtype) - cy)[None, :, None]
        t = (np.arange(S).astype(dtype) - tc)[:, None, None]
        x = cx + ((a * rx + b * ex) + t * dx)
        z = cz + ((a * rz + b * ez) + t * dz)
        y = np.broadcast_to(cy + (b * ey + t * dy), x.shape)                                      # no column enters a row's height
        assert x.dtype == dtype and y.dtype == dtype and z.dtype == dtype and x.shape == y.shape == z.shape == (S, H, W)
        z0, y0, x0 = np.floor(z), np.floor(y), np.floor(x)
        self.fz, self.fy, self.fx = z - z0, y - y0, x - x0
        self.shape, self.dtype = shape, dtype
        zi = np.clip(z0, -2, D).astype(np.int64) + 2
        yi = np.clip(y0, -2, H).astype(np.int64) + 2
        xi = np.clip(x0, -2, W).astype(np.int64) + 2
        self.base = (zi * (H + 4) + yi) * (W + 4) + xi
        self.positions = (z, y, x)

    def interpolate(self, field):
        """field [D,H,W] of the grid's dtype -> its trilinear samples [S,H,W], taps outside the field counting as 0."""
        D, H, W = self.shape
        assert field.shape == self.shape and field.dtype == self.dtype
        padded = np.zeros((D + 4, H + 4, W + 4), self.dtype)
        padded[2:-2, 2:-2, 2:-2] = field
        flat = padded.reshape(-1)
        sy, sz = W + 4, (H + 4) * (W + 4)

        def tap(dz, dy, dx):
            return flat[self.base + (dz * sz + dy * sy + dx)]

        one = self.dtype(1)
        gx, gy = one - self.fx, one - self.fy

        def plane(dz):
            return gy * (gx * tap(dz, 0, 0) + self.fx * tap(dz, 0, 1)) + self.fy * (gx * tap(dz, 1, 0) + self.fx * tap(dz, 1, 1))

        out = (one - self.fz) * plane(0) + self.fz * plane(1)
        assert out.dtype == self.dtype
        return out


def camera_grid(shape, phi, theta, dtype=np.float64):
    return CameraGrid(tuple(shape), phi, theta, dtype)


def camera_samples_fp64(rho, phi, theta, grid=None):
    """rho [D,H,W] -> rho_s [S,H,W] in float64."""
    rho = np.asarray(rho, np.float64)
    return (grid or camera_grid(rho.shape, phi, theta)).interpolate(rho)


def camera_light_samples_fp64(rho, phi, theta, lights=CAMERA_LIGHTS, grid=None):
    """{light: A_s [S,H,W]}: the interpolation of the voxel-grid exclusive prefix along y, for the lit lights among `lights`."""
    rho = np.asarray(rho, np.float64)
    grid = grid or camera_grid(rho.shape, phi, theta)
    return {light: grid.interpolate(np.ascontiguousarray(light_prefix(rho, light))) for light in lights if light != "none"}


def camera_lights_fp64(rho_s, A_s, sigma_view, sigma_light, ambient=0.25, gain=1.0):
    """({light: image}, transmittance) in float64 from the samples rho_s and the sampled prefixes A_s {light: [S,H,W]}; "none" is always
    formed.  Section 10's rule with s in the role of z."""
    rho_s = np.asarray(rho_s, np.float64)
    inc = np.cumsum(rho_s, axis=0)
    base = -np.expm1(-sigma_view * rho_s) * np.exp(-sigma_view * (inc - rho_s))
    images = {"none": gain * base.sum(axis=0)}
    for light, A in A_s.items():
        images[light] = gain * (base * (ambient + (1.0 - ambient) * np.exp(-sigma_light * A))).sum(axis=0)
    return images, np.exp(-sigma_view * inc[-1])


def render_camera_fp64(rho, phi, theta, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [D,H,W] -> (image [H,W], transmittance [H,W]) in float64."""
    if light not in CAMERA_LIGHTS:
        raise ValueError(light)
    rho = np.asarray(rho, np.float64)
    grid = camera_grid(rho.shape, phi, theta)
    images, T = camera_lights_fp64(grid.interpolate(rho), camera_light_samples_fp64(rho, phi, theta, (light,), grid), sigma_view,
                                   sigma_light, ambient, gain)
    return images[light], T


def camera_replay_samples(rho, phi, theta, lights=CAMERA_LIGHTS, grid=None):
    """(rho_s, {light: A_s}) in float32: what the replay marches over (independent of the sigmas)."""
    rho = np.ascontiguousarray(rho, np.float32)
    grid = grid or camera_grid(rho.shape, phi, theta, np.float32)
    A = {}
    for light in lights:
        if light == "none":
            continue
        r = rho if light == "+y" else rho[:, ::-1]
        pre = _running(np.ascontiguousarray(r), 1)[0]
        A[light] = grid.interpolate(np.ascontiguousarray(pre if light == "+y" else pre[:, ::-1]))
    return grid.interpolate(rho), A


def render_camera_fp32_replay(rho, phi, theta, sigma_view=0.1, sigma_light=0.1, ambient=0.25, gain=1.0, light="-y"):
    """rho [D,H,W] -> (image, transmittance) in float32 by the rule's own arithmetic."""
    if light not in CAMERA_LIGHTS:
        raise ValueError(light)
    rho_s, A = camera_replay_samples(rho, phi, theta, lights=(light,))
    images, T = replay_lights_from_samples(rho_s, A, sigma_view, sigma_light, ambient, gain)
    return images[light], T


def reference_of_view(vols, phi, theta, sigmas=SIGMAS, ambient=AMBIENT):
    """vols: a list of volumes of one shape.  -> [{(sv, sl, light): (float64 image, float64 transmittance, the replay's image error, the
    replay's transmittance error)}] per volume.  One grid per precision for all the volumes; the samples of a volume are formed once."""
    shape = vols[0].shape
    g64, g32 = camera_grid(shape, phi, theta, np.float64), camera_grid(shape, phi, theta, np.float32)
    out = []
    for vol in vols:
        v64 = np.asarray(vol, np.float64)
        s64, A64 = g64.interpolate(v64), camera_light_samples_fp64(v64, phi, theta, grid=g64)
        s32, A32 = camera_replay_samples(vol, phi, theta, grid=g32)
        res = {}
        for sv, sl in sigmas:
            images, T = camera_lights_fp64(s64, A64, sv, sl, ambient, 1.0)
            got, gotT = replay_lights_from_samples(s32, A32, sv, sl, ambient, 1.0)
            for light in CAMERA_LIGHTS:
                res[sv, sl, light] = (images[light], T, rel_err(got[light], images[light]), float(np.abs(gotT - T).max()))
        out.append(res)
    return out
