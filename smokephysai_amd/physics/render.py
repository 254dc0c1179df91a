"""Front-view render of smoke volumes [D,H,W] to frames [H,W] on MI355X (SPEC_3D.md section 10; csrc/render.hip, smk_volume_render).

The camera looks along +z (plane 0 nearest); single scattering from one directional light.  No reference counterpart: the reference is
2-D, and its frames are what this operator makes of a 3-D density field.  No CPU path: the numpy form of the rule is the test oracle
(tests/render_oracle.py).  render_volumes is differentiable with respect to the volumes: smk_volume_render_backward, the closed-form
transpose of the rule (section 10, "Gradient"; oracle: tests/render_grad_oracle.py).

render_orbit turns that camera about the vertical axis y (section 10, "Orbit views"; csrc/render_orbit.hip, smk_volume_render_orbit;
oracle: tests/render_orbit_oracle.py): any azimuth, several views per call, forward only.

render_camera adds an elevation to that camera (section 10, "Free camera"; csrc/render_camera.hip, smk_volume_render_camera; oracle:
tests/render_camera_oracle.py): azimuth and elevation paired view by view, trilinear samples, forward only.
"""
import ctypes as C
import math
import numbers
from dataclasses import dataclass
from typing import Optional

import torch

from .. import _lib

MAX_DEPTH = 64             # csrc/render.h RENDER_MAX_DEPTH: one lane keeps the light sum of every plane in registers
SEGMENT_ROWS = 16          # csrc/render.h RENDER_SEG_ROWS: rows per segment of the +-y light prefix (0 would mean: no row segments)
MAX_CELLS = 2 ** 31 - 2 ** 16
LIGHTS = {"none": _lib.SMK_LIGHT_NONE, "+y": _lib.SMK_LIGHT_POS_Y, "-y": _lib.SMK_LIGHT_NEG_Y, "+z": _lib.SMK_LIGHT_POS_Z}


@dataclass(frozen=True)
class RenderSettings:
    """sigma_view / sigma_light: extinction per unit density along the view / light ray; ambient: the share of the light no smoke shadows;
    gain: scale of the image; light: the light's direction of travel.  "-y" is light from above: buoyancy acts along +y (SPEC_3D.md 6.1)."""
    sigma_view: float = 0.1
    sigma_light: float = 0.1
    ambient: float = 0.25
    gain: float = 1.0
    light: str = "-y"

    def __post_init__(self):
        for name in ("sigma_view", "sigma_light"):
            v = getattr(self, name)
            if not isinstance(v, numbers.Real) or isinstance(v, bool) or not math.isfinite(v) or v < 0:
                raise ValueError(f"RenderSettings.{name}={v!r}: a finite number >= 0")
        a = self.ambient
        if not isinstance(a, numbers.Real) or isinstance(a, bool) or not (0 <= a <= 1):
            raise ValueError(f"RenderSettings.ambient={a!r}: a number in [0, 1]")
        g = self.gain
        if not isinstance(g, numbers.Real) or isinstance(g, bool) or not math.isfinite(g) or g <= 0:
            raise ValueError(f"RenderSettings.gain={g!r}: a finite number > 0")
        if self.light not in LIGHTS:
            raise ValueError(f"RenderSettings.light={self.light!r}: one of {sorted(LIGHTS)}")

    def desc(self) -> "_lib.SmkRenderDesc":
        return _lib.SmkRenderDesc(float(self.sigma_view), float(self.sigma_light), float(self.ambient), float(self.gain), LIGHTS[self.light])


def render_supported(D: int, H: int, W: int) -> bool:
    """Whether smk_volume_render takes volumes of this shape: 1 <= D <= 64, H, W >= 1, D*H*W <= 2^31 - 2^16."""
    for v in (D, H, W):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"render_supported: integer extents, got {v!r}")
    return 1 <= D <= MAX_DEPTH and H >= 1 and W >= 1 and D * H * W <= MAX_CELLS


def render_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none);
    reusable across calls on one stream."""
    if light not in LIGHTS:
        raise ValueError(f"light={light!r}: one of {sorted(LIGHTS)}")
    d, h, w = shape
    if n < 1 or not render_supported(int(d), int(h), int(w)):
        raise ValueError(f"render_volumes: n={n}, shape={tuple(shape)} is not supported (n >= 1, 1 <= D <= {MAX_DEPTH}, H, W >= 1, "
                         f"at most 2^31 - 2^16 cells)")
    nbytes = _lib.load().smk_volume_render_workspace(n, d, h, w, LIGHTS[light])
    if nbytes < 0:
        raise ValueError(f"render_volumes: n={n}, shape={tuple(shape)}, light={light!r} is not supported")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _dense(v: torch.Tensor) -> bool:
    """The last three dimensions are one dense [D][H][W] block."""
    want = 1
    for size, stride in zip(reversed(v.shape[-3:]), reversed(v.stride()[-3:])):
        if size != 1 and stride != want:
            return False
        want *= size
    return True


def _runs(lead_shape, lead_stride, cells):
    """The leading (batch) dimensions as a list of (element offset, count, stride) runs of equally spaced volumes."""
    dims = [(s, st) for s, st in zip(lead_shape, lead_stride) if s != 1]
    while len(dims) > 1 and dims[-2][1] == dims[-1][0] * dims[-1][1]:          # two dimensions that are one arithmetic progression
        (s0, _), (s1, st1) = dims[-2], dims[-1]
        dims[-2:] = [(s0 * s1, st1)]
    if not dims:
        return [(0, 1, cells)]
    runs = [(0,)]
    for s, st in dims[:-1]:
        runs = [(r[0] + i * st,) for r in runs for i in range(s)]
    return [(r[0], dims[-1][0], dims[-1][1]) for r in runs]


def render_backward_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_backward wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none:
    "none" and "+z"); reusable across calls on one stream."""
    if light not in LIGHTS:
        raise ValueError(f"light={light!r}: one of {sorted(LIGHTS)}")
    d, h, w = shape
    if n < 1 or not render_supported(int(d), int(h), int(w)):
        raise ValueError(f"render_volumes: n={n}, shape={tuple(shape)} is not supported (n >= 1, 1 <= D <= {MAX_DEPTH}, H, W >= 1, "
                         f"at most 2^31 - 2^16 cells)")
    nbytes = _lib.load().smk_volume_render_backward_workspace(n, d, h, w, LIGHTS[light])
    if nbytes < 0:
        raise ValueError(f"render_volumes: n={n}, shape={tuple(shape)}, light={light!r} is not supported")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _render_backward(vols: torch.Tensor, settings: RenderSettings, grad_image, grad_trans) -> torch.Tensor:
    """smk_volume_render_backward over the runs of `vols` (checked by render_volumes): the gradient in vols' shape, contiguous.
    grad_image / grad_trans: the leading dimensions + [H, W], or None (= zero); not both None."""
    dev = vols.device
    D, H, W = (int(s) for s in vols.shape[-3:])
    lead = tuple(vols.shape[:-3])
    cells, HW = D * H * W, H * W
    gi = None if grad_image is None else grad_image.to(torch.float32).contiguous()
    gt = None if grad_trans is None else grad_trans.to(torch.float32).contiguous()
    grad = torch.empty(lead + (D, H, W), dtype=torch.float32, device=dev)           # every element is written exactly once
    runs = _runs(lead, vols.stride()[:-3], cells)
    biggest = max(r[1] for r in runs)
    L = _lib.load()
    need = L.smk_volume_render_backward_workspace(biggest, D, H, W, LIGHTS[settings.light])
    if need < 0:
        raise ValueError(f"render_volumes: {biggest} volumes of {(D, H, W)} are not supported")
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
    desc = settings.desc()
    st = _lib.stream_ptr(dev)
    base, gbase = vols.data_ptr(), grad.data_ptr()
    ibase, tbase = (0 if gi is None else gi.data_ptr()), (0 if gt is None else gt.data_ptr())
    done = 0
    for off, count, stride in runs:
        _lib.check(L.smk_volume_render_backward(base + 4 * off, stride if count > 1 else cells, count, D, H, W, C.byref(desc),
                                                (ibase + 4 * done * HW) if gi is not None else None, HW,
                                                (tbase + 4 * done * HW) if gt is not None else None, HW,
                                                gbase + 4 * done * cells, cells, ws.data_ptr() if need else None, need, st))
        done += count
    return grad


class _RenderVolumes(torch.autograd.Function):
    """render_volumes with a backward: the forward is the plain call (the same values bit for bit), the backward is
    smk_volume_render_backward on the saved volumes.  Differentiable once."""

    @staticmethod
    def forward(ctx, vols, settings, transmittance, workspace):
        ctx.settings = settings
        ctx.set_materialize_grads(False)           # an unused output's gradient arrives as None: the NULL of the entry point
        ctx.save_for_backward(vols)
        return _render(vols, settings, transmittance=transmittance, out=None, workspace=workspace)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_image, grad_trans=None):
        (vols,) = ctx.saved_tensors
        if grad_image is None and grad_trans is None:
            return None, None, None, None
        return _render_backward(vols, ctx.settings, grad_image, grad_trans), None, None, None


def render_volumes(vols: torch.Tensor, settings: Optional[RenderSettings] = None, *, transmittance: bool = False,
                   out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Render [D,H,W], [n,D,H,W] or [B,T,D,H,W] float32 volumes on the device.  The batch dimensions may have any non-negative strides;
    every volume must be dense.  Returns the image with the leading dimensions kept ([H,W], [n,H,W], [B,T,H,W]), or
    (image, transmittance).  out: a contiguous float32 tensor of the image's shape to write into.  workspace: render_workspace(...) of at
    least this call's size, to reuse across calls.

    Differentiable with respect to the volumes (SPEC_3D.md section 10, "Gradient"; smk_volume_render_backward): when autograd is on and
    `vols.requires_grad`, the outputs carry a backward that takes the gradients of the image and, with transmittance=True, of the
    transmittance, and returns a gradient of vols' shape.  `out=` raises ValueError then (an autograd output cannot be the caller's
    buffer), and a second derivative is not supported (RuntimeError from autograd).  Every other call is the plain path."""
    if torch.is_grad_enabled() and isinstance(vols, torch.Tensor) and vols.requires_grad:
        if out is not None:
            raise ValueError("render_volumes: out= cannot be used when the volumes require a gradient (an autograd output cannot be the "
                             "caller's buffer); call under torch.no_grad() or detach the volumes")
        settings = RenderSettings() if settings is None else settings
        if not isinstance(settings, RenderSettings):
            raise TypeError("render_volumes: settings must be a RenderSettings")
        return _RenderVolumes.apply(vols, settings, bool(transmittance), workspace)
    return _render(vols, settings, transmittance=transmittance, out=out, workspace=workspace)


def _render(vols, settings, *, transmittance, out, workspace):
    """The plain path of render_volumes (its checks and the calls of smk_volume_render)."""
    settings = RenderSettings() if settings is None else settings
    if not isinstance(settings, RenderSettings):
        raise TypeError("render_volumes: settings must be a RenderSettings")
    dev = _lib.require_cuda(vols.device, "render_volumes")
    if vols.dim() not in (3, 4, 5) or vols.dtype != torch.float32:
        raise ValueError("render_volumes: float32 [D,H,W], [n,D,H,W] or [B,T,D,H,W]")
    D, H, W = (int(s) for s in vols.shape[-3:])
    lead = tuple(vols.shape[:-3])
    n = math.prod(lead)
    if n < 1 or not render_supported(D, H, W):
        raise ValueError(f"render_volumes: shape {tuple(vols.shape)} is not supported (at least one volume, 1 <= D <= {MAX_DEPTH}, H, W >= 1, "
                         f"at most 2^31 - 2^16 cells per volume)")
    if not _dense(vols):
        raise ValueError("render_volumes: every volume must be dense ([D][H][W] with strides (H*W, W, 1)); only the batch may be strided")
    if any(st < 0 for st in vols.stride()[:-3]):
        raise ValueError("render_volumes: negative batch strides")
    if out is None:
        out = torch.empty(lead + (H, W), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != lead + (H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"render_volumes: out must be a contiguous float32 tensor of shape {lead + (H, W)} on {dev}")
    trans = torch.empty(lead + (H, W), dtype=torch.float32, device=dev) if transmittance else None
    cells, HW = D * H * W, H * W
    runs = _runs(lead, vols.stride()[:-3], cells)
    biggest = max(r[1] for r in runs)
    L = _lib.load()
    need = L.smk_volume_render_workspace(biggest, D, H, W, LIGHTS[settings.light])
    if need < 0:
        raise ValueError(f"render_volumes: {biggest} volumes of {(D, H, W)} are not supported")
    if need and workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    if need and (workspace.device != dev or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need):
        raise ValueError(f"render_volumes: workspace of {need} bytes needed on {dev} (render_workspace)")
    desc = settings.desc()
    st = _lib.stream_ptr(dev)
    base, obase, tbase = vols.data_ptr(), out.data_ptr(), trans.data_ptr() if transmittance else 0
    done = 0
    for off, count, stride in runs:
        _lib.check(L.smk_volume_render(base + 4 * off, stride if count > 1 else cells, count, D, H, W, C.byref(desc),
                                       obase + 4 * done * HW, HW, (tbase + 4 * done * HW) if transmittance else None, HW,
                                       workspace.data_ptr() if need else None, workspace.numel() * workspace.element_size() if need else 0, st))
        done += count
    return (out, trans) if transmittance else out


# ---- orbit views (SPEC_3D.md section 10, "Orbit views"; csrc/render_orbit.hip, smk_volume_render_orbit) ------------------------------
ORBIT_MAX_WIDTH = 1024     # csrc/orbit_plan.h ORBIT_MAX_WIDTH
ORBIT_LIGHTS = ("none", "+y", "-y")


def orbit_supported(D: int, H: int, W: int) -> bool:
    """Whether smk_volume_render_orbit takes volumes of this shape: 1 <= D <= 64, H >= 1, 1 <= W <= 1024, D*H*W <= 2^31 - 2^16."""
    for v in (D, H, W):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"orbit_supported: integer extents, got {v!r}")
    return 1 <= D <= MAX_DEPTH and H >= 1 and 1 <= W <= ORBIT_MAX_WIDTH and D * H * W <= MAX_CELLS


def orbit_samples(D: int, W: int) -> int:
    """S, the samples on a ray of an orbit view: the smallest integer >= hypot(D, W) with the parity of D (csrc/orbit_plan.h)."""
    if D < 1 or W < 1:
        raise ValueError(f"orbit_samples: D, W >= 1, got {(D, W)}")
    q = D * D + W * W
    s = math.isqrt(q)
    s += s * s < q
    return s + ((s - D) & 1)


def orbit_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_orbit wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none:
    "none"; the prefix along y, n*D*H*W floats, under "+y" / "-y"); the same for any number of views; reusable on one stream."""
    if light not in ORBIT_LIGHTS:
        raise ValueError(f"render_orbit: light={light!r}: one of {list(ORBIT_LIGHTS)} (a world-fixed '+z' light is not built for orbit views)")
    d, h, w = (int(s) for s in shape)
    if n < 1 or not orbit_supported(d, h, w):
        raise ValueError(f"render_orbit: n={n}, shape={tuple(shape)} is not supported (n >= 1, 1 <= D <= {MAX_DEPTH}, H >= 1, "
                         f"1 <= W <= {ORBIT_MAX_WIDTH}, at most 2^31 - 2^16 cells)")
    nbytes = _lib.load().smk_volume_render_orbit_workspace(n, d, h, w, LIGHTS[light])
    if nbytes < 0:
        raise ValueError(f"render_orbit: n={n}, shape={tuple(shape)}, light={light!r} is not supported")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _azimuths(azimuth, n: int):
    """azimuth in one of its three forms -> ([n][V] doubles on the host as a float64 tensor, whether the result has a view dimension)."""
    if isinstance(azimuth, bool):
        raise ValueError("render_orbit: azimuth is a number of degrees, a sequence of them or an [n, V] array")
    try:
        t = azimuth.detach().to("cpu", torch.float64) if isinstance(azimuth, torch.Tensor) else torch.as_tensor(azimuth, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"render_orbit: azimuth is a number of degrees, a sequence of them or an [n, V] array ({e})") from None
    if t.dim() == 0:
        table, views = t.reshape(1, 1).expand(n, 1), False
    elif t.dim() == 1 and t.numel() >= 1:
        table, views = t.reshape(1, -1).expand(n, t.numel()), True
    elif t.dim() == 2 and t.shape[0] == n and t.shape[1] >= 1:
        table, views = t, True
    else:
        raise ValueError(f"render_orbit: azimuth of shape {tuple(t.shape)}: a number, a sequence of V >= 1 numbers or an [n={n}, V] array")
    if not bool(torch.isfinite(table).all()):
        raise ValueError("render_orbit: azimuths must be finite numbers of degrees")
    return table.contiguous(), views


def render_orbit(vols: torch.Tensor, azimuth, settings: Optional[RenderSettings] = None, *, transmittance: bool = False,
                 out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Render [n,D,H,W] or [D,H,W] float32 volumes from an orthographic camera that orbits the vertical axis y (SPEC_3D.md section 10,
    "Orbit views").  azimuth, in degrees (0: the front view of render_volumes; positive turns the viewing direction from +z toward +x):
      a number                  -> [n,H,W]    ([H,W] for one [D,H,W] volume)
      a sequence of V numbers   -> [n,V,H,W]  ([V,H,W]), the same views of every volume
      an [n,V] array or tensor  -> [n,V,H,W], one list per volume
    Returns the image, or (image, transmittance).  The batch may have any non-negative stride; every volume must be dense.  Lights:
    "none", "+y", "-y" ("+z" raises ValueError).  out: a contiguous float32 tensor of the image's shape to write into.  workspace:
    orbit_workspace(...) of at least this call's size.  One call renders all the views.  There is no backward yet: volumes that require a
    gradient raise RuntimeError (call under torch.no_grad() or detach them)."""
    settings = RenderSettings() if settings is None else settings
    if not isinstance(settings, RenderSettings):
        raise TypeError("render_orbit: settings must be a RenderSettings")
    if settings.light not in ORBIT_LIGHTS:
        raise ValueError(f"render_orbit: light={settings.light!r} is not built for orbit views (a world-fixed +z light seen obliquely is "
                         f"another prefix); one of {list(ORBIT_LIGHTS)}")
    if not isinstance(vols, torch.Tensor) or vols.dim() not in (3, 4) or vols.dtype != torch.float32:
        raise ValueError("render_orbit: float32 [D,H,W] or [n,D,H,W]")
    D, H, W = (int(s) for s in vols.shape[-3:])
    lead = tuple(vols.shape[:-3])
    n = math.prod(lead)
    if n < 1:
        raise ValueError(f"render_orbit: shape {tuple(vols.shape)}: at least one volume")
    table, views = _azimuths(azimuth, n)
    V = int(table.shape[1])
    if torch.is_grad_enabled() and vols.requires_grad:
        raise RuntimeError("render_orbit: the orbit render has no backward yet, and the volumes require a gradient; call under "
                           "torch.no_grad() or detach them (render_volumes, the front view, is differentiable)")
    dev = _lib.require_cuda(vols.device, "render_orbit")
    if not orbit_supported(D, H, W):
        raise ValueError(f"render_orbit: shape {tuple(vols.shape)} is not supported (1 <= D <= {MAX_DEPTH}, H >= 1, 1 <= W <= {ORBIT_MAX_WIDTH}, "
                         f"at most 2^31 - 2^16 cells per volume)")
    if not _dense(vols):
        raise ValueError("render_orbit: every volume must be dense ([D][H][W] with strides (H*W, W, 1)); only the batch may be strided")
    if any(st < 0 for st in vols.stride()[:-3]):
        raise ValueError("render_orbit: negative batch strides")
    shape = lead + ((V,) if views else ()) + (H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"render_orbit: out must be a contiguous float32 tensor of shape {shape} on {dev}")
    trans = torch.empty(shape, dtype=torch.float32, device=dev) if transmittance else None
    cells, HW = D * H * W, H * W
    runs = _runs(lead, vols.stride()[:-3], cells)
    biggest = max(r[1] for r in runs)
    L = _lib.load()
    need = L.smk_volume_render_orbit_workspace(biggest, D, H, W, LIGHTS[settings.light])
    if need < 0:
        raise ValueError(f"render_orbit: {biggest} volumes of {(D, H, W)} are not supported")
    if need and workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    if need and (workspace.device != dev or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need):
        raise ValueError(f"render_orbit: workspace of {need} bytes needed on {dev} (orbit_workspace)")
    desc = settings.desc()
    st = _lib.stream_ptr(dev)
    base, obase, tbase = vols.data_ptr(), out.data_ptr(), trans.data_ptr() if transmittance else 0
    flat = table.reshape(-1).tolist()
    done = 0
    for off, count, stride in runs:
        az = (C.c_double * (count * V))(*flat[done * V:(done + count) * V])
        _lib.check(L.smk_volume_render_orbit(base + 4 * off, stride if count > 1 else cells, count, D, H, W, C.byref(desc), az, V,
                                             obase + 4 * done * V * HW, HW, (tbase + 4 * done * V * HW) if transmittance else None, HW,
                                             workspace.data_ptr() if need else None, workspace.numel() * workspace.element_size() if need else 0,
                                             st))
        done += count
    return (out, trans) if transmittance else out


# ---- free camera (SPEC_3D.md section 10, "Free camera"; csrc/render_camera.hip, smk_volume_render_camera) -----------------------------
CAMERA_MAX_WIDTH = 1024    # csrc/camera_plan.h CAMERA_MAX_WIDTH
CAMERA_MAX_HEIGHT = 65536  # csrc/camera_plan.h CAMERA_MAX_HEIGHT: the image row enters the fp32 positions
CAMERA_LIGHTS = ORBIT_LIGHTS


def camera_supported(D: int, H: int, W: int) -> bool:
    """Whether smk_volume_render_camera takes volumes of this shape: 1 <= D <= 64, 1 <= H <= 65536, 1 <= W <= 1024,
    D*H*W <= 2^31 - 2^16."""
    for v in (D, H, W):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"camera_supported: integer extents, got {v!r}")
    return 1 <= D <= MAX_DEPTH and 1 <= H <= CAMERA_MAX_HEIGHT and 1 <= W <= CAMERA_MAX_WIDTH and D * H * W <= MAX_CELLS


def camera_samples(D: int, H: int, W: int) -> int:
    """S, the samples on a ray of a free-camera view: the smallest integer >= sqrt(D^2 + H^2 + W^2) with the parity of D
    (csrc/camera_plan.h)."""
    if D < 1 or H < 1 or W < 1:
        raise ValueError(f"camera_samples: D, H, W >= 1, got {(D, H, W)}")
    q = D * D + H * H + W * W
    s = math.isqrt(q)
    s += s * s < q
    return s + ((s - D) & 1)


def camera_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_camera wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none:
    "none"; the prefix along y, n*D*H*W floats, under "+y" / "-y"); the same for any number of views; reusable on one stream."""
    if light not in CAMERA_LIGHTS:
        raise ValueError(f"render_camera: light={light!r}: one of {list(CAMERA_LIGHTS)} (a world-fixed '+z' light is not built for a "
                         f"moving camera)")
    d, h, w = (int(s) for s in shape)
    if n < 1 or not camera_supported(d, h, w):
        raise ValueError(f"render_camera: n={n}, shape={tuple(shape)} is not supported (n >= 1, 1 <= D <= {MAX_DEPTH}, "
                         f"1 <= H <= {CAMERA_MAX_HEIGHT}, 1 <= W <= {CAMERA_MAX_WIDTH}, at most 2^31 - 2^16 cells)")
    nbytes = _lib.load().smk_volume_render_camera_workspace(n, d, h, w, LIGHTS[light])
    if nbytes < 0:
        raise ValueError(f"render_camera: n={n}, shape={tuple(shape)}, light={light!r} is not supported")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _angle(value, n: int, name: str):
    """One angle argument in one of its three forms -> a float64 host tensor of 0, 1 ([V]) or 2 ([n, V]) dimensions."""
    forms = f"render_camera: {name} is a number of degrees, a sequence of them or an [n, V] array"
    if isinstance(value, bool):
        raise ValueError(forms)
    try:
        t = value.detach().to("cpu", torch.float64) if isinstance(value, torch.Tensor) else torch.as_tensor(value, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{forms} ({e})") from None
    if not (t.dim() == 0 or (t.dim() == 1 and t.numel() >= 1) or (t.dim() == 2 and t.shape[0] == n and t.shape[1] >= 1)):
        raise ValueError(f"render_camera: {name} of shape {tuple(t.shape)}: a number, a sequence of V >= 1 numbers or an [n={n}, V] array")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"render_camera: {name}s must be finite numbers of degrees")
    return t


def _camera_angles(azimuth, elevation, n: int):
    """The two angle arguments, paired -> ([n][V] azimuths, [n][V] elevations as float64 host tensors, whether the result has a view
    dimension)."""
    az, el = _angle(azimuth, n, "azimuth"), _angle(elevation, n, "elevation")
    if bool(((el < -90.0) | (el > 90.0)).any()):
        raise ValueError("render_camera: elevations must lie in [-90, 90] degrees")
    counts = {int(t.shape[-1]) for t in (az, el) if t.dim() > 0}
    if len(counts) > 1:
        raise ValueError(f"render_camera: azimuth and elevation are paired view by view: {tuple(az.shape)} against {tuple(el.shape)}")
    V = counts.pop() if counts else 1
    tables = [(t.reshape(1, -1) if t.dim() < 2 else t).expand(n, V).contiguous() for t in (az, el)]
    return tables[0], tables[1], az.dim() > 0 or el.dim() > 0


def render_camera(vols: torch.Tensor, azimuth, elevation, settings: Optional[RenderSettings] = None, *, transmittance: bool = False,
                  out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Render [n,D,H,W] or [D,H,W] float32 volumes from an orthographic camera with an azimuth and an elevation (SPEC_3D.md section 10,
    "Free camera").  azimuth: render_orbit's, in degrees.  elevation, in degrees in [-90, 90]: positive raises the camera toward larger
    y, so that it looks down on the smoke (90: the top view).  Each of the two is
      a number                  the same for every view
      a sequence of V numbers   the same views of every volume
      an [n,V] array or tensor  one list per volume
    and they are paired view by view (two sequences have the same V), not multiplied out.  The result is [n,H,W] ([H,W] for one [D,H,W]
    volume) when both are numbers and [n,V,H,W] ([V,H,W]) otherwise.  Returns the image, or (image, transmittance).  The batch may have
    any non-negative stride; every volume must be dense.  Lights: "none", "+y", "-y", fixed to the world ("+z" raises ValueError).  out: a
    contiguous float32 tensor of the image's shape to write into.  workspace: camera_workspace(...) of at least this call's size.  One
    call renders all the views.  elevation=0 is the orbit's view on a longer ray: close to render_orbit's image, not equal to it.  There is
    no backward yet: volumes that require a gradient raise RuntimeError (call under torch.no_grad() or detach them)."""
    settings = RenderSettings() if settings is None else settings
    if not isinstance(settings, RenderSettings):
        raise TypeError("render_camera: settings must be a RenderSettings")
    if settings.light not in CAMERA_LIGHTS:
        raise ValueError(f"render_camera: light={settings.light!r} is not built for a moving camera (a world-fixed +z light seen obliquely "
                         f"is another prefix); one of {list(CAMERA_LIGHTS)}")
    if not isinstance(vols, torch.Tensor) or vols.dim() not in (3, 4) or vols.dtype != torch.float32:
        raise ValueError("render_camera: float32 [D,H,W] or [n,D,H,W]")
    D, H, W = (int(s) for s in vols.shape[-3:])
    lead = tuple(vols.shape[:-3])
    n = math.prod(lead)
    if n < 1:
        raise ValueError(f"render_camera: shape {tuple(vols.shape)}: at least one volume")
    az_table, el_table, views = _camera_angles(azimuth, elevation, n)
    V = int(az_table.shape[1])
    if torch.is_grad_enabled() and vols.requires_grad:
        raise RuntimeError("render_camera: the free-camera render has no backward yet, and the volumes require a gradient; call under "
                           "torch.no_grad() or detach them (render_volumes, the front view, is differentiable)")
    dev = _lib.require_cuda(vols.device, "render_camera")
    if not camera_supported(D, H, W):
        raise ValueError(f"render_camera: shape {tuple(vols.shape)} is not supported (1 <= D <= {MAX_DEPTH}, 1 <= H <= {CAMERA_MAX_HEIGHT}, "
                         f"1 <= W <= {CAMERA_MAX_WIDTH}, at most 2^31 - 2^16 cells per volume)")
    if not _dense(vols):
        raise ValueError("render_camera: every volume must be dense ([D][H][W] with strides (H*W, W, 1)); only the batch may be strided")
    if any(st < 0 for st in vols.stride()[:-3]):
        raise ValueError("render_camera: negative batch strides")
    shape = lead + ((V,) if views else ()) + (H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"render_camera: out must be a contiguous float32 tensor of shape {shape} on {dev}")
    trans = torch.empty(shape, dtype=torch.float32, device=dev) if transmittance else None
    cells, HW = D * H * W, H * W
    runs = _runs(lead, vols.stride()[:-3], cells)
    biggest = max(r[1] for r in runs)
    L = _lib.load()
    need = L.smk_volume_render_camera_workspace(biggest, D, H, W, LIGHTS[settings.light])
    if need < 0:
        raise ValueError(f"render_camera: {biggest} volumes of {(D, H, W)} are not supported")
    if need and workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    if need and (workspace.device != dev or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need):
        raise ValueError(f"render_camera: workspace of {need} bytes needed on {dev} (camera_workspace)")
    desc = settings.desc()
    st = _lib.stream_ptr(dev)
    base, obase, tbase = vols.data_ptr(), out.data_ptr(), trans.data_ptr() if transmittance else 0
    flat_az, flat_el = az_table.reshape(-1).tolist(), el_table.reshape(-1).tolist()
    done = 0
    for off, count, stride in runs:
        az = (C.c_double * (count * V))(*flat_az[done * V:(done + count) * V])
        el = (C.c_double * (count * V))(*flat_el[done * V:(done + count) * V])
        _lib.check(L.smk_volume_render_camera(base + 4 * off, stride if count > 1 else cells, count, D, H, W, C.byref(desc), az, el, V,
                                              obase + 4 * done * V * HW, HW, (tbase + 4 * done * V * HW) if transmittance else None, HW,
                                              workspace.data_ptr() if need else None,
                                              workspace.numel() * workspace.element_size() if need else 0, st))
        done += count
    return (out, trans) if transmittance else out
