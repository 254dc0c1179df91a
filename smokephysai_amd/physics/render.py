"""Front-view render of smoke volumes [D,H,W] to frames [H,W] on MI355X (SPEC_3D.md section 10; csrc/render.hip, smk_volume_render).

The camera looks along +z (plane 0 nearest); single scattering from one directional light.  No reference counterpart: the reference is
2-D, and its frames are what this operator makes of a 3-D density field.  No CPU path: the numpy form of the rule is the test oracle
(tests/render_oracle.py).  render_volumes is differentiable with respect to the volumes: smk_volume_render_backward, the closed-form
transpose of the rule (section 10, "Gradient"; oracle: tests/render_grad_oracle.py).

render_orbit turns that camera about the vertical axis y (section 10, "Orbit views"; csrc/render_orbit.hip, smk_volume_render_orbit;
oracle: tests/render_orbit_oracle.py): any azimuth, several views per call.  With differentiable=True it carries a backward with respect to
the volumes: smk_volume_render_orbit_backward (csrc/render_orbit_grad.hip), the front view's gradient rule over the samples followed by the
transpose of the interpolation, summed over the views (section 10, "Orbit views -- Gradient"; oracle: tests/render_orbit_grad_oracle.py).

render_camera adds an elevation to that camera (section 10, "Free camera"; csrc/render_camera.hip, smk_volume_render_camera; oracle:
tests/render_camera_oracle.py): azimuth and elevation paired view by view, trilinear samples.  With differentiable=True it carries a
backward too: smk_volume_render_camera_backward (csrc/render_camera_grad.hip; section 10, "Free camera -- Gradient"; oracle:
tests/render_camera_grad_oracle.py).
"""
import ctypes as C
import math
import numbers
from dataclasses import dataclass
from typing import NamedTuple, Optional

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




# ---- what the three renderers share: limits, workspaces, the checked call ------------------------------------------------------------
ORBIT_MAX_WIDTH = 1024     # csrc/orbit_plan.h ORBIT_MAX_WIDTH
ORBIT_LIGHTS = ("none", "+y", "-y")
CAMERA_MAX_WIDTH = 1024    # csrc/camera_plan.h CAMERA_MAX_WIDTH
CAMERA_MAX_HEIGHT = 65536  # csrc/camera_plan.h CAMERA_MAX_HEIGHT: the image row enters the fp32 positions
CAMERA_GRAD_MAX_HEIGHT = 4096  # csrc/camera_grad_plan.h CAMERA_GRAD_MAX_HEIGHT: the margin of the gather's candidate window
CAMERA_LIGHTS = ORBIT_LIGHTS


class _Kind(NamedTuple):
    """One entry point of the library as this module sees it."""
    fn: str                 # the public function that error messages name
    stem: str               # <stem>_supported, <stem>_workspace
    entry: str              # the entry point ...
    query: str              # ... and its workspace query
    max_h: Optional[int]    # None: no limit of its own
    max_w: Optional[int]
    lights: tuple
    forms: str              # the shapes of `vols` it takes
    dims: tuple
    what: str = ""          # a moving camera: what a world-fixed light is not built for, and what has no backward by default
    render: str = ""

    def limits(self) -> str:
        h = "H >= 1" if self.max_h is None else f"1 <= H <= {self.max_h}"
        w = "W >= 1" if self.max_w is None else f"1 <= W <= {self.max_w}"
        return f"1 <= D <= {MAX_DEPTH}, {h}, {w}, at most 2^31 - 2^16 cells"


_FRONT = _Kind("render_volumes", "render", "smk_volume_render", "smk_volume_render_workspace", None, None, tuple(sorted(LIGHTS)),
               "float32 [D,H,W], [n,D,H,W] or [B,T,D,H,W]", (3, 4, 5))
_BACKWARD = _FRONT._replace(stem="render_backward", entry="smk_volume_render_backward",
                           query="smk_volume_render_backward_workspace")
_ORBIT = _Kind("render_orbit", "orbit", "smk_volume_render_orbit", "smk_volume_render_orbit_workspace", None, ORBIT_MAX_WIDTH, ORBIT_LIGHTS,
               "float32 [D,H,W] or [n,D,H,W]", (3, 4), "orbit views", "orbit")
_ORBIT_BACKWARD = _ORBIT._replace(stem="orbit_backward", entry="smk_volume_render_orbit_backward",
                                 query="smk_volume_render_orbit_backward_workspace")
_CAMERA = _Kind("render_camera", "camera", "smk_volume_render_camera", "smk_volume_render_camera_workspace", CAMERA_MAX_HEIGHT,
                CAMERA_MAX_WIDTH, CAMERA_LIGHTS, "float32 [D,H,W] or [n,D,H,W]", (3, 4), "a moving camera", "free-camera")
_CAMERA_BACKWARD = _CAMERA._replace(stem="camera_backward", entry="smk_volume_render_camera_backward",
                                   query="smk_volume_render_camera_backward_workspace", max_h=CAMERA_GRAD_MAX_HEIGHT)


def _within(kind: _Kind, D: int, H: int, W: int) -> bool:
    return 1 <= D <= MAX_DEPTH and 1 <= H <= (kind.max_h or H) and 1 <= W <= (kind.max_w or W) and D * H * W <= MAX_CELLS


def _supported(kind: _Kind, D, H, W) -> bool:
    for v in (D, H, W):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{kind.stem}_supported: integer extents, got {v!r}")
    return _within(kind, D, H, W)


def _bad_light(kind: _Kind, light) -> ValueError:
    why = f" is not built for {kind.what} (a world-fixed +z light seen obliquely is another prefix);" if kind.what else ":"
    return ValueError(f"{kind.fn}: light={light!r}{why} one of {list(kind.lights)}")


def _workspace(kind: _Kind, n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    if light not in kind.lights:
        raise _bad_light(kind, light)
    d, h, w = (int(s) for s in shape)
    if n < 1 or not _within(kind, d, h, w):
        raise ValueError(f"{kind.fn}: n={n}, shape={tuple(shape)} is not supported (n >= 1, {kind.limits()})")
    nbytes = getattr(_lib.load(), kind.query)(n, d, h, w, LIGHTS[light])
    if nbytes < 0:
        raise ValueError(f"{kind.fn}: n={n}, shape={tuple(shape)}, light={light!r} is not supported")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def render_supported(D: int, H: int, W: int) -> bool:
    """Whether smk_volume_render takes volumes of this shape: 1 <= D <= 64, H, W >= 1, D*H*W <= 2^31 - 2^16."""
    return _supported(_FRONT, D, H, W)


def orbit_supported(D: int, H: int, W: int) -> bool:
    """Whether smk_volume_render_orbit takes volumes of this shape: 1 <= D <= 64, H >= 1, 1 <= W <= 1024, D*H*W <= 2^31 - 2^16."""
    return _supported(_ORBIT, D, H, W)


def camera_supported(D: int, H: int, W: int) -> bool:
    """Whether smk_volume_render_camera takes volumes of this shape: 1 <= D <= 64, 1 <= H <= 65536, 1 <= W <= 1024,
    D*H*W <= 2^31 - 2^16."""
    return _supported(_CAMERA, D, H, W)


def camera_backward_supported(D: int, H: int, W: int) -> bool:
    """Whether smk_volume_render_camera_backward takes volumes of this shape: camera_supported's limits and H <= 4096."""
    return _supported(_CAMERA_BACKWARD, D, H, W)


def render_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none);
    reusable across calls on one stream."""
    return _workspace(_FRONT, n, shape, light, device)


def render_backward_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_backward wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none:
    "none" and "+z"); reusable across calls on one stream."""
    return _workspace(_BACKWARD, n, shape, light, device)


def orbit_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_orbit wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none:
    "none"; the prefix along y, n*D*H*W floats, under "+y" / "-y"); the same for any number of views; reusable on one stream."""
    return _workspace(_ORBIT, n, shape, light, device)


def orbit_backward_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_orbit_backward wants for n volumes of `shape` = (D, H, W) under `light`: one value per ray of
    at most 16 volumes under "none"; the prefix along y and the shadow sums (n*D*H*W floats each) and at most 256 MiB of per-sample
    scratch under "+y" / "-y"; the same for any number of views; reusable on one stream."""
    return _workspace(_ORBIT_BACKWARD, n, shape, light, device)


def camera_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_camera wants for n volumes of `shape` = (D, H, W) under `light` (None when it wants none:
    "none"; the prefix along y, n*D*H*W floats, under "+y" / "-y"); the same for any number of views; reusable on one stream."""
    return _workspace(_CAMERA, n, shape, light, device)


def camera_backward_workspace(n: int, shape, light: str, device) -> Optional[torch.Tensor]:
    """The scratch buffer smk_volume_render_camera_backward wants for n volumes of `shape` = (D, H, W) under `light`: one value per ray of
    a band of image rows of at most 16 volumes under "none"; the prefix along y and the shadow sums (n*D*H*W floats each) and at most
    256 MiB of banded per-sample scratch under "+y" / "-y"; the same for any number of views; reusable on one stream."""
    return _workspace(_CAMERA_BACKWARD, n, shape, light, device)


def _ray_samples(q: int, D: int) -> int:
    """The smallest integer >= sqrt(q) with the parity of D (csrc/view_plan.h ray_samples)."""
    s = math.isqrt(q)
    s += s * s < q
    return s + ((s - D) & 1)


def orbit_samples(D: int, W: int) -> int:
    """S, the samples on a ray of an orbit view: the smallest integer >= hypot(D, W) with the parity of D (csrc/orbit_plan.h)."""
    if D < 1 or W < 1:
        raise ValueError(f"orbit_samples: D, W >= 1, got {(D, W)}")
    return _ray_samples(D * D + W * W, D)


def camera_samples(D: int, H: int, W: int) -> int:
    """S, the samples on a ray of a free-camera view: the smallest integer >= sqrt(D^2 + H^2 + W^2) with the parity of D
    (csrc/camera_plan.h)."""
    if D < 1 or H < 1 or W < 1:
        raise ValueError(f"camera_samples: D, H, W >= 1, got {(D, H, W)}")
    return _ray_samples(D * D + H * H + W * W, D)


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


def _angle(value, n: int, name: str, fn: str = "render_camera"):
    """One angle argument in one of its three forms -> a float64 host tensor of 0, 1 ([V]) or 2 ([n, V]) dimensions."""
    forms = f"{fn}: {name} is a number of degrees, a sequence of them or an [n, V] array"
    if isinstance(value, bool):
        raise ValueError(forms)
    try:
        t = value.detach().to("cpu", torch.float64) if isinstance(value, torch.Tensor) else torch.as_tensor(value, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{forms} ({e})") from None
    if not (t.dim() == 0 or (t.dim() == 1 and t.numel() >= 1) or (t.dim() == 2 and t.shape[0] == n and t.shape[1] >= 1)):
        raise ValueError(f"{fn}: {name} of shape {tuple(t.shape)}: a number, a sequence of V >= 1 numbers or an [n={n}, V] array")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{fn}: {name}s must be finite numbers of degrees")
    return t


def _tables(angles, n: int, fn: str):
    """Angle arguments out of _angle, paired -> (an [n][V] float64 host tensor of each, whether the result has a view dimension)."""
    counts = {int(t.shape[-1]) for t in angles if t.dim() > 0}
    if len(counts) > 1:
        raise ValueError(f"{fn}: azimuth and elevation are paired view by view: " + " against ".join(str(tuple(t.shape)) for t in angles))
    views, V = bool(counts), counts.pop() if counts else 1
    return [(t.reshape(1, -1) if t.dim() < 2 else t).expand(n, V).contiguous() for t in angles], views


def _camera_angles(azimuth, elevation, n: int):
    """The two angle arguments, paired -> ([n][V] azimuths, [n][V] elevations as float64 host tensors, whether the result has a view
    dimension)."""
    az, el = _angle(azimuth, n, "azimuth"), _angle(elevation, n, "elevation")
    if bool(((el < -90.0) | (el > 90.0)).any()):
        raise ValueError("render_camera: elevations must lie in [-90, 90] degrees")
    (az, el), views = _tables((az, el), n, "render_camera")
    return az, el, views


def _call_workspace(kind: _Kind, biggest: int, shape, light: str, workspace, dev):
    """The workspace of one call whose longest run has `biggest` volumes: (tensor or None, its bytes or 0); `workspace`: the caller's."""
    need = getattr(_lib.load(), kind.query)(biggest, *shape, LIGHTS[light])
    if need < 0:
        raise ValueError(f"{kind.fn}: {biggest} volumes of {tuple(shape)} are not supported")
    if not need:
        return None, 0
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    if workspace.device != dev or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"{kind.fn}: workspace of {need} bytes needed on {dev} ({kind.stem}_workspace)")
    return workspace, workspace.numel() * workspace.element_size()


def _each_run(kind: _Kind, vols, runs, shape, settings, middle, workspace, nbytes):
    """Hand every run of equally spaced volumes to the entry point.  middle(done, count): the arguments between desc and the workspace
    for the run's `count` volumes, `done` volumes into the call: angles, and the (pointer, stride) of every buffer."""
    D, H, W = shape
    cells = D * H * W
    entry = getattr(_lib.load(), kind.entry)
    desc = C.byref(settings.desc())
    tail = (workspace.data_ptr() if nbytes else None, nbytes, _lib.stream_ptr(vols.device))
    base = vols.data_ptr()
    done = 0
    for off, count, stride in runs:
        _lib.check(entry(base + 4 * off, stride if count > 1 else cells, count, D, H, W, desc, *middle(done, count), *tail))
        done += count


def _forward(kind: _Kind, vols, settings, angles, *, transmittance, out, workspace, differentiable=False, tables_out=None):
    """The call path of the three forward renders.  angles: None (the front view) or n -> (the [n][V] tables that the entry point takes,
    whether the result has a view dimension); it runs where the moving cameras parse their angles.  differentiable: the caller carries
    the backward (no refusal of volumes that require a gradient); tables_out: a list that receives the angle tables."""
    settings = RenderSettings() if settings is None else settings
    if not isinstance(settings, RenderSettings):
        raise TypeError(f"{kind.fn}: settings must be a RenderSettings")
    if settings.light not in kind.lights:
        raise _bad_light(kind, settings.light)
    if angles is None:
        dev = _lib.require_cuda(vols.device, kind.fn)
    if not isinstance(vols, torch.Tensor) or vols.dim() not in kind.dims or vols.dtype != torch.float32:
        raise ValueError(f"{kind.fn}: {kind.forms}")
    shape = D, H, W = tuple(int(s) for s in vols.shape[-3:])
    lead = tuple(vols.shape[:-3])
    n = math.prod(lead)
    if n < 1:
        raise ValueError(f"{kind.fn}: shape {tuple(vols.shape)}: at least one volume")
    tables, views = ((), False) if angles is None else angles(n)
    if angles is not None:
        if not differentiable and torch.is_grad_enabled() and vols.requires_grad:
            raise RuntimeError(f"{kind.fn}: the {kind.render} render has no backward unless it is asked for, and the volumes require a "
                               "gradient; pass differentiable=True, call under torch.no_grad() or detach them")
        if tables_out is not None:
            tables_out.extend(tables)
        dev = _lib.require_cuda(vols.device, kind.fn)
    if not _within(kind, D, H, W):
        raise ValueError(f"{kind.fn}: shape {tuple(vols.shape)} is not supported ({kind.limits()} per volume)")
    if differentiable and kind is _CAMERA and not _within(_CAMERA_BACKWARD, D, H, W):
        raise ValueError(f"render_camera: shape {tuple(vols.shape)} has no backward ({_CAMERA_BACKWARD.limits()} per volume); call "
                         "without differentiable=True")
    if vols.is_contiguous():                       # the usual case: nothing to check, and what _runs makes of it
        runs = [(0, n, D * H * W)]
    else:
        if not _dense(vols):
            raise ValueError(f"{kind.fn}: every volume must be dense ([D][H][W] with strides (H*W, W, 1)); only the batch may be strided")
        if any(st < 0 for st in vols.stride()[:-3]):
            raise ValueError(f"{kind.fn}: negative batch strides")
        runs = _runs(lead, vols.stride()[:-3], D * H * W)
    V = int(tables[0].shape[1]) if tables else 1
    oshape = lead + ((V,) if views else ()) + (H, W)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != oshape or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"{kind.fn}: out must be a contiguous float32 tensor of shape {oshape} on {dev}")
    trans = torch.empty(oshape, dtype=torch.float32, device=dev) if transmittance else None
    workspace, nbytes = _call_workspace(kind, max(r[1] for r in runs), shape, settings.light, workspace, dev)
    flat, n_views = [t.reshape(-1).tolist() for t in tables], (V,) if tables else ()
    HW, obase, tbase = H * W, out.data_ptr(), trans.data_ptr() if transmittance else None

    def middle(done, count):                       # the run's angles and V (nothing for the front view), image, transmittance
        angles = [(C.c_double * (count * V))(*f[done * V:(done + count) * V]) for f in flat]
        at = 4 * done * V * HW
        return (*angles, *n_views, obase + at, HW, tbase and tbase + at, HW)
    _each_run(kind, vols, runs, shape, settings, middle, workspace, nbytes)
    return (out, trans) if transmittance else out


def _render_backward(vols: torch.Tensor, settings: RenderSettings, grad_image, grad_trans) -> torch.Tensor:
    """smk_volume_render_backward over the runs of `vols` (checked by render_volumes): the gradient in vols' shape, contiguous.
    grad_image / grad_trans: the leading dimensions + [H, W], or None (= zero); not both None."""
    shape = D, H, W = tuple(int(s) for s in vols.shape[-3:])
    lead = tuple(vols.shape[:-3])
    cells, HW = D * H * W, H * W
    gi = None if grad_image is None else grad_image.to(torch.float32).contiguous()
    gt = None if grad_trans is None else grad_trans.to(torch.float32).contiguous()
    grad = torch.empty(lead + shape, dtype=torch.float32, device=vols.device)      # every element is written exactly once
    runs = _runs(lead, vols.stride()[:-3], cells)
    ws, nbytes = _call_workspace(_BACKWARD, max(r[1] for r in runs), shape, settings.light, None, vols.device)
    ibase, tbase, gbase = gi is not None and gi.data_ptr(), gt is not None and gt.data_ptr(), grad.data_ptr()

    def middle(done, count):                       # the upstream gradients (None: zero) and the result
        return (ibase and ibase + 4 * done * HW, HW, tbase and tbase + 4 * done * HW, HW, gbase + 4 * done * cells, cells)
    _each_run(_BACKWARD, vols, runs, shape, settings, middle, ws, nbytes)
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
    return _forward(_FRONT, vols, settings, None, transmittance=transmittance, out=out, workspace=workspace)


def _orbit_angles(azimuth):
    return lambda n: _tables((_angle(azimuth, n, "azimuth", "render_orbit"),), n, "render_orbit")


def _moving_backward(kind: _Kind, vols: torch.Tensor, settings: RenderSettings, tables, grad_image, grad_trans) -> torch.Tensor:
    """The backward entry point of a moving camera (_ORBIT_BACKWARD, _CAMERA_BACKWARD) over the runs of `vols` (checked by the forward):
    the gradient in vols' shape, contiguous.  tables: the [n][V] angle tables of the forward, as the entry point takes them;
    grad_image / grad_trans: the image's shape, or None (= zero); not both None."""
    shape = D, H, W = tuple(int(s) for s in vols.shape[-3:])
    lead = tuple(vols.shape[:-3])
    cells, HW, V = D * H * W, H * W, int(tables[0].shape[1])
    gi = None if grad_image is None else grad_image.to(torch.float32).contiguous()
    gt = None if grad_trans is None else grad_trans.to(torch.float32).contiguous()
    grad = torch.empty(lead + shape, dtype=torch.float32, device=vols.device)      # every element is written
    runs = _runs(lead, vols.stride()[:-3], cells)
    ws, nbytes = _call_workspace(kind, max(r[1] for r in runs), shape, settings.light, None, vols.device)
    ibase, tbase, gbase = gi is not None and gi.data_ptr(), gt is not None and gt.data_ptr(), grad.data_ptr()
    flat = [t.reshape(-1).tolist() for t in tables]

    def middle(done, count):                       # the run's angles and V, the upstream gradients (None: zero) and the result
        at = 4 * done * V * HW
        return (*((C.c_double * (count * V))(*f[done * V:(done + count) * V]) for f in flat), V, ibase and ibase + at, HW,
                tbase and tbase + at, HW, gbase + 4 * done * cells, cells)
    _each_run(kind, vols, runs, shape, settings, middle, ws, nbytes)
    return grad


class _RenderOrbit(torch.autograd.Function):
    """render_orbit with a backward: the forward is the plain call (the same values bit for bit), the backward is
    smk_volume_render_orbit_backward on the saved volumes and the forward's angle table.  Differentiable once."""

    @staticmethod
    def forward(ctx, vols, azimuth, settings, transmittance, workspace):
        ctx.settings = settings
        ctx.set_materialize_grads(False)           # an unused output's gradient arrives as None: the NULL of the entry point
        ctx.save_for_backward(vols)
        tables = []
        res = _forward(_ORBIT, vols, settings, _orbit_angles(azimuth), transmittance=transmittance, out=None, workspace=workspace,
                       differentiable=True, tables_out=tables)
        ctx.table = tables[0]
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_image, grad_trans=None):
        (vols,) = ctx.saved_tensors
        if grad_image is None and grad_trans is None:
            return None, None, None, None, None
        return _moving_backward(_ORBIT_BACKWARD, vols, ctx.settings, (ctx.table,), grad_image, grad_trans), None, None, None, None


def render_orbit(vols: torch.Tensor, azimuth, settings: Optional[RenderSettings] = None, *, transmittance: bool = False,
                 out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, differentiable: bool = False):
    """Render [n,D,H,W] or [D,H,W] float32 volumes from an orthographic camera that orbits the vertical axis y (SPEC_3D.md section 10,
    "Orbit views").  azimuth, in degrees (0: the front view of render_volumes; positive turns the viewing direction from +z toward +x):
      a number                  -> [n,H,W]    ([H,W] for one [D,H,W] volume)
      a sequence of V numbers   -> [n,V,H,W]  ([V,H,W]), the same views of every volume
      an [n,V] array or tensor  -> [n,V,H,W], one list per volume
    Returns the image, or (image, transmittance).  The batch may have any non-negative stride; every volume must be dense.  Lights:
    "none", "+y", "-y" ("+z" raises ValueError).  out: a contiguous float32 tensor of the image's shape to write into.  workspace:
    orbit_workspace(...) of at least this call's size.  One call renders all the views.

    differentiable=False (the default): there is no backward, and volumes that require a gradient raise RuntimeError (call under
    torch.no_grad(), detach them, or pass differentiable=True).  differentiable=True: when autograd is on and `vols.requires_grad`, the
    outputs carry a backward with respect to the volumes (SPEC_3D.md section 10, "Orbit views -- Gradient";
    smk_volume_render_orbit_backward): it takes the gradient of the image ([n,(V),H,W]) and, with transmittance=True, of the
    transmittance, and returns a gradient of vols' shape, the views summed.  The forward values are the plain call's bit for bit.
    `out=` raises ValueError then (an autograd output cannot be the caller's buffer), and a second derivative is not supported
    (RuntimeError from autograd).  With nothing that requires a gradient it is the plain path."""
    if differentiable and torch.is_grad_enabled() and isinstance(vols, torch.Tensor) and vols.requires_grad:
        if out is not None:
            raise ValueError("render_orbit: out= cannot be used when the volumes require a gradient (an autograd output cannot be the "
                             "caller's buffer); call under torch.no_grad() or detach the volumes")
        settings = RenderSettings() if settings is None else settings
        if not isinstance(settings, RenderSettings):
            raise TypeError("render_orbit: settings must be a RenderSettings")
        return _RenderOrbit.apply(vols, azimuth, settings, bool(transmittance), workspace)
    return _forward(_ORBIT, vols, settings, _orbit_angles(azimuth), transmittance=transmittance, out=out, workspace=workspace)


def _camera_angle_tables(azimuth, elevation):
    def angles(n):
        az, el, views = _camera_angles(azimuth, elevation, n)
        return (az, el), views
    return angles


class _RenderCamera(torch.autograd.Function):
    """render_camera with a backward: the forward is the plain call (the same values bit for bit), the backward is
    smk_volume_render_camera_backward on the saved volumes and the forward's angle tables.  Differentiable once."""

    @staticmethod
    def forward(ctx, vols, azimuth, elevation, settings, transmittance, workspace):
        ctx.settings = settings
        ctx.set_materialize_grads(False)           # an unused output's gradient arrives as None: the NULL of the entry point
        ctx.save_for_backward(vols)
        tables = []
        res = _forward(_CAMERA, vols, settings, _camera_angle_tables(azimuth, elevation), transmittance=transmittance, out=None,
                       workspace=workspace, differentiable=True, tables_out=tables)
        ctx.tables = tuple(tables)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_image, grad_trans=None):
        (vols,) = ctx.saved_tensors
        if grad_image is None and grad_trans is None:
            return None, None, None, None, None, None
        return _moving_backward(_CAMERA_BACKWARD, vols, ctx.settings, ctx.tables, grad_image, grad_trans), None, None, None, None, None


def render_camera(vols: torch.Tensor, azimuth, elevation, settings: Optional[RenderSettings] = None, *, transmittance: bool = False,
                  out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, **options):
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
    call renders all the views.  elevation=0 is the orbit's view on a longer ray: close to render_orbit's image, not equal to it.

    differentiable=False (the default): there is no backward, and volumes that require a gradient raise RuntimeError (call under
    torch.no_grad(), detach them, or pass differentiable=True).  differentiable=True: when autograd is on and `vols.requires_grad`, the
    outputs carry a backward with respect to the volumes (SPEC_3D.md section 10, "Free camera -- Gradient";
    smk_volume_render_camera_backward; H <= 4096, camera_backward_supported): it takes the gradient of the image ([n,(V),H,W]) and, with
    transmittance=True, of the transmittance, and returns a gradient of vols' shape, the views summed.  The forward values are the plain
    call's bit for bit.  `out=` raises ValueError then (an autograd output cannot be the caller's buffer), and a second derivative is
    not supported (RuntimeError from autograd).  With nothing that requires a gradient it is the plain path.

    `differentiable` is the one keyword taken through **options (any other raises TypeError, as a named parameter list would): the named
    parameters are those of the forward-only render, which tests/test_render_orbit_grad_host.py holds in place."""
    differentiable = options.pop("differentiable", False)
    if options:
        raise TypeError(f"render_camera() got an unexpected keyword argument {next(iter(options))!r}")
    if differentiable and torch.is_grad_enabled() and isinstance(vols, torch.Tensor) and vols.requires_grad:
        if out is not None:
            raise ValueError("render_camera: out= cannot be used when the volumes require a gradient (an autograd output cannot be the "
                             "caller's buffer); call under torch.no_grad() or detach the volumes")
        settings = RenderSettings() if settings is None else settings
        if not isinstance(settings, RenderSettings):
            raise TypeError("render_camera: settings must be a RenderSettings")
        return _RenderCamera.apply(vols, azimuth, elevation, settings, bool(transmittance), workspace)
    return _forward(_CAMERA, vols, settings, _camera_angle_tables(azimuth, elevation), transmittance=transmittance, out=out,
                    workspace=workspace)
