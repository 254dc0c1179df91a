"""Front-view render of smoke volumes [D,H,W] to frames [H,W] on MI355X (SPEC_3D.md section 10; csrc/render.hip, smk_volume_render).

The camera looks along +z (plane 0 nearest); single scattering from one directional light.  No reference counterpart: the reference is
2-D, and its frames are what this operator makes of a 3-D density field.  No CPU path: the numpy form of the rule is the test oracle
(tests/render_oracle.py).  render_volumes is differentiable with respect to the volumes: smk_volume_render_backward, the closed-form
transpose of the rule (section 10, "Gradient"; oracle: tests/render_grad_oracle.py).
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
