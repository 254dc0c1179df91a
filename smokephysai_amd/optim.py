"""HipAdamW: torch.optim.AdamW whose step -- and, on request, the gradient clip in front of it -- runs on libsmokehip.

`step(clip_max_norm=c)` is `utils.distributed.clip_grad_norm_(params, c)` followed by `torch.optim.AdamW.step()` as two kinds of launch:
smk_grad_norm reads every gradient once (fp64 partial sums in a fixed order that depends on the tensor sizes only, so DDP's unaligned
bucket views need no clone), and smk_adamw_step reads p, g, m, v and writes p, m, v once, with the clip coefficient taken from device
memory as a scale of g: no host synchronisation, no temporaries.  The constructor, the `state` layout (per parameter `step`, `exp_avg`,
`exp_avg_sq`) and the state_dict are torch.optim.AdamW's, so checkpoints load across the two classes in both directions.
"""
import ctypes as C
import warnings
from typing import Optional

import torch
from torch.optim.optimizer import _get_scalar_dtype

from . import _lib
from .utils.distributed import clip_grad_norm_

__all__ = ["HipAdamW", "hip_adamw_supported"]

_UNSUPPORTED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable", "fused")


def _dense_f32(t, device) -> bool:
    return (torch.is_tensor(t) and t.dtype == torch.float32 and t.layout == torch.strided and t.device == device and t.is_contiguous())


def hip_adamw_supported(group: dict, params) -> bool:
    """True when smk_grad_norm / smk_adamw_step can take `params` (those of `group` that have a gradient): float32, dense, contiguous
    parameter and gradient on one ROCm device (and, where the caller passes them as (p, exp_avg, exp_avg_sq) triples, the same of the two
    moments), a float learning rate, and none of amsgrad, maximize, capturable, differentiable (or torch's own fused kernel)."""
    if any(group.get(k) for k in _UNSUPPORTED_FLAGS) or torch.is_tensor(group.get("lr")):
        return False
    device = None
    for item in params:
        p, moments = (item[0], item[1:]) if isinstance(item, tuple) else (item, ())
        if device is None:
            device = p.device
            if device.type != "cuda":
                return False
        if not _dense_f32(p, device) or not _dense_f32(p.grad, device) or not all(_dense_f32(m, device) for m in moments):
            return False
    return True


class HipAdamW(torch.optim.AdamW):
    """torch.optim.AdamW on libsmokehip (see the module docstring).

    clip_writes_grad (default False): with `step(clip_max_norm=...)` the clip coefficient is applied to the gradient on its way into the
        update and `.grad` KEEPS THE UNCLIPPED gradient, which saves one write of every gradient per step.  True also stores the clipped
        gradient, i.e. reproduces torch's in-place clip_grad_norm_ for code that reads `.grad` after the step.
    last_grad_norm: after a step with clip_max_norm, the gradients' total 2-norm before clipping (a 0-d tensor on the parameters' device;
        reading it on the host is the only synchronisation).

    Parameters the kernels cannot take (`hip_adamw_supported`) send the WHOLE step down the existing route -- clip_grad_norm_ and then
    torch.optim.AdamW.step -- with one warning; CPU parameters take it silently."""

    def __init__(self, params, *args, clip_writes_grad: bool = False, **kwargs):
        super().__init__(params, *args, **kwargs)
        self.clip_writes_grad = bool(clip_writes_grad)
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._table = None             # (data_ptr key, (ctypes rows, [(group index, first row, rows)], rows, device) or None)
        self._workspace = None
        self._warned = False

    # ---- state (torch.optim.Adam._init_group's lazy initialisation, same tensors) ----------------------------------------------
    def _rows(self):
        """[(group, [(p, exp_avg, exp_avg_sq, step)])] over the parameters that have a gradient, creating missing state as AdamW does."""
        out = []
        for group in self.param_groups:
            rows = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:
                    on_device = group["capturable"] or group["fused"]
                    state["step"] = (torch.zeros((), dtype=_get_scalar_dtype(is_fused=group["fused"]), device=p.device) if on_device
                                     else torch.tensor(0.0, dtype=_get_scalar_dtype()))
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                rows.append((p, state["exp_avg"], state["exp_avg_sq"], state["step"]))
            out.append((group, rows))
        return out

    def _tensor_table(self, groups):
        """The host table of smk_opt_tensor rows, or None when `hip_adamw_supported` refuses a group.  Both are rebuilt only when a
        data_ptr() changed (zero_grad(set_to_none=True) reallocates the gradients; DDP's bucket views stay)."""
        key = [t.data_ptr() for _, rows in groups for p, m, v, _ in rows for t in (p, p.grad, m, v)]
        if self._table is not None and self._table[0] == key:
            return self._table[1]
        dev = next(r[0].device for _, rows in groups for r in rows)
        ok = all(hip_adamw_supported(g, [r[:3] for r in rows]) and all(r[0].device == dev for r in rows) for g, rows in groups)
        table = None
        if ok:
            flat = [r for _, rows in groups for r in rows]
            arr = (_lib.SmkOptTensor * len(flat))()
            for row, (p, m, v, _) in zip(arr, flat):
                row.param, row.grad, row.exp_avg, row.exp_avg_sq, row.n = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            spans, first = [], 0
            for gi, (_, rows) in enumerate(groups):
                spans.append((gi, first, len(rows)))
                first += len(rows)
            table = (arr, spans, len(flat), dev)
        elif not self._warned:
            self._warned = True
            warnings.warn("HipAdamW: a parameter, gradient, state tensor or option is outside the HIP kernels' domain (float32, dense, "
                          "contiguous, one ROCm device; no amsgrad / maximize / capturable / differentiable / fused): the step runs "
                          "clip_grad_norm_ and torch.optim.AdamW.step")
        self._table = (key, table)
        return table

    @staticmethod
    def _at(arr, first):
        return C.c_void_p(C.addressof(arr) + first * C.sizeof(_lib.SmkOptTensor))

    @torch.no_grad()
    def step(self, closure=None, *, clip_max_norm: Optional[float] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        first = next((p for g in self.param_groups for p in g["params"] if p.grad is not None), None)
        table = None
        if first is not None and first.device.type == "cuda":          # CPU parameters: torch's route, silently
            groups = self._rows()
            table = self._tensor_table(groups)
        if table is None:
            if clip_max_norm is not None:
                self.last_grad_norm = clip_grad_norm_([p for g in self.param_groups for p in g["params"]], clip_max_norm)
            super().step()
            return loss

        arr, spans, n_rows, dev = table
        L = _lib.load()
        stream = _lib.stream_ptr(dev)
        scale = None
        if clip_max_norm is not None:
            need = int(L.smk_grad_norm_workspace(arr, n_rows))
            if self._workspace is None or self._workspace.numel() * 8 < need or self._workspace.device != dev:
                self._workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
            out = torch.empty(2, dtype=torch.float32, device=dev)
            _lib.check(L.smk_grad_norm(arr, n_rows, float(clip_max_norm), out.data_ptr(), self._workspace.data_ptr(),
                                       self._workspace.numel() * 8, stream))
            self.last_grad_norm = out[0]
            scale = out.data_ptr() + 4
        write_grad = int(self.clip_writes_grad and scale is not None)
        for gi, first, count in spans:
            if count == 0:
                continue
            group, rows = groups[gi]
            for _, _, _, step_t in rows:
                step_t += 1
            steps = torch.stack([r[3] for r in rows]).tolist()
            beta1, beta2 = group["betas"]
            if min(steps) == max(steps):
                calls = [(self._at(arr, first), count, steps[0])]
            else:                                   # parameters that joined later: one call per distinct step count
                calls = []
                for s in sorted(set(steps)):
                    idx = [i for i, v in enumerate(steps) if v == s]
                    sub = (_lib.SmkOptTensor * len(idx))(*[arr[first + i] for i in idx])
                    calls.append((sub, len(idx), s))
            for rows_ptr, n, s in calls:
                _lib.check(L.smk_adamw_step(rows_ptr, n, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                                            float(group["weight_decay"]), 1.0 - float(beta1) ** s, 1.0 - float(beta2) ** s, scale,
                                            write_grad, stream))
        return loss
