"""Smoke simulation system on MI355X -- drop-in for src/physics/smoke_simulator.py:8-139.

simulate_step = one fused stencil step of the batched solver; the fractal perturbation is applied to the emitted
frame only (the solver keeps the unperturbed density, smoke_simulator.py:36-39) inside the density-advect kernel.
The chaos statistics (smoke_simulator.py:47-140) use the HIP reductions of csrc/chaos.hip (mean, box counts, histogram,
frame-difference norms); the scalar formulas on their results run on the host, as in the reference, or -- for callers that want
the labels as tensors -- on the device (chaos_features_device, get_chaos_features(as_tensor=True)).
"""
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .fractal_generator import FractalGenerator
from .navier_stokes import NavierStokesSimulator


class SmokeSimulator(nn.Module):
    def __init__(self, grid_size: tuple = (128, 128), dt: float = 0.01, viscosity: float = 0.001,
                 device: str = "cuda", batch_size: Optional[int] = None, jacobi_iters: int = 20):
        super().__init__()
        self.ns_solver = NavierStokesSimulator(grid_size, dt, viscosity, device, batch_size=batch_size,
                                               jacobi_iters=jacobi_iters)
        self.fractal_gen = FractalGenerator(device)
        self.device = device
        self.batch_size = batch_size
        self.history = []          # smoke_simulator.py:22-24
        self.max_history = 100
        self._feature_rows = {}    # (grids, frames per grid, history length) -> (pos, hist_len) device tensors of get_chaos_features(as_tensor=True)

    def add_incense_source(self, positions: list, intensities: list, grid: Optional[int] = None):
        """smoke_simulator.py:26-29 (radius 8).  Batched: `grid` selects the grid, None = every grid."""
        ns = self.ns_solver
        grids = range(ns._B) if grid is None else [grid]
        ns.add_smoke_sources([(g, x, y, 8, inten) for g in grids for (x, y), inten in zip(positions, intensities)])

    def simulate_step(self, add_fractal: bool = True) -> torch.Tensor:
        """smoke_simulator.py:31-45."""
        ns = self.ns_solver
        frame = torch.empty(ns._B, ns.h, ns.w, device=ns._dev)
        ns.step_into(frame, 1, add_fractal=add_fractal, fractal_intensity=0.05)
        density = frame if self.batch_size is not None else frame[0]
        self.history.append(density.clone())
        if len(self.history) > self.max_history:
            self.history.pop(0)
        return density

    def simulate_sequence(self, n_steps: int, add_fractal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n_steps frames per grid straight into one [B, n_steps, H, W] tensor (no history bookkeeping)."""
        ns = self.ns_solver
        if out is None:
            out = torch.empty(ns._B, n_steps, ns.h, ns.w, device=ns._dev)
        ns.step_into(out, n_steps, add_fractal=add_fractal, fractal_intensity=0.05)
        ns.check()                 # all n_steps were enqueued at once: a timed-out projection among them is reported HERE, not a call later
        return out

    # ---- chaos statistics (smoke_simulator.py:47-140) -------------------------------------------------------
    def get_chaos_features(self, as_tensor: bool = False):
        """Un-batched: the reference's dict (or {} with fewer than 10 frames).  Batched: a list with one dict per grid.
        as_tensor=True: (lyapunov, fractal dimension, entropy) as an fp64 device tensor instead, [B,3] batched / [3] un-batched,
        None with fewer than 10 frames; the formulas run on the device and nothing is copied to the host."""
        if len(self.history) < 10:
            if as_tensor:
                return None
            return {} if self.batch_size is None else [{} for _ in range(self.ns_solver._B)]
        self.ns_solver.check()     # the statistics leave the simulator: the frames behind them must be real
        if as_tensor:
            return self._chaos_features_tensor()
        if self.batch_size is None:
            return {"lyapunov_exponent": self.compute_lyapunov_exponent(),
                    "fractal_dimension": self.compute_fractal_dimension(),
                    "entropy": self.compute_entropy()}
        cur = self.history[-1]                                           # [B,H,W]
        _, box, hist = chaos_stats(cur)
        box, hist = box.cpu().numpy(), hist.cpu().numpy()
        lyap = [0.0] * cur.shape[0]
        if len(self.history) >= 20:
            states = torch.stack(self.history[-20:], dim=1)             # [B,20,H,W]
            # one launch over the flat stream of B x 20 frames and one copy to the host; the pair (last of grid b, first of b+1) is unused
            d = frame_diff_norms(states.view(-1, *states.shape[2:])).cpu().numpy()
            lyap = [lyapunov_from_norms(d[20 * b:20 * b + 19]) for b in range(cur.shape[0])]
        return [{"lyapunov_exponent": lyap[b], "fractal_dimension": fractal_dimension_from_counts(box[b]),
                 "entropy": entropy_from_hist(hist[b])} for b in range(cur.shape[0])]

    def _chaos_features_tensor(self) -> torch.Tensor:
        B = self.ns_solver._B
        n = 20 if len(self.history) >= 20 else 1                        # frames per grid the formulas look at
        hist_len = min(len(self.history), 20)                            # the formulas only ask "below 20?"
        states = torch.stack(self.history[-n:], dim=-3)                  # [B,n,H,W] ([n,H,W] un-batched): one flat stream, grid after grid
        stream = states.view(-1, *states.shape[-2:])
        key = (B, n, hist_len)
        if key not in self._feature_rows:
            pos = torch.arange(n - 1, B * n, n, dtype=torch.int32, device=stream.device)     # each grid's newest frame
            self._feature_rows[key] = (pos, torch.full_like(pos, hist_len))
        # smk_chaos_features indexes all three results by one stream position, so both reductions run over the whole stream: the pair
        # (last frame of grid b, first of b+1) and the statistics of the 19 older frames per grid are computed and never read (microseconds)
        norms = frame_diff_norms(stream) if B * n > 1 else None
        _, box, hist = chaos_stats(stream)
        feats = chaos_features_device(norms, box, hist, *self._feature_rows[key])
        return feats if self.batch_size is not None else feats[0]

    def flow_lyapunov(self, n_steps: int = 20, **kw):
        """The largest Lyapunov exponent of the flow per unit time from the simulator's CURRENT state: physics.lyapunov_exponents
        (Benettin's method on the tangent-linear step) over n_steps further steps, run on clones -- the
        simulator, its history and get_chaos_features() (whose `lyapunov_exponent` stays the reference's frame-difference proxy) are
        untouched.  kw: lyapunov_exponents' keywords (renorm_every, seed, route, tangent0 in the batched
        shapes of ns_solver.state(), B = 1 when un-batched); k is 1.  A float when un-batched, an fp64
        tensor [B] when batched."""
        from .fluid_tangent import lyapunov_exponents
        ns = self.ns_solver
        ns.check()
        res = lyapunov_exponents(*ns.state(), n_steps, k=1, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters, **kw)
        return res.exponents[:, 0] if self.batch_size is not None else float(res.exponents[0, 0])

    def flow_chaos(self, n_steps: int = 20, k: int = 4, **kw):
        """The k largest Lyapunov exponents of the flow from the simulator's CURRENT state and what they say about it: physics.flow_chaos
         over n_steps further steps, run on clones -- the simulator, its history and get_chaos_features() (whose
        three labels stay the reference's proxies) are untouched, as with flow_lyapunov.  kw: flow_chaos's keywords (renorm_every, seed,
        route, gram_schmidt).  Batched: a FlowChaos of fp64 tensors [B, ...].  Un-batched: a dict of floats -- "lyapunov" (the largest
        exponent per unit time), "kaplan_yorke" (the attractor's dimension; a lower bound where "truncated" is True), "ks_entropy" (the
        sum of the positive exponents) -- with "exponents", the k floats sorted descending."""
        from .fluid_tangent import flow_chaos
        ns = self.ns_solver
        ns.check()
        res = flow_chaos(*ns.state(), n_steps, k=k, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters, **kw)
        if self.batch_size is not None:
            return res
        return {"lyapunov": float(res.lyapunov[0]), "kaplan_yorke": float(res.kaplan_yorke[0]), "ks_entropy": float(res.ks_entropy[0]),
                "truncated": bool(res.truncated[0]), "exponents": [float(x) for x in res.exponents[0]]}

    def flow_ftle(self, n_steps: int = 20, **kw):
        """The finite-time Lyapunov exponent field of the flow from the simulator's CURRENT state: physics.flow_ftle (DESIGN.md section
        3.14) over n_steps further steps, run on clones -- the simulator, its history and get_chaos_features() are untouched, as with
        flow_chaos.  kw: flow_ftle's keywords (direction, route).  Batched: an FtleResult of tensors [B, ...].  Un-batched: an FtleResult
        with the [H, W] field, the [2, H, W] displacement, mean and max as floats, and the state in ns_solver.state()'s shapes (B = 1)."""
        from .flow_map import FtleResult, flow_ftle
        ns = self.ns_solver
        ns.check()
        res = flow_ftle(*ns.state(), n_steps, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters, **kw)
        if self.batch_size is not None:
            return res
        return FtleResult(res.ftle[0], res.displacement[0], float(res.mean[0]), float(res.max[0]), res.state)

    def _single_grid(self, what):
        if self.batch_size is not None:
            raise ValueError(f"{what}: batched simulator -- use get_chaos_features(), which returns one dict per grid")

    def compute_lyapunov_exponent(self) -> float:
        self._single_grid("compute_lyapunov_exponent")
        if len(self.history) < 20:
            return 0.0
        return lyapunov_from_frames(torch.stack(self.history[-20:]))

    def compute_fractal_dimension(self) -> float:
        self._single_grid("compute_fractal_dimension")
        if not self.history:
            return 0.0
        return fractal_dimension(self.history[-1])

    def compute_entropy(self) -> float:
        self._single_grid("compute_entropy")
        if not self.history:
            return 0.0
        return histogram_entropy(self.history[-1])


# ---- chaos statistics: HIP reductions (csrc/chaos.hip) + the reference's tiny host-side formulas ---------------
def chaos_stats(frames: torch.Tensor):
    """means [n] fp32, box counts [n,5] int32 (scales 2..32 of frame > mean), histogram [n,256] int32 of n frames
    [n,H,W] on the device (smoke_simulator.py:89-140's reductions, one launch).  Frames above 512 x 512 and volumes [n,D,H,W]
    (cubic boxes, SPEC_3D.md section 9) go to the multi-workgroup kernel (volume_stats)."""
    dev = _lib.require_cuda(frames.device, "chaos_stats")
    f = frames.to(torch.float32)
    if f.dim() == 2:
        f = f[None]
    if f.dim() == 4 or (f.dim() == 3 and (f.shape[1] // 2) * (f.shape[2] // 2) > 65536):
        return volume_stats(f)[:3]
    if f.stride(2) != 1 or f.stride(1) != f.shape[2]:
        f = f.contiguous()
    n, h, w = f.shape
    means = torch.empty(n, device=dev)
    box = torch.empty(n, 5, dtype=torch.int32, device=dev)
    hist = torch.empty(n, 256, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().smk_chaos_stats(f.data_ptr(), f.stride(0), n, h, w, means.data_ptr(), box.data_ptr(),
                                           hist.data_ptr(), _lib.stream_ptr(dev)))
    return means, box, hist


def frame_diff_norms(frames: torch.Tensor) -> torch.Tensor:
    """||frames[i+1] - frames[i]||_2 for consecutive frames [n,H,W] -> [n-1] fp32 (smoke_simulator.py:73-79); volumes [n,D,H,W] too."""
    dev = _lib.require_cuda(frames.device, "frame_diff_norms")
    if frames.dim() == 4:
        return volume_stats(frames, norms=True)[3]
    f = frames.to(torch.float32).contiguous()
    n, h, w = f.shape
    out = torch.empty(n - 1, device=dev)
    _lib.check(_lib.load().smk_frame_diff_norms(f.data_ptr(), f.stride(0), n, h, w, out.data_ptr(), _lib.stream_ptr(dev)))
    return out


def volume_stats_workspace(n: int, shape, device) -> torch.Tensor:
    """The scratch buffer smk_volume_stats wants for n volumes of `shape` = (D, H, W) or (H, W); reusable across calls on one stream."""
    d, h, w = (1, *shape) if len(shape) == 2 else shape
    nbytes = _lib.load().smk_volume_stats_workspace(n, d, h, w)
    if nbytes <= 0:
        raise ValueError(f"volume_stats: n={n}, shape={tuple(shape)} is not supported (n >= 1, H, W >= 2, below 2^31 - 2^16 cells)")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def volume_stats(vols: torch.Tensor, norms: bool = False, workspace: Optional[torch.Tensor] = None):
    """chaos_stats and (norms=True) frame_diff_norms of n volumes [n,D,H,W] in one pass of the multi-workgroup kernel
    (csrc/chaos_nd.hip; SPEC_3D.md section 9): means [n] fp32, box counts [n,5] int32 (cubes of edge 2..32), histogram [n,256] int32,
    and norms [n-1] fp32 or None.  [n,H,W] is the 2-axis instance (squares; no size limit).  Each volume must be dense; the stride
    between volumes is free.  Bit-reproducible."""
    dev = _lib.require_cuda(vols.device, "volume_stats")
    f = vols.to(torch.float32)
    if f.dim() not in (3, 4):
        raise ValueError("volume_stats: [n,D,H,W] volumes or [n,H,W] frames")
    if not f[0].is_contiguous() or (f.shape[0] > 1 and f.stride(0) < f[0].numel()):
        f = f.contiguous()
    n, shape = f.shape[0], tuple(f.shape[1:])
    d, h, w = (1, *shape) if len(shape) == 2 else shape
    if len(shape) == 3 and d < 2:
        raise ValueError("volume_stats: a 3-D grid has D >= 2 (pass [n,H,W] for frames)")
    if workspace is None:
        workspace = volume_stats_workspace(n, shape, dev)
    means = torch.empty(n, device=dev)
    box = torch.empty(n, 5, dtype=torch.int32, device=dev)
    hist = torch.empty(n, 256, dtype=torch.int32, device=dev)
    out = torch.empty(n - 1, device=dev) if norms and n > 1 else None
    _lib.check(_lib.load().smk_volume_stats(f.data_ptr(), f.stride(0) if n > 1 else f[0].numel(), n, d, h, w, means.data_ptr(),
                                            box.data_ptr(), hist.data_ptr(), out.data_ptr() if out is not None else None,
                                            workspace.data_ptr(), workspace.numel() * workspace.element_size(), _lib.stream_ptr(dev)))
    return means, box, hist, out


def chaos_features_device(norms: Optional[torch.Tensor], box: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor,
                          hist_len: torch.Tensor, groups: Optional[int] = None):
    """The label scalars of smoke_simulator.py:47-140 on the device, from frame_diff_norms' [S-1] and chaos_stats' [S,5] / [S,256]
    over one stream of S frames.  Row k reads frame pos[k] of the stream with the history length hist_len[k] the reference's
    simulator would hold there (int32 device tensors [F]).  Returns features [F,3] fp64 = (lyapunov, fractal dimension, entropy);
    with groups=g (g divides F) also means [g,3], the mean over each F/g consecutive rows.  One launch, no copy to the host."""
    dev = _lib.require_cuda(box.device, "chaos_features_device")
    S, F = box.shape[0], pos.shape[0]
    if tuple(box.shape) != (S, 5) or tuple(hist.shape) != (S, 256) or box.dtype != torch.int32 or hist.dtype != torch.int32:
        raise ValueError("box must be int32 [S,5] and hist int32 [S,256] (chaos_stats' outputs)")
    if norms is not None and (tuple(norms.shape) != (S - 1,) or norms.dtype != torch.float32):
        raise ValueError(f"norms must be fp32 [S-1] = [{S - 1}] (frame_diff_norms' output)")
    if pos.dtype != torch.int32 or hist_len.dtype != torch.int32 or tuple(hist_len.shape) != (F,) or pos.dim() != 1:
        raise ValueError("pos and hist_len must be int32 [F]")
    if groups is not None and (groups < 1 or F % groups):
        raise ValueError(f"groups={groups} must divide the {F} feature rows")
    args = [t.contiguous() if t is not None else None for t in (norms, box, hist, pos, hist_len)]
    if any(t is not None and t.device != dev for t in args):
        raise ValueError("all inputs must live on the same ROCm device")
    feats = torch.empty(F, 3, dtype=torch.float64, device=dev)
    means = torch.empty(groups, 3, dtype=torch.float64, device=dev) if groups is not None else None
    ptr = [t.data_ptr() if t is not None else None for t in args]
    _lib.check(_lib.load().smk_chaos_features(ptr[0], ptr[1], ptr[2], S, ptr[3], ptr[4], F, groups or 0, feats.data_ptr(),
                                              means.data_ptr() if means is not None else None, _lib.stream_ptr(dev)))
    return feats if groups is None else (feats, means)


def lyapunov_from_norms(distances) -> float:
    """smoke_simulator.py:81-87: mean(diff(log(d + 1e-8))) clamped at 0 (host, float64 like the reference)."""
    d = np.asarray(distances, dtype=np.float64)
    if len(d) > 1:
        return max(0, float(np.mean(np.diff(np.log(d + 1e-8)))))
    return 0.0


def fractal_dimension_from_counts(counts) -> float:
    """smoke_simulator.py:116-122: |slope| of log(count+1) vs log(scale)."""
    slope = np.polyfit(np.log([2, 4, 8, 16, 32]), np.log(np.asarray(counts, dtype=np.float64) + 1), 1)[0]
    return abs(float(slope))


def entropy_from_hist(hist) -> float:
    """smoke_simulator.py:136-140: -sum(p * log2(p + 1e-8)), p = counts / total, fp32 like the reference."""
    h = np.asarray(hist).astype(np.float32)
    probs = h / h.sum(dtype=np.float32)
    return float(-np.sum(probs * np.log2(probs + np.float32(1e-8)), dtype=np.float32))


def lyapunov_from_frames(states: torch.Tensor) -> float:
    return lyapunov_from_norms(frame_diff_norms(states).cpu().numpy())


def fractal_dimension(frame: torch.Tensor) -> float:
    return fractal_dimension_from_counts(chaos_stats(frame)[1][0].cpu().numpy())


def histogram_entropy(frame: torch.Tensor) -> float:
    return entropy_from_hist(chaos_stats(frame)[2][0].cpu().numpy())
