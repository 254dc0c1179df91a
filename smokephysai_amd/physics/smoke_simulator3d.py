"""Smoke simulation system for 3-D grids on MI355X (BASELINE configs[4]) -- SmokeSimulator's surface (src/physics/smoke_simulator.py:8-139)
for grids `(D, H, W)`; semantics: SPEC_3D.md section 9, the rule-by-rule generalisation of the 2-D code.

simulate_step = one step of the batched 3-D solver; the fractal perturbation goes onto the emitted volume only, every plane with the [W][H]
shape-only field (the solver keeps the unperturbed density, smoke_simulator.py:36-39), inside the advection kernel.  The chaos features are
DEFINED on the list of emitted volumes exactly as in 2-D (smoke_simulator.py:47-140), but that list is never kept -- 100 volumes of
configs[4] are 53 GB.  What the formulas read of it is kept on the device instead: the newest volume's box counts and histogram, the last 19
distances between consecutive volumes per grid, and the history length (capped at 100).  Every simulate_step makes one smk_volume_stats call
over {previous volume, current volume} of every grid (csrc/chaos_nd.hip).
"""
from typing import Optional

import torch
import torch.nn as nn

from .navier_stokes3d import NavierStokesSimulator3D
from .render import RenderSettings, render_camera, render_orbit, render_volumes, render_workspace
from .smoke_simulator import (chaos_features_device, entropy_from_hist, fractal_dimension_from_counts, lyapunov_from_norms, volume_stats,
                              volume_stats_workspace)

WINDOW = 20          # smoke_simulator.py:69-79: the Lyapunov estimate reads the last 20 states = 19 distances


class SmokeSimulator3D(nn.Module):
    def __init__(self, grid_size: tuple = (64, 128, 128), dt: float = 0.01, viscosity: float = 0.001,
                 device: str = "cuda", batch_size: Optional[int] = None, jacobi_iters: int = 20):
        super().__init__()
        self.ns_solver = NavierStokesSimulator3D(grid_size, dt, viscosity, device, batch_size=batch_size, jacobi_iters=jacobi_iters)
        self.device = device
        self.batch_size = batch_size
        self.max_history = 100
        self.history_len = 0       # len(self.history) of the reference (smoke_simulator.py:22-24,41-43), capped at max_history
        ns = self.ns_solver
        B, dev = ns._B, ns._dev
        # the previous and the current emitted volume of every grid, side by side: [B][2] is one stream of 2B volumes for smk_volume_stats,
        # whose norm 2b is the distance between the two volumes of grid b whichever of them is the newer (the norm is symmetric)
        self._pair = torch.zeros(B, 2, *ns.grid_size, device=dev)
        self._slot = 1             # the slot of the newest volume; simulate_step writes the other one
        self._ws = volume_stats_workspace(2 * B, ns.grid_size, dev)
        # what smk_chaos_features reads, laid out as a stream of WINDOW "frames" per grid of which only the newest has statistics:
        # norms[20 b .. 20 b + 18] = the last 19 distances of grid b, oldest first; box / hist row 20 b + 19 = the newest volume's
        self._norms = torch.zeros(B * WINDOW - 1, device=dev)
        self._ring = self._norms.as_strided((B, WINDOW - 1), (WINDOW, 1))
        self._box = torch.zeros(B * WINDOW, 5, dtype=torch.int32, device=dev)
        self._hist = torch.zeros(B * WINDOW, 256, dtype=torch.int32, device=dev)
        self._pos = torch.arange(WINDOW - 1, B * WINDOW, WINDOW, dtype=torch.int32, device=dev)
        self._pos64 = self._pos.long()
        self._hist_len = {}        # min(history length, 20) -> int32 [B] device tensor (the formulas only ask "below 20?")

    def add_incense_source(self, positions: list, intensities: list, grid: Optional[int] = None):
        """smoke_simulator.py:26-29 (radius 8) with positions (x, y, z).  Batched: `grid` selects the grid, None = every grid."""
        ns = self.ns_solver
        grids = range(ns._B) if grid is None else [grid]
        ns.add_smoke_sources([(g, x, y, z, 8, inten) for g in grids for (x, y, z), inten in zip(positions, intensities)])

    def simulate_step(self, add_fractal: bool = True, copy: bool = True) -> torch.Tensor:
        """smoke_simulator.py:31-45.  Returns the emitted volume(s), [B,D,H,W] batched / [D,H,W] un-batched.  copy=False returns the
        simulator's own buffer instead of a copy of it: valid until the next-but-one simulate_step overwrites it."""
        ns = self.ns_solver
        B = ns._B
        slot = 1 - self._slot
        cur = self._pair[:, slot]
        ns.step_into(cur, 1, add_fractal=add_fractal, fractal_intensity=0.05)
        if self.history_len == 0:                                        # no previous volume yet: statistics only
            _, box, hist, _ = volume_stats(cur, workspace=self._ws)
        else:
            _, box, hist, norms = volume_stats(self._pair.view(2 * B, *ns.grid_size), norms=True, workspace=self._ws)
            box, hist = box[slot::2], hist[slot::2]
            self._ring[:, :-1] = self._ring[:, 1:].clone()
            self._ring[:, -1] = norms[0::2]
        self._box.index_copy_(0, self._pos64, box)
        self._hist.index_copy_(0, self._pos64, hist)
        self._slot = slot
        self.history_len = min(self.history_len + 1, self.max_history)
        out = cur.clone() if copy else cur
        return out if self.batch_size is not None else out[0]

    def simulate_sequence(self, n_steps: int, add_fractal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n_steps volumes per grid straight into one [B, n_steps, D, H, W] tensor (no history bookkeeping)."""
        ns = self.ns_solver
        if out is None:
            out = torch.empty(ns._B, n_steps, *ns.grid_size, device=ns._dev)
        ns.step_into(out, n_steps, add_fractal=add_fractal, fractal_intensity=0.05)
        return out

    # ---- rendered frames (SPEC_3D.md section 10; csrc/render.hip) ------------------------------------------------------------
    def render(self, settings: Optional[RenderSettings] = None, transmittance: bool = False):
        """The front-view image of the newest emitted volume(s): [B,H,W] batched / [H,W] un-batched, or (image, transmittance).
        Reads the simulator's own copy of that volume; changes no state."""
        if self.history_len == 0:
            raise RuntimeError("render: no volume has been emitted yet (call simulate_step first)")
        res = render_volumes(self._pair[:, self._slot], settings, transmittance=transmittance)
        if self.batch_size is not None:
            return res
        return (res[0][0], res[1][0]) if transmittance else res[0]

    def render_orbit(self, azimuth, settings: Optional[RenderSettings] = None, transmittance: bool = False):
        """The newest emitted volume(s) seen from an orbiting camera (physics.render_orbit; azimuth in degrees: a number, a sequence of V
        numbers, or [B, V]): [B,H,W] or [B,V,H,W] batched, [H,W] or [V,H,W] un-batched, or (image, transmittance).  Reads the simulator's
        own copy of that volume; changes no state."""
        if self.history_len == 0:
            raise RuntimeError("render_orbit: no volume has been emitted yet (call simulate_step first)")
        res = render_orbit(self._pair[:, self._slot], azimuth, settings, transmittance=transmittance)
        if self.batch_size is not None:
            return res
        return (res[0][0], res[1][0]) if transmittance else res[0]

    def render_camera(self, azimuth, elevation, settings: Optional[RenderSettings] = None, transmittance: bool = False):
        """The newest emitted volume(s) seen from a camera with an azimuth and an elevation (physics.render_camera; degrees, each a number,
        a sequence of V numbers, or [B, V], paired view by view): [B,H,W] or [B,V,H,W] batched, [H,W] or [V,H,W] un-batched, or (image,
        transmittance).  Reads the simulator's own copy of that volume; changes no state."""
        if self.history_len == 0:
            raise RuntimeError("render_camera: no volume has been emitted yet (call simulate_step first)")
        res = render_camera(self._pair[:, self._slot], azimuth, elevation, settings, transmittance=transmittance)
        if self.batch_size is not None:
            return res
        return (res[0][0], res[1][0]) if transmittance else res[0]

    def simulate_frames(self, n_steps: int, settings: Optional[RenderSettings] = None, add_fractal: bool = True,
                        out: Optional[torch.Tensor] = None, chunk: int = 4) -> torch.Tensor:
        """simulate_sequence followed by render_volumes, without the sequence: n_steps rendered frames per grid in one
        [B, n_steps, H, W] tensor, bit-equal to render_volumes(simulate_sequence(n_steps)).  At most `chunk` steps of volumes exist at
        a time.  No history bookkeeping, and the chaos-feature state is left alone."""
        if chunk < 1:
            raise ValueError("simulate_frames: chunk >= 1")
        ns = self.ns_solver
        B, (D, H, W) = ns._B, ns.grid_size
        settings = RenderSettings() if settings is None else settings
        if out is None:
            out = torch.empty(B, n_steps, H, W, device=ns._dev)
        elif (tuple(out.shape) != (B, n_steps, H, W) or out.dtype != torch.float32 or out.device != ns._dev
              or not all(out[b].is_contiguous() for b in range(B))):
            raise ValueError(f"simulate_frames: out must be float32 [B={B}, n_steps={n_steps}, {H}, {W}] on the simulator's device, "
                             "the frames of one grid contiguous")
        c = min(chunk, max(n_steps, 1))
        vols = torch.empty(B, c, D, H, W, device=ns._dev)
        ws = render_workspace(c, ns.grid_size, settings.light, ns._dev)
        for t0 in range(0, n_steps, c):
            k = min(c, n_steps - t0)
            ns.step_into(vols[:, :k], k, add_fractal=add_fractal, fractal_intensity=0.05)
            for b in range(B):                                           # out[b, t0:t0+k] is contiguous whatever out's batch stride
                render_volumes(vols[b, :k], settings, out=out[b, t0:t0 + k], workspace=ws)
        return out

    # ---- chaos statistics (smoke_simulator.py:47-140 on the list of emitted volumes) ------------------------------------
    def get_chaos_features(self, as_tensor: bool = False):
        """Un-batched: the reference's dict (or {} with fewer than 10 volumes).  Batched: a list with one dict per grid.
        as_tensor=True: (lyapunov, fractal dimension, entropy) as an fp64 device tensor instead, [B,3] batched / [3] un-batched,
        None with fewer than 10 volumes; the formulas run on the device and nothing is copied to the host."""
        B = self.ns_solver._B
        if self.history_len < 10:
            if as_tensor:
                return None
            return {} if self.batch_size is None else [{} for _ in range(B)]
        if as_tensor:
            hl = min(self.history_len, WINDOW)
            if hl not in self._hist_len:
                self._hist_len[hl] = torch.full_like(self._pos, hl)
            feats = chaos_features_device(self._norms if B * WINDOW > 1 else None, self._box, self._hist, self._pos, self._hist_len[hl])
            return feats if self.batch_size is not None else feats[0]
        box, hist = self._box[self._pos64].cpu().numpy(), self._hist[self._pos64].cpu().numpy()
        lyap = [0.0] * B
        if self.history_len >= WINDOW:
            d = self._ring.cpu().numpy()
            lyap = [lyapunov_from_norms(d[b]) for b in range(B)]
        feats = [{"lyapunov_exponent": lyap[b], "fractal_dimension": fractal_dimension_from_counts(box[b]),
                  "entropy": entropy_from_hist(hist[b])} for b in range(B)]
        return feats if self.batch_size is not None else feats[0]

    def flow_lyapunov(self, n_steps: int = 20, **kw):
        """The largest Lyapunov exponent of the flow per unit time from the simulator's CURRENT state: physics.lyapunov_exponents3d
        (Benettin's method on the tangent-linear step) over n_steps further steps, run on clones -- the
        simulator, its ring of norms and get_chaos_features() (whose `lyapunov_exponent` stays the frame-difference proxy) are untouched.
        kw: lyapunov_exponents3d's keywords (renorm_every, seed, route, tangent0 in the batched shapes of ns_solver.state(), B = 1 when
        un-batched); k is 1.  A float when un-batched, an fp64 tensor [B] when batched."""
        from .fluid_tangent3d import lyapunov_exponents3d
        ns = self.ns_solver
        res = lyapunov_exponents3d(*ns.state(), n_steps, k=1, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters, **kw)
        return res.exponents[:, 0] if self.batch_size is not None else float(res.exponents[0, 0])

    def flow_chaos(self, n_steps: int = 20, k: int = 4, **kw):
        """The k largest Lyapunov exponents of the flow from the simulator's CURRENT state and what they say about it: physics.flow_chaos3d
         over n_steps further steps, run on clones -- the simulator, its ring of norms and get_chaos_features() (whose
        three labels stay the frame-difference, box-count and histogram proxies) are untouched, as with flow_lyapunov.  kw: flow_chaos3d's keywords (renorm_every, seed,
        route, gram_schmidt).  Batched: a FlowChaos of fp64 tensors [B, ...].  Un-batched: a dict of floats -- "lyapunov" (the largest
        exponent per unit time), "kaplan_yorke" (the attractor's dimension; a lower bound where "truncated" is True), "ks_entropy" (the
        sum of the positive exponents) -- with "exponents", the k floats sorted descending."""
        from .fluid_tangent3d import flow_chaos3d
        ns = self.ns_solver
        res = flow_chaos3d(*ns.state(), n_steps, k=k, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters, **kw)
        if self.batch_size is not None:
            return res
        return {"lyapunov": float(res.lyapunov[0]), "kaplan_yorke": float(res.kaplan_yorke[0]), "ks_entropy": float(res.ks_entropy[0]),
                "truncated": bool(res.truncated[0]), "exponents": [float(x) for x in res.exponents[0]]}

    def flow_ftle(self, n_steps: int = 20, **kw):
        """The finite-time Lyapunov exponent field of the flow from the simulator's CURRENT state: physics.flow_ftle3d (DESIGN.md section
        3.15) over n_steps further steps, run on clones -- the simulator, its ring of norms and get_chaos_features() are untouched, as
        with flow_chaos.  kw: flow_ftle3d's keywords (direction, route).  Batched: an FtleResult of tensors [B, ...].  Un-batched: an
        FtleResult with the [D, H, W] field, the [3, D, H, W] displacement, mean and max as floats, and the state in ns_solver.state()'s
        shapes (B = 1)."""
        from .flow_map3d import FtleResult, flow_ftle3d
        ns = self.ns_solver
        res = flow_ftle3d(*ns.state(), n_steps, dt=ns.dt, viscosity=ns.viscosity, jacobi_iters=ns.jacobi_iters, **kw)
        if self.batch_size is not None:
            return res
        return FtleResult(res.ftle[0], res.displacement[0], float(res.mean[0]), float(res.max[0]), res.state)

    def _single_grid(self, what):
        if self.batch_size is not None:
            raise ValueError(f"{what}: batched simulator -- use get_chaos_features(), which returns one dict per grid")

    def compute_lyapunov_exponent(self) -> float:
        self._single_grid("compute_lyapunov_exponent")
        if self.history_len < WINDOW:
            return 0.0
        return lyapunov_from_norms(self._ring[0].cpu().numpy())

    def compute_fractal_dimension(self) -> float:
        self._single_grid("compute_fractal_dimension")
        if self.history_len == 0:
            return 0.0
        return fractal_dimension_from_counts(self._box[WINDOW - 1].cpu().numpy())

    def compute_entropy(self) -> float:
        self._single_grid("compute_entropy")
        if self.history_len == 0:
            return 0.0
        return entropy_from_hist(self._hist[WINDOW - 1].cpu().numpy())
