"""Figures of the reference's src/utils/visualization.py (SmokeVisualizer: the same three methods and argument names), drawn with
matplotlib alone, and two the reference has no like of: plot_turntable, a row of orbit views of one volume (physics.render_orbit), and
plot_ftle, a frame beside the finite-time Lyapunov exponent field of its flow (physics.flow_ftle).  The attention panel takes what SmokePhysNet.attention_maps returns: the full [B, heads, L, L] weights as in the
reference, or the `received` map [B, heads, h, w] the libsmokehip kernels produce without ever forming an L x L tensor.
Without a display the Agg backend is used; plt.show() is called only on an interactive backend."""
import math
import os
import sys
from typing import Dict, List, Optional

import matplotlib

if not (os.environ.get("DISPLAY") or os.environ.get("WAYLAND_DISPLAY") or os.environ.get("MPLBACKEND")
        or sys.platform in ("win32", "darwin")):
    matplotlib.use("Agg")
import matplotlib.pyplot as plt      # noqa: E402
import numpy as np                   # noqa: E402


def _numpy(a) -> np.ndarray:
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _finish(fig, save_path: Optional[str]):
    fig.tight_layout()
    if save_path:
        fig.savefig(save_path, dpi=150, bbox_inches="tight")
    if matplotlib.get_backend().lower() in (b.lower() for b in _interactive_backends()):
        plt.show()
    return fig


def _interactive_backends():
    try:
        from matplotlib.backends import backend_registry, BackendFilter
        return backend_registry.list_builtin(BackendFilter.INTERACTIVE)
    except ImportError:                                      # matplotlib < 3.9
        from matplotlib import rcsetup
        return rcsetup.interactive_bk


class SmokeVisualizer:
    def __init__(self, figsize: tuple = (12, 8)):
        self.figsize = figsize
        plt.style.use("dark_background")

    def plot_smoke_evolution(self, density_sequence: List, save_path: Optional[str] = None):
        """One 'hot' panel per frame, at most 8 per row, titled 'Frame i'; the cells past the last frame stay empty.  Returns the figure."""
        n = len(density_sequence)
        cols = max(1, min(8, n))
        rows = max(1, (n + cols - 1) // cols)
        fig, axes = plt.subplots(rows, cols, figsize=(cols * 2, rows * 2), squeeze=False)
        for ax in axes.flat:
            ax.axis("off")
        for i, density in enumerate(density_sequence):
            ax = axes[i // cols, i % cols]
            ax.imshow(_numpy(density), cmap="hot", interpolation="bilinear")
            ax.set_title(f"Frame {i}")
        return _finish(fig, save_path)

    def plot_chaos_features(self, chaos_metrics: Dict[str, List[float]], save_path: Optional[str] = None):
        """Lyapunov exponent, fractal dimension and entropy over the time steps, side by side; a metric the dict lacks leaves its panel blank."""
        fig, axes = plt.subplots(1, 3, figsize=self.figsize)
        for ax, key, title in zip(axes, ("lyapunov_exponent", "fractal_dimension", "entropy"),
                                  ("Lyapunov Exponent", "Fractal Dimension", "Entropy")):
            if key in chaos_metrics:
                ax.plot(_numpy(chaos_metrics[key]), "o-", linewidth=2, markersize=4)
                ax.set_title(title)
                ax.set_xlabel("Time Step")
                ax.grid(True, alpha=0.3)
        return _finish(fig, save_path)

    def plot_attention_maps(self, attention_weights, input_image, save_path: Optional[str] = None, received=None):
        """The frame, the attention matrix of (batch 0, head 0) and the attention its keys receive, laid out as an image.
        attention_weights: [B, heads, L, L], or None when received [B, heads, h, w] is given (the matrix panel is then left out).
        Without `received` the third panel is attention_weights[0, 0].mean(0) reshaped to sqrt(L) x sqrt(L) when L is a perfect square
        (the reference's rule); another L leaves that panel out.  input_image: [B, 1, H, W] tensor, or a 2-D array."""
        if attention_weights is None and received is None:
            raise ValueError("plot_attention_maps: attention_weights or received")
        attn = None if attention_weights is None else _numpy(attention_weights[0, 0])
        recv = None
        if received is not None:
            recv = _numpy(received[0, 0])
        elif attn is not None:
            avg = attn.mean(axis=0)
            side = math.isqrt(len(avg))
            if side * side == len(avg):
                recv = avg.reshape(side, side)
        img = _numpy(input_image)
        while img.ndim > 2:
            img = img[0]
        n = 1 + (attn is not None) + (recv is not None)
        fig, axes = plt.subplots(1, n, figsize=(5 * n, 5), squeeze=False)
        axes = list(axes[0])
        ax = axes.pop(0)
        ax.imshow(img, cmap="hot")
        ax.set_title("Input Smoke")
        ax.axis("off")
        if attn is not None:
            ax = axes.pop(0)
            im = ax.imshow(attn, cmap="viridis")
            ax.set_title("Attention Matrix")
            ax.set_xlabel("Key Position")
            ax.set_ylabel("Query Position")
            fig.colorbar(im, ax=ax)
        if recv is not None:
            ax = axes.pop(0)
            im = ax.imshow(recv, cmap="plasma")
            ax.set_title("Average Attention")
            ax.axis("off")
            fig.colorbar(im, ax=ax)
        return _finish(fig, save_path)

    def plot_ftle(self, frame, ftle, path: Optional[str] = None):
        """The frame, the finite-time Lyapunov exponent field of its flow (physics.flow_ftle) and the field's upper decile as a contour
        over the frame: where the backward field's ridges lie, smoke filaments collect.  frame, ftle: [H, W] arrays or tensors (leading
        dimensions of size 1, or a batch whose first entry is drawn, are dropped as plot_attention_maps drops them).  A constant field
        has no upper decile and gets no contour."""
        img, field = _numpy(frame), _numpy(ftle)
        while img.ndim > 2:
            img = img[0]
        while field.ndim > 2:
            field = field[0]
        return self._draw_ftle("plot_ftle", img, field, "FTLE", path)

    def plot_ftle3d(self, frame, ftle, path: Optional[str] = None):
        """plot_ftle for a volume: the rendered frame [H, W] (SmokeSimulator3D.render), the FTLE volume [D, H, W] of its flow
        (physics.flow_ftle3d) as its maximum over depth -- the view of the default render, along z -- and that image's upper decile as a
        contour over the frame.  Leading dimensions of size 1, or a batch whose first entry is drawn, are dropped.  torch or numpy; not
        a hot path."""
        img, vol = _numpy(frame), _numpy(ftle)
        while img.ndim > 2:
            img = img[0]
        while vol.ndim > 3:
            vol = vol[0]
        if vol.ndim != 3:
            raise ValueError(f"plot_ftle3d: ftle must be a [D, H, W] volume, got {vol.shape}")
        return self._draw_ftle("plot_ftle3d", img, vol.max(axis=0), "FTLE (max over depth)", path)

    @staticmethod
    def _draw_ftle(what, img, field, title, path):
        """The three panels of plot_ftle / plot_ftle3d: img and field [H, W] numpy arrays."""
        if img.shape != field.shape:
            raise ValueError(f"{what}: frame and ftle must have one shape, got {img.shape} and {field.shape}")
        fig, axes = plt.subplots(1, 3, figsize=(15, 5))
        axes[0].imshow(img, cmap="hot")
        axes[0].set_title("Input Smoke")
        im = axes[1].imshow(field, cmap="plasma")
        axes[1].set_title(title)
        fig.colorbar(im, ax=axes[1])
        axes[2].imshow(img, cmap="hot")
        level = float(np.quantile(field, 0.9))
        if np.isfinite(level) and float(field.max()) > level:
            axes[2].contour(field, levels=[level], colors="cyan", linewidths=1.0)
        axes[2].set_title("FTLE Upper Decile")
        for ax in axes:
            ax.axis("off")
        return _finish(fig, path)

    def plot_turntable(self, frames, azimuths, save_path: Optional[str] = None):
        """One 'hot' panel per orbit view (render_orbit's [V, H, W] frames of one volume), at most 8 per row, titled by the view's azimuth in
        degrees; all panels share one colour scale, so a view that sees less smoke looks dimmer.  Returns the figure."""
        views = _numpy(frames)
        angles = [float(a) for a in _numpy(azimuths).reshape(-1)]
        if views.ndim != 3 or len(angles) != views.shape[0] or not angles:
            raise ValueError(f"plot_turntable: frames [V, H, W] and V azimuths, got {views.shape} and {len(angles)}")
        n = len(angles)
        cols = min(8, n)
        rows = (n + cols - 1) // cols
        fig, axes = plt.subplots(rows, cols, figsize=(cols * 2, rows * 2), squeeze=False)
        for ax in axes.flat:
            ax.axis("off")
        top = max(float(views.max()), 1e-12)
        for i, (view, angle) in enumerate(zip(views, angles)):
            ax = axes[i // cols, i % cols]
            ax.imshow(view, cmap="hot", interpolation="bilinear", vmin=0.0, vmax=top)
            ax.set_title(f"{angle:g}\N{DEGREE SIGN}")
        return _finish(fig, save_path)
