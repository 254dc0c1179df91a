"""numpy oracle of the n-axis chaos statistics (SPEC_3D.md section 9): one code path for any number of axes, whose 2-axis instance is the
reference's rule (smoke_simulator.py:47-140) and reproduces tests/golden/chaos_stats_64.npz.  A plain helper module, not a test file.

    stats_nd(vol, mean=None) -> (mean fp32, counts int64 [5], hist int64 [256])
    diff_norm(a, b)          -> ||b - a||_2, fp64 accumulation, as fp64 (the device rounds it to fp32)
    history_features(vols)   -> the reference's get_chaos_features() on the full list of emitted volumes
"""
import numpy as np

from smokephysai_amd.physics.smoke_simulator import entropy_from_hist, fractal_dimension_from_counts, lyapunov_from_norms

SCALES = (2, 4, 8, 16, 32)


def mean_nd(vol):
    """fp64 accumulation over all cells, rounded once to fp32 (csrc/chaos.hip:3)."""
    v = np.asarray(vol, np.float32)
    return np.float32(v.astype(np.float64).sum() / v.size)


def box_counts_nd(vol, mean):
    """binary = vol > mean; boxes of edge s along every axis on the (n_k // s) grid, upper remainders ignored (smoke_simulator.py:96-115)."""
    binary = np.asarray(vol, np.float32) > np.float32(mean)
    counts = np.zeros(5, np.int64)
    for i, s in enumerate(SCALES):
        nb = [n // s for n in binary.shape]
        if min(nb) == 0:
            continue                                       # a scale with no whole box counts 0
        b = binary[tuple(slice(0, k * s) for k in nb)]
        b = b.reshape([x for k in nb for x in (k, s)])     # (n0, s, n1, s, ...)
        counts[i] = int(b.any(axis=tuple(range(1, 2 * len(nb), 2))).sum())
    return counts


def hist256(vol):
    """torch.histogram(bins=256, range=(0,1)) counts: outside [0,1] dropped (NaN too), 1.0 -> bin 255, bin = int(x * 256)."""
    x = np.asarray(vol, np.float32).ravel()
    x = x[(x >= 0) & (x <= 1)]
    b = np.minimum((x * np.float32(256.0)).astype(np.int64), 255)
    return np.bincount(b, minlength=256).astype(np.int64)


def stats_nd(vol, mean=None):
    m = mean_nd(vol) if mean is None else np.float32(mean)
    return m, box_counts_nd(vol, m), hist256(vol)


def diff_norm(a, b):
    d = np.asarray(b, np.float32).astype(np.float64) - np.asarray(a, np.float32).astype(np.float64)
    return float(np.sqrt((d * d).sum()))


def history_features(vols):
    """smoke_simulator.py:47-140 on `vols`, every emitted volume so far (the caller caps the list at 100): {} below 10 volumes, Lyapunov 0
    below 20, else from the 19 distances between the last 20 volumes (each rounded to fp32, as torch.norm of fp32 tensors returns it)."""
    if len(vols) < 10:
        return {}
    lyap = 0.0
    if len(vols) >= 20:
        st = vols[-20:]
        lyap = lyapunov_from_norms([np.float32(diff_norm(st[i], st[i + 1])) for i in range(19)])
    _, counts, hist = stats_nd(vols[-1])
    return {"lyapunov_exponent": lyap, "fractal_dimension": fractal_dimension_from_counts(counts), "entropy": entropy_from_hist(hist)}


def brute_box_counts_3d(vol, mean):
    """The reference's Python loops (smoke_simulator.py:100-113) with a third axis, literally."""
    binary = np.asarray(vol, np.float32) > np.float32(mean)
    d, h, w = binary.shape
    counts = []
    for s in SCALES:
        c = 0
        for k in range(d // s):
            for i in range(h // s):
                for j in range(w // s):
                    if binary[k * s:(k + 1) * s, i * s:(i + 1) * s, j * s:(j + 1) * s].any():
                        c += 1
        counts.append(c)
    return np.array(counts, np.int64)
