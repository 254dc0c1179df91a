"""Synthetic smoke dataset on MI355X -- drop-in for src/utils/data_loader.py:10-184.

The reference generates `num_samples` sequences by looping a single-grid simulator in Python
(data_loader.py:44-97).  Here the same samples come from the batched HIP stepper: the source lists are drawn from
the global np.random stream in the reference's exact order (so a given seed gives the same sources), `sim_batch`
grids are simulated per launch, and the chaos-statistics labels come from the HIP reductions -- including the
reference's quirk that the simulator history is never cleared between samples (data_loader.py:46 resets only the
solver), so sample i's Lyapunov window reaches back into sample i-1's frames.
"""
import os
import pickle
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .. import _lib
from ..physics.smoke_simulator import (SmokeSimulator, chaos_features_device, chaos_stats, entropy_from_hist,
                                       fractal_dimension_from_counts, frame_diff_norms, lyapunov_from_norms, volume_stats)
from ..physics.render import RenderSettings, render_supported, render_volumes
from ..physics.smoke_simulator3d import SmokeSimulator3D
from .distributed import shard_range


def draw_source_configs(num_samples: int, grid_size: Tuple[int, int]) -> List[Dict]:
    """data_loader.py:49-58: per sample k=randint(1,4), then k x (x, y, intensity), from the global np.random."""
    cfgs = []
    for _ in range(num_samples):
        k = np.random.randint(1, 4)
        pos, inten = [], []
        for _ in range(k):
            x = np.random.randint(20, grid_size[1] - 20)
            y = np.random.randint(20, grid_size[0] - 20)
            intensity = np.random.uniform(0.5, 2.0)
            pos.append((x, y))
            inten.append(intensity)
        cfgs.append({"positions": pos, "intensities": inten})
    return cfgs


def labels_from_stats(diff_norms, box_counts, hists, T: int, off: int, start: int = 10) -> Tuple[dict, List[dict]]:
    """Host part of the labels (data_loader.py:71-88 + smoke_simulator.py:47-140's scalar formulas).
    diff_norms: distances between consecutive frames of the extended history (off frames of the previous sample, then
    this sample's T frames); box_counts / hists: per frame t = start..T-1."""
    d = np.asarray(diff_norms, dtype=np.float64)
    feats = []
    for t in range(start, T):
        e = off + t                                        # index of frame t in the history; history length = e + 1
        if e + 1 < 10:
            continue                                       # smoke_simulator.py:49-50 -> {} (not appended)
        lyap = 0.0
        if e + 1 >= 20:                                    # smoke_simulator.py:69-70
            lyap = lyapunov_from_norms(d[e - 19:e])        # 19 distances between the last 20 frames
        feats.append({"lyapunov_exponent": lyap,
                      "fractal_dimension": fractal_dimension_from_counts(box_counts[t - start]),
                      "entropy": entropy_from_hist(hists[t - start])})
    if feats:
        avg = {k: np.mean([f[k] for f in feats]) for k in ("lyapunov_exponent", "fractal_dimension", "entropy")}
    else:
        avg = {"lyapunov_exponent": 0.0, "fractal_dimension": 1.0, "entropy": 0.0}
    return avg, feats


def chaos_labels(seq: torch.Tensor, prev_tail: Optional[torch.Tensor], start: int = 10) -> Tuple[dict, List[dict]]:
    """Labels of one sample: average over t=start..T-1 of get_chaos_features() (data_loader.py:71-88).
    seq [T,H,W] on the device; prev_tail = the frames the simulator history held before this sample (19 are used)."""
    T = seq.shape[0]
    ext = seq if prev_tail is None or prev_tail.shape[0] == 0 else torch.cat([prev_tail[-19:], seq])
    off = ext.shape[0] - T
    d = frame_diff_norms(ext).cpu().numpy()
    _, box, hist = chaos_stats(seq[start:])
    return labels_from_stats(d, box.cpu().numpy(), hist.cpu().numpy(), T, off, start)


HIST_TAIL = 19      # frames of earlier samples a Lyapunov window can reach back into (smoke_simulator.py:69-79: the last 20 states)


def chunk_chaos_labels(buf: torch.Tensor, n_samples: int, T: int, valid_head: int, start: int = 10) -> List[Tuple[dict, List[dict]]]:
    """Labels of a whole chunk of samples from ONE pass of each reduction and one device-to-host copy per result.

    buf [HIST_TAIL + n_samples * T, H, W]: the last HIST_TAIL frames the simulator history held before this chunk (only the final
    `valid_head` of them are real), then the chunk's samples back to back -- the order in which the reference's never-cleared history
    sees them (data_loader.py:46 resets only the solver), so the distance between the last frame of sample i-1 and the first of sample i
    is simply one more pair of the flat stream.  Launches: smk_frame_diff_norms over the stream, smk_chaos_stats over the chunk's
    frames (all T per sample; t < start is 2x redundant work on a reduction that costs microseconds, and keeps one frame stride)."""
    frames = buf[HIST_TAIL:]
    d = frame_diff_norms(buf).cpu().numpy()                                   # d[k] = ||buf[k+1] - buf[k]||
    _, box, hist = chaos_stats(frames)
    box, hist = box.cpu().numpy(), hist.cpu().numpy()
    out = []
    for i in range(n_samples):
        off = min(HIST_TAIL, valid_head + i * T)                              # earlier frames the history holds for this sample
        lo = HIST_TAIL + i * T - off                                          # buf index of the first of them
        sl = slice(i * T + start, (i + 1) * T)
        out.append(labels_from_stats(d[lo:HIST_TAIL + (i + 1) * T - 1], box[sl], hist[sl], T, off, start))
    return out


def chaos_label_rows(n_samples: int, T: int, valid_head: int, start: int = 10) -> Tuple[np.ndarray, np.ndarray]:
    """The feature rows of a chunk buffer (layout: chunk_chaos_labels) as smk_chaos_features wants them: for sample i and frame
    t = start..T-1, in that order, the buffer index of the frame and the length of the history the reference's simulator holds
    once it has appended that frame -- labels_from_stats' `e + 1` with off = min(HIST_TAIL, valid_head + i * T); only "below 10"
    and "below 20" are ever asked of it, so the cap at HIST_TAIL earlier frames changes nothing.  int32 [n_samples * (T - start)]."""
    i = np.repeat(np.arange(n_samples), max(T - start, 0))
    t = np.tile(np.arange(start, T), n_samples)
    off = np.minimum(HIST_TAIL, valid_head + i * T)
    return (HIST_TAIL + i * T + t).astype(np.int32), (off + t + 1).astype(np.int32)


_LABEL_ROWS = {}     # (n_samples, T, valid_head, start, device) -> chaos_label_rows on that device: built once per shape


def chunk_chaos_labels_device(buf: torch.Tensor, n_samples: int, T: int, valid_head: int, start: int = 10) -> torch.Tensor:
    """chunk_chaos_labels without the host: the same buffer, the same two reductions (the statistics over the whole buffer, so
    that one frame index serves all three results), then one smk_chaos_features launch for the scalars of every frame
    t = start..T-1 and their per-sample means.  Returns [n_samples, 3] fp64 on the device (lyapunov, fractal dimension, entropy).
    start >= 9 only: below that labels_from_stats skips frames whose history is shorter than 10, which is not emulated."""
    if start < 9:
        raise ValueError(f"start={start}: frames with fewer than 10 frames of history are skipped by the host route; use start >= 9")
    if tuple(buf.shape[:1]) != (HIST_TAIL + n_samples * T,) or not 0 <= valid_head <= HIST_TAIL:
        raise ValueError(f"buf must hold HIST_TAIL + n_samples * T = {HIST_TAIL + n_samples * T} frames, valid_head in 0..{HIST_TAIL}")
    dev = _lib.require_cuda(buf.device, "chunk_chaos_labels_device")
    if T <= start:                                                            # no frame contributes: labels_from_stats' defaults
        return torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64, device=dev).repeat(n_samples, 1)
    key = (n_samples, T, valid_head, start, dev)
    if key not in _LABEL_ROWS:
        _LABEL_ROWS[key] = tuple(torch.from_numpy(a).to(dev) for a in chaos_label_rows(n_samples, T, valid_head, start))
    norms = frame_diff_norms(buf)
    _, box, hist = chaos_stats(buf)              # the HIST_TAIL head frames too (never read by a row): one index for all results
    return chaos_features_device(norms, box, hist, *_LABEL_ROWS[key], groups=n_samples)[1]


_LABEL_KEYS = ("lyapunov_exponent", "fractal_dimension", "entropy")


class SyntheticSmokeDataset(Dataset):
    """Same constructor/items as the reference (data_loader.py:13-123).  Extra keyword-only knobs:
    sim_batch (grids per launch), jacobi_iters, storage_device (where sequences are kept; default = device),
    rank/world (generate and hold only this rank's contiguous block of the global sample list),
    labels ("host": the label formulas run in numpy on copied-back reduction results, as the reference computes them;
    "device": they run in one HIP launch per chunk and come to the host once, after the last chunk -- same frames, same
    sources, labels equal to ~1e-6 (entropy is fp32 on the host route); items and caches have the same schema either way)."""

    def __init__(self, num_samples: int = 1000, grid_size: Tuple[int, int] = (128, 128), sequence_length: int = 20,
                 device: str = "cuda", cache_path: Optional[str] = None, *, sim_batch: int = 64, jacobi_iters: int = 20,
                 storage_device: Optional[str] = None, rank: int = 0, world: int = 1, labels: str = "host"):
        if labels not in ("host", "device"):
            raise ValueError(f"labels={labels!r}: 'host' or 'device'")
        self.labels = labels
        self.num_samples = num_samples
        self.grid_size = tuple(grid_size)
        self.sequence_length = sequence_length
        self.device = device
        self.cache_path = cache_path
        self.sim_batch = sim_batch
        self.jacobi_iters = jacobi_iters
        self.storage_device = storage_device if storage_device is not None else device
        self.rank, self.world = rank, world
        if self.cache_path and os.path.exists(self.cache_path):
            with open(self.cache_path, "rb") as f:
                self.data = pickle.load(f)
            print(f"Loaded synthetic data from {self.cache_path}")
        else:
            self.data = self._generate_synthetic_data()
            if self.cache_path:
                os.makedirs(os.path.dirname(self.cache_path) or ".", exist_ok=True)
                with open(self.cache_path, "wb") as f:
                    pickle.dump([dict(d, sequence=d["sequence"].cpu()) for d in self.data], f)
                print(f"Saved synthetic data to {self.cache_path}")

    def _generate_synthetic_data(self) -> List[Dict]:
        if self.labels == "device":
            return self._generate_device_labels()
        dev = _lib.require_cuda(self.device, "SyntheticSmokeDataset")
        cfgs = draw_source_configs(self.num_samples, self.grid_size)       # every rank draws the full list
        lo, hi = shard_range(self.num_samples, self.rank, self.world)
        first = max(lo - 1, 0)                                              # one extra sample: its frames seed the history
        data = []
        T = self.sequence_length
        H, W = self.grid_size
        tail, valid_head = None, 0                                          # the history's last HIST_TAIL frames before the chunk
        for c0 in range(first, hi, self.sim_batch):
            c1 = min(c0 + self.sim_batch, hi)
            n = c1 - c0
            sim = SmokeSimulator(self.grid_size, device=dev, batch_size=n, jacobi_iters=self.jacobi_iters)
            srcs = [(i - c0, x, y, 8, inten) for i in range(c0, c1)
                    for (x, y), inten in zip(cfgs[i]["positions"], cfgs[i]["intensities"])]
            sim.ns_solver.add_smoke_sources(srcs)
            # one buffer per chunk: [history tail | sample 0's T frames | sample 1's ...]; the stepper writes the frames in place
            buf = torch.empty(HIST_TAIL + n * T, H, W, device=dev)
            if tail is not None:
                buf[HIST_TAIL - tail.shape[0]:HIST_TAIL] = tail
            seqs = buf[HIST_TAIL:].view(n, T, H, W)
            sim.simulate_sequence(T, add_fractal=True, out=seqs)            # raises here if a persistent projection timed out
            labels = chunk_chaos_labels(buf, n, T, valid_head)
            for i in range(c0, c1):
                if i >= lo:
                    data.append({"sequence": seqs[i - c0].to(self.storage_device).clone(), "chaos_features": labels[i - c0][0],
                                 "source_config": cfgs[i]})
            # the reference's history keeps the last 100 frames across samples (smoke_simulator.py:41-43); 19 can matter
            tail = buf[HIST_TAIL - valid_head:][-HIST_TAIL:].clone()        # (buf[HIST_TAIL - valid_head:] = every real frame in the buffer)
            valid_head = tail.shape[0]
            del sim
        return data

    def _generate_device_labels(self) -> List[Dict]:
        """The generator above with the labels left on the device (chunk_chaos_labels_device): no copy to the host and no host
        formula per chunk, one [samples, 3] copy at the end.  Same draws, chunks, buffers and stepper calls, so the frames are
        the host mode's bit for bit.  Also dropped, because they change no result: the simulator is built once per chunk size
        and zeroed between chunks (setup_grid) instead of created per chunk, and with storage_device == device a sample is a
        view of its chunk buffer instead of a copy."""
        dev = _lib.require_cuda(self.device, "SyntheticSmokeDataset")
        cfgs = draw_source_configs(self.num_samples, self.grid_size)
        lo, hi = shard_range(self.num_samples, self.rank, self.world)
        first = max(lo - 1, 0)
        T = self.sequence_length
        H, W = self.grid_size
        in_place = torch.device(self.storage_device) == dev or str(self.storage_device) == str(self.device)
        data, chunk_labels, sims = [], [], {}
        tail, valid_head = None, 0
        for c0 in range(first, hi, self.sim_batch):
            c1 = min(c0 + self.sim_batch, hi)
            n = c1 - c0
            if n in sims:
                sim = sims[n]
                sim.ns_solver.setup_grid()
            else:
                sim = sims[n] = SmokeSimulator(self.grid_size, device=dev, batch_size=n, jacobi_iters=self.jacobi_iters)
            sim.ns_solver.add_smoke_sources([(i - c0, x, y, 8, inten) for i in range(c0, c1)
                                             for (x, y), inten in zip(cfgs[i]["positions"], cfgs[i]["intensities"])])
            buf = torch.empty(HIST_TAIL + n * T, H, W, device=dev)
            if tail is not None:
                buf[HIST_TAIL - tail.shape[0]:HIST_TAIL] = tail
            seqs = buf[HIST_TAIL:].view(n, T, H, W)
            sim.simulate_sequence(T, add_fractal=True, out=seqs)
            chunk_labels.append(chunk_chaos_labels_device(buf, n, T, valid_head)[max(lo - c0, 0):])
            for i in range(max(c0, lo), c1):
                seq = seqs[i - c0]
                data.append({"sequence": seq if in_place else seq.to(self.storage_device).clone(), "chaos_features": None,
                             "source_config": cfgs[i]})
            tail = buf[HIST_TAIL - valid_head:][-HIST_TAIL:].clone()
            valid_head = tail.shape[0]
        if data:
            for d, row in zip(data, torch.cat(chunk_labels).cpu().tolist()):     # the one device-to-host copy of the labels
                d["chaos_features"] = dict(zip(_LABEL_KEYS, row))
        return data

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, idx: int) -> Dict:
        sample = self.data[idx]
        frame_idx = np.random.randint(5, self.sequence_length - 5)         # data_loader.py:108
        return {"input": sample["sequence"][frame_idx].unsqueeze(0),
                "target": sample["sequence"][frame_idx + 1].unsqueeze(0),
                "chaos_features": torch.tensor([sample["chaos_features"]["lyapunov_exponent"],
                                                sample["chaos_features"]["fractal_dimension"],
                                                sample["chaos_features"]["entropy"]], dtype=torch.float32),
                "sequence": sample["sequence"]}


# ---- 3-D volumes (BASELINE configs[4]; SPEC_3D.md section 9) ---------------------------------------------------------------------------
def draw_source_configs3d(num_samples: int, grid_size: Tuple[int, int, int]) -> List[Dict]:
    """data_loader.py:49-58 with a depth index: per sample k=randint(1,4), then k x (x, y, z, intensity) in that order from the global
    np.random; z keeps the 20-cell margin where the depth allows it, m = min(20, D // 4)."""
    D, H, W = grid_size
    m = min(20, D // 4)
    cfgs = []
    for _ in range(num_samples):
        k = np.random.randint(1, 4)
        pos, inten = [], []
        for _ in range(k):
            x = np.random.randint(20, W - 20)
            y = np.random.randint(20, H - 20)
            z = np.random.randint(m, D - m)
            intensity = np.random.uniform(0.5, 2.0)
            pos.append((x, y, z))
            inten.append(intensity)
        cfgs.append({"positions": pos, "intensities": inten})
    return cfgs


def chunk_chaos_labels_device3d(buf: torch.Tensor, n_samples: int, T: int, valid_head: int, start: int = 10) -> torch.Tensor:
    """chunk_chaos_labels_device for a chunk buffer of volumes [HIST_TAIL + n_samples * T, D, H, W]: one smk_volume_stats call over the
    whole buffer (statistics and distances), then the same smk_chaos_features launch on the same rows.  [n_samples, 3] fp64, on the device."""
    if start < 9:
        raise ValueError(f"start={start}: frames with fewer than 10 frames of history are skipped by the host route; use start >= 9")
    if buf.dim() != 4 or buf.shape[0] != HIST_TAIL + n_samples * T or not 0 <= valid_head <= HIST_TAIL:
        raise ValueError(f"buf must hold HIST_TAIL + n_samples * T = {HIST_TAIL + n_samples * T} volumes, valid_head in 0..{HIST_TAIL}")
    dev = _lib.require_cuda(buf.device, "chunk_chaos_labels_device3d")
    if T <= start:
        return torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64, device=dev).repeat(n_samples, 1)
    key = (n_samples, T, valid_head, start, dev)
    if key not in _LABEL_ROWS:
        _LABEL_ROWS[key] = tuple(torch.from_numpy(a).to(dev) for a in chaos_label_rows(n_samples, T, valid_head, start))
    _, box, hist, norms = volume_stats(buf, norms=True)
    return chaos_features_device(norms, box, hist, *_LABEL_ROWS[key], groups=n_samples)[1]


class SyntheticSmokeDataset3D(Dataset):
    """SyntheticSmokeDataset for volumes: the same item schema (input / target [1,D,H,W], chaos_features [3], sequence [T,D,H,W]) and the
    same sim_batch, jacobi_iters, storage_device and rank/world knobs.  Sources: draw_source_configs3d.  The labels are computed on
    the device only (chunk_chaos_labels_device3d) and come to the host once; the never-cleared-history quirk across samples is kept
    (data_loader.py:46 resets only the solver)."""

    def __init__(self, num_samples: int = 100, grid_size: Tuple[int, int, int] = (64, 128, 128), sequence_length: int = 20,
                 device: str = "cuda", cache_path: Optional[str] = None, *, sim_batch: int = 8, jacobi_iters: int = 20,
                 storage_device: Optional[str] = None, rank: int = 0, world: int = 1):
        self.num_samples = num_samples
        self.grid_size = tuple(grid_size)
        if len(self.grid_size) != 3:
            raise ValueError("grid_size must be (D, H, W)")
        self.sequence_length = sequence_length
        self.device = device
        self.cache_path = cache_path
        self.sim_batch = sim_batch
        self.jacobi_iters = jacobi_iters
        self.storage_device = storage_device if storage_device is not None else device
        self.rank, self.world = rank, world
        if self.cache_path and os.path.exists(self.cache_path):
            with open(self.cache_path, "rb") as f:
                self.data = pickle.load(f)
            print(f"Loaded synthetic data from {self.cache_path}")
        else:
            self.data = self._generate_synthetic_data()
            if self.cache_path:
                os.makedirs(os.path.dirname(self.cache_path) or ".", exist_ok=True)
                with open(self.cache_path, "wb") as f:
                    pickle.dump([dict(d, sequence=d["sequence"].cpu()) for d in self.data], f)
                print(f"Saved synthetic data to {self.cache_path}")

    def _generate_synthetic_data(self) -> List[Dict]:
        dev = _lib.require_cuda(self.device, "SyntheticSmokeDataset3D")
        cfgs = draw_source_configs3d(self.num_samples, self.grid_size)      # every rank draws the full list
        lo, hi = shard_range(self.num_samples, self.rank, self.world)
        first = max(lo - 1, 0)                                              # one extra sample: its volumes seed the history
        T = self.sequence_length
        in_place = torch.device(self.storage_device) == dev or str(self.storage_device) == str(self.device)
        data, chunk_labels, sims = [], [], {}
        tail, valid_head = None, 0
        for c0 in range(first, hi, self.sim_batch):
            c1 = min(c0 + self.sim_batch, hi)
            n = c1 - c0
            if n in sims:
                sim = sims[n]
                sim.ns_solver.setup_grid()
            else:
                sim = sims[n] = SmokeSimulator3D(self.grid_size, device=dev, batch_size=n, jacobi_iters=self.jacobi_iters)
            sim.ns_solver.add_smoke_sources([(i - c0, x, y, z, 8, inten) for i in range(c0, c1)
                                             for (x, y, z), inten in zip(cfgs[i]["positions"], cfgs[i]["intensities"])])
            # one buffer per chunk: [history tail | sample 0's T volumes | sample 1's ...]; the stepper writes the volumes in place
            buf = torch.empty(HIST_TAIL + n * T, *self.grid_size, device=dev)
            buf[:HIST_TAIL].zero_()                                         # slots no row reads, but the reductions run over them
            if tail is not None:
                buf[HIST_TAIL - tail.shape[0]:HIST_TAIL] = tail
            seqs = buf[HIST_TAIL:].view(n, T, *self.grid_size)
            sim.simulate_sequence(T, add_fractal=True, out=seqs)
            chunk_labels.append(chunk_chaos_labels_device3d(buf, n, T, valid_head)[max(lo - c0, 0):])
            stored = self._stored_sequences(seqs)
            for i in range(max(c0, lo), c1):
                seq = stored[i - c0]
                data.append({"sequence": seq if in_place else seq.to(self.storage_device).clone(), "chaos_features": None,
                             "source_config": cfgs[i]})
            tail = buf[HIST_TAIL - valid_head:][-HIST_TAIL:].clone()
            valid_head = tail.shape[0]
        if data:
            for d, row in zip(data, torch.cat(chunk_labels).cpu().tolist()):     # the one device-to-host copy of the labels
                d["chaos_features"] = dict(zip(_LABEL_KEYS, row))
        return data

    def _stored_sequences(self, seqs: torch.Tensor) -> torch.Tensor:
        """What a sample keeps of its chunk's volumes [n, T, D, H, W]: here the volumes themselves (views of the chunk buffer)."""
        return seqs

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, idx: int) -> Dict:
        sample = self.data[idx]
        frame_idx = np.random.randint(5, self.sequence_length - 5)         # data_loader.py:108
        return {"input": sample["sequence"][frame_idx].unsqueeze(0),
                "target": sample["sequence"][frame_idx + 1].unsqueeze(0),
                "chaos_features": torch.tensor([sample["chaos_features"][k] for k in _LABEL_KEYS], dtype=torch.float32),
                "sequence": sample["sequence"]}


def as_render_settings(render) -> RenderSettings:
    """None (the defaults), a RenderSettings, or a mapping of its fields (the `mi355x.render` section of a config)."""
    if render is None:
        return RenderSettings()
    if isinstance(render, RenderSettings):
        return render
    return RenderSettings(**dict(render))


class RenderedSmokeDataset(SyntheticSmokeDataset3D):
    """Camera frames of simulated 3-D smoke with the labels of the 3-D flow, in SyntheticSmokeDataset's 2-D item schema (input / target
    [1,H,W], chaos_features [3], sequence [T,H,W]): what SmokePhysNet and train.py consume.  Draws, chunks, stepper calls and device
    labels are SyntheticSmokeDataset3D's, so the frames are the render (SPEC_3D.md section 10) of that dataset's volumes bit for bit and
    the labels are its labels.  A sample keeps its T frames, never its volumes: one render_volumes call per chunk buffer, which is then
    dropped.  grid_size is (D, H, W); render: RenderSettings, a mapping of its fields, or None for the defaults."""

    def __init__(self, num_samples: int = 100, grid_size: Tuple[int, int, int] = (64, 128, 128), sequence_length: int = 20,
                 device: str = "cuda", cache_path: Optional[str] = None, *, render=None, **kwargs):
        self.render = as_render_settings(render)                            # a bad value raises here, before any device work
        if len(tuple(grid_size)) != 3:
            raise ValueError("grid_size must be (D, H, W)")
        if not render_supported(*(int(s) for s in grid_size)):
            raise ValueError(f"RenderedSmokeDataset: grid_size={tuple(grid_size)} cannot be rendered (1 <= D <= 64)")
        super().__init__(num_samples, grid_size, sequence_length, device, cache_path, **kwargs)

    def _stored_sequences(self, seqs: torch.Tensor) -> torch.Tensor:
        return render_volumes(seqs, self.render)                            # [n, T, D, H, W] -> [n, T, H, W], a tensor of its own


class VolumeFrameDataset(SyntheticSmokeDataset3D):
    """Volumes in, camera frames out: the samples SmokePhysNet3D trains on (SPEC_3D.md section 11).  Draws, chunks, stepper calls and device
    labels are SyntheticSmokeDataset3D's, the frames RenderedSmokeDataset's.  Item: input [1,D,H,W] the emitted volume t, target [1,H,W] the
    render (section 10) of volume t + 1, sequence [T,H,W] the rendered frames, chaos_features [3] -- a 2-D target, so the loss, the physics
    regulariser and the HIP loss kernels apply unchanged.  A sample keeps its T frames and only the volumes __getitem__ can draw,
    sequence[5 : T - 5] (randint(5, T - 5)), as a copy of their own: the chunk buffer of all T volumes is dropped."""

    def __init__(self, num_samples: int = 100, grid_size: Tuple[int, int, int] = (64, 128, 128), sequence_length: int = 20,
                 device: str = "cuda", cache_path: Optional[str] = None, *, render=None, **kwargs):
        self.render = as_render_settings(render)
        if len(tuple(grid_size)) != 3:
            raise ValueError("grid_size must be (D, H, W)")
        if not render_supported(*(int(s) for s in grid_size)):
            raise ValueError(f"VolumeFrameDataset: grid_size={tuple(grid_size)} cannot be rendered (1 <= D <= 64)")
        if sequence_length < 11:
            raise ValueError("VolumeFrameDataset: sequence_length >= 11 (an item is drawn from volumes 5 .. T - 6)")
        super().__init__(num_samples, grid_size, sequence_length, device, cache_path, **kwargs)

    def _generate_synthetic_data(self) -> List[Dict]:
        self._chunk_volumes = []
        data = super()._generate_synthetic_data()
        rows = [v for chunk in self._chunk_volumes for v in chunk]          # one entry per simulated sample, the history seed included
        del self._chunk_volumes
        for d, v in zip(data, rows[len(rows) - len(data):]):
            d["volumes"] = v
        return data

    def _stored_sequences(self, seqs: torch.Tensor) -> torch.Tensor:
        T = self.sequence_length
        self._chunk_volumes.append(seqs[:, 5:T - 5].to(self.storage_device).clone())       # [n, T - 10, D, H, W]
        return render_volumes(seqs, self.render)

    def __getitem__(self, idx: int) -> Dict:
        sample = self.data[idx]
        frame_idx = np.random.randint(5, self.sequence_length - 5)         # data_loader.py:108
        return {"input": sample["volumes"][frame_idx - 5].unsqueeze(0),
                "target": sample["sequence"][frame_idx + 1].unsqueeze(0),
                "chaos_features": torch.tensor([sample["chaos_features"][k] for k in _LABEL_KEYS], dtype=torch.float32),
                "sequence": sample["sequence"]}


def create_data_loaders(batch_size: int = 16, num_train: int = 800, num_val: int = 200,
                        grid_size: Tuple[int, int] = (128, 128), device: str = "cuda", cache_dir: Optional[str] = None,
                        render_depth: int = 0, render=None, volume_depth: int = 0, **dataset_kwargs) -> Tuple[DataLoader, DataLoader]:
    """data_loader.py:126-184.  Sequences live on the device, so the loaders run in-process (num_workers=0): the
    reference forks workers only after generation, and forking after HIP initialisation is not allowed here.
    render_depth = D > 0: the samples are RenderedSmokeDataset((D, H, W)) -- camera frames of 3-D smoke under the settings `render`, same
    item schema; its labels are computed on the device (`labels` is not forwarded), and its caches carry their own names.
    volume_depth = D > 0: the samples are VolumeFrameDataset((D, H, W)) -- the volume as the input, the rendered next frame as the target
    (SmokePhysNet3D's training data); caches again under names of their own.  Both depths at once is an error."""
    rank, world = dataset_kwargs.get("rank", 0), dataset_kwargs.get("world", 1)
    suffix = "" if world == 1 else f".rank{rank}of{world}"
    if render_depth and volume_depth:
        raise ValueError("render_depth (frames of 3-D smoke into the 2-D model) and volume_depth (volumes into the 3-D model) exclude each other")
    if render_depth or volume_depth:
        depth = int(render_depth or volume_depth)
        if depth < 0:
            raise ValueError(f"render_depth / volume_depth = {depth}: 0 (2-D simulator) or the depth D of the simulated grid")
        rs = as_render_settings(render)
        tag = f".{'volume' if volume_depth else 'render'}{depth}_{rs.light}_{rs.sigma_view:g}_{rs.sigma_light:g}_{rs.ambient:g}_{rs.gain:g}"
        kw = {k: v for k, v in dataset_kwargs.items() if k != "labels"}
        grid3 = (depth,) + tuple(grid_size)
        cls = VolumeFrameDataset if volume_depth else RenderedSmokeDataset

        def make(num, name):
            return cls(num_samples=num, grid_size=grid3, device=device, render=rs,
                                        cache_path=os.path.join(cache_dir, f"{name}{tag}{suffix}.pkl") if cache_dir else None, **kw)
    else:
        def make(num, name):
            return SyntheticSmokeDataset(num_samples=num, grid_size=grid_size, device=device,
                                         cache_path=os.path.join(cache_dir, f"{name}{suffix}.pkl") if cache_dir else None, **dataset_kwargs)
    train_dataset = make(num_train, "train_data")
    val_dataset = make(num_val, "val_data")
    train_loader = DataLoader(train_dataset, batch_size=batch_size, shuffle=True, num_workers=0)
    val_loader = DataLoader(val_dataset, batch_size=batch_size, shuffle=False, num_workers=0)
    return train_loader, val_loader
