"""Time of SyntheticSmokeDataset generation on the device (reference: 1.3-4.2 s per sample on CPU), per label mode.

    python tools/dataset_probe.py [--labels host|device|both] [--samples 512] [--sizes 128 256] [--reps 5] [--out FILE.json]

For every grid size: one warm-up generation per mode, then `reps` timed generations per mode, the modes alternating inside one process
(host clock around a generation that ends in a device synchronise), then ONE more generation per mode taken apart into its phases, each
phase closed by a synchronise: stepper, reductions, feature kernel, device-to-host copies, host label loop, per-sample clones, set-up.
The split runs the generator's own steps one by one (it adds a synchronise per phase, so its sum is a little above a timed generation;
both are printed).  For kernel times run it under the profiler in a run of its own, the program after `--`:
    rocprofv3 --kernel-trace --stats -d OUTDIR -- python tools/dataset_probe.py --labels both --reps 1 --sizes 128
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smokephysai_amd.physics.smoke_simulator import SmokeSimulator, chaos_features_device, chaos_stats, frame_diff_norms
from smokephysai_amd.utils import data_loader as dl
from smokephysai_amd.utils.data_loader import HIST_TAIL, SyntheticSmokeDataset

PHASES = ("setup", "stepper", "reductions", "feature_kernel", "d2h_copies", "host_label_loop", "sample_clones")


def generate(mode, n, N):
    np.random.seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = SyntheticSmokeDataset(num_samples=n, grid_size=(N, N), device="cuda", labels=mode)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert len(ds) == n
    return dt


class Clock:
    def __init__(self):
        self.t = dict.fromkeys(PHASES, 0.0)
        torch.cuda.synchronize()
        self.last = time.perf_counter()

    def lap(self, phase):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.t[phase] += now - self.last
        self.last = now


def split(mode, n, N, sim_batch=64, T=20):
    """One generation of SyntheticSmokeDataset(labels=mode), its steps in the generator's order with a synchronise after each phase."""
    np.random.seed(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    ck = Clock()
    cfgs = dl.draw_source_configs(n, (N, N))
    data, chunk_labels, sims = [], [], {}
    tail, valid_head = None, 0
    for c0 in range(0, n, sim_batch):
        c1 = min(c0 + sim_batch, n)
        m = c1 - c0
        if mode == "device" and m in sims:
            sim = sims[m]
            sim.ns_solver.setup_grid()
        else:
            sim = sims[m] = SmokeSimulator((N, N), device=dev, batch_size=m)
        sim.ns_solver.add_smoke_sources([(i - c0, x, y, 8, inten) for i in range(c0, c1)
                                         for (x, y), inten in zip(cfgs[i]["positions"], cfgs[i]["intensities"])])
        buf = torch.empty(HIST_TAIL + m * T, N, N, device=dev)
        if tail is not None:
            buf[HIST_TAIL - tail.shape[0]:HIST_TAIL] = tail
        seqs = buf[HIST_TAIL:].view(m, T, N, N)
        ck.lap("setup")
        sim.simulate_sequence(T, add_fractal=True, out=seqs)
        ck.lap("stepper")
        if mode == "host":
            d = frame_diff_norms(buf)
            _, box, hist = chaos_stats(buf[HIST_TAIL:])
            ck.lap("reductions")
            d, box, hist = d.cpu().numpy(), box.cpu().numpy(), hist.cpu().numpy()
            ck.lap("d2h_copies")
            labels = []
            for i in range(m):
                off = min(HIST_TAIL, valid_head + i * T)
                lo = HIST_TAIL + i * T - off
                sl = slice(i * T + 10, (i + 1) * T)
                labels.append(dl.labels_from_stats(d[lo:HIST_TAIL + (i + 1) * T - 1], box[sl], hist[sl], T, off))
            ck.lap("host_label_loop")
            for i in range(m):
                data.append({"sequence": seqs[i].to(dev).clone(), "chaos_features": labels[i][0], "source_config": cfgs[c0 + i]})
        else:
            d = frame_diff_norms(buf)
            _, box, hist = chaos_stats(buf)
            ck.lap("reductions")
            rows = dl._LABEL_ROWS.get((m, T, valid_head, 10, dev))
            if rows is None:
                rows = dl._LABEL_ROWS[(m, T, valid_head, 10, dev)] = tuple(torch.from_numpy(a).to(dev) for a in dl.chaos_label_rows(m, T, valid_head))
                ck.lap("setup")
            chunk_labels.append(chaos_features_device(d, box, hist, *rows, groups=m)[1])
            ck.lap("feature_kernel")
            for i in range(m):
                data.append({"sequence": seqs[i], "chaos_features": None, "source_config": cfgs[c0 + i]})
        tail = buf[HIST_TAIL - valid_head:][-HIST_TAIL:].clone()
        valid_head = tail.shape[0]
        ck.lap("sample_clones")
        if mode == "host":
            del sim, sims[m]                                             # a simulator per chunk: its release counts as the next set-up
    if mode == "device":
        rows = torch.cat(chunk_labels).cpu().tolist()
        ck.lap("d2h_copies")
        for s, r in zip(data, rows):
            s["chaos_features"] = dict(zip(dl._LABEL_KEYS, r))
        ck.lap("host_label_loop")
    return ck.t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--labels", choices=("host", "device", "both"), default="both")
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5, help="timed generations per mode (at least 3 for a spread)")
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dataset_probe: no ROCm device; this probe measures on the GPU only")
    modes = ("host", "device") if args.labels == "both" else (args.labels,)
    n = args.samples
    import bench
    result = {"samples": n, "frames_per_sample": 20, "reps": args.reps, "device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(),
              "sizes": {}}
    for N in args.sizes:
        for mode in modes:
            generate(mode, min(n, 128), N)                               # warm-up: kernels, constants, both chunk sizes' allocations
        times = {mode: [] for mode in modes}
        for _ in range(args.reps):
            for mode in modes:                                           # alternate: drift of the box hits both modes alike
                times[mode].append(generate(mode, n, N))
        entry = {}
        for mode in modes:
            rates = sorted(n / t for t in times[mode])
            parts = split(mode, n, N)
            total = sum(parts.values())
            entry[mode] = {"samples_per_s_median": statistics.median(rates), "samples_per_s_min": rates[0], "samples_per_s_max": rates[-1],
                           "samples_per_s_all": [n / t for t in times[mode]], "frames_per_s_median": statistics.median(rates) * 20,
                           "split_ms": {k: v * 1e3 for k, v in parts.items()}, "split_total_ms": total * 1e3,
                           "split_share": {k: v / total for k, v in parts.items()},
                           "timed_generation_ms_median": statistics.median(times[mode]) * 1e3}
            e = entry[mode]
            print(f"{N}^2 labels={mode}: {n} samples x 20 frames: median {e['samples_per_s_median']:.0f} samples/s "
                  f"(min {rates[0]:.0f}, max {rates[-1]:.0f}, {args.reps} generations) = {e['frames_per_s_median']:.0f} frames/s, "
                  f"{e['timed_generation_ms_median']:.1f} ms per generation", flush=True)
            print(f"    split of one generation ({total * 1e3:.1f} ms with a synchronise per phase): " +
                  ", ".join(f"{k} {parts[k] * 1e3:.1f} ms ({parts[k] / total * 100:.0f} %)" for k in PHASES), flush=True)
        if len(modes) == 2:
            entry["device_over_host"] = entry["device"]["samples_per_s_median"] / entry["host"]["samples_per_s_median"]
            print(f"{N}^2: device / host = {entry['device_over_host']:.2f}x", flush=True)
        result["sizes"][str(N)] = entry
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
