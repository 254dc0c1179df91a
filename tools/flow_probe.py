"""Times of the optical-flow baselines (csrc/flow.hip) for 64 frame pairs at 128 x 128 and 256 x 256, one process:

  1. each method as benchmark.py calls it (flow, then warp + error), per pair;
  2. each stage through its own library call: level image, polynomial expansion and one iteration per pyramid level, the warp, the
     eigenvalue map, corner selection, tracking and the scatter.
Device events, 5 windows of 20 calls after warm-up, the median reported.  Beside each stage: the bytes it has to move over the
6.29 TB/s float4-copy rate of the MI355X.  One JSON line per measurement, all of them also written to argv[1]
(default profiles/r16/flow_probe.json).  The reference's 3.98 ms (Farneback) and 0.71 ms (Lucas-Kanade) per pair are CPU OpenCV figures."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import optical_flow_oracle as ofo
from smokephysai_amd.evaluation import optical_flow as of

COPY_RATE = 6.29e12              # bytes / s, float4 copy
WINDOWS, CALLS, PAIRS = 5, 20, 64
dev = torch.device("cuda:0")
results = []


def emit(rec):
    results.append(rec)
    print(json.dumps(rec), flush=True)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / CALLS)
    return float(np.median(ms)), [round(float(x), 4) for x in ms]


def stage(size, what, fn, need):
    med, win = timed(fn)
    emit({"what": what, "pairs": PAIRS, "size": size, "ms": round(med, 4), "windows": win, "bytes_needed": int(need),
          "ms_at_copy_rate": round(need / COPY_RATE * 1e3, 5)})


for N in (128, 256):
    frames = [np.stack([ofo.shifted_pair(N, N, seed=100 + i, shift=(2, -1))[j] for i in range(PAIRS)]) for j in range(2)]
    prev, nxt = (torch.from_numpy(f).to(dev) for f in frames)
    px = PAIRS * N * N
    for name, fn in (("Farneback", of.farneback_optical_flow), ("Lucas-Kanade", of.lucas_kanade_optical_flow)):
        med, win = timed(lambda: of.predict_and_score(prev, fn(prev, nxt), nxt))
        emit({"what": "method", "method": name, "pairs": PAIRS, "size": N, "ms_per_pair": round(med / PAIRS, 5), "ms": round(med, 4),
              "windows": win, "note": "flow + warp + error, workspace allocation included, as benchmark.evaluate_traditional_cv calls it"})
    flow = of.farneback_optical_flow(prev, nxt)
    stage(N, "warp + error", lambda: of.predict_and_score(prev, flow, nxt), px * (1 + 8 + 1 + 1))
    for k in range(ofo.level_count(N, N)):
        h, w = ofo.level_size(N, N, k)
        lp = PAIRS * h * w
        img0, img1 = of.level_image(prev, k), of.level_image(nxt, k)
        stage(N, f"level image {k}", lambda: of.level_image(prev, k), px * (1 + (8 if k else 0)) + lp * 4)
        c0, c1 = of.poly_expansion(img0), of.poly_expansion(img1)
        stage(N, f"polynomial expansion, level {k}", lambda: of.poly_expansion(img0), lp * 24)
        f0 = torch.zeros(PAIRS, h, w, 2, device=dev)
        stage(N, f"matrix update + box mean + solve, level {k} (with the flow's copy)", lambda: of.farneback_iteration(c0, c1, f0),
              lp * (40 + 8 + 20 + 20 + 8 + 16))
    eig = of.min_eigen_map(prev)
    stage(N, "eigenvalue map", lambda: of.min_eigen_map(prev), px * 5)
    pts, counts = of.good_features(eig)
    stage(N, "corner selection", lambda: of.good_features(eig), px * 4)
    out, status = of.lk_track(prev, nxt, pts, counts)
    stage(N, "pyramids + tracking", lambda: of.lk_track(prev, nxt, pts, counts), 2 * px * (1 + 4 + 1 + 0.25 + 0.25 + 0.0625))
    stage(N, "scatter (with the field's zero fill)", lambda: of.lk_scatter(pts, out, status, counts, N, N), px * 8)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16", "flow_probe.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "windows": WINDOWS, "calls_per_window": CALLS, "results": results}, f, indent=1)
