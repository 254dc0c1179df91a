"""Attention maps ("Attention maps"): the `received` map of one layer -- hip_attention_maps with the forward's lse given, and
with the lse pass included -- against the same map from a materialised torch.softmax(q k^T * scale).mean(2), at 1, 8 and 64 x 1024 tokens
x 8 heads.  Reports the time of each (device events, the median of 5 windows after warm-up), the peak allocated bytes of each above the
inputs, and how far the two maps are apart.  Writes the JSON given by --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "attention_maps_probe.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from smokephysai_amd.models.attention import attention_maps_torch, hip_attention_lse, hip_attention_maps
    dev = torch.device("cuda:0")
    L, H, D = 1024, 8, 512
    scale = 0.125

    def timed(fn, warmup=3, reps=10, windows=5):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / reps)
        return float(np.median(ms)), [round(float(m), 4) for m in ms]

    def peak_bytes(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return int(peak)

    result = {"device": torch.cuda.get_device_name(0), "stamp": bench.source_stamp(), "L": L, "heads": H, "cases": []}
    for B in args.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        qkv = torch.randn(B, L, 3 * D, device=dev, generator=g)                 # the layout the q | k | v launch writes
        q, k = qkv[..., :D], qkv[..., D:2 * D]
        lse = hip_attention_lse(q, k, H, scale)
        hip = lambda: hip_attention_maps(q, k, H, scale, lse=lse)
        hip_with_lse = lambda: hip_attention_maps(q, k, H, scale)
        torch_ = lambda: attention_maps_torch(q, k, H, scale)
        apart = float((hip() - torch_()).abs().max() / torch_().abs().max())
        reps = 3 if B >= 64 else 10
        ms_hip, win_hip = timed(hip, reps=reps)
        ms_lse, win_lse = timed(hip_with_lse, reps=reps)
        ms_torch, win_torch = timed(torch_, reps=reps)
        rec = {"B": B, "hip_ms": round(ms_hip, 4), "hip_windows": win_hip, "hip_with_lse_ms": round(ms_lse, 4), "hip_with_lse_windows": win_lse,
               "torch_ms": round(ms_torch, 4), "torch_windows": win_torch, "hip_peak_bytes": peak_bytes(hip),
               "hip_with_lse_peak_bytes": peak_bytes(hip_with_lse), "torch_peak_bytes": peak_bytes(torch_), "max_rel_diff": apart}
        result["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        del qkv, q, k, lse
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
