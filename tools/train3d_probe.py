"""A/B of training the 3-D encoder (SPEC_3D.md section 11): Encoder3D's hip route (csrc/conv3d_train.hip) against its torch route
(PyTorch-ROCm's nn.Conv3d / nn.BatchNorm3d on MIOpen: what a user had before), forward + backward.

    python tools/train3d_probe.py [--cases 8x16x128x128,2x64x128x128] [--rounds 3] [--steps 3] [--out profiles/r17/train3d_probe.json]
                                  [--no-trace] [--no-step]

Every measurement runs in a child process with a time limit; the first child that fails ends the probe.  Per case B x D x H x W:
  first   one fresh child per route: wall time of its first forward + backward (library load; on the torch route MIOpen's find pass) and
          of its second -- reported apart, never averaged into the steady numbers;
  steady  one child, both routes on the same weights: after two warm-up passes per route, `rounds` windows per route, alternated, of
          `steps` forward + backward passes each between device events; median and spread (max - min) of the ms per pass.  The hip route
          "wins" when its median is below the torch route's by more than the larger of the two spreads;
  passes  the three conv2 kernels and conv1's forward alone (device events, median of `rounds` windows) and their counted TFLOP/s from the
          per-voxel FLOP counts (conv2 forward / data gradient / weight gradient 442,368 each, conv1 forward 43,904), and conv1's weight
          gradient (the explicit route) as a share of the encoder's backward;
  kernels (first case only) one `rocprofv3 --kernel-trace --stats` run of its own over three hip passes: time per kernel name.
step      the full train.py step (default SmokePhysNet3D body, AdamW, clip) at batch 8 of 16 x 128 x 128 volumes on both routes, alternated.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOP = {"conv2_forward": 442368, "conv2_dgrad": 442368, "conv2_wgrad": 442368, "conv1_forward": 43904}


def _encoders(torch, dev):
    import copy
    from smokephysai_amd.models import Encoder3D
    torch.manual_seed(0)
    hip = Encoder3D(route="hip").to(dev).train()
    ref = copy.deepcopy(hip)
    ref.route = "torch"
    return hip, ref


def _inputs(torch, shape, dev):
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand(shape[0], 1, *shape[1:], device=dev, generator=g)
    r = torch.randn(shape[0], 1024, 128, device=dev, generator=g)
    return x, r


def _pass(enc, x, r):
    for p in enc.parameters():
        p.grad = None
    (enc.tokens(x) * r).sum().backward()


def _windows(torch, fns, rounds, steps):
    """fns: {name: callable}.  `rounds` windows per name, alternated; ms per call of each window."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / steps)
    return out


def _summary(ms):
    return {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "windows_ms": ms}


def child_first(shape, route):
    t0 = time.perf_counter()
    import torch
    dev = torch.device("cuda:0")
    hip, ref = _encoders(torch, dev)
    enc = hip if route == "hip" else ref
    x, r = _inputs(torch, shape, dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _pass(enc, x, r)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    _pass(enc, x, r)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return {"setup_s": t1 - t0, "first_pass_s": t2 - t1, "second_pass_s": t3 - t2}


def child_steady(shape, rounds, steps):
    import torch
    from smokephysai_amd.models import encoder3d as E
    dev = torch.device("cuda:0")
    hip, ref = _encoders(torch, dev)
    x, r = _inputs(torch, shape, dev)
    fns = {"hip": lambda: _pass(hip, x, r), "torch": lambda: _pass(ref, x, r)}
    for fn in fns.values():
        fn(); fn()
    res = {k: _summary(v) for k, v in _windows(torch, fns, rounds, steps).items()}
    gap = res["torch"]["median_ms"] - res["hip"]["median_ms"]
    res["hip_wins"] = bool(gap > max(res["hip"]["spread_ms"], res["torch"]["spread_ms"]))
    res["peak_memory_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    res["device"], res["torch_version"] = torch.cuda.get_device_name(0), torch.__version__
    # the kernels alone
    B, D, H, W = shape
    vox = B * D * H * W
    g = torch.Generator(device=dev).manual_seed(6)
    vol = x[:, 0].contiguous()
    a1 = torch.relu(torch.randn(B, D, H, W, 64, device=dev, generator=g))
    dz2 = torch.randn(B, D, H, W, 128, device=dev, generator=g)
    dz1 = torch.randn(B, D, H, W, 64, device=dev, generator=g)
    c1, c2 = hip.net[0], hip.net[3]
    w1, b1, w2, b2 = (t.detach() for t in (c1.weight, c1.bias, c2.weight, c2.bias))
    kern = {"conv2_forward": lambda: E.hip_conv3d_cl_forward_raw(a1, w2, b2), "conv2_dgrad": lambda: E.hip_conv3d_cl_dgrad(dz2, w2),
            "conv2_wgrad": lambda: E.hip_conv3d_cl_wgrad(dz2, a1), "conv1_forward": lambda: E._HipConv3dS7TrainFn.apply(vol, w1, b1),
            "conv1_wgrad_explicit": lambda: E.hip_conv3d_s7_wgrad(vol, dz1)}
    for fn in kern.values():
        fn()
    passes = {k: _summary(v) for k, v in _windows(torch, kern, rounds, steps).items()}
    for k, f in FLOP.items():
        passes[k]["counted_tflops"] = f * vox / (passes[k]["median_ms"] * 1e-3) / 1e12

    def backward_only():
        for p in hip.parameters():
            p.grad = None
        loss = (hip.tokens(x) * r).sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss.backward()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    bwd = statistics.median(backward_only() for _ in range(max(rounds, 3)))
    passes["encoder_backward_ms"] = bwd
    passes["conv1_wgrad_share_of_backward"] = passes["conv1_wgrad_explicit"]["median_ms"] / bwd
    res["passes"] = passes
    return res


def child_trace(shape):
    import torch
    dev = torch.device("cuda:0")
    hip, _ = _encoders(torch, dev)
    x, r = _inputs(torch, shape, dev)
    for _ in range(3):
        _pass(hip, x, r)
    torch.cuda.synchronize()
    return {"passes": 3}


def child_step(rounds, steps):
    import torch
    from smokephysai_amd.models import SmokePhysNet3D
    from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
    from train import batch_losses
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    B = 8
    batch = {"input": torch.rand(B, 1, 16, 128, 128, device=dev, generator=g), "target": torch.rand(B, 1, 128, 128, device=dev, generator=g),
             "chaos_features": torch.rand(B, 3, device=dev, generator=g), "sequence": torch.rand(B, 20, 128, 128, device=dev, generator=g)}
    reg = PhysicsRegularizer()
    fns = {}
    for route in ("hip", "torch"):
        torch.manual_seed(0)
        model = SmokePhysNet3D(volume_encoder=route).to(dev).train()
        opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01)

        def step(model=model, opt=opt):
            opt.zero_grad()
            total, *_ = batch_losses(model, reg, batch, dev)
            total.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
            opt.step()
        fns[route] = step
    for fn in fns.values():
        fn(); fn()
    return {k: _summary(v) for k, v in _windows(torch, fns, rounds, steps).items()}


def _run_child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise RuntimeError(f"child {args} failed ({p.returncode}): {p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _kernel_stats(shape, limit):
    """One rocprofv3 --kernel-trace --stats run of its own; {kernel name: {calls, total_ms, share}} for the kernels above 0.5 % of the time."""
    with tempfile.TemporaryDirectory() as d:
        _run_child(["trace", "x".join(map(str, shape))], limit, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t3d", "--"))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"not measured": "rocprofv3 wrote no kernel_stats.csv"}
        rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    out = {}
    for r in rows:
        ns = float(r["TotalDurationNs"])
        if ns / total >= 0.005:
            out[r["Name"][:120]] = {"calls": int(r["Calls"]), "total_ms": ns / 1e6, "share": ns / total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="*")
    ap.add_argument("--cases", default="8x16x128x128,2x64x128x128")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "train3d_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        kind, rest = a.child[0], a.child[1:]
        shape = tuple(int(v) for v in rest[0].split("x")) if rest and "x" in rest[0] else None
        if kind == "first":
            res = child_first(shape, rest[1])
        elif kind == "steady":
            res = child_steady(shape, int(rest[1]), int(rest[2]))
        elif kind == "trace":
            res = child_trace(shape)
        else:
            res = child_step(int(rest[0]), int(rest[1]))
        print("RESULT " + json.dumps(res))
        return
    report = {"rounds": a.rounds, "steps_per_window": a.steps, "cases": {}}          # (this process never opens the device: the children do)
    for i, case in enumerate(a.cases.split(",")):
        shape = tuple(int(v) for v in case.split("x"))
        entry = {"first": {r: _run_child(["first", case, r], a.limit) for r in ("torch", "hip")},
                 "steady": _run_child(["steady", case, a.rounds, a.steps], a.limit)}
        if i == 0 and not a.no_trace:
            entry["kernels"] = _kernel_stats(shape, a.limit)
        report["cases"][case] = entry
        print(case, json.dumps({k: entry["steady"][k] if k == "hip_wins" else entry["steady"][k]["median_ms"] for k in ("hip", "torch", "hip_wins")}))
    if not a.no_step:
        report["train_step_batch8_16x128x128"] = _run_child(["step", a.rounds, a.steps], a.limit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
