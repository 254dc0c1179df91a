"""A/B of the train.py step at frame sizes beyond 128^2 / 256^2: the encoder on libsmokehip (this commit's route) against the same step with the
encoder on the generic PyTorch-ROCm branch (SMK_TRAIN_ENCODER_HIP=0: what the step ran at these sizes before), full default SmokePhysNet,
recon_head hip and torch.

    python tools/train_sizes_probe.py [--cases 64x64,512x16,1024x4] [--rounds 5] [--steps 3] [--out profiles/r13/train_sizes_probe.json]

Every measurement runs in a child process with a time limit; the first child that fails ends the probe.  Per case:
  first   one child per route (head hip): wall time of the first optimisation step of a fresh process (library load, MIOpen's find pass where
          there is one) and of the second;
  steady  one child per head: after two warm-up steps per route, `rounds` alternated measurements of `steps` steps each per route (DESIGN
          section 9's A/B scheme): median and range of the ms per step;
  passes  the BatchNorm + ReLU + pool forward and backward of the second block (128 channels) alone, against the device copy rate measured
          the way bench.py measures it: the forward moves two reads of z, the backward two reads and one write.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _batch(torch, B, N, dev):
    g = torch.Generator(device=dev).manual_seed(5)
    seq = torch.rand(B, 20, N, N, device=dev, generator=g)
    return {"input": seq[:, 9:10].contiguous(), "target": seq[:, 10:11].contiguous(), "chaos_features": torch.rand(B, 3, device=dev, generator=g),
            "sequence": seq}


def _stepper(torch, head, B, N, dev):
    from smokephysai_amd.models import SmokePhysNet
    from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
    from train import batch_losses
    torch.manual_seed(0)
    model = SmokePhysNet(head_train=head).to(dev).train()
    reg = PhysicsRegularizer()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    batch = _batch(torch, B, N, dev)

    def step():
        opt.zero_grad()
        total, *_ = batch_losses(model, reg, batch, dev)
        total.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        opt.step()
        return total
    return model, batch, step


def child_first(N, B, route, head):
    os.environ["SMK_TRAIN_ENCODER_HIP"] = "1" if route == "hip" else "0"
    t_start = time.perf_counter()
    import torch
    dev = torch.device("cuda:0")
    model, batch, step = _stepper(torch, head, B, N, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    name = type(model.encode_frames(batch["input"]).grad_fn).__name__
    return {"first_step_s": t1 - t0, "second_step_s": t2 - t1, "import_and_setup_s": t0 - t_start, "encoder_grad_fn": name}


def child_steady(N, B, head, rounds, steps):
    import torch
    from smokephysai_amd.models import smokephys_net
    dev = torch.device("cuda:0")
    model, batch, step = _stepper(torch, head, B, N, dev)
    ms = {"generic": [], "hip": []}
    for route in ("generic", "hip"):                             # warm-up: the find pass of the generic branch, the lazily built mirrors
        smokephys_net._HIP_ENCODER_TRAIN = route == "hip"
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for route in ("generic", "hip"):
            smokephys_net._HIP_ENCODER_TRAIN = route == "hip"
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms[route].append((time.perf_counter() - t0) / steps * 1e3)
    out = {r: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": v} for r, v in ms.items()}
    out["peak_memory_GiB"] = torch.cuda.max_memory_allocated() / 2 ** 30
    return out


def child_passes(N, B):
    import torch
    from smokephysai_amd import _lib
    dev = torch.device("cuda:0")
    L = _lib.load()
    a = torch.empty(2 ** 28, device=dev)
    b = torch.empty_like(a)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3
    copy_gbs = 2 * a.numel() * 4 / timed(lambda: b.copy_(a), 10) / 1e9
    del a, b
    C, P = 128, N // 32
    z = torch.randn(B, C, N, N, device=dev)
    dz = torch.empty_like(z)
    out = torch.empty(B, C, 32, 32, device=dev)
    dout = torch.randn(B, C, 32, 32, device=dev)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
    stats, dwb = torch.empty(3, C, device=dev), torch.empty(2, C, device=dev)
    ws = torch.empty(int(L.smk_bn_train_workspace(B, C, N, N, P)), device=dev, dtype=torch.uint8)
    st = _lib.stream_ptr(dev)
    fwd = lambda: _lib.check(L.smk_bn_relu_pool_forward(z.data_ptr(), B, C, N, N, gamma.data_ptr(), beta.data_ptr(), 1e-5, P, out.data_ptr(),
                                                        stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), ws.data_ptr(), st))
    bwd = lambda: _lib.check(L.smk_bn_relu_pool_backward(z.data_ptr(), dout.data_ptr(), B, C, N, N, gamma.data_ptr(), beta.data_ptr(),
                                                         stats[0].data_ptr(), stats[2].data_ptr(), P, dz.data_ptr(), dwb[0].data_ptr(),
                                                         dwb[1].data_ptr(), ws.data_ptr(), st))
    tf, tb = timed(fwd, 20), timed(bwd, 20)
    nbytes = z.numel() * 4
    return {"pool": P, "z_MiB": nbytes / 2 ** 20, "copy_GBs": copy_gbs, "forward_ms": tf * 1e3, "backward_ms": tb * 1e3,
            "forward_GBs": 2 * nbytes / tf / 1e9, "backward_GBs": 3 * nbytes / tb / 1e9,
            "forward_fraction_of_copy": 2 * nbytes / tf / 1e9 / copy_gbs, "backward_fraction_of_copy": 3 * nbytes / tb / 1e9 / copy_gbs}


def _run_child(args, limit):
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], capture_output=True, text=True, timeout=limit,
                       cwd=ROOT)
    if p.returncode != 0:
        raise SystemExit(f"child {args} failed with status {p.returncode}; nothing more is started\n{p.stderr[-3000:]}")
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"  {' '.join(map(str, args))}: {time.perf_counter() - t0:.0f} s  {json.dumps(res)[:400]}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--cases", default="64x64,512x16,1024x4", help="frame size x batch, comma separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--heads", default="hip,torch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        kind, N, B = a.child[0], int(a.child[1]), int(a.child[2])
        res = (child_first(N, B, a.child[3], a.child[4]) if kind == "first" else
               child_steady(N, B, a.child[3], int(a.child[4]), int(a.child[5])) if kind == "steady" else child_passes(N, B))
        print(json.dumps(res))
        return
    result = {"what": "train.py step, default SmokePhysNet: encoder on libsmokehip ('hip') against the generic PyTorch-ROCm branch ('generic')",
              "rounds": a.rounds, "steps_per_measurement": a.steps, "cases": {}}
    for case in a.cases.split(","):
        N, B = (int(v) for v in case.split("x"))
        print(f"{N}^2 x {B}", flush=True)
        r = {"first": {}, "steady": {}}
        for route in ("hip", "generic"):
            r["first"][route] = _run_child(["first", N, B, route, "hip"], 420)
        for head in a.heads.split(","):
            r["steady"][f"head_{head}"] = _run_child(["steady", N, B, head, a.rounds, a.steps], 420)
        r["passes"] = _run_child(["passes", N, B], 120)
        result["cases"][f"{N}x{N}x{B}"] = r
        if a.out:                                               # after every case: a later failure keeps what was measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
