"""The train step tail on libsmokehip against the PyTorch ops it replaces: the default model with
mi355x.recon_head = hip at 64 frames of 256 x 256, one process.

  1. the whole step of train.py's loop body with {losses, optimizer} = {torch, torch}, {hip, torch}, {torch, hip}, {hip, hip}: the four
     configurations take turns window by window (5 windows of 20 steps each, device events, after warm-up; the median is reported);
  2. clip + AdamW alone on the model's parameters with synthetic gradients, both routes, and the host time of one step() call;
  3. the loss forward + backward alone (prediction [64, 1, 128, 128], sequence [64, 20, 256, 256]), both routes.
Beside each isolated time: the bytes the algorithm has to move over the 6.29 TB/s float4-copy rate of the MI355X.
One JSON line per measurement, all of them also written to argv[1] (default train_tail_probe.json)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import train
from smokephysai_amd.models import SmokePhysNet
from smokephysai_amd.models.losses import hip_train_losses, hip_train_losses_supported
from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
from smokephysai_amd.optim import HipAdamW
from smokephysai_amd.utils.distributed import clip_grad_norm_

COPY_RATE = 6.29e12              # bytes / s, float4 copy
WINDOWS, STEPS = 5, 20
dev = torch.device("cuda:0")
results = []


def emit(rec):
    results.append(rec)
    print(json.dumps(rec), flush=True)


def window(fn, steps=STEPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def alternating(fns, warmup=3):
    """{name: (median ms, windows)}: the functions take turns, one window each, WINDOWS times."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            ms[k].append(window(fn))
    return {k: (float(np.median(v)), [round(float(x), 4) for x in v]) for k, v in ms.items()}


# ---- 1. the whole step ------------------------------------------------------------------------------------------------------------
B, N = 64, 256
gen = torch.Generator().manual_seed(1)
batch = {k: v.to(dev) for k, v in {"input": torch.rand(B, 1, N, N, generator=gen), "target": torch.rand(B, 1, N, N, generator=gen),
                                   "chaos_features": torch.rand(B, 3, generator=gen),
                                   "sequence": torch.rand(B, 20, N, N, generator=gen)}.items()}
reg = PhysicsRegularizer()


def make_step(losses, optimizer):
    torch.manual_seed(1234)
    model = SmokePhysNet(head_train="hip").to(dev).train()
    opt = (HipAdamW if optimizer == "hip" else torch.optim.AdamW)(model.parameters(), lr=1e-4, weight_decay=0.01)

    def step():                                   # train_epoch's loop body, the logging synchronisation included
        opt.zero_grad()
        (total, recon, phys, chaos), vec = train._batch_loss_terms(model, reg, batch, dev, losses=losses)
        total.backward()
        if optimizer == "hip":
            opt.step(clip_max_norm=1.0)
        else:
            clip_grad_norm_(model.parameters(), max_norm=1.0)
            opt.step()
        return [total.item(), recon.item(), phys.item(), chaos.item()] if vec is None else vec.tolist()[:4]
    return step, model, opt


combos = [("torch", "torch"), ("hip", "torch"), ("torch", "hip"), ("hip", "hip")]
built = {f"losses={l},optimizer={o}": make_step(l, o) for l, o in combos}
for name, (med, win) in alternating({k: v[0] for k, v in built.items()}).items():
    emit({"what": "train_step", "B": B, "N": N, "recon_head": "hip", "config": name, "ms": round(med, 3), "windows": win})

# ---- 2. clip + AdamW alone ----------------------------------------------------------------------------------------------------------
model = built["losses=torch,optimizer=torch"][1]
n_params = sum(p.numel() for p in model.parameters())
n_tensors = sum(1 for _ in model.parameters())
del built
torch.cuda.empty_cache()


def make_opt(route):
    params = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    g = torch.Generator(device=dev).manual_seed(2)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
    opt = (HipAdamW if route == "hip" else torch.optim.AdamW)(params, lr=1e-4, weight_decay=0.01)

    def step():
        if route == "hip":
            opt.step(clip_max_norm=1.0)
        else:
            clip_grad_norm_(params, max_norm=1.0)
            opt.step()
    return step


opt_steps = {route: make_opt(route) for route in ("torch", "hip")}
need = 4 * n_params * (1 + 4 + 3)                 # the norm reads g; the update reads p, g, m, v and writes p, m, v
for route, (med, win) in alternating(opt_steps).items():
    emit({"what": "clip_adamw", "route": route, "tensors": n_tensors, "elements": n_params, "ms": round(med, 4), "windows": win,
          "bytes_needed": need, "ms_at_copy_rate": round(need / COPY_RATE * 1e3, 4)})
for route, fn in opt_steps.items():               # host time of the call itself: the device is idle before, nothing waits on it inside
    host = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        host.append((time.perf_counter() - t0) / STEPS * 1e3)
        torch.cuda.synchronize()
    emit({"what": "clip_adamw_host", "route": route, "ms": round(float(np.median(host)), 4), "windows": [round(h, 4) for h in host],
          "note": "wall time of the Python call without a synchronisation; a call that outruns the device queues behind it"})
del opt_steps
torch.cuda.empty_cache()

# ---- 3. the loss alone ---------------------------------------------------------------------------------------------------------------
pred = torch.rand(B, 1, 128, 128, device=dev, requires_grad=True)
target = F.adaptive_avg_pool2d(batch["target"], (128, 128))
chaos_pred = torch.rand(B, 3, device=dev, requires_grad=True)
assert hip_train_losses_supported(pred, target, chaos_pred, batch["chaos_features"], batch["sequence"])


def loss_step(route):
    pred.grad = chaos_pred.grad = None
    if route == "hip":
        total = hip_train_losses(pred, target, chaos_pred, batch["chaos_features"], batch["sequence"], reg)[0]
    else:
        recon = F.mse_loss(pred, target)
        chaos = F.mse_loss(chaos_pred, batch["chaos_features"])
        phys = reg({"density": pred, "density_sequence": batch["sequence"]}, {"density": target})["total_physics_loss"]
        total = recon + 0.1 * chaos + 0.05 * phys
    total.backward()


need = 4 * (batch["sequence"].numel() + 2 * pred.numel() + 3 * pred.numel())      # forward: sequence, pred, target; backward: pred, target, d_pred
for route, (med, win) in alternating({r: (lambda r=r: loss_step(r)) for r in ("torch", "hip")}).items():
    emit({"what": "loss_fwd_bwd", "route": route, "B": B, "sequence": list(batch["sequence"].shape), "ms": round(med, 4), "windows": win,
          "bytes_needed": need, "ms_at_copy_rate": round(need / COPY_RATE * 1e3, 4)})

out = sys.argv[1] if len(sys.argv) > 1 else "train_tail_probe.json"
with open(out, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "windows": WINDOWS, "steps_per_window": STEPS, "results": results}, f, indent=1)
