"""Training-route timings of the reconstruction head: the head's forward + backward at batch 8 and 64 with
head_train = "torch" (PyTorch modules on MIOpen) and "hip" (models/decoder_train.py), and one full training step of the default model
at 64 x 256^2 with mi355x.recon_head off and on.  Device-event timing after warm-up, the median of 5 windows; one JSON line per
measurement, all of them also written to the path given as argv[1] (default head_train_probe.json)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import train
from smokephysai_amd.models import SmokePhysNet
from smokephysai_amd.models.decoder_train import hip_head_train, hip_head_train_supported
from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer

dev = torch.device("cuda:0")
results = []


def timed(fn, warmup=3, reps=10, windows=5):
    """ms per call: device events around `reps` calls after `warmup`, the median of `windows` such windows."""
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


def emit(rec):
    results.append(rec)
    print(json.dumps(rec), flush=True)


# ---- 1. the head alone: forward + backward from tokens [B, 1024, 64] ------------------------------------------------------------
for B in (8, 64):
    torch.manual_seed(0)
    head = SmokePhysNet().reconstruction_head.to(dev).train()
    tok = torch.randn(B, 1024, 64, device=dev, requires_grad=True)
    r = torch.randn(B, 1, 128, 128, device=dev)
    assert hip_head_train_supported(head, tok)

    def step(hip):
        head.zero_grad(set_to_none=True)
        tok.grad = None
        y = hip_head_train(head, tok) if hip else head(tok.transpose(1, 2).reshape(B, 64, 32, 32))
        (y * r).sum().backward()

    for route in ("torch", "hip"):
        med, win = timed(lambda: step(route == "hip"))
        emit({"what": "head_fwd_bwd", "B": B, "route": route, "ms": round(med, 4), "windows": win})

# ---- 2. one full training step of the default model at 64 x 256^2 -----------------------------------------------------------
B, N = 64, 256
gen = torch.Generator().manual_seed(1)
batch = {"input": torch.rand(B, 1, N, N, generator=gen), "target": torch.rand(B, 1, N, N, generator=gen),
         "chaos_features": torch.rand(B, 3, generator=gen), "sequence": torch.rand(B, 20, N, N, generator=gen)}
batch = {k: v.to(dev) for k, v in batch.items()}
for route in ("torch", "hip", "torch", "hip"):            # interleaved: each route measured twice
    torch.manual_seed(1234)
    model = SmokePhysNet(head_train=route).to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
    reg = PhysicsRegularizer()

    def train_step():
        opt.zero_grad()
        total, *_ = train.batch_losses(model, reg, batch, dev)
        total.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        opt.step()

    med, win = timed(train_step, warmup=3, reps=3, windows=5)
    emit({"what": "train_step", "B": B, "N": N, "recon_head": route, "ms": round(med, 3), "windows": win})
    del model, opt
    torch.cuda.empty_cache()

out = sys.argv[1] if len(sys.argv) > 1 else "head_train_probe.json"
with open(out, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
