#!/usr/bin/env python3
"""SmokePhysAI training on MI355X -- CLI and function surface of the reference's train.py (41-280):
load_config / setup_experiment / train_epoch / validate_epoch / main, same loss decomposition
(recon MSE + 0.1 chaos MSE + 0.05 physics), clip 1.0, AdamW + CosineAnnealingLR, best-val checkpoint schema.

New: data-parallel training, one process per GPU (`python -m torch.distributed.run --nproc-per-node N train.py`):
each rank simulates and holds its own block of the samples (no data exchange), gradients are averaged with a bucketed
RCCL all-reduce overlapped with backward (DistributedDataParallel); rank 0 writes the checkpoint.
TensorBoard logging is optional (the module is not required).
"""
import argparse
import os
import warnings
from datetime import datetime
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim
import yaml
from torch.utils.data import DataLoader
from tqdm import tqdm

from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
from smokephysai_amd.utils.data_loader import create_data_loaders
from smokephysai_amd.utils.distributed import (all_reduce_weighted_mean, clip_grad_norm_, ddp_bucket_report, init_distributed,
                                               max_over_ranks, wrap_ddp)


class _NullWriter:
    def add_scalar(self, *a, **k): pass
    def close(self): pass


def load_config(config_path: str) -> dict:
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def setup_experiment(config: dict, rank: int = 0, local_rank: int = 0):
    """train.py:25-39 of the reference: experiment dir + writer + device."""
    timestamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    exp_dir = f"experiments/smokephys_{timestamp}"
    writer = _NullWriter()
    if rank == 0:
        os.makedirs(exp_dir, exist_ok=True)
        with open(os.path.join(exp_dir, "config.yaml"), "w") as f:
            yaml.dump(config, f)
        try:
            from torch.utils.tensorboard import SummaryWriter
            writer = SummaryWriter(os.path.join(exp_dir, "logs"))
        except Exception:
            pass
    device = torch.device("cuda", local_rank)
    if not torch.cuda.is_available():
        raise RuntimeError("train.py needs a ROCm GPU: smokephysai_amd has no CPU fallback for the simulator")
    torch.cuda.set_device(device)
    print(f"Using device: {device}")
    return exp_dir, writer, device


LOSS_ROUTES = ("torch", "hip")
OPTIMIZER_ROUTES = ("torch", "hip")
VOLUME_ENCODER_ROUTES = ("hip", "torch")
VOLUME_ENCODER_DEFAULT = "hip"
_warned_losses = False


def _route(value, choices, key: str) -> str:
    value = str(value)
    if value not in choices:
        raise ValueError(f"{key} must be one of {', '.join(repr(c) for c in choices)}, not {value!r}")
    return value


def loss_route(config: dict) -> str:
    """The config's `mi355x.losses` ('torch', the default, or 'hip': models/losses.py)."""
    return _route((config.get("mi355x", {}) or {}).get("losses", "torch"), LOSS_ROUTES, "mi355x.losses")


def ssim_settings(config: dict):
    """(weight, window) of the opt-in SSIM term from `mi355x.ssim_weight` (0.0, the default: no term) and `mi355x.ssim_window` (11)."""
    hw = config.get("mi355x", {}) or {}
    weight, window = float(hw.get("ssim_weight", 0.0)), hw.get("ssim_window", 11)
    if not weight >= 0.0:
        raise ValueError(f"mi355x.ssim_weight must be >= 0, not {weight!r}")
    if isinstance(window, bool) or not isinstance(window, int) or window < 1 or window % 2 == 0:
        raise ValueError(f"mi355x.ssim_window must be an odd positive integer, not {window!r}")
    return weight, window


def build_optimizer(config: dict, params) -> optim.Optimizer:
    """AdamW from the config's `training` section; `mi355x.optimizer: hip` makes it smokephysai_amd.optim.HipAdamW (same state,
    same state_dict: a checkpoint resumes across the switch)."""
    route = _route((config.get("mi355x", {}) or {}).get("optimizer", "torch"), OPTIMIZER_ROUTES, "mi355x.optimizer")
    kwargs = dict(lr=config["training"]["learning_rate"], weight_decay=config["training"]["weight_decay"])
    if route == "hip":
        from smokephysai_amd.optim import HipAdamW
        return HipAdamW(params, **kwargs)
    return optim.AdamW(params, **kwargs)


def _batch_loss_terms(model, physics_regularizer, batch, device, chaos_noise=None, losses="torch", ssim_weight=0.0, ssim_window=11):
    """batch_losses' four values and, on the hip route, the device vector they are views of (else None).  ssim_weight > 0 adds
    ssim_weight * ssim_loss(reconstructed, targets, ssim_window) to the total (models/losses.py); the other three keep their values."""
    global _warned_losses
    _route(losses, LOSS_ROUTES, "losses")
    inputs = batch["input"].to(device)
    targets = batch["target"].to(device)
    chaos_targets = batch["chaos_features"].to(device)
    outputs = model(inputs) if chaos_noise is None else model(inputs, chaos_noise=chaos_noise)
    if targets.shape[-2:] != outputs["reconstructed"].shape[-2:]:
        # The reconstruction head always emits 128x128 (smokephys_net.py:57-66,117-118), so the reference's own
        # F.mse_loss raises for any other grid size.  For BASELINE config 4 (256^2 grids) the target is block-averaged
        # to the head's resolution (2x2 mean at 256^2); at 128^2 this branch is never taken.
        targets = F.adaptive_avg_pool2d(targets, outputs["reconstructed"].shape[-2:])
    if losses == "hip":
        from smokephysai_amd.models.losses import hip_train_losses, hip_train_losses_supported
        sequence = batch["sequence"].to(device)
        if hip_train_losses_supported(outputs["reconstructed"], targets, outputs["physics_features"], chaos_targets, sequence):
            vec = hip_train_losses(outputs["reconstructed"], targets, outputs["physics_features"], chaos_targets, sequence,
                                   physics_regularizer, w_chaos=0.1, w_physics=0.05)
            if ssim_weight > 0:                                    # one add: the SSIM term into slot 0 of the vector
                from smokephysai_amd.models.losses import ssim_loss
                vec = vec + F.pad((ssim_weight * ssim_loss(outputs["reconstructed"], targets, ssim_window)).reshape(1), (0, vec.numel() - 1))
            return (vec[0], vec[1], vec[2], vec[3]), vec
        if outputs["reconstructed"].device.type == "cuda" and not _warned_losses:      # CPU tensors take the torch formulas silently
            _warned_losses = True
            warnings.warn("losses='hip': tensors outside the HIP loss kernels' domain (float32, contiguous, one ROCm device, equal shapes, "
                          "no gradient into targets or sequence): the torch formulas run")
    recon_loss = F.mse_loss(outputs["reconstructed"], targets)
    chaos_loss = F.mse_loss(outputs["physics_features"], chaos_targets)
    physics_losses = physics_regularizer({"density": outputs["reconstructed"],
                                          "density_sequence": batch["sequence"].to(device)}, {"density": targets})
    physics_loss = physics_losses["total_physics_loss"]
    total = recon_loss + 0.1 * chaos_loss + 0.05 * physics_loss
    if ssim_weight > 0:
        from smokephysai_amd.models.losses import ssim_loss
        total = total + ssim_weight * ssim_loss(outputs["reconstructed"], targets, ssim_window)
    return (total, recon_loss, physics_loss, chaos_loss), None


def batch_losses(model, physics_regularizer, batch, device, chaos_noise=None, losses="torch", ssim_weight=0.0, ssim_window=11):
    """Forward + the reference's loss decomposition (train.py:59-85). Returns (total, recon, physics, chaos); with losses="hip" the four
    are views of the one device vector smokephysai_amd.models.losses.hip_train_losses computes."""
    return _batch_loss_terms(model, physics_regularizer, batch, device, chaos_noise, losses, ssim_weight, ssim_window)[0]


def _rank_invariant_batches(loader: DataLoader, device):
    """Every rank must run the same number of optimisation steps: DDP's gradient all-reduce is a collective, and the ranks'
    sample blocks differ by up to one sample (shard_range), i.e. possibly by one batch.  The step count is the maximum over
    ranks; a rank that runs out of batches starts its (shuffled) loader again, so no sample is dropped and no rank waits
    in a collective the others never enter."""
    steps = max_over_ranks(len(loader), device)
    it = iter(loader)
    for _ in range(steps):
        try:
            batch = next(it)
        except StopIteration:
            it = iter(loader)
            batch = next(it)
        yield batch


def train_epoch(model: nn.Module, train_loader: DataLoader, optimizer: optim.Optimizer,
                physics_regularizer: PhysicsRegularizer, device, epoch: int, writer, losses: str = "torch",
                ssim_weight: float = 0.0, ssim_window: int = 11) -> Dict[str, float]:
    """One epoch.  A HipAdamW clips inside its step (`step(clip_max_norm=1.0)`: smk_grad_norm + smk_adamw_step); any other optimizer gets
    clip_grad_norm_ and step() as before.  losses="hip": the four logged values come from one .tolist() of the loss vector."""
    from smokephysai_amd.optim import HipAdamW
    fused_clip = isinstance(optimizer, HipAdamW)
    model.train()
    sums, seen = [0.0, 0.0, 0.0, 0.0], 0
    steps = max_over_ranks(len(train_loader), device)
    pbar = tqdm(_rank_invariant_batches(train_loader, device), total=steps, desc=f"Training Epoch {epoch+1}", leave=True)
    for batch_idx, batch in enumerate(pbar):
        optimizer.zero_grad()
        (total, recon, phys, chaos), vec = _batch_loss_terms(model, physics_regularizer, batch, device, losses=losses,
                                                             ssim_weight=ssim_weight, ssim_window=ssim_window)
        total.backward()                      # DDP: bucketed RCCL all-reduce (mean over ranks) overlaps this backward
        if fused_clip:
            optimizer.step(clip_max_norm=1.0)
        else:
            clip_grad_norm_(model.parameters(), max_norm=1.0)     # (= torch's; layout-independent under DDP's bucket views)
            optimizer.step()
        vals = [total.item(), recon.item(), phys.item(), chaos.item()] if vec is None else vec.tolist()[:4]
        n = int(batch["input"].shape[0])
        sums = [s + v * n for s, v in zip(sums, vals)]
        seen += n
        if batch_idx % 50 == 0:
            step = epoch * steps + batch_idx
            for name, v in zip(("Total", "Recon", "Physics", "Chaos"), vals):
                writer.add_scalar(f"Train/Batch_{name}_Loss", v, step)
        pbar.set_postfix({"loss": f"{vals[0]:.4f}", "recon": f"{vals[1]:.4f}", "phys": f"{vals[2]:.4f}"})
    avg = all_reduce_weighted_mean(sums, seen, device)        # sample-weighted over all ranks (blocks differ in size)
    return dict(zip(("total_loss", "recon_loss", "physics_loss", "chaos_loss"), avg))


def validate_epoch(model: nn.Module, val_loader: DataLoader, physics_regularizer: PhysicsRegularizer,
                   device, losses: str = "torch", ssim_weight: float = 0.0, ssim_window: int = 11) -> Dict[str, float]:
    """No collective inside the loop (the unwrapped model, eval-mode BatchNorm), so ranks may run different batch counts."""
    model.eval()
    sums, seen = [0.0, 0.0, 0.0, 0.0], 0
    with torch.no_grad():
        pbar = tqdm(val_loader, desc="Validation", leave=True)
        for batch in pbar:
            terms, vec = _batch_loss_terms(model, physics_regularizer, batch, device, losses=losses, ssim_weight=ssim_weight,
                                           ssim_window=ssim_window)
            vals = [v.item() if torch.is_tensor(v) else float(v) for v in terms] if vec is None else vec.tolist()[:4]
            n = int(batch["input"].shape[0])
            sums = [s + v * n for s, v in zip(sums, vals)]
            seen += n
            pbar.set_postfix({"loss": f"{vals[0]:.4f}", "recon": f"{vals[1]:.4f}"})
    avg = all_reduce_weighted_mean(sums, seen, device)
    return dict(zip(("total_loss", "recon_loss", "physics_loss", "chaos_loss"), avg))


def build_model(config: dict):
    """SmokePhysNet from the config's `model` section and the optional `mi355x` keys (encoder_dtype, recon_head, input_grad), on the CPU.
    `mi355x.volume_depth: D > 0` makes it a SmokePhysNet3D (volumes through a trainable Encoder3D; `mi355x.volume_encoder`: hip | torch)."""
    from smokephysai_amd.models.smokephys_net import SmokePhysNet, SmokePhysNet3D
    hw = config.get("mi355x", {}) or {}
    cls, extra = SmokePhysNet, {}
    if int(hw.get("volume_depth", 0) or 0) > 0:
        if hw.get("sync_bn", False):
            raise ValueError("mi355x.volume_depth with mi355x.sync_bn: the 3-D encoder's BatchNorm statistics are per process; set sync_bn: false")
        cls, extra = SmokePhysNet3D, dict(volume_encoder=_route(hw.get("volume_encoder", VOLUME_ENCODER_DEFAULT), VOLUME_ENCODER_ROUTES,
                                                                "mi355x.volume_encoder"))
    return cls(**extra, input_dim=config["model"]["input_dim"], hidden_dim=config["model"]["hidden_dim"],
               num_layers=config["model"]["num_layers"], num_heads=config["model"]["num_heads"],
               chaos_strength=config["model"]["chaos_strength"],
               encoder_dtype=hw.get("encoder_dtype", "bf16x3"), head_train=str(hw.get("recon_head", "torch")),
               input_grad=None if hw.get("input_grad") is None else str(hw["input_grad"]))


def data_loader_kwargs(config: dict, rank: int = 0, world: int = 1) -> dict:
    """create_data_loaders' keyword arguments (all but `device`) from the config's `training` / `data` sections and the optional
    `mi355x` keys (sim_batch, jacobi_iters, dataset_labels, render_depth or volume_depth + render); a missing key or a missing section means the reference-equivalent default."""
    hw = config.get("mi355x", {}) or {}
    kw = dict(batch_size=config["training"]["batch_size"], num_train=config["data"]["num_train"], num_val=config["data"]["num_val"],
              grid_size=tuple(config["data"]["grid_size"]), cache_dir=config["data"]["cache_dir"], sim_batch=hw.get("sim_batch", 64),
              jacobi_iters=hw.get("jacobi_iters", 20), labels=str(hw.get("dataset_labels", "host")), rank=rank, world=world)
    if hw.get("render_depth", 0):           # camera frames of 3-D smoke (RenderedSmokeDataset); nothing is added without the key
        kw.update(render_depth=int(hw["render_depth"]), render=dict(hw.get("render") or {}))
    if hw.get("volume_depth", 0):           # volumes in, rendered next frame out (VolumeFrameDataset, for SmokePhysNet3D)
        if hw.get("render_depth", 0):
            raise ValueError("mi355x.render_depth and mi355x.volume_depth exclude each other")
        kw.update(volume_depth=int(hw["volume_depth"]), render=dict(hw.get("render") or {}))
    return kw


def main():
    parser = argparse.ArgumentParser(description="SmokePhysAI Training")
    parser.add_argument("--config", type=str, default="config/config.yaml", help="Path to config file")
    parser.add_argument("--resume", type=str, default=None, help="Path to checkpoint to resume from")
    args = parser.parse_args()
    config = load_config(args.config)
    ssim_weight, ssim_window = ssim_settings(config)               # a bad value stops here, before any data is generated
    hw = config.get("mi355x", {}) or {}
    if hw.get("deterministic", False):
        # run-to-run reproducible steps: MIOpen's default backward-weights solvers for the reconstruction head's three convolutions
        # accumulate with atomics (the only non-reproducible op of the step: tools/rccl_diag.py); this restricts MIOpen to its
        # deterministic solvers.  Every libsmokehip kernel is deterministic either way: with mi355x.recon_head = hip the head runs on
        # libsmokehip (models/decoder_train.py) and the step is reproducible without this flag.
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False
        # ... and keeps what MIOpen finds under that restriction out of the account's ordinary find-db (utils/miopen_db.py: a later
        # non-deterministic run would reuse the slow entries: 60 -> 485 ms per step measured)
        from smokephysai_amd.utils.miopen_db import use_private_find_db
        use_private_find_db("deterministic")
    rank, world, local_rank = init_distributed()
    exp_dir, writer, device = setup_experiment(config, rank, local_rank)

    train_loader, val_loader = create_data_loaders(device=device, **data_loader_kwargs(config, rank, world))

    model = build_model(config).to(device)
    physics_regularizer = PhysicsRegularizer(conservation_weight=config["physics"]["conservation_weight"],
                                             continuity_weight=config["physics"]["continuity_weight"],
                                             energy_weight=config["physics"]["energy_weight"])
    start_epoch = 0
    ckpt = None
    if args.resume:                       # the reference parses --resume but never reads it (train.py:186-187)
        ckpt = torch.load(args.resume, map_location=device)
        model.load_state_dict(ckpt["model_state_dict"])
        start_epoch = int(ckpt.get("epoch", -1)) + 1
    ddp_model = wrap_ddp(model, device, sync_bn=bool(hw.get("sync_bn", False)), grad_exchange=str(hw.get("grad_exchange", "rccl")))
    if ddp_model is not model:                         # SyncBatchNorm conversion replaces modules: validate on the wrapped network
        model = ddp_model.module
        if rank == 0:
            print(f"DDP gradient exchange: {ddp_bucket_report(ddp_model)}")
    optimizer = build_optimizer(config, ddp_model.parameters())
    losses = loss_route(config)
    scheduler = optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=config["training"]["num_epochs"])
    if ckpt is not None:
        optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        scheduler.load_state_dict(ckpt["scheduler_state_dict"])

    best_val_loss = float("inf")
    for epoch in range(start_epoch, config["training"]["num_epochs"]):
        print(f"\nEpoch {epoch + 1}/{config['training']['num_epochs']}")
        train_metrics = train_epoch(ddp_model, train_loader, optimizer, physics_regularizer, device, epoch, writer, losses=losses,
                                    ssim_weight=ssim_weight, ssim_window=ssim_window)
        val_metrics = validate_epoch(model, val_loader, physics_regularizer, device, losses=losses, ssim_weight=ssim_weight,
                                     ssim_window=ssim_window)
        scheduler.step()
        writer.add_scalar("Train/Epoch_Loss", train_metrics["total_loss"], epoch)
        writer.add_scalar("Val/Epoch_Loss", val_metrics["total_loss"], epoch)
        writer.add_scalar("Learning_Rate", optimizer.param_groups[0]["lr"], epoch)
        if rank == 0:
            print("\nEpoch Summary:")
            print(f"Train Loss: {train_metrics['total_loss']:.4f}")
            print(f"Val Loss: {val_metrics['total_loss']:.4f}")
            print(f"Learning Rate: {optimizer.param_groups[0]['lr']:.6f}")
        if val_metrics["total_loss"] < best_val_loss:
            best_val_loss = val_metrics["total_loss"]
            if rank == 0:                  # same schema as the reference (train.py:268-277)
                torch.save({"epoch": epoch, "model_state_dict": model.state_dict(),
                            "optimizer_state_dict": optimizer.state_dict(),
                            "scheduler_state_dict": scheduler.state_dict(),
                            "val_loss": val_metrics["total_loss"], "config": config},
                           os.path.join(exp_dir, "best_model.pth"))
    print("Training completed!")
    writer.close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
