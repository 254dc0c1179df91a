#!/usr/bin/env python3
"""SmokePhysAI inference on MI355X -- the reference's inference.py CLI (same --config / --checkpoint flags).

Simulates the reference's 3-source test scene for 20 frames, runs the model over the first 19 frames as ONE batched forward
(the reference makes 19 batch-1 calls) and writes, under --output_dir:
  predictions.npy         [19, H', W'] reconstructions (H' x W' = the reconstruction head's 128 x 128)
  physics_features.npy    [19, 3]
  inference_metrics.json  per frame i: SSIM / PSNR / MSE of prediction i against ground-truth frame i+1 (RobustnessEvaluator's
                          image_quality, one launch); written only when the prediction and frame shapes match
  comparison.png          the reference's ground truth vs prediction figure (frames first, middle, last), unless --no_plots
  attention_maps.png      with --attention-maps [LAYER] (default layer: the last): SmokeVisualizer.plot_attention_maps of the first frame --
                          the frame, the attention matrix of (batch 0, head 0) and the attention the tokens receive (head 0), both from
                          SmokePhysNet.attention_maps (libsmokehip kernels: no [B, heads, L, L] tensor)
"""
import argparse
import json
import math
import os

import numpy as np
import torch
import yaml

from benchmark import load_model
from smokephysai_amd.evaluation import RobustnessEvaluator
from smokephysai_amd.physics import SmokeSimulator

POSITIONS = [(64, 64), (32, 32), (96, 96)]      # inference.py:39-41 of the reference
INTENSITIES = [1.5, 1.0, 0.8]


def load_config(config_path: str) -> dict:
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def generate_test_sequence(simulator: SmokeSimulator, sequence_length: int = 20) -> torch.Tensor:
    """The reference's scene (setup_grid, three incense sources, sequence_length fractal-perturbed steps): [T, H, W] on the device."""
    simulator.ns_solver.setup_grid()
    simulator.add_incense_source(POSITIONS, INTENSITIES)
    return simulator.simulate_sequence(sequence_length)[0]


def run_inference(model, sequence: torch.Tensor):
    """Frames 0..T-2 as one batch: (reconstructions [T-1, H', W'], physics features [T-1, 3]) on the device."""
    with torch.no_grad():
        out = model(sequence[:-1, None].contiguous())
    return out["reconstructed"][:, 0], out["physics_features"]


def frame_metrics(predictions: torch.Tensor, ground_truth: torch.Tensor):
    """Per frame i: SSIM / PSNR / MSE of predictions[i] against ground_truth[i+1]; None when the shapes differ."""
    target = ground_truth[1:]
    if predictions.shape != target.shape:
        return None
    q = RobustnessEvaluator(device=str(predictions.device)).image_quality(predictions[:, None], target[:, None].contiguous())
    finite = lambda v: v if math.isfinite(v) else None           # identical frames: PSNR +inf -> null (strict JSON)
    return [{"frame": i + 1, "ssim": float(q["ssim"][i]), "psnr": finite(float(q["psnr"][i])), "mse": float(q["mse"][i])}
            for i in range(predictions.shape[0])]


def save_comparison(ground_truth: np.ndarray, predictions: np.ndarray, path: str):
    """The reference's comparison figure (inference.py:100-115): ground truth row over predicted row at the first, middle and last
    prediction.  The last column pairs prediction i with ground-truth frame i+1 like the others (the reference's index -1 + 1
    shows frame 0 there)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, axes = plt.subplots(2, 3, figsize=(18, 12))
    for i, idx in enumerate([0, len(predictions) // 2, len(predictions) - 1]):
        axes[0, i].imshow(ground_truth[idx + 1], cmap="hot")
        axes[0, i].set_title(f"Ground Truth Frame {idx + 1}")
        axes[0, i].axis("off")
        axes[1, i].imshow(predictions[idx], cmap="hot")
        axes[1, i].set_title(f"Predicted Frame {idx + 1}")
        axes[1, i].axis("off")
    plt.tight_layout()
    plt.savefig(path, dpi=150)
    plt.close(fig)


def save_attention_maps(model, sequence: torch.Tensor, layer: int, path: str):
    """attention_maps.png for the first frame: layer `layer` (negative: from the last), the matrix of (batch 0, head 0) and head 0's received map."""
    from smokephysai_amd.utils import SmokeVisualizer
    import matplotlib.pyplot as plt
    frame = sequence[:1, None].contiguous()
    layer = layer % len(model.chaos_layers)
    out = model.attention_maps(frame, layers=[layer], probs_for=(0, 1, 0, 1))
    fig = SmokeVisualizer().plot_attention_maps(out["attention_probs"][layer], frame, save_path=path, received=out["attention_received"][layer])
    plt.close(fig)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="SmokePhysAI Inference Script")
    parser.add_argument("--config", type=str, default="config/config.yaml", help="Path to configuration file")
    parser.add_argument("--checkpoint", type=str, required=True, help="Path to model checkpoint")
    parser.add_argument("--output_dir", type=str, default=".", help="Directory the outputs are written to")
    parser.add_argument("--no_plots", action="store_true", help="Do not write comparison.png")
    parser.add_argument("--attention-maps", dest="attention_maps", type=int, nargs="?", const=-1, default=None, metavar="LAYER",
                        help="Write attention_maps.png for transformer layer LAYER (default: the last one)")
    return parser


def main():
    args = build_parser().parse_args()
    config = load_config(args.config)
    if not torch.cuda.is_available():
        raise RuntimeError("inference.py needs a ROCm GPU: smokephysai_amd has no CPU fallback")
    device = torch.device("cuda")
    print(f"Using device: {device}")
    model = load_model(config, args.checkpoint, str(device))
    sim_cfg = config["simulation"]
    hw = config.get("mi355x", {}) or {}
    simulator = SmokeSimulator(grid_size=tuple(sim_cfg["grid_size"]), dt=sim_cfg["dt"], viscosity=sim_cfg["viscosity"],
                               device=str(device), jacobi_iters=hw.get("jacobi_iters", 20))
    sequence = generate_test_sequence(simulator, sequence_length=20)
    predictions, physics_features = run_inference(model, sequence)
    metrics = frame_metrics(predictions, sequence)
    os.makedirs(args.output_dir, exist_ok=True)
    gt, pred = sequence.cpu().numpy(), predictions.cpu().numpy()
    np.save(os.path.join(args.output_dir, "predictions.npy"), pred)
    np.save(os.path.join(args.output_dir, "physics_features.npy"), physics_features.cpu().numpy())
    if metrics is not None:
        with open(os.path.join(args.output_dir, "inference_metrics.json"), "w") as f:
            json.dump(metrics, f, indent=1)
        print(f"mean SSIM {np.mean([m['ssim'] for m in metrics]):.4f}, mean MSE {np.mean([m['mse'] for m in metrics]):.6f}")
    else:
        print(f"predictions {tuple(pred.shape[1:])} and frames {tuple(gt.shape[1:])} differ in shape: no inference_metrics.json")
    if not args.no_plots:
        save_comparison(gt, pred, os.path.join(args.output_dir, "comparison.png"))
    if args.attention_maps is not None:
        save_attention_maps(model, sequence, args.attention_maps, os.path.join(args.output_dir, "attention_maps.png"))
    print(f"Results have been saved to {args.output_dir}")


if __name__ == "__main__":
    main()
