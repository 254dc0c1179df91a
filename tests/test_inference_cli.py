"""inference.py (the reference's inference CLI) end to end on the MI355X: a random-weight checkpoint in the reference's schema,
a small model config, the 3-source scene, one batched forward, the output files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = dict(input_dim=32, hidden_dim=128, num_layers=2, num_heads=2, output_channels=64, chaos_strength=0.1)


def test_inference_cli_writes_predictions_features_and_metrics(tmp_path):
    from smokephysai_amd.models import SmokePhysNet
    torch.manual_seed(0)
    model = SmokePhysNet(**MODEL)
    ckpt = tmp_path / "best_model.pth"
    torch.save({"epoch": 0, "model_state_dict": model.state_dict(), "val_loss": 1.0}, str(ckpt))
    with open(os.path.join(ROOT, "config", "config.yaml")) as f:
        config = yaml.safe_load(f)
    config["model"] = dict(MODEL)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(yaml.safe_dump(config))
    out = tmp_path / "out"
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--config", str(cfg), "--checkpoint", str(ckpt),
                           "--output_dir", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    pred = np.load(out / "predictions.npy")
    feats = np.load(out / "physics_features.npy")
    assert pred.shape == (19, 128, 128) and pred.dtype == np.float32 and np.isfinite(pred).all()
    assert feats.shape == (19, 3) and np.isfinite(feats).all()
    metrics = json.loads((out / "inference_metrics.json").read_text())
    assert len(metrics) == 19 and [m["frame"] for m in metrics] == list(range(1, 20))
    assert all(np.isfinite(m["ssim"]) and -1.0 <= m["ssim"] <= 1.0 and m["mse"] >= 0 for m in metrics)
    assert (out / "comparison.png").stat().st_size > 0
