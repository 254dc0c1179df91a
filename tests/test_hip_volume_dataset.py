"""VolumeFrameDataset (volumes in, rendered next frame out; SPEC_3D.md section 11) against the two datasets it is made of, and one epoch of
train.main() on a tiny volume_depth config."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu


def test_volume_frame_dataset_is_the_volume_dataset_with_rendered_targets():
    from smokephysai_amd.utils.data_loader import RenderedSmokeDataset, SyntheticSmokeDataset3D, VolumeFrameDataset
    kw = dict(num_samples=3, grid_size=(8, 64, 64), sequence_length=20, sim_batch=2)
    np.random.seed(21)
    vf = VolumeFrameDataset(**kw)
    np.random.seed(21)
    rd = RenderedSmokeDataset(**kw)
    np.random.seed(21)
    vd = SyntheticSmokeDataset3D(**kw)
    assert len(vf) == len(rd) == len(vd) == 3
    for f, r, v in zip(vf.data, rd.data, vd.data):
        assert torch.equal(f["sequence"], r["sequence"]) and f["chaos_features"] == r["chaos_features"] == v["chaos_features"]
        assert f["volumes"].shape == (10, 8, 64, 64) and torch.equal(f["volumes"], v["sequence"][5:15])      # only the drawable volumes
    for i in range(3):
        for seed in (0, 1, 2):                                # the same draw of the frame index in all three
            np.random.seed(seed)
            a = vf[i]
            np.random.seed(seed)
            b = vd[i]
            np.random.seed(seed)
            c = rd[i]
            assert torch.equal(a["input"], b["input"]) and torch.equal(a["target"], c["target"]) and torch.equal(a["sequence"], c["sequence"])
            assert torch.equal(a["chaos_features"], c["chaos_features"])
    item = vf[1]
    assert item["input"].shape == (1, 8, 64, 64) and item["target"].shape == (1, 64, 64) and item["sequence"].shape == (20, 64, 64)
    assert item["chaos_features"].shape == (3,) and all(item[k].dtype == torch.float32 for k in item)


def test_train_main_runs_an_epoch_on_volumes(tmp_path, monkeypatch):
    """train.main() with mi355x.volume_depth: 8 -- one epoch of two steps, one validation batch; the checkpoint loads into a SmokePhysNet3D."""
    import train
    from smokephysai_amd.models import SmokePhysNet3D
    cfg = {"data": {"grid_size": [64, 64], "sequence_length": 20, "num_train": 4, "num_val": 2, "cache_dir": str(tmp_path / "cache")},
           "model": {"input_dim": 32, "hidden_dim": 128, "num_layers": 1, "num_heads": 2, "output_channels": 64, "chaos_strength": 0.1},
           "physics": {"conservation_weight": 1.0, "continuity_weight": 1.0, "energy_weight": 0.5},
           "training": {"batch_size": 2, "num_epochs": 1, "learning_rate": 1e-3, "weight_decay": 0.01},
           "mi355x": {"volume_depth": 8, "sim_batch": 2, "jacobi_iters": 4}}
    path = tmp_path / "config.yaml"
    path.write_text(yaml.dump(cfg))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["train.py", "--config", str(path)])
    np.random.seed(3)
    torch.manual_seed(3)
    train.main()
    runs = sorted(os.listdir(tmp_path / "experiments"))
    assert len(runs) == 1
    ckpt = torch.load(tmp_path / "experiments" / runs[0] / "best_model.pth", map_location="cuda", weights_only=False)
    assert np.isfinite(ckpt["val_loss"]) and any(k.startswith("encoder3d.net.0.") for k in ckpt["model_state_dict"])
    model = train.build_model(ckpt["config"])
    assert type(model) is SmokePhysNet3D
    model.load_state_dict(ckpt["model_state_dict"])
    assert int(model.encoder3d.net[1].num_batches_tracked) == 2          # two training steps went through the 3-D BatchNorms
    assert sorted(p.name for p in (tmp_path / "cache").iterdir()) == sorted(
        f"{n}.volume8_-y_0.1_0.1_0.25_1.pkl" for n in ("train_data", "val_data"))
