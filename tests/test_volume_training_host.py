"""Host side of training on volumes (SPEC_3D.md section 11), no GPU: Encoder3D's torch route against the fp64 numpy oracle of section 8,
SmokePhysNet3D's state-dict keys, and train.py's config keys (mi355x.volume_depth, mi355x.volume_encoder)."""
import numpy as np
import pytest
import torch

from conftest import rel_err


def _config(**hw):
    return {"data": {"grid_size": [64, 64], "num_train": 4, "num_val": 2, "cache_dir": "./cache"},
            "model": {"input_dim": 32, "hidden_dim": 128, "num_layers": 1, "num_heads": 2, "output_channels": 64, "chaos_strength": 0.1},
            "training": {"batch_size": 2, "num_epochs": 1, "learning_rate": 1e-3, "weight_decay": 0.01},
            "mi355x": hw}


def test_encoder3d_torch_route_is_the_oracle_of_section_8():
    """Eval mode, fp64, on the CPU: the module chain + block mean equals oracle.encoder3d.encoder3d_features (two adaptive pools with the
    depth pooled to 1) to 1e-10, on a volume whose token block is 2 x 1 and on one whose shape is outside the pool rule."""
    from oracle.encoder3d import encoder3d_features
    from smokephysai_amd.models import Encoder3D
    torch.manual_seed(5)
    enc = Encoder3D(route="hip").double().eval()              # on the CPU every call takes the torch route
    with torch.no_grad():
        for bn in (enc.net[1], enc.net[4]):
            bn.running_mean.normal_(0.0, 0.2)
            bn.running_var.uniform_(0.3, 1.3)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.1)
    w = {k: v.detach().numpy() for k, v in enc.weight_dict().items()}
    assert sorted(w) == sorted(["conv1_w", "conv1_b", "bn1_w", "bn1_b", "bn1_mean", "bn1_var", "conv2_w", "conv2_b", "bn2_w", "bn2_b",
                                "bn2_mean", "bn2_var"])
    plain = torch.nn.Sequential(torch.nn.Conv3d(1, 64, 7, padding=3), torch.nn.BatchNorm3d(64), torch.nn.ReLU(),
                                torch.nn.Conv3d(64, 128, 3, padding=1), torch.nn.BatchNorm3d(128), torch.nn.ReLU())
    assert sorted(enc.state_dict()) == sorted("net." + k for k in plain.state_dict())          # torch's keys
    for shape in [(3, 64, 32), (2, 48, 40)]:
        vol = torch.rand(shape, dtype=torch.float64)
        with torch.no_grad():
            tok = enc.tokens(vol[None, None])[0]              # [1024, 128]
        ref, _ = encoder3d_features(vol.numpy(), w)           # [128, 32, 32]
        assert tok.shape == (1024, 128)
        assert rel_err(tok.numpy().T.reshape(128, 32, 32), ref) < 1e-10, shape


def test_smokephysnet3d_state_dict_is_the_2d_keys_plus_encoder3d():
    from smokephysai_amd.models import SmokePhysNet, SmokePhysNet3D
    kw = dict(input_dim=32, hidden_dim=64, num_layers=1, num_heads=1, output_channels=16)
    m2, m3 = SmokePhysNet(**kw), SmokePhysNet3D(**kw, volume_encoder="torch")
    k2, k3 = set(m2.state_dict()), set(m3.state_dict())
    assert k2 < k3 and all(k.startswith("encoder3d.net.") for k in k3 - k2)
    res = m3.load_state_dict(m2.state_dict(), strict=False)
    assert not res.unexpected_keys and res.missing_keys and all(k.startswith("encoder3d.") for k in res.missing_keys)
    assert all(not p.requires_grad for p in m3.input_encoder.parameters())
    assert all(p.requires_grad for p in m3.encoder3d.parameters())
    assert all(p.requires_grad for p in m2.input_encoder.parameters())          # the 2-D model is untouched
    with pytest.raises(ValueError):
        SmokePhysNet3D(**kw, volume_encoder="triton")


def test_data_loader_kwargs_forwards_volume_depth():
    import train
    base = train.data_loader_kwargs(_config())
    assert "volume_depth" not in base and "render_depth" not in base and "render" not in base
    assert train.data_loader_kwargs(_config(volume_depth=0)) == base
    kw = train.data_loader_kwargs(_config(volume_depth=8, render={"light": "+z"}))
    assert kw["volume_depth"] == 8 and kw["render"] == {"light": "+z"} and "render_depth" not in kw
    assert {k: v for k, v in kw.items() if k not in ("volume_depth", "render")} == base
    with pytest.raises(ValueError):
        train.data_loader_kwargs(_config(volume_depth=8, render_depth=8))


def test_create_data_loaders_refuses_both_depths():
    from smokephysai_amd.utils.data_loader import create_data_loaders
    with pytest.raises(ValueError, match="exclude"):
        create_data_loaders(batch_size=1, num_train=1, num_val=1, grid_size=(64, 64), device="cuda", render_depth=8, volume_depth=8)


def test_build_model_returns_the_class_the_config_names():
    import train
    from smokephysai_amd.models import SmokePhysNet, SmokePhysNet3D
    assert type(train.build_model(_config())) is SmokePhysNet
    assert type(train.build_model(_config(volume_depth=0, volume_encoder="torch"))) is SmokePhysNet
    m = train.build_model(_config(volume_depth=8))
    assert type(m) is SmokePhysNet3D and m.encoder3d.route == train.VOLUME_ENCODER_DEFAULT
    assert train.build_model(_config(volume_depth=8, volume_encoder="torch")).encoder3d.route == "torch"
    with pytest.raises(ValueError):
        train.build_model(_config(volume_depth=8, volume_encoder="cuda"))
    with pytest.raises(ValueError, match="sync_bn"):
        train.build_model(_config(volume_depth=8, sync_bn=True))
    assert type(train.build_model(_config(sync_bn=True))) is SmokePhysNet
