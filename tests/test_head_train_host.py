"""CPU checks of the opt-in training route of the reconstruction head (models/decoder_train.py): the constructor option, the predicate
that decides when the libsmokehip kernels serve a call, train.py's model helper, and the C ABI entries.  No kernel runs here."""
import copy
import os
import pickle
import re
import types

import pytest
import torch
from torch import nn

from smokephysai_amd import _lib
from smokephysai_amd.models import SmokePhysNet
from smokephysai_amd.models.decoder_train import hip_head_train_supported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4)


def _tokens(B=8, C0=64, is_cuda=True, dtype=torch.float32):
    """A stand-in for ROCm tokens [B, 1024, C0]: the predicate reads only these attributes (no device needed)."""
    return types.SimpleNamespace(is_cuda=is_cuda, dtype=dtype, shape=(B, 1024, C0), dim=lambda: 3)


def test_head_train_option():
    assert SmokePhysNet(**SMALL).head_train == "torch"
    m = SmokePhysNet(**SMALL, head_train="hip")
    assert m.head_train == "hip"
    m.head_train = "torch"
    assert m.head_train == "torch"
    with pytest.raises(ValueError):
        SmokePhysNet(**SMALL, head_train="miopen")
    with pytest.raises(ValueError):
        m.head_train = "fast"
    m.head_train = "hip"
    assert copy.deepcopy(m).head_train == "hip" and pickle.loads(pickle.dumps(m)).head_train == "hip"
    # the state_dict keys do not depend on the route: checkpoints load both ways
    assert list(SmokePhysNet(**SMALL).state_dict()) == list(m.state_dict())
    m.load_state_dict(SmokePhysNet(**SMALL).state_dict())


def test_predicate_accepts_the_default_head_and_c0_16():
    head = SmokePhysNet().reconstruction_head.train()
    assert hip_head_train_supported(head, _tokens(8, 64))
    assert hip_head_train_supported(head, _tokens(1, 64)) and hip_head_train_supported(head, _tokens(65535, 64))
    small = SmokePhysNet(**SMALL, output_channels=16).reconstruction_head.train()
    assert hip_head_train_supported(small, _tokens(3, 16))
    assert hip_head_train_supported(SmokePhysNet(**SMALL, output_channels=48).reconstruction_head.train(), _tokens(2, 48))


def test_predicate_rejects_what_the_kernels_do_not_implement():
    head = SmokePhysNet().reconstruction_head.train()
    assert not hip_head_train_supported(head, _tokens(8, 64, dtype=torch.float64))
    assert not hip_head_train_supported(head, _tokens(8, 64, is_cuda=False))
    assert not hip_head_train_supported(head, torch.zeros(2, 1024, 64))                  # a real CPU tensor
    assert not hip_head_train_supported(head, _tokens(65536, 64))                         # gridDim.z
    assert not hip_head_train_supported(head, _tokens(8, 32))                             # token width != C0
    assert not hip_head_train_supported(copy.deepcopy(head).double(), _tokens(8, 64))    # the float64 copies tests make
    assert not hip_head_train_supported(SmokePhysNet(**SMALL, output_channels=24).reconstruction_head.train(), _tokens(2, 24))

    def changed(i, m):
        h = copy.deepcopy(head)
        h[i] = m
        return h
    assert not hip_head_train_supported(changed(0, nn.ConvTranspose2d(64, 32, 3, stride=2, padding=1)), _tokens())
    assert not hip_head_train_supported(changed(0, nn.ConvTranspose2d(64, 32, 4, stride=1, padding=1)), _tokens())
    assert not hip_head_train_supported(changed(0, nn.ConvTranspose2d(64, 24, 4, stride=2, padding=1)), _tokens())
    assert not hip_head_train_supported(changed(0, nn.ConvTranspose2d(64, 32, 4, stride=2, padding=1, bias=False)), _tokens())
    assert not hip_head_train_supported(changed(3, nn.ConvTranspose2d(32, 16, 4, stride=2, padding=2)), _tokens())
    assert not hip_head_train_supported(changed(6, nn.Conv2d(16, 1, 5, padding=2)), _tokens())
    assert not hip_head_train_supported(changed(7, nn.Tanh()), _tokens())
    assert not hip_head_train_supported(head[:7], _tokens())
    frozen = copy.deepcopy(head)
    frozen[1].eval()                                                                      # a frozen BatchNorm inside a training model
    assert not hip_head_train_supported(frozen, _tokens())
    assert not hip_head_train_supported(copy.deepcopy(head).eval(), _tokens())
    cumulative = copy.deepcopy(head)
    cumulative[4].momentum = None
    assert not hip_head_train_supported(cumulative, _tokens())


def test_cpu_training_forward_keeps_the_modules():
    """On the CPU the option changes nothing: the predicate fails and the modules run (same numbers as the default route)."""
    torch.manual_seed(0)
    a = SmokePhysNet(**SMALL, output_channels=16).train()
    b = copy.deepcopy(a)
    b.head_train = "hip"
    tok = torch.randn(2, 1024, 128)             # encoder tokens
    torch.manual_seed(1)                         # dropout and the chaos noise draw from the generator
    ya = a.forward_tokens(tok)["reconstructed"]
    torch.manual_seed(1)
    yb = b.forward_tokens(tok)["reconstructed"]
    assert torch.equal(ya, yb) and ya.shape == (2, 1, 128, 128)


def _config(**hw):
    cfg = {"model": dict(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4, chaos_strength=0.1)}
    if hw is not None:
        cfg["mi355x"] = hw
    return cfg


def test_train_build_model_passes_recon_head():
    import train
    assert train.build_model({"model": _config()["model"]}).head_train == "torch"         # no mi355x section
    assert train.build_model(_config(sim_batch=8)).head_train == "torch"                  # section without the key
    m = train.build_model(_config(recon_head="hip", encoder_dtype="f32"))
    assert isinstance(m, SmokePhysNet) and m.head_train == "hip" and m.encoder_dtype == "f32" and m.hidden_dim == 64
    assert next(m.parameters()).device.type == "cpu"
    with pytest.raises(ValueError):
        train.build_model(_config(recon_head="cudnn"))


def test_config_documents_recon_head_default_torch():
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "config.yaml")))
    assert cfg["mi355x"]["recon_head"] == "torch"


NEW = ("smk_convt4s2_train_forward", "smk_convt4s2_train_dgrad", "smk_convt4s2_train_wgrad_workspace", "smk_convt4s2_train_wgrad",
       "smk_conv3_sigmoid_train_forward", "smk_conv3_sigmoid_train_workspace", "smk_conv3_sigmoid_train_backward")


def test_new_symbols_declared_exported_bound():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    L = _lib.load()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert n in _lib.EXPORTS and hasattr(L, n), n
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == L.smk_abi_version()


def test_workspace_queries_are_host_only_and_refuse_bad_shapes():
    L = _lib.load()
    assert L.smk_convt4s2_train_wgrad_workspace(8, 64, 32, 32, 32) > 0
    assert L.smk_convt4s2_train_wgrad_workspace(8, 32, 16, 64, 64) > 0
    assert L.smk_convt4s2_train_wgrad_workspace(65536, 64, 32, 32, 32) == 0
    assert L.smk_convt4s2_train_wgrad_workspace(8, 24, 32, 32, 32) == 0
    assert L.smk_conv3_sigmoid_train_workspace(8, 128, 128) >= 8 * 128 * 128 * 4
    assert L.smk_conv3_sigmoid_train_workspace(65536, 128, 128) == 0
    # argument checks run before any device work
    assert L.smk_convt4s2_train_forward(None, None, None, 1, 64, 32, 32, 32, 1, None, None) == -1
    assert L.smk_convt4s2_train_dgrad(16, 16, 65536, 64, 32, 32, 32, 1, 16, None) == -3
