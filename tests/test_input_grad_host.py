"""Host side of the eval-mode input-gradient route (no GPU): the smk_conv1_train_dgrad export, the pure route predicate, the split of the
first convolution's shape rules and the input_grad switch."""
import copy
import os
import pickle
import re
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from conftest import ROOT
from smokephysai_amd import _lib
from smokephysai_amd.models.conv import hip_conv1_frozen_supported, hip_conv1_train_supported
from smokephysai_amd.models.decoder_train import hip_head_frozen_supported, hip_head_train_supported
from smokephysai_amd.models.norm import hip_frozen_bn_relu_pool_supported
from smokephysai_amd.models.smokephys_net import SmokePhysNet, hip_input_grad_supported

SMALL = dict(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4, output_channels=16)


def _fake(*shape, is_cuda=True, dtype=torch.float32, requires_grad=False):
    return SimpleNamespace(shape=torch.Size(shape), is_cuda=is_cuda, dtype=dtype, dim=lambda: len(shape), requires_grad=requires_grad)


def test_conv1_dgrad_is_exported_bound_and_declared():
    assert "smk_conv1_train_dgrad" in _lib.EXPORTS
    assert len(_lib._SIGNATURES["smk_conv1_train_dgrad"]) == 7
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    m = re.search(r"int\s+smk_conv1_train_dgrad\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 7
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17        # additive: the version stays
    assert "keeps PyTorch-ROCm's" not in hdr


def test_route_predicate_shapes():
    assert hip_input_grad_supported(128, 128, 32) and hip_input_grad_supported(256, 256, 32)
    assert hip_input_grad_supported(128, 128, 128) and hip_input_grad_supported(256, 256, 128) and hip_input_grad_supported(256, 256, 256)
    for H, W in ((64, 64), (512, 512), (96, 160), (128, 256), (1024, 1024)):
        assert not hip_input_grad_supported(H, W, 32), (H, W)
    assert not hip_input_grad_supported(128, 128, 256)           # an up-sampling first pool: not one block mean
    assert not hip_input_grad_supported(128, 128, 48) and not hip_input_grad_supported(128, 128, 0)


@pytest.mark.parametrize("flag", ["eval_mode", "on_device", "grad_enabled", "input_requires_grad", "frozen_bn"])
def test_route_predicate_needs_every_flag(flag):
    assert not hip_input_grad_supported(128, 128, 32, **{flag: False})


def test_route_predicate_refuses_parameters_that_want_gradients():
    assert not hip_input_grad_supported(128, 128, 32, params_require_grad=True)
    assert not hip_input_grad_supported(256, 256, 128, params_require_grad=True)


def test_conv1_shape_rules_are_split():
    conv = nn.Conv2d(1, 64, 7, padding=3)
    assert hip_conv1_frozen_supported(_fake(2, 1, 7, 12), conv) and not hip_conv1_train_supported(_fake(2, 1, 7, 12), conv)
    assert hip_conv1_frozen_supported(_fake(1, 1, 1, 4), conv) and hip_conv1_frozen_supported(_fake(1, 1, 5, 260), conv)
    assert hip_conv1_train_supported(_fake(2, 1, 128, 128), conv) and hip_conv1_frozen_supported(_fake(2, 1, 128, 128), conv)
    assert not hip_conv1_train_supported(_fake(1, 1, 30, 64), conv) and hip_conv1_frozen_supported(_fake(1, 1, 30, 64), conv)
    assert not hip_conv1_frozen_supported(_fake(2, 1, 7, 6), conv)
    assert not hip_conv1_frozen_supported(_fake(0, 1, 8, 8), conv) and not hip_conv1_frozen_supported(_fake(65536, 1, 8, 8), conv)
    assert not hip_conv1_frozen_supported(_fake(2, 1, 8, 8, is_cuda=False), conv)
    assert not hip_conv1_frozen_supported(_fake(2, 1, 8, 8, dtype=torch.float64), conv)
    assert not hip_conv1_frozen_supported(_fake(2, 1, 8, 8), nn.Conv2d(1, 64, 7, padding=3, padding_mode="reflect"))
    assert not hip_conv1_frozen_supported(_fake(2, 1, 8, 8), nn.Conv2d(1, 64, 5, padding=2))


def test_frozen_bn_shape_rule():
    for pool in (1, 4, 8):
        assert hip_frozen_bn_relu_pool_supported(_fake(2, 16, 32 * pool, 32 * pool), pool)
    assert hip_frozen_bn_relu_pool_supported(_fake(2, 64, 128, 128), 1) and hip_frozen_bn_relu_pool_supported(_fake(2, 32, 64, 64), 1)
    assert not hip_frozen_bn_relu_pool_supported(_fake(2, 16, 128, 128), 8) and not hip_frozen_bn_relu_pool_supported(_fake(2, 16, 256, 256), 4)
    assert not hip_frozen_bn_relu_pool_supported(_fake(2, 16, 64, 64), 2)
    assert not hip_frozen_bn_relu_pool_supported(_fake(2, 16, 3, 5), 1)
    assert not hip_frozen_bn_relu_pool_supported(_fake(2, 16, 32, 32, is_cuda=False), 1)


def test_head_frozen_predicate():
    head = SmokePhysNet(**SMALL).reconstruction_head.eval()
    tok = _fake(2, 1024, 16)
    assert not hip_head_frozen_supported(head, tok)              # its parameters still want gradients
    for p in head.parameters():
        p.requires_grad_(False)
    assert hip_head_frozen_supported(head, tok) and not hip_head_train_supported(head, tok)
    assert not hip_head_frozen_supported(copy.deepcopy(head).train(), tok)
    assert not hip_head_frozen_supported(copy.deepcopy(head).double(), tok)
    assert not hip_head_frozen_supported(head, _fake(2, 1024, 16, is_cuda=False))
    assert not hip_head_frozen_supported(head, _fake(2, 1024, 32))


def test_input_grad_option():
    m = SmokePhysNet(**SMALL)
    assert m.input_grad == SmokePhysNet.INPUT_GRAD_DEFAULT and m.input_grad in ("hip", "torch")
    m.input_grad = "torch"
    assert m.input_grad == "torch" and SmokePhysNet(**SMALL).input_grad == SmokePhysNet.INPUT_GRAD_DEFAULT
    assert copy.deepcopy(m).input_grad == "torch" and pickle.loads(pickle.dumps(m)).input_grad == "torch"
    assert SmokePhysNet(**SMALL, input_grad="hip").input_grad == "hip"
    with pytest.raises(ValueError):
        m.input_grad = "miopen"
    with pytest.raises(ValueError):
        SmokePhysNet(**SMALL, input_grad="fast")


def test_config_carries_input_grad():
    import yaml

    import train
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "config.yaml")))
    assert cfg["mi355x"]["input_grad"] == SmokePhysNet.INPUT_GRAD_DEFAULT
    small = {"model": dict(input_dim=32, hidden_dim=64, num_layers=1, num_heads=4, chaos_strength=0.1)}
    assert train.build_model(small).input_grad == SmokePhysNet.INPUT_GRAD_DEFAULT
    assert train.build_model(dict(small, mi355x={"input_grad": "torch"})).input_grad == "torch"


def test_cpu_frames_keep_their_route():
    m = SmokePhysNet(**SMALL).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.rand(1, 1, 128, 128, requires_grad=True)
    assert m._encoder_route(x) == "hip"                          # eval off-GPU: the product refuses, as before
