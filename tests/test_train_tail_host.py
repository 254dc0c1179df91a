"""Host-side contract of the train step tail on libsmokehip (smk_grad_norm, smk_adamw_step, smk_train_loss_*): the ABI surface, the
`mi355x.optimizer` / `mi355x.losses` switches of train.py, HipAdamW's torch route on CPU parameters and its state_dict, and the two
eligibility predicates.  No GPU: the kernels themselves are tested in tests/test_hip_train_tail.py."""
import copy
import os
import re

import pytest
import torch

from smokephysai_amd import _lib
from smokephysai_amd.models.losses import hip_train_losses_supported
from smokephysai_amd.models.physics_regularizer import PhysicsRegularizer
from smokephysai_amd.optim import HipAdamW, hip_adamw_supported
from smokephysai_amd.utils.distributed import clip_grad_norm_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smk_grad_norm_workspace", "smk_grad_norm", "smk_adamw_step", "smk_train_loss_workspace", "smk_train_loss_forward",
               "smk_train_loss_backward")


def test_header_and_binding_declare_the_train_tail():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/smokehip.h"
        assert name in _lib.EXPORTS, f"{name} is missing from _lib.EXPORTS"
        assert hasattr(L, name), f"{name} is not exported by libsmokehip.so"
    assert "smk_opt_tensor" in code
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == L.smk_abi_version() == 17


def _config(**hw):
    return {"training": {"learning_rate": 2e-3, "weight_decay": 0.03}, "mi355x": hw}


def test_build_optimizer_and_loss_route_switches():
    import train
    params = [torch.nn.Parameter(torch.zeros(3))]
    for cfg in (_config(), {"training": _config()["training"]}, _config(optimizer="torch")):
        opt = train.build_optimizer(cfg, params)
        assert type(opt) is torch.optim.AdamW
        assert opt.defaults["lr"] == 2e-3 and opt.defaults["weight_decay"] == 0.03
        assert train.loss_route(cfg) == "torch"
    opt = train.build_optimizer(_config(optimizer="hip"), params)
    assert type(opt) is HipAdamW and isinstance(opt, torch.optim.AdamW)
    assert opt.defaults["lr"] == 2e-3 and opt.defaults["weight_decay"] == 0.03 and opt.clip_writes_grad is False
    assert train.loss_route(_config(losses="hip")) == "hip"
    with pytest.raises(ValueError, match=r"'torch'.*'hip'"):
        train.build_optimizer(_config(optimizer="fused"), params)
    with pytest.raises(ValueError, match=r"'torch'.*'hip'"):
        train.loss_route(_config(losses="triton"))
    with pytest.raises(ValueError, match=r"'torch'.*'hip'"):
        train.batch_losses(None, None, {}, "cpu", losses="cuda")


def test_config_yaml_carries_both_switches_at_their_defaults():
    import train
    cfg = train.load_config(os.path.join(ROOT, "config", "config.yaml"))
    assert cfg["mi355x"]["optimizer"] == "torch" and cfg["mi355x"]["losses"] == "torch"


def _cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 7), (13,), (2, 3, 4), (1,))]


def _set_grads(params, step):
    g = torch.Generator().manual_seed(100 + step)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g) * 3.0


def test_cpu_step_is_torchs_clip_and_adamw_bit_for_bit():
    a, b = _cpu_params(), _cpu_params()
    hip = HipAdamW(a, lr=1e-2, weight_decay=0.05)
    ref = torch.optim.AdamW(b, lr=1e-2, weight_decay=0.05)
    for step in range(3):
        _set_grads(a, step)
        _set_grads(b, step)
        hip.step(clip_max_norm=1.0)
        norm = clip_grad_norm_(b, max_norm=1.0)
        ref.step()
        assert torch.equal(hip.last_grad_norm, norm)
        for p, q in zip(a, b):
            assert torch.equal(p, q) and torch.equal(p.grad, q.grad)
    for p, q in zip(a, b):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(hip.state[p][k], ref.state[q][k]), k


def test_state_dict_round_trips_with_torch_adamw():
    a, b = _cpu_params(), _cpu_params()
    hip = HipAdamW(a, lr=1e-2, weight_decay=0.05)
    _set_grads(a, 0)
    hip.step(clip_max_norm=1.0)
    sd = hip.state_dict()
    ref = torch.optim.AdamW(b, lr=1.0)
    _set_grads(b, 0)
    ref.step()
    ref_sd = ref.state_dict()
    assert sd["param_groups"][0].keys() == ref_sd["param_groups"][0].keys()          # no key of HipAdamW's own in the checkpoint
    assert sd["state"].keys() == ref_sd["state"].keys()
    assert all(sd["state"][k].keys() == ref_sd["state"][k].keys() for k in sd["state"])
    ref.load_state_dict(copy.deepcopy(sd))
    assert ref.state_dict()["param_groups"] == sd["param_groups"]
    back = HipAdamW(_cpu_params(), lr=0.5)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    got = back.state_dict()
    assert got["param_groups"] == sd["param_groups"]
    for k, st in sd["state"].items():
        for name, v in st.items():
            assert torch.equal(got["state"][k][name], v), (k, name)


def test_hip_adamw_supported_refuses_what_the_kernels_do_not_take():
    group = HipAdamW([torch.nn.Parameter(torch.zeros(2))]).param_groups[0]
    ok = torch.nn.Parameter(torch.zeros(4, 4))
    ok.grad = torch.zeros(4, 4)
    f64 = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    f64.grad = torch.zeros(4, dtype=torch.float64)
    strided = torch.nn.Parameter(torch.zeros(4, 6)[:, ::2])
    strided.grad = torch.zeros(4, 3)
    strided_grad = torch.nn.Parameter(torch.zeros(4, 3))
    strided_grad.grad = torch.zeros(4, 6)[:, ::2]
    assert not strided.is_contiguous() and not strided_grad.grad.is_contiguous()
    for p in (f64, strided, strided_grad, ok):                     # `ok` is a CPU tensor: not on a ROCm device
        assert hip_adamw_supported(group, [p]) is False
    assert hip_adamw_supported(dict(group, amsgrad=True), [ok]) is False
    if torch.cuda.is_available():
        dev = torch.nn.Parameter(torch.zeros(4, 4, device="cuda"))
        dev.grad = torch.zeros(4, 4, device="cuda")
        assert hip_adamw_supported(group, [dev]) is True
        for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
            assert hip_adamw_supported(dict(group, **{flag: True}), [dev]) is False, flag
        d64 = torch.nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float64))
        d64.grad = torch.zeros_like(d64)
        assert hip_adamw_supported(group, [d64]) is False


def test_hip_train_losses_supported_refuses_what_the_kernels_do_not_take():
    pred, target = torch.rand(2, 1, 8, 8), torch.rand(2, 1, 8, 8)
    cp, ct, seq = torch.rand(2, 3), torch.rand(2, 3), torch.rand(2, 4, 8, 8)
    assert hip_train_losses_supported(pred, target, cp, ct, seq) is False                    # CPU tensors
    if torch.cuda.is_available():
        d = [t.cuda() for t in (pred, target, cp, ct, seq)]
        assert hip_train_losses_supported(*d) is True
        assert hip_train_losses_supported(d[0], d[1][:, :, :4].contiguous(), d[2], d[3], d[4]) is False      # mismatched shapes
        assert hip_train_losses_supported(d[0], d[1], d[2], d[3], d[4].clone().requires_grad_()) is False
        assert hip_train_losses_supported(d[0].transpose(2, 3), d[1], d[2], d[3], d[4]) is False
    assert hip_train_losses_supported(pred, target[:, :, :4], cp, ct, seq) is False
    assert hip_train_losses_supported(pred, target, cp, ct, seq.clone().requires_grad_()) is False


class _TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)
        self.head = torch.nn.Linear(16 * 16, 3)

    def forward(self, x):
        y = torch.sigmoid(self.conv(x))
        return {"reconstructed": y, "physics_features": self.head(y.flatten(1))}


def test_batch_losses_hip_on_cpu_tensors_is_the_torch_route_exactly():
    import train
    torch.manual_seed(5)
    model = _TinyNet()
    batch = {"input": torch.rand(3, 1, 16, 16), "target": torch.rand(3, 1, 16, 16), "chaos_features": torch.rand(3, 3),
             "sequence": torch.rand(3, 5, 16, 16)}
    reg = PhysicsRegularizer(conservation_weight=0.7, continuity_weight=1.3)
    ref = train.batch_losses(model, reg, batch, "cpu")
    got = train.batch_losses(model, reg, batch, "cpu", losses="hip")
    assert len(got) == len(ref) == 4
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    got[0].backward()
    grads = [p.grad.clone() for p in model.parameters()]
    model.zero_grad()
    ref[0].backward()
    for a, p in zip(grads, model.parameters()):
        assert torch.equal(a, p.grad)
