"""CPU checks beside tests/test_hip_decoder.py: the stage-1 error bound of that module is satisfiable by plain float32 arithmetic and
bites on the two mistakes a sub-pixel transposed convolution invites, and hip_decoder_supported (models/decoder.py) refuses every
head the folded kernels would compute wrongly.  No kernel runs here."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from smokephysai_amd.models import SmokePhysNet
from smokephysai_amd.models.decoder import hip_decoder_supported
from test_hip_decoder import convt_stage_reference, head_params64, make_head, outside_bound, tokens_as_image

S = 16
# output row 2i + p reads (ky, input row i + d): y = 2 iy - 1 + ky (decoder.hip); columns likewise
TAPS = {0: ((1, 0), (3, -1)), 1: ((0, 1), (2, 0))}
SWAPPED = {0: ((3, 0), (1, -1)), 1: TAPS[1]}              # the kx = 1 and kx = 3 taps exchanged


def stage1_float32(tokens, p, col_taps=TAPS, pad_mode="constant"):
    """tmp1 [32, 2S, 2S] of one frame in float32 numpy: BatchNorm folded into weights and shift in float32, the transposed
    convolution as four 2 x 2 sub-pixel convolutions, accumulated in float32 over the 64 channels (vectorised over the outputs)."""
    f = np.float32
    w, b, gamma, beta, mean, var = (p[k].numpy().astype(f) for k in ("ct1_w", "ct1_b", "bn1_w", "bn1_b", "bn1_mean", "bn1_var"))
    s = (gamma / np.sqrt(var + f(1e-5))).astype(f)
    wf = (w * s[None, :, None, None]).astype(f)
    shift = ((b - mean) * s + beta).astype(f)
    x = np.pad(tokens.numpy().astype(f).reshape(S, S, 64).transpose(2, 0, 1), ((0, 0), (1, 1), (1, 1)), mode=pad_mode)
    out = np.zeros((32, 2 * S, 2 * S), f)
    for py in (0, 1):
        for px in (0, 1):
            acc = np.zeros((32, S, S), f)
            for c in range(64):
                for ky, dy in TAPS[py]:
                    for kx, dx in col_taps[px]:
                        acc += x[c, 1 + dy:1 + dy + S, 1 + dx:1 + dx + S][None] * wf[c, :, ky, kx][:, None, None]
            out[:, py::2, px::2] = np.maximum(acc + shift[:, None, None], f(0))
    assert out.dtype == f
    return out


@pytest.fixture(scope="module")
def stage1():
    head = make_head("cpu")
    p = {k: v.float() for k, v in head_params64(head).items()}
    tokens = torch.randn(1, S * S, 64, generator=torch.Generator().manual_seed(1))
    p64 = head_params64(head)
    with torch.no_grad():
        ref, bound = convt_stage_reference(tokens_as_image(tokens), p64["ct1_w"], p64["ct1_b"], p64["bn1_w"], p64["bn1_b"],
                                           p64["bn1_mean"], p64["bn1_var"])
    return p, tokens[0], ref[0], bound[0]


def test_float32_restatement_lies_inside_the_stage_bound(stage1):
    p, tokens, ref, bound = stage1
    bad, worst = outside_bound(torch.from_numpy(stage1_float32(tokens, p)), ref, bound)
    assert int(bad.sum()) == 0 and worst < 1.0, worst
    assert float(ref.max()) > 0.1 and float((ref == 0).double().mean()) > 0.05          # both sides of the ReLU are present


def test_swapped_column_taps_fall_outside_the_stage_bound(stage1):
    p, tokens, ref, bound = stage1
    bad, _ = outside_bound(torch.from_numpy(stage1_float32(tokens, p, col_taps=SWAPPED)), ref, bound)
    assert int(bad.sum()) >= 1
    assert int(bad[:, :, 1::2].sum()) == 0                   # (only the swapped parity is wrong)


def test_replicate_padding_falls_outside_the_stage_bound(stage1):
    p, tokens, ref, bound = stage1
    bad, _ = outside_bound(torch.from_numpy(stage1_float32(tokens, p, pad_mode="edge")), ref, bound)
    assert int(bad.sum()) >= 1
    assert int(bad[:, 1:-1, 1:-1].sum()) == 0                # (only the image border is wrong)


def test_a_nan_counts_as_outside_the_bound(stage1):
    p, tokens, ref, bound = stage1
    got = torch.from_numpy(stage1_float32(tokens, p))
    got[3, 5, 7] = float("nan")
    bad, worst = outside_bound(got, ref, bound)
    assert int(bad.sum()) == 1 and bool(bad[3, 5, 7]) and worst == float("inf")


# ------------------------------------------------------------------------------------------------ the route predicate
_HEAD = []


def _default():
    if not _HEAD:
        _HEAD.append(SmokePhysNet().reconstruction_head.eval())
    return copy.deepcopy(_HEAD[0])


def _with(i, module):
    head = _default()
    head[i] = module.eval()
    return head


def _bn(i, **attrs):
    head = _default()
    for k, v in attrs.items():
        setattr(head[i], k, v)
    return head


REFUSED = {
    "LeakyReLU at 2": lambda: _with(2, nn.LeakyReLU(0.01)),
    "LeakyReLU at 5": lambda: _with(5, nn.LeakyReLU(0.01)),
    "bn1.eps 1e-3": lambda: _bn(1, eps=1e-3),
    "bn2.eps 1e-3": lambda: _bn(4, eps=1e-3),
    "bn1 in train mode": lambda: _bn(1, training=True),
    "bn2 in train mode": lambda: _bn(4, training=True),
    "bn1 affine=False": lambda: _with(1, nn.BatchNorm2d(32, affine=False)),
    "bn2 track_running_stats=False": lambda: _with(4, nn.BatchNorm2d(16, track_running_stats=False)),
    "c3 dilation 2": lambda: _with(6, nn.Conv2d(16, 1, 3, padding=1, dilation=2)),
    "c2 groups 2": lambda: _with(3, nn.ConvTranspose2d(32, 16, 4, stride=2, padding=1, groups=2)),
    "c3 padding_mode reflect": lambda: _with(6, nn.Conv2d(16, 1, 3, padding=1, padding_mode="reflect")),
    "c3 stride 2": lambda: _with(6, nn.Conv2d(16, 1, 3, stride=2, padding=1)),
    "c1 output_padding 1": lambda: _with(0, nn.ConvTranspose2d(64, 32, 4, stride=2, padding=1, output_padding=1)),
    "7 modules": lambda: _default()[:7],
    "float64 parameters": lambda: _default().double(),
    "float64 running statistics": lambda: _bn(1, running_var=torch.ones(32, dtype=torch.float64)),
    "the whole head in train mode": lambda: _default().train(),
}


def test_predicate_accepts_the_default_head_in_eval_mode():
    head = _default()
    assert hip_decoder_supported(head, 32) and hip_decoder_supported(head, 16) and hip_decoder_supported(head, 48)
    assert hip_decoder_supported(copy.deepcopy(head), 32)
    assert hip_decoder_supported(make_head("cpu"), 32)                    # other statistics and affine parameters: still the same head


@pytest.mark.parametrize("change", list(REFUSED))
def test_predicate_refuses(change):
    assert not hip_decoder_supported(REFUSED[change](), 32)


@pytest.mark.parametrize("side", [24, 8, 0, 40])
def test_predicate_refuses_token_grids_the_tiles_do_not_cover(side):
    assert not hip_decoder_supported(_default(), side)
