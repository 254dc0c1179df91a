"""Host side of training on 64^2, 512^2 and 1024^2 frames (no GPU): the pure predicate of the train-mode encoder route, the shape rule of the
BatchNorm + ReLU + pool kernels at pools 2 / 16 / 32, and the single statement of their chunk size."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from smokephysai_amd.models.encoder import HIP_ENCODER_SIZES, hip_encoder_supported
from smokephysai_amd.models.norm import BN_CHUNK_FLOATS, hip_bn_relu_pool_supported
from smokephysai_amd.models.smokephys_net import hip_train_encoder_supported


def _fake(*shape, is_cuda=True, dtype=torch.float32):
    return SimpleNamespace(shape=torch.Size(shape), is_cuda=is_cuda, dtype=dtype, dim=lambda: len(shape))


def test_train_route_predicate():
    for H, W, d in ((64, 64, 128), (64, 64, 32), (128, 128, 32), (256, 256, 128), (512, 512, 128), (512, 512, 32), (1024, 1024, 128)):
        assert hip_train_encoder_supported(H, W, d), (H, W, d)
    for H, W, d in ((96, 160, 32), (128, 256, 32), (2048, 2048, 128), (128, 128, 48)):
        assert not hip_train_encoder_supported(H, W, d), (H, W, d)


def test_train_route_predicate_equals_the_eval_encoders():
    for H in (32, 64, 96, 128, 192, 256, 512, 1024, 2048):
        for W in (H, 2 * H):
            for d in (0, 32, 48, 64, 96, 128, 256, 512, 1024):
                assert hip_train_encoder_supported(H, W, d) == hip_encoder_supported(H, W, d), (H, W, d)
    assert {H // 32 for H in HIP_ENCODER_SIZES} == {2, 4, 8, 16, 32} == set(BN_CHUNK_FLOATS) - {1}


def test_encode_frames_asks_the_predicate():
    src = open(os.path.join(ROOT, "smokephysai_amd", "models", "smokephys_net.py")).read()
    assert "hip_train_encoder_supported(H, W, mid)" in src and "P in (4, 8)" not in src


@pytest.mark.parametrize("pool,chunk", [(2, 4096), (16, 8192), (32, 32768)])
def test_bn_shape_rule_new_pools(pool, chunk):
    W = 32 * pool
    rows = chunk // W                                             # rows of one chunk: the smallest plane
    assert hip_bn_relu_pool_supported(_fake(2, 3, rows, W), pool)
    assert hip_bn_relu_pool_supported(_fake(1, 128, W, W), pool)           # the encoder's own plane
    assert hip_bn_relu_pool_supported(_fake(1, 2, 3 * rows, W), pool)
    assert not hip_bn_relu_pool_supported(_fake(2, 3, rows, 2 * W), pool)          # W == 32 * pool
    assert not hip_bn_relu_pool_supported(_fake(2, 3, 2 * rows, W // 2), pool)
    assert not hip_bn_relu_pool_supported(_fake(2, 3, rows + rows // 2, W), pool)  # whole chunks
    assert not hip_bn_relu_pool_supported(_fake(2, 3, rows, W, is_cuda=False), pool)
    assert not hip_bn_relu_pool_supported(_fake(2, 3, rows, W, dtype=torch.float64), pool)
    assert not hip_bn_relu_pool_supported(_fake(3, rows, W), pool)


def test_bn_shape_rule_other_pools():
    assert not hip_bn_relu_pool_supported(_fake(2, 3, 96, 96), 3)
    assert not hip_bn_relu_pool_supported(_fake(2, 3, 64, 2048), 64)
    assert not hip_bn_relu_pool_supported(_fake(2, 3, 64, 64, is_cuda=False), 1)
    # the rule of the pools that were there before is unchanged
    assert hip_bn_relu_pool_supported(_fake(2, 3, 64, 64), 1) and hip_bn_relu_pool_supported(_fake(2, 3, 128, 128), 4)
    assert hip_bn_relu_pool_supported(_fake(2, 3, 64, 256), 8) and not hip_bn_relu_pool_supported(_fake(2, 3, 32, 256), 8)
    assert not hip_bn_relu_pool_supported(_fake(2, 3, 128, 128), 8)


def test_chunk_size_has_one_statement_in_the_library():
    """bn_chunk_floats in norm.h is the only place that spells the chunk sizes; api.hip and norm.hip call it, and the Python table agrees."""
    csrc = os.path.join(ROOT, "smokephysai_amd", "csrc")
    hdr = open(os.path.join(csrc, "norm.h")).read()
    m = re.search(r"constexpr int bn_chunk_floats\(int pool\) \{ return (.*?); \}", hdr)
    assert m, "bn_chunk_floats"
    expr = m.group(1)                                            # pool == 8 ? 16384 : pool == 16 ? 8192 : ... : 4096
    for pool, chunk in BN_CHUNK_FLOATS.items():
        got = eval(re.sub(r"(pool == \d+) \? (\d+) :", r"\2 if \1 else", expr), {"pool": pool})
        assert got == chunk, (pool, got, chunk)
    for name in ("norm.hip", "api.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert "? 16384 : 4096" not in src, name
    api = open(os.path.join(csrc, "api.hip")).read()
    body = api[api.index("static int bn_check("):]
    body = body[:body.index("\n}\n")]
    assert "bn_chunk_floats(pool)" in body and "bn_pool_built(pool)" in body
    norm = open(os.path.join(csrc, "norm.hip")).read()
    assert norm.count("bn_chunks_per_plane(") == 2               # the launch grids and the workspace size


def test_abi_version_and_header_comment():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17        # a widening: refused calls now succeed
    assert "{1, 2, 4, 8, 16, 32}" in hdr
