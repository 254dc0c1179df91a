"""smk_conv3d_s7_dgrad (csrc/conv3d_train.hip: k_c3t_conv1_dgrad), the data gradient of Conv3d(1, 64, 7, padding 3), alone through the C ABI
against F.conv_transpose3d in float64 on the CPU.  dz1 is randn with half its entries zeroed (as a ReLU mask leaves it), the weight a
default-initialised nn.Conv3d(1, 64, 7).  Bound: 1e-5 in conftest.rel_err's max-norm, SPEC_3D.md section 11's gradient bound; torch's own CPU
fp32 conv_transpose3d gives 3.9e-7 .. 1.2e-6 on these inputs, so an fp32 kernel has a tenfold margin.
Shapes, the smallest at which each part can go wrong: (2,3,8,16) one tile per plane and every kz reaching outside (and an odd depth: the
second plane of the last pair does not exist); (1,9,16,32) interior planes, four tiles per plane sharing halos; (2,1,24,48) D = 1 and 3 x 3
tiles."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import rel_err
from smokephysai_amd import _lib

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3                 # SMK_ERR_UNSUPPORTED (include/smokehip.h)
SHAPES = [(2, 3, 8, 16), (1, 9, 16, 32), (2, 1, 24, 48)]
_REF = {}


def _reference(shape):
    """Inputs (CPU fp32) and the fp64 gradient of one shape, computed once and shared by the tests."""
    if shape not in _REF:
        B, D, H, W = shape
        torch.manual_seed(B * 1000 + D * 100 + H + W)
        w = nn.Conv3d(1, 64, 7, padding=3).weight.detach().clone()
        dz1 = torch.randn(B, D, H, W, 64) * (torch.rand(B, D, H, W, 64) < 0.5)
        ref = F.conv_transpose3d(dz1.double().permute(0, 4, 1, 2, 3), w.double(), padding=3)[:, 0]
        _REF[shape] = dict(w=w, dz1=dz1, ref=ref)
    return _REF[shape]


def _dgrad(dz1, w):
    L = _lib.load()
    B, D, H, W, _ = dz1.shape
    dvol = torch.full((B, D, H, W), float("nan"), device="cuda")
    ws = torch.empty(int(L.smk_conv3d_train_workspace()), device="cuda", dtype=torch.uint8)
    _lib.check(L.smk_conv3d_s7_dgrad(dz1.data_ptr(), w.data_ptr(), B, D, H, W, dvol.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dz1.device)))
    return dvol


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_float64_conv_transpose3d(shape):
    r = _reference(shape)
    dz1, w = r["dz1"].cuda(), r["w"].cuda()
    dvol = _dgrad(dz1, w)
    assert not torch.isnan(dvol).any()                           # every element written
    err = rel_err(dvol.cpu().numpy(), r["ref"].numpy())
    print(f"conv3d s7 dgrad {shape}: rel err {err:.3e}")
    assert err < 1e-5, err
    assert torch.equal(_dgrad(dz1, w), dvol)                     # bit-identical when repeated
    # the Python wrapper hands out exactly this
    from smokephysai_amd.models.encoder3d import hip_conv3d_s7_dgrad
    assert torch.equal(hip_conv3d_s7_dgrad(dz1, w), dvol)


def test_a_sample_does_not_depend_on_its_batch_mates():
    r = _reference((2, 3, 8, 16))
    dz1, w = r["dz1"].cuda(), r["w"].cuda()
    both = _dgrad(dz1, w)
    for b in (0, 1):
        assert torch.equal(_dgrad(dz1[b:b + 1].contiguous(), w)[0], both[b])


@pytest.mark.parametrize("voxel", [(0, 0, 0), (4, 9, 17)], ids=["corner", "interior"])
def test_one_hot_reproduces_the_flipped_kernel_exactly(voxel):
    """dz1 = 1 at one voxel of one channel: dvol[z][y][x] = w[c][voxel + 3 - (z, y, x)] where that index is inside the kernel, else 0 -- a
    single product with 1, so exact."""
    B, D, H, W = 1, 9, 16, 32
    c = 37
    w = _reference((1, 9, 16, 32))["w"]
    dz1 = torch.zeros(B, D, H, W, 64)
    dz1[(0,) + voxel + (c,)] = 1.0
    want = torch.zeros(D, H, W)
    for kz in range(7):
        for ky in range(7):
            for kx in range(7):
                z, y, x = voxel[0] - 3 + kz, voxel[1] - 3 + ky, voxel[2] - 3 + kx      # the output voxel whose tap (kz, ky, kx) reads `voxel`
                if 0 <= z < D and 0 <= y < H and 0 <= x < W:
                    want[z, y, x] = w[c, 0, kz, ky, kx]
    got = _dgrad(dz1.cuda(), w.cuda())[0].cpu()
    assert float(want.abs().max()) > 0
    assert torch.equal(got, want)


def test_refuses_bad_shapes_without_launching():
    L = _lib.load()
    dz1 = torch.randn(1, 2, 16, 32, 64, device="cuda")
    w = torch.randn(64, 1, 7, 7, 7, device="cuda")
    dvol = torch.full((1, 2, 16, 32), float("nan"), device="cuda")
    ws = torch.empty(int(L.smk_conv3d_train_workspace()), device="cuda", dtype=torch.uint8)
    st = _lib.stream_ptr(dz1.device)
    call = lambda B, D, H, W, off=0: L.smk_conv3d_s7_dgrad(dz1.data_ptr() + off, w.data_ptr(), B, D, H, W, dvol.data_ptr(), ws.data_ptr(), st)
    assert call(1, 2, 12, 32) == UNSUPPORTED                     # H = 12
    assert b"multiple of 8" in L.smk_last_error()
    assert call(1, 2, 16, 24) == UNSUPPORTED                     # W = 24
    assert call(0, 2, 16, 32) == UNSUPPORTED and call(1, 0, 16, 32) == UNSUPPORTED
    assert call(1, 2, 16, 32, off=4) != 0                        # alignment
    torch.cuda.synchronize()
    assert torch.isnan(dvol).all()
