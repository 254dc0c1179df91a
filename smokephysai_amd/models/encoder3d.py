"""3-D input encoder on MI355X (BASELINE configs[4]: "MFMA conv3d encoder").

The reference's encoder is 2-D (src/models/smokephys_net.py:24-32,87-91); SPEC_3D.md section 8 generalises it axis by axis:
Conv3d(1, 64, 7, padding 3) + BatchNorm3d + ReLU -> Conv3d(64, 128, 3, padding 1) + BatchNorm3d + ReLU -> the two adaptive average
pools with the depth axis pooled to 1 -> features [B, 128, 32, 32], i.e. exactly the tensor SmokePhysNet tokenises (smokephys_net.py:95),
so the rest of the network applies unchanged.  Eval mode (running statistics folded into the weights, as HipEncoder does in 2-D).

Execution (csrc/conv3d_march.hip): both convolutions on split-bf16 MFMAs (fp32-class accuracy), activations channels-last [D, H, W, C].
conv1 (`smk_conv3d_s7_march_forward`): a workgroup marches an 8 x 16 column of voxels along z, weights in registers, each input plane expanded
once into a table of ready MFMA fragments in LDS.  conv2 (`smk_conv3d_cl_zsum_forward`): the same march with three input planes in LDS, all
27 taps read from there, `relu(conv + bias)` summed over z in registers -- the depth half of the pooling -- so the activated conv2 output is
never written; `smk_pool3d_accumulate` reduces the depth sums to the 32 x 32 token sums.
`conv2_mode="implicit"` keeps the first form built (both convolutions as implicit GEMMs on the layer kernel: `smk_conv3d_cl_forward`,
`smk_conv3d_s7_forward`), `"im2col"` the explicit one (`smk_conv3d_im2col` -> [voxels, taps x channels] -> `smk_linear_forward`), for A/B runs.

Training (SPEC_3D.md section 11; csrc/conv3d_train.hip): `Encoder3D` is the nn.Module form of the same chain with train-mode BatchNorm3d.
Its autograd functions keep the activations channels-last [B, D, H, W, C] from the volume to the tokens: `hip_conv3d_s7_train` (conv1;
weight gradient through the explicit patch matrix), `hip_conv3d_cl_train` (conv2: forward, data gradient and implicit weight gradient
kernels) and `hip_bn3d_cl` (batch statistics + ReLU, for the second block fused with the token pooling).

Input gradients: a volume that requires a gradient gets it from `hip_conv3d_s7_dgrad` (smk_conv3d_s7_dgrad).  In eval mode under autograd with
every parameter frozen (PGD, saliency) `Encoder3D` takes its 'frozen' route: the same two convolutions with `hip_bn3d_cl_frozen` (BatchNorm3d
from the running statistics, gradient to its input only); `hip_volume_input_grad_supported` is the route's pure predicate.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib
from .linear import HipLinear

_KEYS = ("conv1_w", "conv1_b", "bn1_w", "bn1_b", "bn1_mean", "bn1_var",
         "conv2_w", "conv2_b", "bn2_w", "bn2_b", "bn2_mean", "bn2_var")


class HipEncoder3D:
    def __init__(self, weights: dict, device="cuda", eps: float = 1e-5, slab_bytes: int = 2 << 30, conv2_mode: str = "march",
                 a2_bytes: int = 128 << 20):
        self._dev = _lib.require_cuda(device, "HipEncoder3D")
        self._L = _lib.load()
        w = {k: torch.as_tensor(weights[k]).detach().to(self._dev, torch.float64) for k in _KEYS}
        if tuple(w["conv1_w"].shape) != (64, 1, 7, 7, 7) or tuple(w["conv2_w"].shape) != (128, 64, 3, 3, 3):
            raise ValueError("HipEncoder3D: weights must be Conv3d(1,64,7) / Conv3d(64,128,3) (SPEC_3D.md section 8)")
        s1 = w["bn1_w"] / torch.sqrt(w["bn1_var"] + eps)
        s2 = w["bn2_w"] / torch.sqrt(w["bn2_var"] + eps)
        # column order of smk_conv3d_im2col: tap * C + c, tap = (kz * k + ky) * k + kx
        w1 = torch.zeros(64, 384, dtype=torch.float64, device=self._dev)
        w1[:, :343] = w["conv1_w"].reshape(64, 343) * s1[:, None]
        w2 = (w["conv2_w"].permute(0, 2, 3, 4, 1).reshape(128, 27 * 64) * s2[:, None]).contiguous()
        b1 = (w["conv1_b"] - w["bn1_mean"]) * s1 + w["bn1_b"]
        b2 = (w["conv2_b"] - w["bn2_mean"]) * s2 + w["bn2_b"]
        self._lin1 = HipLinear(w1.float(), b1.float(), device=self._dev)
        # implicit-GEMM layout of conv1: 56 window rows (kz * 7 + ky; 49 used) x 8 kx slots (7 used)
        w1i = torch.zeros(64, 56, 8, dtype=torch.float64, device=self._dev)
        w1i[:, :49, :7] = (w["conv1_w"].reshape(64, 49, 7) * s1[:, None, None])
        self._lin1i = HipLinear(w1i.reshape(64, 448).float(), b1.float(), device=self._dev)
        # marched form of conv1 (smk_conv3d_s7_march_forward): 7 kz x 8 ky slots x 8 kx slots
        w1m = torch.zeros(64, 7, 8, 8, dtype=torch.float64, device=self._dev)
        w1m[:, :, :7, :7] = w["conv1_w"].reshape(64, 7, 7, 7) * s1[:, None, None, None]
        self._lin1m = HipLinear(w1m.reshape(64, 448).float(), b1.float(), device=self._dev)
        self._lin2 = HipLinear(w2.float(), b2.float(), device=self._dev)
        self.slab_bytes = int(slab_bytes)
        self._bufs = {}
        # the activated conv2 slab is written by the GEMM and read back by the pooling launch right behind it: kept within the 256 MB
        # Infinity Cache it is read from there (512 x 512 planes: one plane per launch; measured 34.4 -> 29.8 ms per 64-plane volume)
        self.a2_bytes = int(a2_bytes)
        if conv2_mode not in ("march", "implicit", "im2col"):
            raise ValueError("conv2_mode: 'march' (smk_conv3d_cl_zsum_forward: conv2 marched along z with its input planes in LDS, depth pooling "
                             "fused), 'implicit' (smk_conv3d_cl_forward: implicit GEMM, no patch matrix) or 'im2col' (explicit GEMM)")
        self.conv2_mode = conv2_mode
        self.conv1_mode = conv2_mode

    def _buffer(self, name, shape):
        """Activation buffers are kept between calls (a 512 x 512 x 64 volume's conv1 output is 4.3 GB: a fresh allocation per call costs
        more than the convolution)."""
        buf = self._bufs.get(name)
        if buf is None or tuple(buf.shape) != tuple(shape):
            self._bufs.pop(name, None)
            buf = self._bufs[name] = torch.empty(*shape, device=self._dev)
        return buf

    def _im2col(self, src, C, D, H, W, k, z0, nz, kpad):
        cols = torch.empty(nz * H * W, kpad, device=self._dev)
        _lib.check(self._L.smk_conv3d_im2col(src.data_ptr(), C, D, H, W, k, z0, nz, cols.data_ptr(), kpad, _lib.stream_ptr(self._dev)))
        return cols

    def conv1_activations(self, vol: torch.Tensor) -> torch.Tensor:
        """One volume [D, H, W] -> relu(bn1(conv1)) channels-last [D, H, W, 64]."""
        D, H, W = vol.shape
        a1 = self._buffer("a1", (D, H, W, 64))
        if self.conv1_mode == "march" and H % 8 == 0 and W % 16 == 0 and H * W * 256 < (1 << 31):
            _lib.check(self._L.smk_conv3d_s7_march_forward(self._lin1m._handle, vol.data_ptr(), D, H, W, a1.data_ptr(), _lib.SMK_ACT_RELU,
                                                           _lib.stream_ptr(self._dev)))
            return a1
        if self.conv1_mode != "im2col" and H <= 1023 and W <= 1023:
            nz = max(1, min(D, ((1 << 32) - 512) // (H * W * 4) - 6, 1000, ((1 << 31) - 512) // (H * W)))
            for z0 in range(0, D, nz):
                n = min(nz, D - z0)
                _lib.check(self._L.smk_conv3d_s7_forward(self._lin1i._handle, vol.data_ptr(), D, H, W, z0, n, a1[z0:z0 + n].data_ptr(), 64,
                                                         _lib.SMK_ACT_RELU, _lib.stream_ptr(self._dev)))
            return a1
        nz = max(1, min(D, self.slab_bytes // (H * W * 384 * 4)))
        for z0 in range(0, D, nz):
            n = min(nz, D - z0)
            cols = self._im2col(vol, 1, D, H, W, 7, z0, n, 384)
            self._lin1(cols, activation="relu", out=a1[z0:z0 + n].view(n * H * W, 64))
        return a1

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, 1, D, H, W] or [B, D, H, W] float32 -> features [B, 128, 32, 32] (H, W multiples of 32)."""
        if x.dim() == 5:
            if x.shape[1] != 1:
                raise ValueError("the 3-D encoder takes one channel")
            x = x[:, 0]
        if x.dim() != 4:
            raise ValueError("x must be [B, 1, D, H, W] or [B, D, H, W]")
        x = x.to(self._dev, torch.float32).contiguous()
        B, D, H, W = x.shape
        for n in (H, W):
            if n % 32 or not (n % 128 == 0 or 128 % n == 0):
                raise ValueError("HipEncoder3D: H and W must be 32, 64 or a multiple of 128 (the two adaptive pools then compose to a "
                                 "uniform block mean)")
        out = torch.empty(B, 128, 32, 32, device=self._dev)
        march = self.conv2_mode == "march" and H * W * 256 < (1 << 31)           # (H % 8, W % 16 hold: multiples of 32)
        implicit = self.conv2_mode == "implicit" or (self.conv2_mode == "march" and not march)
        # implicit GEMM: no patch matrix; a slab is bounded by the activated output it materialises and by 32-bit offsets into a1
        if implicit:
            nz = max(1, min(D, min(self.slab_bytes, self.a2_bytes) // (H * W * 128 * 4), ((1 << 32) - 512) // (H * W * 256) - 2))
        else:
            nz = max(1, min(D, self.slab_bytes // (H * W * 1728 * 4)))
        for b in range(B):
            a1 = self.conv1_activations(x[b])
            sums = torch.zeros(1024, 128, device=self._dev)
            if march:
                zsum = self._buffer("zsum", (H * W, 128))
                _lib.check(self._L.smk_conv3d_cl_zsum_forward(self._lin2._handle, a1.data_ptr(), D, H, W, zsum.data_ptr(), _lib.SMK_ACT_RELU,
                                                              _lib.stream_ptr(self._dev)))
                _lib.check(self._L.smk_pool3d_accumulate(zsum.data_ptr(), 128, H, W, 1, sums.data_ptr(), _lib.stream_ptr(self._dev)))
            for z0 in range(0, D, nz) if not march else ():
                n = min(nz, D - z0)
                if implicit:
                    a2 = self._buffer("a2", (nz * H * W, 128))[:n * H * W]
                    _lib.check(self._L.smk_conv3d_cl_forward(self._lin2._handle, a1.data_ptr(), D, H, W, z0, n, a2.data_ptr(), 128,
                                                             _lib.SMK_ACT_RELU, _lib.stream_ptr(self._dev)))
                else:
                    cols = self._im2col(a1, 64, D, H, W, 3, z0, n, 1728)
                    a2 = self._lin2(cols, activation="relu")                              # [n H W, 128] channels-last
                    del cols
                _lib.check(self._L.smk_pool3d_accumulate(a2.data_ptr(), 128, H, W, n, sums.data_ptr(), _lib.stream_ptr(self._dev)))
                del a2
            out[b] = (sums / float(D * (H // 32) * (W // 32))).t().reshape(128, 32, 32)
        return out

    def tokens(self, x: torch.Tensor) -> torch.Tensor:
        """Same features token-major [B, 1024, 128] (= features.flatten(2).transpose(1, 2), smokephys_net.py:95)."""
        return self(x).flatten(2).transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# Training: autograd functions over csrc/conv3d_train.hip, channels-last activations
def pool_shape_ok(H: int, W: int) -> bool:
    """The pool rule of SPEC_3D.md section 8: H, W in {32, 64} or multiples of 128 (the two adaptive pools are then one uniform block mean)."""
    return all(n >= 32 and n % 32 == 0 and (n % 128 == 0 or 128 % n == 0) for n in (int(H), int(W)))


def hip_conv3d_train_supported(B: int, D: int, H: int, W: int) -> bool:
    """The shape rule of the training convolution kernels (conv3d_train_shape_ok in csrc/conv3d_train.h)."""
    return B >= 1 and D >= 1 and H >= 8 and W >= 16 and H % 8 == 0 and W % 16 == 0 and B * D * (H // 8) * (W // 16) < (1 << 31)


def _ws(nbytes, dev):
    return torch.empty(int(nbytes), device=dev, dtype=torch.uint8)             # torch's caching allocator: stream-ordered reuse


CONV1_WGRAD_SLAB_ROWS = 1 << 17      # voxels per patch-matrix slab of conv1's weight gradient (384 floats each: 192 MB)


def hip_conv3d_s7_wgrad(vol: torch.Tensor, dz1: torch.Tensor):
    """dW1 [64, 1, 7, 7, 7] and db1 [64] of conv1 from the volumes [B, D, H, W] and dz1 [B, D, H, W, 64]: the explicit route -- smk_conv3d_im2col
    (C = 1, k = 7, 384 columns) in slabs of whole planes, then smk_linear_wgrad, the slabs added in order (deterministic)."""
    from .linear import hip_linear_wgrad
    L = _lib.load()
    dev = vol.device
    B, D, H, W = vol.shape
    nz = max(1, min(D, CONV1_WGRAD_SLAB_ROWS // (H * W)))
    dw = db = None
    for b in range(B):
        for z0 in range(0, D, nz):
            n = min(nz, D - z0)
            cols = torch.empty(n * H * W, 384, device=dev, dtype=torch.float32)
            _lib.check(L.smk_conv3d_im2col(vol[b].data_ptr(), 1, D, H, W, 7, z0, n, cols.data_ptr(), 384, _lib.stream_ptr(dev)))
            w, g = hip_linear_wgrad(dz1[b, z0:z0 + n].reshape(n * H * W, 64), cols, want_db=True)
            dw, db = (w, g) if dw is None else (dw.add_(w), db.add_(g))
    return dw[:, :343].reshape(64, 1, 7, 7, 7).contiguous(), db


def hip_conv3d_s7_dgrad(dz1: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """dvol [B, D, H, W] = the data gradient of conv1 from dz1 [B, D, H, W, 64] and the weight [64, 1, 7, 7, 7] (smk_conv3d_s7_dgrad:
    F.conv_transpose3d with padding 3, on the fp32 MFMA; deterministic, no atomics)."""
    L = _lib.load()
    dev = _lib.require_cuda(dz1.device, "hip_conv3d_s7_dgrad")
    if dz1.dim() != 5 or dz1.shape[-1] != 64 or tuple(weight.shape) != (64, 1, 7, 7, 7) or dz1.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError("hip_conv3d_s7_dgrad: float32 dz1 [B, D, H, W, 64] and weight [64, 1, 7, 7, 7]")
    B, D, H, W, _ = dz1.shape
    dz1, weight = dz1.contiguous(), weight.detach().contiguous()
    dvol = torch.empty(B, D, H, W, device=dev, dtype=torch.float32)
    ws = _ws(L.smk_conv3d_train_workspace(), dev)
    _lib.check(L.smk_conv3d_s7_dgrad(dz1.data_ptr(), weight.data_ptr(), B, D, H, W, dvol.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)))
    return dvol


class _HipConv3dS7TrainFn(torch.autograd.Function):
    """z1 [B, D, H, W, 64] = conv1(volumes [B, D, H, W]) + bias on smk_conv3d_s7_train_forward; the volumes' gradient on smk_conv3d_s7_dgrad.
    Only the gradients a call wants are computed (a PGD step does no weight-gradient work)."""

    @staticmethod
    def forward(ctx, vol, weight, bias):
        dev = _lib.require_cuda(vol.device, "hip_conv3d_s7_train")
        L = _lib.load()
        vol = vol.contiguous()
        B, D, H, W = vol.shape
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        z1 = torch.empty(B, D, H, W, 64, device=dev, dtype=torch.float32)
        ws = _ws(L.smk_conv3d_train_workspace(), dev)
        _lib.check(L.smk_conv3d_s7_train_forward(vol.data_ptr(), w.data_ptr(), b.data_ptr(), B, D, H, W, z1.data_ptr(), ws.data_ptr(),
                                                 _lib.stream_ptr(dev)))
        ctx.save_for_backward(vol, w)
        return z1

    @staticmethod
    def backward(ctx, dz1):
        vol, w = ctx.saved_tensors
        dz1 = dz1.contiguous()
        dvol = hip_conv3d_s7_dgrad(dz1, w) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = hip_conv3d_s7_wgrad(vol, dz1)
        return dvol, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None


def hip_conv3d_cl_forward_raw(a1, weight, bias):
    L = _lib.load()
    dev = a1.device
    B, D, H, W, _ = a1.shape
    z2 = torch.empty(B, D, H, W, 128, device=dev, dtype=torch.float32)
    ws = _ws(L.smk_conv3d_train_workspace(), dev)
    _lib.check(L.smk_conv3d_cl_train_forward(a1.data_ptr(), weight.data_ptr(), None if bias is None else bias.data_ptr(), B, D, H, W,
                                             z2.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)))
    return z2


def hip_conv3d_cl_dgrad(dz2, weight):
    L = _lib.load()
    dev = dz2.device
    B, D, H, W, _ = dz2.shape
    da1 = torch.empty(B, D, H, W, 64, device=dev, dtype=torch.float32)
    ws = _ws(L.smk_conv3d_train_workspace(), dev)
    _lib.check(L.smk_conv3d_cl_dgrad(dz2.data_ptr(), weight.data_ptr(), B, D, H, W, da1.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)))
    return da1


def hip_conv3d_cl_wgrad(dz2, a1):
    L = _lib.load()
    dev = dz2.device
    B, D, H, W, _ = dz2.shape
    dw = torch.empty(128, 64, 3, 3, 3, device=dev, dtype=torch.float32)
    db = torch.empty(128, device=dev, dtype=torch.float32)
    nbytes = int(L.smk_conv3d_cl_wgrad_workspace(B, D, H, W))
    if nbytes < 0:
        raise ValueError("hip_conv3d_cl_wgrad: H must be a multiple of 8 and W of 16")
    ws = _ws(nbytes, dev)
    _lib.check(L.smk_conv3d_cl_wgrad(dz2.data_ptr(), a1.data_ptr(), B, D, H, W, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)))
    return dw, db


class _HipConv3dClTrainFn(torch.autograd.Function):
    """z2 [B, D, H, W, 128] = conv2(a1 [B, D, H, W, 64]) + bias: smk_conv3d_cl_train_forward / _dgrad / _wgrad."""

    @staticmethod
    def forward(ctx, a1, weight, bias):
        _lib.require_cuda(a1.device, "hip_conv3d_cl_train")
        a1 = a1.contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        ctx.save_for_backward(a1, w)
        return hip_conv3d_cl_forward_raw(a1, w, b)

    @staticmethod
    def backward(ctx, dz2):
        a1, w = ctx.saved_tensors
        dz2 = dz2.contiguous()
        da1 = hip_conv3d_cl_dgrad(dz2, w) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = hip_conv3d_cl_wgrad(dz2, a1)
        return da1, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None


def hip_conv3d_s7_train(vol: torch.Tensor, conv: nn.Conv3d) -> torch.Tensor:
    return _HipConv3dS7TrainFn.apply(vol, conv.weight, conv.bias)


def hip_conv3d_cl_train(a1: torch.Tensor, conv: nn.Conv3d) -> torch.Tensor:
    return _HipConv3dClTrainFn.apply(a1, conv.weight, conv.bias)


BN_STATS, BN_APPLY, BN_BWD_SUMS, BN_BWD_DZ = 0, 1, 2, 3


def _bn_cl_phase(L, phase, z, dout, pooled, gamma, beta, eps, stats, out, dz, dwb, count, ws, dev):
    """One phase of smk_bn_cl_phase.  z, out, dout and dz 16-byte aligned; ws (BN_STATS and BN_BWD_SUMS only): smk_bn_cl_workspace bytes,
    8-byte aligned -- it holds fp64 partial sums, and the entry point refuses a weaker alignment (a torch allocation always has it)."""
    B, D, H, W, C = z.shape
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(L.smk_bn_cl_phase(phase, z.data_ptr(), ptr(dout), B, D, H, W, C, int(pooled), gamma.data_ptr(), beta.data_ptr(), float(eps),
                                 stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), ptr(out), ptr(dz),
                                 None if dwb is None else dwb[0].data_ptr(), None if dwb is None else dwb[1].data_ptr(), float(count), ptr(ws),
                                 _lib.stream_ptr(dev)))


class _HipBn3dClFn(torch.autograd.Function):
    """relu(bn(z)) on batch statistics for z [B, D, H, W, C] (C 64 or 128).  pooled: the output is the token means [B, 1024, C] over
    D x H/32 x W/32 and the activation is never written.  Returns (out, stats = mean | biased var | rstd)."""

    @staticmethod
    def forward(ctx, z, weight, bias, eps, pooled):
        dev = _lib.require_cuda(z.device, "hip_bn3d_cl")
        L = _lib.load()
        z = z.contiguous()
        B, D, H, W, C = z.shape
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        stats = torch.empty(3, C, device=dev, dtype=torch.float32)
        nbytes = int(L.smk_bn_cl_workspace(B, D, H, W, C))
        if nbytes < 0:
            raise ValueError("hip_bn3d_cl: z must be [B, D, H, W, C] with C 64 or 128")
        ws = _ws(nbytes, dev)
        _bn_cl_phase(L, BN_STATS, z, None, pooled, w, b, eps, stats, None, None, None, 0.0, ws, dev)
        if pooled:
            out = torch.empty(B, 1024, C, device=dev, dtype=torch.float32)
            _bn_cl_phase(L, BN_APPLY, z, None, 1, w, b, eps, stats, out, None, None, 0.0, None, dev)
            out.mul_(1.0 / (D * (H // 32) * (W // 32)))
        else:
            out = torch.empty_like(z)
            _bn_cl_phase(L, BN_APPLY, z, None, 0, w, b, eps, stats, out, None, None, 0.0, None, dev)
        ctx.save_for_backward(z, w, b, stats)
        ctx.pooled, ctx.eps = pooled, eps
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats):
        z, w, b, stats = ctx.saved_tensors
        L = _lib.load()
        dev = z.device
        B, D, H, W, C = z.shape
        dout = dout.contiguous()
        dwb = torch.empty(2, C, device=dev, dtype=torch.float32)          # dgamma | dbeta
        ws = _ws(L.smk_bn_cl_workspace(B, D, H, W, C), dev)
        _bn_cl_phase(L, BN_BWD_SUMS, z, dout, ctx.pooled, w, b, ctx.eps, stats, None, None, dwb, 0.0, ws, dev)
        dz = torch.empty_like(z)
        _bn_cl_phase(L, BN_BWD_DZ, z, dout, ctx.pooled, w, b, ctx.eps, stats, None, dz, dwb, float(B * D * H * W), None, dev)
        return dz, dwb[0], dwb[1], None, None


def _bn3d_hip_ok(bn) -> bool:
    return type(bn) is nn.BatchNorm3d and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None


def hip_bn3d_cl(z: torch.Tensor, bn: nn.BatchNorm3d, pooled: bool = False) -> torch.Tensor:
    """relu(bn(z)) (pooled: its token means) with bn in training mode on channels-last z [B, D, H, W, C]; the running statistics are updated
    exactly like nn.BatchNorm3d's: momentum, unbiased variance, num_batches_tracked."""
    if not _bn3d_hip_ok(bn):
        raise ValueError("hip_bn3d_cl: a training-mode affine BatchNorm3d with running statistics and a fixed momentum")
    out, stats = _HipBn3dClFn.apply(z, bn.weight, bn.bias, bn.eps, bool(pooled))
    with torch.no_grad():
        n = z.numel() // z.shape[-1]
        m = bn.momentum
        bn.running_mean.mul_(1 - m).add_(stats[0], alpha=m)
        bn.running_var.mul_(1 - m).add_(stats[1], alpha=m * n / max(n - 1, 1))
        bn.num_batches_tracked += 1
    return out


class _HipBn3dClFrozenFn(torch.autograd.Function):
    """relu((z - mean) * rstd * gamma + beta) (pooled: its token means) with every per-channel tensor a constant: SMK_BN_APPLY forward,
    SMK_BN_BWD_DZ with zero dgamma / dbeta and count 1 backward -- exactly dz = gamma * rstd * dy * [y > 0]."""

    @staticmethod
    def forward(ctx, z, gamma, beta, stats, pooled):
        dev = _lib.require_cuda(z.device, "hip_bn3d_cl_frozen")
        L = _lib.load()
        z = z.contiguous()
        B, D, H, W, C = z.shape
        if pooled:
            out = torch.empty(B, 1024, C, device=dev, dtype=torch.float32)
            _bn_cl_phase(L, BN_APPLY, z, None, 1, gamma, beta, 0.0, stats, out, None, None, 0.0, None, dev)
            out.mul_(1.0 / (D * (H // 32) * (W // 32)))
        else:
            out = torch.empty_like(z)
            _bn_cl_phase(L, BN_APPLY, z, None, 0, gamma, beta, 0.0, stats, out, None, None, 0.0, None, dev)
        ctx.save_for_backward(z, gamma, beta, stats)
        ctx.pooled = pooled
        return out

    @staticmethod
    def backward(ctx, dout):
        z, gamma, beta, stats = ctx.saved_tensors
        L = _lib.load()
        dz = torch.empty_like(z)
        zero = torch.zeros(2, z.shape[-1], device=z.device, dtype=torch.float32)
        _bn_cl_phase(L, BN_BWD_DZ, z, dout.contiguous(), ctx.pooled, gamma, beta, 0.0, stats, None, dz, zero, 1.0, None, z.device)
        return dz, None, None, None, None


def _bn3d_frozen_ok(bn) -> bool:
    """An eval-mode plain affine nn.BatchNorm3d with running statistics: what hip_bn3d_cl_frozen computes."""
    return (type(bn) is nn.BatchNorm3d and not bn.training and bn.affine and bn.track_running_stats and bn.running_mean is not None
            and bn.running_var is not None)


def hip_bn3d_cl_frozen(z: torch.Tensor, bn: nn.BatchNorm3d, pooled: bool = False) -> torch.Tensor:
    """relu(bn(z)) (pooled: its token means [B, 1024, C]) from bn's RUNNING statistics on channels-last z [B, D, H, W, C], differentiable
    with respect to z only: gamma, beta and the statistics are constants, and nothing of bn is updated (SPEC_3D.md section 11)."""
    if not _bn3d_frozen_ok(bn):
        raise ValueError("hip_bn3d_cl_frozen: an eval-mode affine BatchNorm3d with running statistics")
    if z.dim() != 5 or z.shape[-1] not in (64, 128) or z.shape[-1] != bn.num_features or z.dtype != torch.float32:
        raise ValueError("hip_bn3d_cl_frozen: z must be float32 [B, D, H, W, C] with C = bn.num_features in (64, 128)")
    if pooled and not (z.shape[2] % 32 == 0 and z.shape[3] % 32 == 0):
        raise ValueError("hip_bn3d_cl_frozen: pooled needs H and W multiples of 32")
    with torch.no_grad():
        stats = torch.stack([bn.running_mean.float(), bn.running_var.float(), (bn.running_var.double() + bn.eps).rsqrt().float()]).contiguous()
        gamma, beta = bn.weight.detach().float().contiguous(), bn.bias.detach().float().contiguous()
    return _HipBn3dClFrozenFn.apply(z, gamma, beta, stats, bool(pooled))


def hip_volume_input_grad_supported(B: int, D: int, H: int, W: int, *, eval_mode: bool = True, on_device: bool = True,
                                    grad_enabled: bool = True, input_requires_grad: bool = True, params_require_grad: bool = False,
                                    frozen_bn: bool = True) -> bool:
    """Whether Encoder3D's 'frozen' route (eval mode, gradient with respect to the volumes only) serves a call.  Pure: no device, no library.
    The volumes are the ones the training kernels take (pool_shape_ok, hip_conv3d_train_supported) as float32 on a ROCm device (on_device);
    autograd is on, the volumes want a gradient and no parameter of the encoder does; both BatchNorms are eval-mode plain affine
    BatchNorm3d with running statistics (frozen_bn)."""
    shape = pool_shape_ok(H, W) and hip_conv3d_train_supported(int(B), int(D), int(H), int(W))
    return bool(shape and eval_mode and on_device and grad_enabled and input_requires_grad and not params_require_grad and frozen_bn)


class Encoder3D(nn.Module):
    """The trainable 3-D encoder (SPEC_3D.md section 11): Conv3d(1, 64, 7, padding 3) -> BatchNorm3d -> ReLU -> Conv3d(64, 128, 3, padding 1)
    -> BatchNorm3d -> ReLU -> block mean over D x H/32 x W/32 -> tokens [B, 1024, 128].  route: "hip" (libsmokehip wherever a call allows
    it) or "torch" (always the PyTorch modules: the reference of the tests and the A/B partner of tools/train3d_probe.py)."""

    def __init__(self, route: str = "hip"):
        super().__init__()
        if route not in ("hip", "torch"):
            raise ValueError(f"Encoder3D route: 'hip' (libsmokehip kernels) or 'torch' (PyTorch modules), not {route!r}")
        self.route = route
        self.net = nn.Sequential(nn.Conv3d(1, 64, 7, padding=3), nn.BatchNorm3d(64), nn.ReLU(inplace=True),
                                 nn.Conv3d(64, 128, 3, padding=1), nn.BatchNorm3d(128), nn.ReLU(inplace=True))
        self.__dict__["_hip_eval"] = None                      # (HipEncoder3D, weight fingerprint)

    def __getstate__(self):                                    # copy.deepcopy / pickling: the eval mirror is per instance, rebuilt on use
        d = self.__dict__.copy()
        d["_hip_eval"] = None
        return d

    def weight_dict(self) -> dict:
        """The 12 tensors under HipEncoder3D's key names (its constructor takes this dict)."""
        c1, b1, _, c2, b2, _ = self.net
        return dict(conv1_w=c1.weight, conv1_b=c1.bias, bn1_w=b1.weight, bn1_b=b1.bias, bn1_mean=b1.running_mean, bn1_var=b1.running_var,
                    conv2_w=c2.weight, conv2_b=c2.bias, bn2_w=b2.weight, bn2_b=b2.bias, bn2_mean=b2.running_mean, bn2_var=b2.running_var)

    def hip_eval_encoder(self) -> HipEncoder3D:
        """The folded eval encoder for the current weights (rebuilt when a weight or a running statistic changes)."""
        ws = self.weight_dict()
        fp = tuple((t.data_ptr(), t._version) for t in ws.values())
        cur = self.__dict__.get("_hip_eval")
        if cur is None or cur[1] != fp:
            cur = (HipEncoder3D(ws, device=ws["conv1_w"].device, eps=self.net[1].eps), fp)
            self.__dict__["_hip_eval"] = cur
        return cur[0]

    def _route(self, x: torch.Tensor, input_grad: str = "hip") -> str:
        """'train': training mode, fp32 volumes of a supported shape on a ROCm device -> the training kernels (batch statistics; a volume
        that requires a gradient gets it from smk_conv3d_s7_dgrad);
        'eval': eval mode under no_grad on the device -> the folded HipEncoder3D;
        'frozen': eval mode, autograd on, a gradient wanted with respect to the volumes ONLY (every encoder parameter frozen) and
        input_grad == "hip" -> the training convolutions with BatchNorm from the running statistics (hip_volume_input_grad_supported);
        'torch': everything else."""
        B, D, H, W = x.shape
        c1, b1, _, c2, b2, _ = self.net
        if self.route != "hip" or not x.is_cuda or x.dtype != torch.float32 or c1.weight.dtype != torch.float32 or not pool_shape_ok(H, W):
            return "torch"
        if self.training:
            ok = (_bn3d_hip_ok(b1) and _bn3d_hip_ok(b2) and b1.eps == b2.eps and hip_conv3d_train_supported(B, D, H, W)
                  and c1.bias is not None and c2.bias is not None)
            return "train" if ok else "torch"
        if not torch.is_grad_enabled():
            return "eval" if b1.eps == b2.eps else "torch"
        ok = (input_grad == "hip" and b1.eps == b2.eps and c1.bias is not None and c2.bias is not None
              and hip_volume_input_grad_supported(B, D, H, W, eval_mode=True, on_device=True, grad_enabled=True,
                                                  input_requires_grad=x.requires_grad,
                                                  params_require_grad=any(p.requires_grad for p in self.parameters()),
                                                  frozen_bn=_bn3d_frozen_ok(b1) and _bn3d_frozen_ok(b2)))
        return "frozen" if ok else "torch"

    def tokens(self, volumes: torch.Tensor, input_grad: str = "hip") -> torch.Tensor:
        """volumes [B, 1, D, H, W] or [B, D, H, W] -> tokens [B, 1024, 128].  input_grad: "torch" keeps an eval-mode call under autograd on
        the PyTorch modules (SmokePhysNet3D passes its own switch: the A/B partner of the 'frozen' route)."""
        x = volumes
        if x.dim() == 5:
            if x.shape[1] != 1:
                raise ValueError("the 3-D encoder takes one channel")
            x = x[:, 0]
        if x.dim() != 4:
            raise ValueError("volumes must be [B, 1, D, H, W] or [B, D, H, W]")
        route = self._route(x, input_grad)
        if route == "train":
            c1, b1, _, c2, b2, _ = self.net
            a1 = hip_bn3d_cl(hip_conv3d_s7_train(x, c1), b1)
            return hip_bn3d_cl(hip_conv3d_cl_train(a1, c2), b2, pooled=True)
        if route == "frozen":                                  # d / d volumes with everything else a constant: no MIOpen call, no find pass
            c1, b1, _, c2, b2, _ = self.net
            a1 = hip_bn3d_cl_frozen(hip_conv3d_s7_train(x, c1), b1)
            return hip_bn3d_cl_frozen(hip_conv3d_cl_train(a1, c2), b2, pooled=True)
        if route == "eval":
            return self.hip_eval_encoder().tokens(x)
        B, D, H, W = x.shape
        y = self.net(x[:, None])                               # [B, 128, D, H, W]
        if pool_shape_ok(H, W):                                # the two adaptive pools as the one block mean they compose to
            y = y.mean(dim=2)
            k = (H // 32, W // 32)
            y = y if k == (1, 1) else F.avg_pool2d(y, k)
        else:
            y = F.adaptive_avg_pool3d(F.adaptive_avg_pool3d(y, (1, 128, 128)), (1, 32, 32))[:, :, 0]
        return y.flatten(2).transpose(1, 2)

    def forward(self, volumes: torch.Tensor) -> torch.Tensor:
        return self.tokens(volumes)
