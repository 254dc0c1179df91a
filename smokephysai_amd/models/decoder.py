"""Host side of libsmokehip's reconstruction head (smk_decoder_*): SmokePhysNet.reconstruction_head in eval mode as three
direct fp32 kernels with the BatchNorms folded in (smokephys_net.py:57-66,117-118)."""
import ctypes as C

import torch
from torch import nn

from .. import _lib
from .decoder_train import _convt_ok, frozen_bn_ok

_KEYS = ("ct1_w", "ct1_b", "bn1_w", "bn1_b", "bn1_mean", "bn1_var", "ct2_w", "ct2_b", "bn2_w", "bn2_b", "bn2_mean", "bn2_var",
         "conv_w", "conv_b")


def decoder_weight_dict(head: nn.Sequential) -> dict:
    """The 14 eval-mode tensors of reconstruction_head (indices 0,1,3,4,6 of the Sequential)."""
    c1, b1, c2, b2, c3 = head[0], head[1], head[3], head[4], head[6]
    return dict(ct1_w=c1.weight, ct1_b=c1.bias, bn1_w=b1.weight, bn1_b=b1.bias, bn1_mean=b1.running_mean, bn1_var=b1.running_var,
                ct2_w=c2.weight, ct2_b=c2.bias, bn2_w=b2.weight, bn2_b=b2.bias, bn2_mean=b2.running_mean, bn2_var=b2.running_var,
                conv_w=c3.weight, conv_b=c3.bias)


def hip_decoder_supported(head: nn.Sequential, S: int) -> bool:
    """Whether smk_decoder_forward computes this head on an S x S token grid.  Pure: no device, no library.  Everything the kernels
    hard-code is checked, as strictly as the training-side predicate (decoder_train._head_ok with frozen_bn_ok):
      - exactly 8 modules: ConvTranspose2d, BatchNorm2d, ReLU, ConvTranspose2d, BatchNorm2d, ReLU, Conv2d, Sigmoid (exact types);
      - both transposed convolutions kernel 4, stride 2, padding 1, output_padding 0, dilation 1, groups 1, zero padding, with bias,
        64 -> 32 and 32 -> 16 channels;
      - the last convolution 16 -> 1, kernel 3, stride 1, padding 1, dilation 1, groups 1, zero padding, with bias;
      - both BatchNorms plain nn.BatchNorm2d in eval mode, affine, with running statistics (frozen_bn_ok), 32 and 16 features, and
        eps == 1e-5 (k_fold_decoder folds with that constant);
      - every parameter and buffer of the head float32;
      - S >= 16 and S % 16 == 0 (the tiled kernels' 16 x 16 tiles).
    Any other head runs the PyTorch modules (forward_tokens)."""
    try:
        if len(head) != 8:
            return False
        c1, b1, r1, c2, b2, r2, c3, sg = head
    except (TypeError, ValueError):
        return False
    ok = (_convt_ok(c1, 64, 32) and c1.in_channels == 64 and _convt_ok(c2, 32, 16) and c2.in_channels == 32 and type(c3) is nn.Conv2d
          and (c3.in_channels, c3.out_channels) == (16, 1) and c3.kernel_size == (3, 3) and c3.stride == (1, 1) and c3.padding == (1, 1)
          and c3.dilation == (1, 1) and c3.groups == 1 and c3.padding_mode == "zeros" and c3.bias is not None
          and type(r1) is nn.ReLU and type(r2) is nn.ReLU and type(sg) is nn.Sigmoid
          and frozen_bn_ok(b1) and frozen_bn_ok(b2) and b1.num_features == 32 and b2.num_features == 16
          and b1.eps == 1e-5 and b2.eps == 1e-5)
    if not ok or not all(t.dtype == torch.float32 for t in decoder_weight_dict(head).values()):
        return False
    return S >= 16 and S % 16 == 0


class HipDecoder:
    def __init__(self, weights: dict, device="cuda"):
        self._dev = _lib.require_cuda(device, "HipDecoder")
        self._L = _lib.load()
        ws = {k: torch.as_tensor(weights[k]).detach().to(self._dev, torch.float32).contiguous() for k in _KEYS}
        packed = _lib.SmkDecoderWeights(*[ws[k].data_ptr() for k in _KEYS])
        handle = C.c_void_p()
        _lib.check(self._L.smk_decoder_create(C.byref(packed), self._dev.index, _lib.stream_ptr(self._dev), C.byref(handle)))
        torch.cuda.current_stream(self._dev).synchronize()      # the fold kernel has read `ws`
        self._handle = handle
        self._tmp = {}

    def close(self):
        if getattr(self, "_handle", None):
            self._L.smk_decoder_destroy(self._handle)
            self._handle = None

    __del__ = close

    def __call__(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens [B, S*S, 64] float32 (output_decoder's result) -> reconstructed [B, 1, 4S, 4S]."""
        if tokens.device != self._dev or tokens.dtype != torch.float32 or tokens.dim() != 3 or tokens.shape[2] != 64:
            raise ValueError(f"HipDecoder: tokens must be float32 [B, S*S, 64] on {self._dev}")
        B, L, _ = tokens.shape
        S = int(round(L ** 0.5))
        if S * S != L:
            raise ValueError("HipDecoder: the token count must be a square")
        tokens = tokens.contiguous()
        tmp = self._tmp.get(B * 4096 + S)
        if tmp is None:                                          # scratch, reused across calls (stream-ordered)
            tmp = self._tmp[B * 4096 + S] = (torch.empty(B, 32, 2 * S, 2 * S, device=self._dev),
                                             torch.empty(B, 16, 4 * S, 4 * S, device=self._dev))
        out = torch.empty(B, 1, 4 * S, 4 * S, device=self._dev)
        _lib.check(self._L.smk_decoder_forward(self._handle, tokens.data_ptr(), B, S, tmp[0].data_ptr(), tmp[1].data_ptr(),
                                               out.data_ptr(), _lib.stream_ptr(self._dev)))
        return out
