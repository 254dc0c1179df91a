"""Host side of libsmokehip's training-mode reconstruction head (csrc/decoder_train.hip): SmokePhysNet.reconstruction_head
(smokephys_net.py:57-66,117-118) under autograd.  The two ConvTranspose2d(k4, s2, p1) layers and the Conv2d(16, 1, 3) + Sigmoid run
forward, data gradient and weight / bias gradients on plain fp32 kernels; the BatchNorms between them run on the training-mode
BatchNorm + ReLU kernels (models/norm.py, pool 1).  Every reduction is a fixed-order sum of per-workgroup partials: a training step
through this head is bit-reproducible without restricting MIOpen (there is no MIOpen call left in it)."""
import torch
from torch import nn

from .. import _lib
from .norm import hip_bn_relu_pool, hip_frozen_bn_relu_pool, hip_sync_bn_relu_pool
from .sync_bn import SyncBatchNorm2d

_TOKENS = 1024               # forward_tokens always reshapes to a 32 x 32 token grid
_SIDE = 32


def _convt_ok(m, cin_mult: int, cout: int) -> bool:
    return (type(m) is nn.ConvTranspose2d and m.out_channels == cout and m.in_channels % cin_mult == 0 and m.kernel_size == (4, 4)
            and m.stride == (2, 2) and m.padding == (1, 1) and m.output_padding == (0, 0) and m.dilation == (1, 1) and m.groups == 1
            and m.padding_mode == "zeros" and m.bias is not None)


def _head_ok(head: nn.Sequential, tokens, bn_ok) -> bool:
    try:
        if len(head) != 8:
            return False
        c1, b1, r1, c2, b2, r2, c3, sg = head
    except (TypeError, ValueError):
        return False
    ok = (_convt_ok(c1, 16, 32) and _convt_ok(c2, 32, 16) and c2.in_channels == 32 and type(c3) is nn.Conv2d
          and (c3.in_channels, c3.out_channels) == (16, 1) and c3.kernel_size == (3, 3) and c3.stride == (1, 1) and c3.padding == (1, 1)
          and c3.dilation == (1, 1) and c3.groups == 1 and c3.padding_mode == "zeros" and c3.bias is not None
          and type(r1) is nn.ReLU and type(r2) is nn.ReLU and type(sg) is nn.Sigmoid
          and bn_ok(b1) and bn_ok(b2) and b1.num_features == 32 and b2.num_features == 16)
    if not ok or not all(p.dtype == torch.float32 for p in head.parameters()):
        return False
    return (bool(tokens.is_cuda) and tokens.dtype == torch.float32 and tokens.dim() == 3 and tokens.shape[1] == _TOKENS
            and tokens.shape[2] == c1.in_channels and 1 <= tokens.shape[0] <= 65535)


def hip_head_train_supported(head: nn.Sequential, tokens) -> bool:
    """Whether hip_head_train serves this call: the default head structure (ConvT(C0, 32) + BN + ReLU, ConvT(32, 16) + BN + ReLU,
    Conv2d(16, 1, 3, padding 1) + Sigmoid) for any C0 that is a multiple of 16, both BatchNorms in the form the libsmokehip
    BatchNorm kernels implement (smokephys_net._hip_bn_ok: training mode, affine, running statistics, fixed momentum), float32
    parameters, and float32 ROCm tokens [B, 1024, C0] with 1 <= B <= 65535.  Anything else -- the float64 copies tests make, CPU
    tensors, a frozen BatchNorm, another head -- runs the PyTorch modules."""
    from .smokephys_net import _hip_bn_ok
    return _head_ok(head, tokens, _hip_bn_ok)


def frozen_bn_ok(bn) -> bool:
    """An eval-mode plain affine nn.BatchNorm2d with running statistics: what hip_frozen_bn_relu_pool computes."""
    return (type(bn) is nn.BatchNorm2d and not bn.training and bn.affine and bn.track_running_stats and bn.running_mean is not None
            and bn.running_var is not None)


def hip_head_frozen_supported(head: nn.Sequential, tokens) -> bool:
    """Whether hip_head_frozen serves this call: the same head structure and tokens as hip_head_train_supported, both BatchNorms in eval
    mode (frozen_bn_ok) and no head parameter asking for a gradient -- the gradient goes to the tokens only."""
    return _head_ok(head, tokens, frozen_bn_ok) and not any(p.requires_grad for p in head.parameters())


class _HipConvT4s2Fn(torch.autograd.Function):
    """ConvTranspose2d(CIN, COUT, 4, 2, 1) + bias.  tok: x is token-major [B, H*W, CIN] (and so is its gradient), else [B, CIN, H, W]."""

    @staticmethod
    def forward(ctx, x, weight, bias, tok, H, W):
        dev = _lib.require_cuda(x.device, "hip_convt4s2_train")
        L = _lib.load()
        x = x.contiguous()
        B, CIN, COUT = x.shape[0], weight.shape[0], weight.shape[1]
        z = torch.empty(B, COUT, 2 * H, 2 * W, device=dev, dtype=torch.float32)
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        _lib.check(L.smk_convt4s2_train_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), B, CIN, COUT, H, W, int(tok), z.data_ptr(),
                                                _lib.stream_ptr(dev)))
        ctx.save_for_backward(x, w)
        ctx.tok, ctx.H, ctx.W = tok, H, W
        return z

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        L = _lib.load()
        dev = x.device
        dz = dz.contiguous()
        B, CIN, COUT = x.shape[0], w.shape[0], w.shape[1]
        H, W, tok = ctx.H, ctx.W, int(ctx.tok)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.check(L.smk_convt4s2_train_dgrad(dz.data_ptr(), w.data_ptr(), B, CIN, COUT, H, W, tok, dx.data_ptr(), _lib.stream_ptr(dev)))
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw = torch.empty_like(w)
            db = torch.empty(COUT, device=dev, dtype=torch.float32)
            ws = torch.empty(int(L.smk_convt4s2_train_wgrad_workspace(B, CIN, COUT, H, W)), device=dev, dtype=torch.uint8)
            _lib.check(L.smk_convt4s2_train_wgrad(dz.data_ptr(), x.data_ptr(), B, CIN, COUT, H, W, tok, dw.data_ptr(), db.data_ptr(),
                                                  ws.data_ptr(), _lib.stream_ptr(dev)))
        return dx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None, None, None


class _HipConv3SigmoidFn(torch.autograd.Function):
    """sigmoid(Conv2d(16, 1, 3, padding 1)(x)); the backward needs only x, the weight and the output."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        dev = _lib.require_cuda(x.device, "hip_conv3_sigmoid_train")
        L = _lib.load()
        x = x.contiguous()
        B, _, H, W = x.shape
        y = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        _lib.check(L.smk_conv3_sigmoid_train_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), B, H, W, y.data_ptr(), _lib.stream_ptr(dev)))
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        L = _lib.load()
        dev = x.device
        dy = dy.contiguous()
        B, _, H, W = x.shape
        dx = torch.empty_like(x)
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dw = torch.empty_like(w) if want_w else None
        db = torch.empty(1, device=dev, dtype=torch.float32) if want_w else None
        ws = torch.empty(int(L.smk_conv3_sigmoid_train_workspace(B, H, W)), device=dev, dtype=torch.uint8)
        _lib.check(L.smk_conv3_sigmoid_train_backward(dy.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(), B, H, W, dx.data_ptr(),
                                                      None if dw is None else dw.data_ptr(), None if db is None else db.data_ptr(),
                                                      ws.data_ptr(), _lib.stream_ptr(dev)))
        return (dx if ctx.needs_input_grad[0] else None, dw if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None)


def hip_convt4s2_train(x: torch.Tensor, conv: nn.ConvTranspose2d, tokens: bool = False) -> torch.Tensor:
    """conv(x) under autograd on libsmokehip.  tokens=True: x is [B, S*S, CIN] token-major (read as the [B, CIN, S, S] image
    `x.transpose(1, 2).reshape(B, CIN, S, S)`, without materialising it); else x is [B, CIN, H, W].  Returns [B, COUT, 2H, 2W]."""
    if tokens:
        S = int(round(x.shape[1] ** 0.5))
        H = W = S
    else:
        H, W = x.shape[-2:]
    return _HipConvT4s2Fn.apply(x, conv.weight, conv.bias, bool(tokens), int(H), int(W))


def hip_conv3_sigmoid_train(x: torch.Tensor, conv: nn.Conv2d) -> torch.Tensor:
    """sigmoid(conv(x)) for the head's last Conv2d(16, 1, 3, padding 1) under autograd on libsmokehip."""
    return _HipConv3SigmoidFn.apply(x, conv.weight, conv.bias)


def _bn_relu(z, bn):
    return hip_sync_bn_relu_pool(z, bn, 1) if isinstance(bn, SyncBatchNorm2d) else hip_bn_relu_pool(z, bn, 1)


def hip_head_train(head: nn.Sequential, tokens: torch.Tensor) -> torch.Tensor:
    """reconstruction_head(tokens.transpose(1, 2).reshape(B, C0, 32, 32)) in training mode on libsmokehip: ConvT (tokens in) ->
    BatchNorm + ReLU -> ConvT -> BatchNorm + ReLU -> Conv2d + Sigmoid.  Running statistics and num_batches_tracked update exactly as
    the modules' do.  Call only where hip_head_train_supported(head, tokens) holds."""
    c1, b1, _, c2, b2, _, c3, _ = head
    a1 = _bn_relu(hip_convt4s2_train(tokens, c1, tokens=True), b1)
    a2 = _bn_relu(hip_convt4s2_train(a1, c2), b2)
    return hip_conv3_sigmoid_train(a2, c3)


class _Detached:
    """A convolution module seen with its weight and bias as constants (the nodes read .weight / .bias only)."""

    def __init__(self, conv):
        self.weight, self.bias = conv.weight.detach(), conv.bias.detach()


def hip_head_frozen(head: nn.Sequential, tokens: torch.Tensor) -> torch.Tensor:
    """reconstruction_head(tokens.transpose(1, 2).reshape(B, C0, 32, 32)) in eval mode under autograd on libsmokehip, differentiable with
    respect to the tokens only: the three convolution nodes of hip_head_train with detached weights, the BatchNorms from their running
    statistics (hip_frozen_bn_relu_pool).  Nothing of the head is updated.  Call only where hip_head_frozen_supported(head, tokens) holds."""
    c1, b1, _, c2, b2, _, c3, _ = head
    a1 = hip_frozen_bn_relu_pool(hip_convt4s2_train(tokens, _Detached(c1), tokens=True), b1, 1)
    a2 = hip_frozen_bn_relu_pool(hip_convt4s2_train(a1, _Detached(c2)), b2, 1)
    return hip_conv3_sigmoid_train(a2, _Detached(c3))
