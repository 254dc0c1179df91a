"""Robustness metrics -- drop-in for src/evaluation/robustness_metrics.py (RobustnessEvaluator).

compute_ssim / compute_psnr / evaluate_reconstruction_quality run the SSIM map and the squared error of fp32 tensors on a
ROCm device as one HIP kernel (csrc/quality.hip: the five pooled moments, the map and both per-plane sums in one launch, plus a
tiny launch that sums each plane's tiles in a fixed order).  Inputs the kernel does not take -- tensors off the GPU or not fp32,
mismatched shapes, an even window or one above 31 -- run the reference's torch formula (`ssim_torch`), which gives its
results.  Both routes return Python floats, as the reference does.

`plane_ssim` is the same SSIM as a tensor under autograd (the training side: models/losses.py `ssim_loss`): on the kernel route its
backward is smk_image_quality_backward, the closed-form gradient of DESIGN.md 8.1.
"""
import math
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib

C1 = 0.01 ** 2           # robustness_metrics.py:96-97
C2 = 0.03 ** 2
MAX_WINDOW = 31          # csrc/quality.h QUALITY_MAX_WINDOW


def ssim_torch(pred: torch.Tensor, target: torch.Tensor, window_size: int = 11) -> torch.Tensor:
    """The reference's SSIM map (robustness_metrics.py:79-99), unchanged: avg_pool2d with count_include_pad, the moments by
    E[x^2] - mu^2."""
    pad = window_size // 2
    mu1 = F.avg_pool2d(pred, window_size, stride=1, padding=pad)
    mu2 = F.avg_pool2d(target, window_size, stride=1, padding=pad)
    mu1_sq = mu1 * mu1
    mu2_sq = mu2 * mu2
    mu1_mu2 = mu1 * mu2
    sigma1_sq = F.avg_pool2d(pred * pred, window_size, stride=1, padding=pad) - mu1_sq
    sigma2_sq = F.avg_pool2d(target * target, window_size, stride=1, padding=pad) - mu2_sq
    sigma12 = F.avg_pool2d(pred * target, window_size, stride=1, padding=pad) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def kernel_supported(pred: torch.Tensor, target: torch.Tensor, window_size: int) -> bool:
    """Whether csrc/quality.hip serves this call: fp32 tensors of one shape on one ROCm device, >= 2 dims, odd window 1..31."""
    return (isinstance(window_size, int) and 1 <= window_size <= MAX_WINDOW and window_size % 2 == 1
            and pred.is_cuda and target.is_cuda and pred.device == target.device
            and pred.dtype == torch.float32 and target.dtype == torch.float32
            and pred.dim() >= 2 and pred.shape == target.shape and pred.numel() > 0)


def _dense_planes(t: torch.Tensor) -> torch.Tensor:
    """[n, H, W] view of the trailing planes with dense rows (a copy only where the layout needs one)."""
    H, W = t.shape[-2:]
    t = t.reshape(-1, H, W)
    return t if t.stride(2) == 1 and t.stride(1) == W else t.contiguous()


def plane_quality_sums(pred: torch.Tensor, target: torch.Tensor, window_size: int = 11, c1: float = C1, c2: float = C2):
    """Per-plane fp64 sums of the SSIM map and of the squared error over the trailing [H, W] planes of two fp32 tensors of one
    shape on a ROCm device (one kernel launch + one summing launch; bit-identical from call to call).
    Returns (ssim_sum, sqerr_sum), each float64 of shape pred.shape[:-2]."""
    dev = _lib.require_cuda(pred.device, "plane_quality_sums")
    if not kernel_supported(pred, target, window_size):
        raise ValueError("plane_quality_sums: needs fp32 tensors of one shape (>= 2 dims) on one ROCm device and an odd "
                         f"window 1..{MAX_WINDOW}; got {tuple(pred.shape)} {pred.dtype} / {tuple(target.shape)} {target.dtype}, "
                         f"window {window_size}")
    H, W = pred.shape[-2:]
    lead = tuple(pred.shape[:-2])
    a, b = _dense_planes(pred), _dense_planes(target)
    n = a.shape[0]
    L = _lib.load()
    ssim = torch.empty(n, dtype=torch.float64, device=dev)
    sqerr = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for s in range(0, n, 65535):                      # the kernel takes up to 65535 planes per call
            m = min(65535, n - s)
            ws_bytes = L.smk_image_quality_workspace(m, H, W)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(L.smk_image_quality(a[s].data_ptr(), a.stride(0), b[s].data_ptr(), b.stride(0), m, H, W, window_size,
                                           float(c1), float(c2), ws.data_ptr(), ws_bytes, ssim[s].data_ptr(), sqerr[s].data_ptr(),
                                           _lib.stream_ptr(dev)))
    return ssim.reshape(lead), sqerr.reshape(lead)


class _PlaneSsim(torch.autograd.Function):
    """Mean SSIM of n planes on csrc/quality.hip: smk_image_quality forward, smk_image_quality_backward for d/d pred."""

    @staticmethod
    def forward(ctx, pred, target, window_size):
        H, W = pred.shape[-2:]
        a, b = _dense_planes(pred), _dense_planes(target)
        ssim_sum, _ = plane_quality_sums(a, b, window_size)
        ctx.save_for_backward(a, b)
        ctx.window_size, ctx.pred_shape = window_size, pred.shape
        return (ssim_sum / (H * W)).to(torch.float32).reshape(pred.shape[:-2])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        a, b = ctx.saved_tensors
        n, H, W = a.shape
        dev = a.device
        g = grad_out.to(torch.float32).reshape(n).contiguous()
        dpred = torch.empty(n, H, W, dtype=torch.float32, device=dev)          # the kernel writes every element
        L = _lib.load()
        with torch.cuda.device(dev):
            for s in range(0, n, 65535):                  # the kernel takes up to 65535 planes per call
                m = min(65535, n - s)
                ws_bytes = L.smk_image_quality_backward_workspace(m, H, W)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                _lib.check(L.smk_image_quality_backward(a[s].data_ptr(), a.stride(0), b[s].data_ptr(), b.stride(0), m, H, W,
                                                        ctx.window_size, float(C1), float(C2), g[s].data_ptr(), ws.data_ptr(), ws_bytes,
                                                        dpred[s].data_ptr(), dpred.stride(0), _lib.stream_ptr(dev)))
        return dpred.reshape(ctx.pred_shape), None, None


def plane_ssim(pred: torch.Tensor, target: torch.Tensor, window_size: int = 11) -> torch.Tensor:
    """Mean SSIM of every trailing [H, W] plane: an fp32 tensor of shape pred.shape[:-2] (the inputs' dtype on the torch route),
    differentiable with respect to pred.  Tensors the kernel serves (`kernel_supported`) with a target that wants no gradient run
    csrc/quality.hip forward and backward (first order only: a second derivative raises; ask `ssim_torch` for it); everything else
    -- CPU tensors, fp64, an even window, a target that requires a gradient -- runs `ssim_torch` under torch's autograd."""
    if kernel_supported(pred, target, window_size) and not target.requires_grad:
        return _PlaneSsim.apply(pred, target, window_size)
    H, W = pred.shape[-2:]
    ssim_map = ssim_torch(pred.reshape(-1, 1, H, W), target.reshape(-1, 1, H, W), window_size)
    return ssim_map.mean((-2, -1)).reshape(pred.shape[:-2])


def _psnr(mse):
    """20 log10(1 / sqrt(mse)); +inf at mse == 0, as torch gives."""
    return 20 * math.log10(1.0 / math.sqrt(mse)) if mse > 0 else float("inf")


class RobustnessEvaluator:
    """Robustness evaluator (robustness_metrics.py:9-108)."""

    def __init__(self, device: str = 'cuda'):
        self.device = device

    def evaluate_physics_consistency(self, model: nn.Module, test_data: torch.Tensor, physics_targets: Dict) -> Dict:
        """Mean absolute error of each physics feature against its target (robustness_metrics.py:15-48)."""
        model.eval()
        with torch.no_grad():
            predictions = model(test_data)
        physics_pred = predictions['physics_features']
        metrics = {}
        for col, key, name in ((0, 'lyapunov', 'lyapunov_mae'), (1, 'fractal_dimension', 'fractal_mae'), (2, 'entropy', 'entropy_mae')):
            if key in physics_targets:
                metrics[name] = torch.abs(physics_pred[:, col] - physics_targets[key]).mean().item()
        return metrics

    def evaluate_reconstruction_quality(self, model: nn.Module, test_data: torch.Tensor, targets: torch.Tensor) -> Dict:
        """{'ssim', 'psnr', 'mse'} of the model's reconstruction (robustness_metrics.py:50-74); on the kernel route all three come
        from one launch."""
        model.eval()
        with torch.no_grad():
            reconstructed = model(test_data)['reconstructed']
        if kernel_supported(reconstructed, targets, 11):
            ssim, sqerr = plane_quality_sums(reconstructed, targets, 11)
            plane = reconstructed.shape[-2] * reconstructed.shape[-1]
            mse = sqerr.sum().item() / reconstructed.numel()
            return {'ssim': ssim.sum().item() / (ssim.numel() * plane), 'psnr': _psnr(mse), 'mse': mse}
        return {'ssim': self.compute_ssim(reconstructed, targets), 'psnr': self.compute_psnr(reconstructed, targets),
                'mse': F.mse_loss(reconstructed, targets).item()}

    def compute_ssim(self, pred: torch.Tensor, target: torch.Tensor, window_size: int = 11, sigma: float = 1.5) -> float:
        """Mean of the SSIM map over every image, channel and pixel (robustness_metrics.py:76-99).  `sigma` is accepted and
        ignored, as in the reference (the window is a box, not a Gaussian)."""
        if kernel_supported(pred, target, window_size):
            ssim, _ = plane_quality_sums(pred, target, window_size)
            return ssim.sum().item() / pred.numel()
        return ssim_torch(pred, target, window_size).mean().item()

    def compute_psnr(self, pred: torch.Tensor, target: torch.Tensor) -> float:
        """20 log10(1 / sqrt(F.mse_loss(pred, target))) (robustness_metrics.py:101-105); +inf for identical inputs."""
        if kernel_supported(pred, target, 1):
            _, sqerr = plane_quality_sums(pred, target, 1)            # window 1: the squared error without the pooled moments' work
            return _psnr(sqerr.sum().item() / pred.numel())
        mse = F.mse_loss(pred, target)
        return (20 * torch.log10(1.0 / torch.sqrt(mse))).item()

    def image_quality(self, pred: torch.Tensor, target: torch.Tensor, window_size: int = 11) -> Dict[str, torch.Tensor]:
        """Per-image metrics of a batch [B, C, H, W] (not in the reference): {'ssim', 'mse', 'psnr'}, each a float64 tensor [B].
        ssim[b] is compute_ssim(pred[b:b+1], target[b:b+1]), mse[b] the mean squared error of image b, psnr[b] its PSNR
        (+inf where mse is 0).  On the kernel route all three come from the channel planes' sums of one launch."""
        if pred.dim() != 4 or target.dim() != 4:
            raise ValueError(f"image_quality: pred and target must be [B, C, H, W], got {tuple(pred.shape)} / {tuple(target.shape)}")
        if kernel_supported(pred, target, window_size):
            ssim_sum, sqerr_sum = plane_quality_sums(pred, target, window_size)
            per_image = pred[0].numel()
            ssim = ssim_sum.sum(dim=1) / per_image
            mse = sqerr_sum.sum(dim=1) / per_image
        else:
            ssim = ssim_torch(pred, target, window_size).double().flatten(1).mean(dim=1)
            mse = (pred - target).double().pow(2).flatten(1).mean(dim=1)
        psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))
        return {'ssim': ssim, 'mse': mse, 'psnr': psnr}
