"""The training loss of train.py's batch_losses on libsmokehip: reconstruction MSE, chaos-feature MSE and PhysicsRegularizer's
mass-conservation and continuity terms from smk_train_loss_forward / smk_train_loss_backward (csrc/loss.hip), under autograd.

`hip_train_losses` returns one device vector [total, recon, physics, chaos, mass, continuity]; a gradient on any of the six is honoured.
Inputs the kernels do not take (`hip_train_losses_supported`) keep the torch formulas (`torch_train_losses`).

`ssim_loss` is the opt-in SSIM term of train.py (`mi355x.ssim_weight`), on the image-quality kernels of csrc/quality.hip.
"""
import torch
import torch.nn.functional as F

from .. import _lib
from ..evaluation.robustness_metrics import plane_ssim

__all__ = ["LOSS_NAMES", "hip_train_losses", "hip_train_losses_supported", "ssim_loss", "torch_train_losses"]

LOSS_NAMES = ("total", "recon", "physics", "chaos", "mass", "continuity")


def _plane_elems(t) -> int:
    """Elements of one plane of mass_conservation_loss: it sums the last two dimensions."""
    return int(t.shape[-1]) * int(t.shape[-2]) if t.dim() >= 2 else int(t.numel())


def hip_train_losses_supported(pred, target, chaos_pred, chaos_target, sequence=None) -> bool:
    """float32 contiguous tensors on one ROCm device, pred.shape == target.shape (at least one element, at least 2-D),
    chaos_pred.shape == chaos_target.shape, a [B, T, ...] sequence (or None) and no gradient asked of the targets or the sequence."""
    tensors = [pred, target, chaos_pred, chaos_target] + ([] if sequence is None else [sequence])
    if not all(torch.is_tensor(t) for t in tensors) or pred.device.type != "cuda":
        return False
    if not all(t.device == pred.device and t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous() for t in tensors):
        return False
    if pred.shape != target.shape or chaos_pred.shape != chaos_target.shape or pred.dim() < 2 or pred.numel() == 0 or chaos_pred.numel() == 0:
        return False
    if target.requires_grad or chaos_target.requires_grad:
        return False
    if sequence is not None and (sequence.requires_grad or sequence.dim() < 2):
        return False
    return max(pred.numel() // _plane_elems(pred), _plane_elems(pred), chaos_pred.numel()) < 2 ** 31


def torch_train_losses(pred, target, chaos_pred, chaos_target, sequence, regularizer, w_chaos=0.1, w_physics=0.05):
    """The six values from the torch formulas of batch_losses (the route of everything the kernels do not take)."""
    recon = F.mse_loss(pred, target)
    chaos = F.mse_loss(chaos_pred, chaos_target)
    mass = regularizer.mass_conservation_loss(pred, target)
    cont = regularizer.continuity_loss(sequence) if sequence is not None else torch.zeros((), device=pred.device)
    physics = regularizer.conservation_weight * mass + regularizer.continuity_weight * cont
    total = recon + w_chaos * chaos + w_physics * physics
    return torch.stack([total, recon, physics, chaos, mass, cont.to(total.dtype)])


def ssim_loss(pred, target, window_size: int = 11):
    """1 - the mean over planes of the SSIM that RobustnessEvaluator reports (evaluation.plane_ssim: csrc/quality.hip forward and
    backward for fp32 tensors on a ROCm device, the torch formula under autograd for everything else)."""
    return 1 - plane_ssim(pred, target, window_size).mean()


class _HipTrainLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, chaos_pred, target, chaos_target, sequence, w_chaos, w_physics, w_mass, w_continuity):
        L = _lib.load()
        dev = pred.device
        plane_elems = _plane_elems(pred)
        planes = pred.numel() // plane_elems
        if sequence is not None and sequence.numel() > 0:
            seq_ptr, seq_batch, seq_T = sequence.data_ptr(), int(sequence.shape[0]), int(sequence.shape[1])
            seq_plane = sequence.numel() // (seq_batch * seq_T)
        else:
            seq_ptr, seq_batch, seq_T, seq_plane = None, 0, 0, 0
        need = int(L.smk_train_loss_workspace(planes, plane_elems, seq_batch, seq_T, seq_plane))
        workspace = torch.empty(max(need // 8, 2), dtype=torch.float64, device=dev)
        out = torch.empty(6, dtype=torch.float32, device=dev)
        mass_diff = torch.empty(planes, dtype=torch.float32, device=dev)
        _lib.check(L.smk_train_loss_forward(pred.data_ptr(), target.data_ptr(), planes, plane_elems, chaos_pred.data_ptr(),
                                            chaos_target.data_ptr(), chaos_pred.numel(), seq_ptr, seq_batch, seq_T, seq_plane, w_chaos,
                                            w_physics, w_mass, w_continuity, out.data_ptr(), mass_diff.data_ptr(), workspace.data_ptr(),
                                            workspace.numel() * 8, _lib.stream_ptr(dev)))
        ctx.save_for_backward(pred, target, chaos_pred, chaos_target, mass_diff)
        ctx.weights = (w_chaos, w_physics, w_mass)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        pred, target, chaos_pred, chaos_target, mass_diff = ctx.saved_tensors
        w_chaos, w_physics, w_mass = ctx.weights
        L = _lib.load()
        g = grad_out.to(torch.float32).contiguous()
        d_pred = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        d_chaos = torch.empty_like(chaos_pred) if ctx.needs_input_grad[1] else None
        plane_elems = _plane_elems(pred)
        _lib.check(L.smk_train_loss_backward(pred.data_ptr(), target.data_ptr(), pred.numel() // plane_elems, plane_elems,
                                             mass_diff.data_ptr(), chaos_pred.data_ptr(), chaos_target.data_ptr(), chaos_pred.numel(),
                                             g.data_ptr(), w_chaos, w_physics, w_mass, None if d_pred is None else d_pred.data_ptr(),
                                             None if d_chaos is None else d_chaos.data_ptr(), _lib.stream_ptr(pred.device)))
        return (d_pred, d_chaos) + (None,) * 7


def hip_train_losses(pred, target, chaos_pred, chaos_target, sequence, regularizer, w_chaos: float = 0.1, w_physics: float = 0.05):
    """[total, recon, physics, chaos, mass, continuity] of batch_losses' decomposition as one device vector:
    total = recon + w_chaos chaos + w_physics physics, physics = conservation_weight mass + continuity_weight continuity.
    Planes are the last two dimensions of pred / target (what mass_conservation_loss sums); `sequence` is [B, T, ...] or None."""
    if not hip_train_losses_supported(pred, target, chaos_pred, chaos_target, sequence):
        return torch_train_losses(pred, target, chaos_pred, chaos_target, sequence, regularizer, w_chaos, w_physics)
    return _HipTrainLosses.apply(pred, chaos_pred, target, chaos_target, sequence, float(w_chaos), float(w_physics),
                                 float(regularizer.conservation_weight), float(regularizer.continuity_weight))
