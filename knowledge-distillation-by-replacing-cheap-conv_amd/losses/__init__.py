"""KD criteria with the reference's class names and constructor arguments (losses/__init__.py:1-7 of the
reference), so `config.init_obj('kd_loss' | 'hint_loss' | 'supervised_loss', losses)` resolves unchanged: CrossEntropyLoss2d,
JSDivergenceLoss, KLDivergenceLoss, MSELoss, FocalLoss, WeightedHintMSELoss, TopkHintMSELoss, EnsembleKLDivergenceLoss.
Each forward is one fused HIP pass producing the loss and its gradient (include/kdcc.h, losses section)."""
import torch
from torch import nn

from .. import ops
from .._lib import KdccError
from ..lazy import LazyLogits, deferred


class _FusedLoss(torch.autograd.Function):
    """loss, d loss / d inputs computed together in forward; backward only scales by the upstream gradient."""

    @staticmethod
    def forward(ctx, kind, inputs, targets, arg, weight):
        want = inputs.requires_grad
        s, t = inputs.detach(), targets.detach()
        if kind == "kld":
            loss, grad = ops.kldiv(s, t, arg, want_grad=want)
        elif kind == "mse":
            loss, grad = ops.hint_mse(s, t, arg, want_grad=want)
        elif kind == "jsd":
            loss, grad = ops.jsdiv(s, t, arg, want_grad=want)
        elif kind == "ekl":
            loss, grad = ops.ensemble_kldiv(s, t, want_grad=want)
        elif kind == "topk":
            loss, grad, _ = ops.topk_hint_mse(s, t, arg, want_grad=want)
        else:
            loss, grad = ops.weighted_hint_mse(s, t, weight, want_grad=want)
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad
        ctx.grad = None
        if grad is None:
            return None, None, None, None, None
        # the stored gradient is this Function's own buffer: scale it in place, and not at all when the upstream factor is 1
        # (loss = sum of hint losses), which the kernel finds out on the device
        if g.numel() == 1 and grad.dtype in (torch.float32, torch.bfloat16) and grad.data_ptr() % 16 == 0:
            return None, ops.scale_by_device_scalar_(grad, g), None, None, None
        return None, grad * g.to(grad.dtype), None, None, None


def _same_device_dtype(inputs, targets):
    if targets.dtype != inputs.dtype and not (targets.dtype in (torch.float32, torch.bfloat16)):
        targets = targets.to(inputs.dtype)
    return targets


class KLDivergenceLoss(nn.Module):
    """kl_div(log_softmax(inputs/T, 1), softmax(targets/T, 1), 'mean') * T^2 * C  (losses/KLDiv.py:15-23)."""

    def __init__(self, temperature=1):
        super().__init__()
        self.temperature = temperature

    def forward(self, inputs, targets):
        if isinstance(inputs, LazyLogits) and isinstance(targets, LazyLogits) and inputs.pending and targets.pending and \
                inputs.size_hw == targets.size_hw and inputs.align_corners == targets.align_corners:
            # both sides are the classifier's half-resolution logits: interpolate in registers (kd_kldiv_up)
            try:
                return deferred(ops.kldiv_up(inputs.low, targets.low, inputs.size_hw, float(self.temperature), inputs.align_corners),
                                "kld", inputs, targets, float(self.temperature))
            except KdccError:
                pass      # resampling ratio / class count outside the kernel's range: materialise
        return _FusedLoss.apply("kld", inputs, _same_device_dtype(inputs, targets), float(self.temperature), None)


class MSELoss(nn.Module):
    """nn.MSELoss(reduction)(inputs, targets) * num_classes  (losses/MSELoss.py:9-16); reduction 'mean' (every shipped config) or 'sum'
    (the same kernel: the mean and its gradient scaled by the element count)."""

    def __init__(self, reduction='mean', num_classes=19):
        super().__init__()
        if reduction not in ('mean', 'sum'):
            raise NotImplementedError("reduction='none' returns a tensor no KD trainer consumes: 'mean' or 'sum'")
        self.reduction = reduction
        self.num_classes = num_classes

    def forward(self, inputs, targets):
        scale = float(self.num_classes) * (inputs.numel() if self.reduction == 'sum' else 1)
        return _FusedLoss.apply("mse", inputs, _same_device_dtype(inputs, targets), scale, None)


class WeightedHintMSELoss(nn.Module):
    """mean_n( sum_c w * mean_hw (s-t)^2 / sum_c w )  (losses/WeightedHintMSELoss.py:5-16); w is (C,) or (N,C)."""

    def __init__(self, reduction='mean', num_classes=19):
        super().__init__()
        self.reduction = reduction
        self.num_classes = num_classes

    def forward(self, inputs, targets, filter_weight):
        return _FusedLoss.apply("whmse", inputs, _same_device_dtype(inputs, targets), None, filter_weight)


class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, ignore_index, weight=None, size_average=True):
        ctx.save_for_backward(inputs.detach(), targets)
        ctx.ignore_index, ctx.weight, ctx.size_average = ignore_index, weight, size_average
        return ops.ce2d(inputs.detach(), targets, ignore_index, weight, size_average)

    @staticmethod
    def backward(ctx, g):
        x, tgt = ctx.saved_tensors
        grad = ops.ce2d_grad(x, tgt, ctx.ignore_index, 1.0, ctx.weight, ctx.size_average)
        return grad * g.to(grad.dtype), None, None, None, None


class CrossEntropyLoss2d(nn.Module):
    """NLLLoss(ignore_index)(log_softmax(inputs, 1), targets)  (losses/CrossEntropy.py:5-14).  A logged metric in the KD
    trainers (forward-only there: `inputs` is detached when nothing asks for its gradient); differentiable for the trainers
    that back-propagate the supervised loss (trainer/taylor_prune_trainer.py:204-206)."""

    def __init__(self, weight=None, size_average=True, ignore_index=255):
        super().__init__()
        # a buffer like nn.NLLLoss(weight)'s: follows .to(device) / state_dict and is uploaded once
        self.register_buffer('weight', None if weight is None else torch.as_tensor(weight, dtype=torch.float32))
        self.size_average = bool(size_average)
        self.ignore_index = ignore_index

    def forward(self, inputs, targets):
        if self.weight is not None and self.weight.device != inputs.device:
            self.weight = self.weight.to(inputs.device)             # once (a criterion that was never moved with .to())
        if self.weight is not None or not self.size_average:       # (kd_ce2d_weighted; no shipped KD config: full-resolution logits)
            if inputs.requires_grad and torch.is_grad_enabled():
                return _CEFunction.apply(inputs, targets, self.ignore_index, self.weight, self.size_average)
            return ops.ce2d(inputs, targets, self.ignore_index, self.weight, self.size_average)
        if isinstance(inputs, LazyLogits) and inputs.pending:
            try:
                return deferred(ops.ce2d_up(inputs.low, targets, inputs.size_hw, self.ignore_index, inputs.align_corners),
                                "ce", inputs, targets, self.ignore_index)
            except KdccError:
                pass
        if inputs.requires_grad and torch.is_grad_enabled():
            return _CEFunction.apply(inputs, targets, self.ignore_index)
        return ops.ce2d(inputs, targets, self.ignore_index)


class JSDivergenceLoss(nn.Module):
    """T^2/(2N) * sum [KL(p_t || q) + KL(p_s || q)], q = (p_s + p_t)/2, p = softmax(./T, 1)  (losses/JSDiv.py:17-26): divided by the
    batch size only; the targets are constants (kd_jsdiv)."""

    def __init__(self, temperature=1):
        super().__init__()
        self.temperature = temperature

    def forward(self, inputs, targets):
        if isinstance(inputs, LazyLogits) and isinstance(targets, LazyLogits) and inputs.pending and targets.pending and \
                inputs.size_hw == targets.size_hw and inputs.align_corners == targets.align_corners:
            try:      # both sides are the classifier's half-resolution logits (kd_jsdiv_up)
                return deferred(ops.jsdiv_up(inputs.low, targets.low, inputs.size_hw, float(self.temperature), inputs.align_corners),
                                "jsd", inputs, targets, float(self.temperature))
            except KdccError:
                pass      # resampling ratio / class count outside the kernel's range: materialise
        return _FusedLoss.apply("jsd", inputs, _same_device_dtype(inputs, targets), float(self.temperature), None)


class EnsembleKLDivergenceLoss(nn.Module):
    """kl_div(log_softmax(inputs, 1), targets, 'mean') * C with `targets` already probabilities (losses/EnsembleKLDiv.py:15-21;
    kd_ensemble_kldiv)."""

    def __init__(self):
        super().__init__()

    def forward(self, inputs, targets):
        return _FusedLoss.apply("ekl", inputs, _same_device_dtype(inputs, targets), None, None)


class TopkHintMSELoss(nn.Module):
    """Hint MSE over each sample's K = int(topk * C) channels of largest target L2 norm: sum mask * mean_hw (s-t)^2 / (N*K)
    (losses/WeightedHintMSELoss.py:19-44; num_classes is not applied).  4-D targets only; equal norms keep the lower channel; K == 0
    raises (the reference divides by zero).  The selection runs on the device (kd_topk_hint_mse)."""

    def __init__(self, reduction='mean', num_classes=19, topk=0.5):
        super().__init__()
        self.reduction = reduction
        self.num_classes = num_classes
        self.topk = topk

    def forward(self, inputs, targets):
        if targets.dim() != 4 or inputs.shape != targets.shape:
            raise ValueError(f"TopkHintMSELoss: (N,C,H,W) inputs and targets of one shape only, got {tuple(inputs.shape)} and "
                             f"{tuple(targets.shape)}")
        num_channels = targets.shape[1]
        k = int(self.topk * num_channels)          # the reference's idx_pivot (WeightedHintMSELoss.py:35)
        if k <= 0:
            raise ValueError(f"TopkHintMSELoss: topk={self.topk} keeps no channel of {num_channels}")
        return _FusedLoss.apply("topk", inputs, _same_device_dtype(inputs, targets), min(k, num_channels), None)


class _FocalFunction(torch.autograd.Function):
    """FocalLoss value (kd_focal) and, in backward, its gradient scaled by the upstream one on the device (kd_focal_grad)."""

    @staticmethod
    def forward(ctx, inputs, targets, gamma, alpha, ignore_index, reduction):
        x = inputs.detach()
        loss, stats, amap, cemap = ops.focal(x, targets, gamma, alpha, ignore_index, reduction)
        ctx.save_for_backward(x, targets)
        ctx.args, ctx.stats, ctx.maps = (gamma, alpha, ignore_index, reduction), stats, (amap, cemap)
        if reduction == 'none':
            # the reference's broadcast (N,1,*sp) * (N,*sp) -> (N,N,*sp): element [i,j] = a_i * ce_j (FocalLoss.py:23)
            N, sp = x.shape[0], tuple(x.shape[2:])
            return amap.view(N, 1, *sp) * cemap.view(N, *sp)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, tgt = ctx.saved_tensors
        gamma, alpha, ignore_index, reduction = ctx.args
        grad = ops.focal_grad(x, tgt, gamma, alpha, ignore_index, reduction, g, ctx.stats, *ctx.maps)
        ctx.stats = ctx.maps = None
        return grad, None, None, None, None, None


class FocalLoss(nn.CrossEntropyLoss):
    """pow(1 - p_y', gamma) * CE with the inner nn.CrossEntropyLoss(weight=alpha, ignore_index) already reduced by `reduction`
    (losses/FocalLoss.py:7-28: the class overwrites `reduction` after __init__).  'mean': mean(a) * CE_mean; 'sum': sum(a) * CE_sum;
    'none' (the default): the (N,N,H,W) broadcast product a_i * ce_j the reference returns.  y' = target where valid, 0 where ignored.
    For gamma < 1 the gradient at p_y' == 1 is 0 (its limit) where the reference's is NaN."""

    def __init__(self, gamma, alpha=None, ignore_index=-100, reduction='none'):
        if alpha is not None and not torch.is_tensor(alpha):
            alpha = torch.as_tensor(alpha, dtype=torch.float32)       # (a config gives a list)
        super().__init__(weight=alpha, ignore_index=ignore_index, reduction='none')
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"FocalLoss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        self.reduction = reduction
        self.gamma = gamma

    def forward(self, input_, target):
        if self.weight is not None and self.weight.device != input_.device:
            self.weight = self.weight.to(input_.device)
        gamma = float(self.gamma)
        if isinstance(input_, LazyLogits) and input_.pending and self.reduction in ('mean', 'sum'):
            try:      # the classifier's half-resolution logits, interpolated in registers (kd_focal_up)
                loss, stats = ops.focal_up(input_.low, target, input_.size_hw, gamma, self.weight, self.ignore_index, self.reduction,
                                           input_.align_corners)
                return deferred(loss, "focal", input_, target, (gamma, self.weight, self.ignore_index, self.reduction, stats))
            except KdccError:
                pass
        return _FocalFunction.apply(input_, target, gamma, self.weight, self.ignore_index, self.reduction)
