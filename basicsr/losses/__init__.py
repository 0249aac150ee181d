"""LOSS_REGISTRY entries the path's callers use (reference basicsr/losses/basic_loss.py:39-232,338-363;
plain torch expressions whose gradients seed the hot path -- SURVEY section 2 #17 keeps them in torch).  The SSIM term of SSIMLoss /
SSIMMSELoss is the exception: the reference's calculate_ssim_pt is five grouped fp64 convolutions and their transposes, here the fused fp64
kernels of dcpt_amd/csrc/ssim_loss.hip (basicsr.metrics.calculate_ssim_pt)."""
from copy import deepcopy

import torch
from torch import nn
from torch.nn import functional as F

from basicsr.utils import get_root_logger
from basicsr.utils.registry import LOSS_REGISTRY

__all__ = ["build_loss", "L1Loss", "MSELoss", "CharbonnierLoss", "PSNRLoss", "CrossEntropyLoss", "SmoothL1Loss", "HuberLoss", "SSIMLoss",
           "SSIMMSELoss"]


def _reduce(loss, reduction):
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    if reduction == "none":
        return loss
    raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: none | mean | sum")


@LOSS_REGISTRY.register()
class L1Loss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        self.loss_weight, self.reduction = loss_weight, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        loss = (pred - target).abs()
        if weight is not None:
            loss = loss * weight
        return self.loss_weight * _reduce(loss, self.reduction)


@LOSS_REGISTRY.register()
class MSELoss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        self.loss_weight, self.reduction = loss_weight, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        loss = (pred - target) ** 2
        if weight is not None:
            loss = loss * weight
        return self.loss_weight * _reduce(loss, self.reduction)


@LOSS_REGISTRY.register()
class CharbonnierLoss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction="mean", eps=1e-12):
        super().__init__()
        self.loss_weight, self.reduction, self.eps = loss_weight, reduction, eps

    def forward(self, pred, target, weight=None, **kwargs):
        loss = torch.sqrt((pred - target) ** 2 + self.eps)
        if weight is not None:
            loss = loss * weight
        return self.loss_weight * _reduce(loss, self.reduction)


@LOSS_REGISTRY.register()
class PSNRLoss(nn.Module):
    """10/ln(10) * log(mse + 1e-8) per image, averaged (reference basic_loss.py PSNRLoss)."""

    def __init__(self, loss_weight=1.0, reduction="mean", toY=False):
        super().__init__()
        assert reduction == "mean"
        self.loss_weight = loss_weight
        self.scale = 10 / torch.log(torch.tensor(10.0)).item()
        self.toY = toY

    def forward(self, pred, target):
        if self.toY:
            coef = torch.tensor([65.481, 128.553, 24.966], device=pred.device).reshape(1, 3, 1, 1)
            pred = ((pred * coef).sum(dim=1, keepdim=True) + 16.0) / 255.0
            target = ((target * coef).sum(dim=1, keepdim=True) + 16.0) / 255.0
        return self.loss_weight * self.scale * torch.log(((pred - target) ** 2).mean(dim=(1, 2, 3)) + 1e-8).mean()


@LOSS_REGISTRY.register()
class CrossEntropyLoss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        self.loss_weight, self.reduction = loss_weight, reduction

    def forward(self, pred, target, **kwargs):
        return self.loss_weight * F.cross_entropy(pred, target, reduction=self.reduction)


def _check_reduction(reduction):
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: ['none', 'mean', 'sum']")


def weight_reduce_loss(loss, weight=None, reduction="mean", wide=False):
    """the reference's rule (loss_util.py:27-56): the element-wise loss times ``weight`` ((N, C, H, W) or (N, 1, H, W)); without a weight, or
    with 'sum', the plain reduction; with a weight and 'mean', the sum divided by the weight's sum (times C for a one-channel weight).
    ``wide``: the fp32 element-wise terms are added up in float64 (the SSIM losses, whose result is float64 either way: the value then does
    not depend on a device's fp32 summation order; the gradient is the same, it passes the cast as fp32)."""
    if weight is not None:
        assert weight.dim() == loss.dim()
        assert weight.size(1) == 1 or weight.size(1) == loss.size(1)
        loss = loss * weight
    if wide:
        loss = loss.double()
    if weight is None or reduction == "sum":
        return _reduce(loss, reduction)
    if reduction == "mean":
        wsum = weight.double().sum() if wide else weight.sum()
        return loss.sum() / (wsum if weight.size(1) > 1 else wsum * loss.size(1))
    return loss


def huber_loss(pred, target, weight=None, reduction="mean", delta=0.01, wide=False):
    """the reference's ``huber_loss`` (basic_loss.py:30-36): 0.5 min(|d|, delta)^2 + (|d| - min(|d|, delta)), not divided by delta"""
    err = (pred - target).abs()
    quad = err.clamp(max=delta)
    return weight_reduce_loss(0.5 * quad.pow(2) + (err - quad), weight, reduction, wide)


@LOSS_REGISTRY.register()
class SmoothL1Loss(nn.Module):
    """reference basic_loss.py:89-118: ``F.smooth_l1_loss`` (beta 1); ``weight`` is accepted and ignored, as there"""

    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        _check_reduction(reduction)
        self.loss_weight, self.reduction = loss_weight, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        return self.loss_weight * F.smooth_l1_loss(pred, target, reduction=self.reduction)


@LOSS_REGISTRY.register()
class HuberLoss(nn.Module):
    """reference basic_loss.py:121-149"""

    def __init__(self, loss_weight=1.0, delta=0.01, reduction="mean"):
        super().__init__()
        _check_reduction(reduction)
        self.loss_weight, self.delta, self.reduction = loss_weight, delta, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        return self.loss_weight * huber_loss(pred, target, weight, self.reduction, self.delta)


def _ssim(pred, target, crop_border, test_y_channel):
    from basicsr.metrics import calculate_ssim_pt

    return calculate_ssim_pt(pred, target, crop_border=crop_border, test_y_channel=test_y_channel, image_range=1)


@LOSS_REGISTRY.register()
class SSIMLoss(nn.Module):
    """reference basic_loss.py:152-190: ``ssim_weight (1 - SSIM) + mse_weight huber_loss(pred, target, weight)`` (delta 0.01), a float64
    scalar.  As in the reference, whose ``calculate_ssim_pt(...)[0].mean()`` indexes the per-image vector before the mean, the SSIM term is
    the FIRST image's SSIM only: images 1.. of the batch get their gradient from the Huber term alone.  The kernels therefore run on the
    ``[:1]`` slice.  The Huber values are fp32 as in the reference, added up in float64 (``weight_reduce_loss``)."""

    def __init__(self, ssim_weight=0.1, mse_weight=1.0, crop_border=0, reduction="mean", test_y_channel=False):
        super().__init__()
        self.ssim_weight, self.mse_weight, self.crop_border = ssim_weight, mse_weight, crop_border
        self.test_y_channel, self.reduction = test_y_channel, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        ssim = _ssim(pred[:1], target[:1], self.crop_border, self.test_y_channel)[0].mean()
        return self.ssim_weight * (1 - ssim) + self.mse_weight * huber_loss(pred, target, weight, self.reduction, wide=True)


@LOSS_REGISTRY.register()
class SSIMMSELoss(nn.Module):
    """reference basic_loss.py:193-232: ``ssim_weight (1 - mean over the batch of SSIM) + mse_weight mse(pred, target)``, a float64 scalar.
    The reference's ``float64=False`` disappears into ``calculate_ssim_pt``'s ``**kwargs``, so the SSIM term is fp64 there and here; a
    ``weight`` is not taken (it would disappear the same way).  The squared errors are fp32, added up in float64."""

    def __init__(self, ssim_weight=0.1, mse_weight=1.0, crop_border=0, reduction="mean", test_y_channel=False):
        super().__init__()
        self.ssim_weight, self.mse_weight, self.crop_border = ssim_weight, mse_weight, crop_border
        self.test_y_channel, self.reduction = test_y_channel, reduction

    def forward(self, pred, target, **kwargs):
        ssim = _ssim(pred, target, self.crop_border, self.test_y_channel).mean()
        return self.ssim_weight * (1 - ssim) + self.mse_weight * weight_reduce_loss((pred - target) ** 2, None, self.reduction, wide=True)


def build_loss(opt):
    opt = deepcopy(opt)
    loss = LOSS_REGISTRY.get(opt.pop("type"))(**opt)
    get_root_logger().info(f"Loss [{loss.__class__.__name__}] is created.")
    return loss
