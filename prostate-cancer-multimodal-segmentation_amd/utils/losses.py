"""Drop-in ``DiceLoss`` / ``BCEDiceLoss`` (utils/losses.py of the reference) on HIP kernels.

DiceLoss(smooth=1.0):   1 - (2 sum(p t) + s) / (sum p + sum t + s),  p = sigmoid(pred),
                        sums over the WHOLE batch (view(-1), utils/losses.py:72-92).
BCEDiceLoss(0.5, 0.5):  bce_weight * mean BCEWithLogits + dice_weight * Dice (:124-152).

Forward: one pass producing fp32 block partials of (sum p t, sum p, sum t, sum bce),
combined in fp64 on device; backward: one elementwise pass for dL/dpred.  No host sync.

Beyond the reference, for small lesions on big grids (kernels of their own, csrc/losses.hip; the
two losses above are untouched): ``TverskyLoss``, ``FocalTverskyLoss``, ``FocalLoss``,
``FocalTverskyFocalLoss`` and the general ``RegionVoxelLoss`` -- a Tversky / focal-Tversky region
term over the batch or per (sample, channel) volume plus a focal voxel term; the fp64 definition
is ``region_voxel_loss_host``.

For mutually exclusive classes (csrc/classes.hip): ``SoftmaxDiceCELoss`` -- softmax cross-entropy
plus a per-class Dice on ``(N, C, ...)`` logits against a class map; the fp64 definition is
``classes.softmax_dice_ce_loss_host``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import _lib
from .._lib import call, query
from ..classes import _validate_loss, softmax_dice_ce_loss


class _LossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, smooth, wb, wd):
        if pred.device.type != "cuda":
            raise RuntimeError("pcms_amd losses run on a ROCm device only (no CPU path)")
        x = pred.detach().contiguous().float()
        t = target.detach().contiguous().to(device=x.device, dtype=torch.float32)
        M = x.numel()
        rows = query("pcms_loss_rows", M)
        part = torch.empty(rows * 4, dtype=torch.float32, device=x.device)
        sums = torch.empty(4, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        call("pcms_loss_fwd", x, t, M, float(smooth), float(wb), float(wd), part, sums, loss)
        ctx.save_for_backward(x, t, sums)
        ctx.cfg = (float(smooth), float(wb), float(wd))
        ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, gout):
        x, t, sums = ctx.saved_tensors
        smooth, wb, wd = ctx.cfg
        dx = torch.empty_like(x)
        g = gout.detach().contiguous().float()
        call("pcms_loss_bwd", x, t, x.numel(), sums, smooth, wb, wd, g, dx)
        return dx.view(ctx.shape), None, None, None, None


def _check(pred, target):
    if pred.shape != target.shape:
        raise ValueError(f"预测值和目标值的形状不匹配: pred.shape={pred.shape}, target.shape={target.shape}")


class DiceLoss(nn.Module):
    """Soft Dice loss on sigmoid(pred), global over the batch (utils/losses.py:16-92)."""

    def __init__(self, smooth: float = 1.0):
        super().__init__()
        self.smooth = smooth

    def forward(self, pred, target):
        _check(pred, target)
        return _LossFunction.apply(pred, target, self.smooth, 0.0, 1.0)


class BCEDiceLoss(nn.Module):
    """bce_weight * BCEWithLogits(mean) + dice_weight * Dice (utils/losses.py:95-152)."""

    def __init__(self, bce_weight: float = 0.5, dice_weight: float = 0.5):
        super().__init__()
        self.bce_weight = bce_weight
        self.dice_weight = dice_weight
        self.bce_loss = nn.BCEWithLogitsLoss()  # attribute parity; the fused kernel computes it
        self.dice_loss = DiceLoss()

    def forward(self, pred, target):
        _check(pred, target)
        return _LossFunction.apply(pred, target, self.dice_loss.smooth, self.bce_weight, self.dice_weight)


# ---- imbalance-aware losses (csrc/losses.hip; not in the reference) ------------------------
#
# A *group* is a contiguous run of the NCDHW tensors: the whole batch (``per_sample=False``, the
# reference's Dice convention) or one (sample, channel) volume (``per_sample=True``, nnU-Net's
# ``batch_dice=False``).  Per group g, with p = sigmoid(pred):
#
#     I = sum p t,  P = sum p,  T = sum t
#     D = (1 - alpha - beta) I + alpha P + beta T + smooth,   TI = (I + smooth) / D
#     region_g = max(1 - TI, 0) ** gamma            (alpha weights false positives, beta misses)
#
# per voxel, with ce = BCE-with-logits and p_t = p t + (1 - p)(1 - t):
#
#     v_i = a_i (1 - p_t) ** focal_gamma * ce,   a_i = focal_alpha t + (1 - focal_alpha)(1 - t),
#                                                or 1 with focal_alpha=None
#     loss = region_weight * mean_g region_g + voxel_weight * mean_i v_i
#
# ``region_voxel_loss_host`` is this definition in fp64 torch on the CPU; the modules run it on
# the HIP kernels.


def _validate(alpha, beta, gamma, smooth, focal_gamma, focal_alpha, region_weight, voxel_weight):
    """The rules of the C entry points' argument checks, as ValueError."""
    import math
    vals = {"alpha": alpha, "beta": beta, "gamma": gamma, "smooth": smooth, "focal_gamma": focal_gamma,
            "region_weight": region_weight, "voxel_weight": voxel_weight}
    if focal_alpha is not None:
        vals["focal_alpha"] = focal_alpha
    for k, v in vals.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{k} must be a finite number, got {v!r}")
    if alpha < 0 or beta < 0:
        raise ValueError(f"alpha and beta must be >= 0, got {alpha}, {beta}")
    if smooth < 0:
        raise ValueError(f"smooth must be >= 0, got {smooth}")
    if gamma <= 0:
        raise ValueError(f"gamma must be > 0, got {gamma}")
    if not (focal_gamma == 0 or focal_gamma >= 1):
        raise ValueError(f"focal_gamma must be 0 or >= 1, got {focal_gamma}")
    if focal_alpha is not None and not 0 <= focal_alpha <= 1:
        raise ValueError(f"focal_alpha must be None or in [0, 1], got {focal_alpha}")


def _groups(shape, per_sample):
    """(groups, nvox) of a (N, C, ...) tensor."""
    M = 1
    for s in shape:
        M *= int(s)
    if not per_sample:
        return 1, M
    if len(shape) < 2:
        raise ValueError(f"per_sample=True needs a (N, C, ...) tensor, got shape {tuple(shape)}")
    g = int(shape[0]) * int(shape[1])
    return g, M // max(g, 1)


def region_voxel_loss_host(pred, target, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, focal_gamma=0.0,
                           focal_alpha=None, region_weight=1.0, voxel_weight=0.0, per_sample=False):
    """The definition of ``RegionVoxelLoss`` (see above) in fp64 torch on the CPU, differentiable by
    autograd with respect to ``pred``: what the kernels are tested against.  Where ``1 - TI <= 0``
    (or ``D <= 0``) a group's region term and its gradient are 0."""
    _check(pred, target)
    _validate(alpha, beta, gamma, smooth, focal_gamma, focal_alpha, region_weight, voxel_weight)
    groups, nvox = _groups(pred.shape, per_sample)
    x = pred.to(device="cpu", dtype=torch.float64).reshape(groups, nvox)
    t = target.detach().to(device="cpu", dtype=torch.float64).reshape(groups, nvox)
    p, q = torch.sigmoid(x), torch.sigmoid(-x)  # q = 1 - p without cancellation
    I, P, T = (p * t).sum(1), p.sum(1), t.sum(1)
    D = (1.0 - alpha - beta) * I + alpha * P + beta * T + smooth
    ok = D > 0
    u = 1.0 - (I + smooth) / torch.where(ok, D, torch.ones_like(D))
    pos = ok & (u > 0)
    # (the inner where keeps pow's derivative at 0 out of the graph: 0 * inf otherwise)
    region = torch.where(pos, torch.where(pos, u, torch.ones_like(u)).pow(gamma), torch.zeros_like(u))
    loss = region_weight * region.mean()
    if voxel_weight != 0:
        ce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
        v = ce
        if focal_gamma != 0:
            v = (t * q + (1.0 - t) * p).pow(focal_gamma) * v  # 1 - p_t = t (1 - p) + (1 - t) p
        if focal_alpha is not None:
            v = (focal_alpha * t + (1.0 - focal_alpha) * (1.0 - t)) * v
        loss = loss + voxel_weight * v.mean()
    return loss


class _RegionVoxelFunction(torch.autograd.Function):
    """pcms_region_loss_fwd / _bwd; cfg = (alpha, beta, gamma, smooth, focal_gamma, focal_alpha or
    None, region_weight, voxel_weight, per_sample)."""

    @staticmethod
    def forward(ctx, pred, target, cfg):
        if pred.device.type != "cuda":
            raise RuntimeError("pcms_amd losses run on a ROCm device only (no CPU path)")
        alpha, beta, gamma, smooth, fg, fa, wr, wv, per_sample = cfg
        x = pred.detach().contiguous().float()
        t = target.detach().contiguous().to(device=x.device, dtype=torch.float32)
        groups, nvox = _groups(x.shape, per_sample)
        rows = query("pcms_region_loss_rows", nvox, groups)
        if rows < 1:
            raise ValueError(f"pcms_region_loss_rows({nvox}, {groups}) = {rows}: empty input")
        part = torch.empty(groups * rows * 4, dtype=torch.float32, device=x.device)
        sums = torch.empty(groups * 4, dtype=torch.float64, device=x.device)
        coef = torch.empty(groups * 2, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        vox = (float(fg), int(fa is not None), float(fa if fa is not None else 0.0))
        call("pcms_region_loss_fwd", x, t, nvox, groups, float(alpha), float(beta), float(gamma), float(smooth),
             *vox, float(wr), float(wv), part, sums, coef, loss)
        ctx.save_for_backward(x, t, coef)
        ctx.cfg = (nvox, groups, vox, float(wv))
        ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, gout):
        x, t, coef = ctx.saved_tensors
        nvox, groups, vox, wv = ctx.cfg
        dx = torch.empty_like(x)
        g = gout.detach().contiguous().float()
        call("pcms_region_loss_bwd", x, t, nvox, groups, *vox, wv, coef, g, dx)
        return dx.view(ctx.shape), None, None


class RegionVoxelLoss(nn.Module):
    """``region_weight`` * Tversky / focal-Tversky region term + ``voxel_weight`` * focal voxel term
    on sigmoid(pred) (the formulas above; ``region_voxel_loss_host`` is the definition).

    ``alpha`` / ``beta`` weight false positives / false negatives (0.5, 0.5, smooth s/2 is the
    reference's Dice with smooth s); ``gamma`` is the focal-Tversky exponent (> 0; 1: plain
    Tversky); ``focal_gamma`` (0 or >= 1) and ``focal_alpha`` (None or in [0, 1]) are torchvision's
    ``sigmoid_focal_loss`` parameters; ``per_sample=True`` takes the region sums per (sample,
    channel) volume and averages the region terms, instead of summing over the batch.

    Two launches forward, one backward, no host sync, fixed-order sums (the same bits on every
    run).  Under data parallelism the loss stays per replica; with ``per_sample=True`` and equal
    shards the mean over ranks equals the single-process loss (both terms are then means of
    per-sample values)."""

    def __init__(self, alpha: float = 0.5, beta: float = 0.5, gamma: float = 1.0, smooth: float = 1.0,
                 focal_gamma: float = 0.0, focal_alpha=None, region_weight: float = 1.0, voxel_weight: float = 0.0,
                 per_sample: bool = False):
        super().__init__()
        _validate(alpha, beta, gamma, smooth, focal_gamma, focal_alpha, region_weight, voxel_weight)
        self.alpha, self.beta, self.gamma, self.smooth = alpha, beta, gamma, smooth
        self.focal_gamma, self.focal_alpha = focal_gamma, focal_alpha
        self.region_weight, self.voxel_weight = region_weight, voxel_weight
        self.per_sample = bool(per_sample)

    def forward(self, pred, target):
        _check(pred, target)
        return _RegionVoxelFunction.apply(pred, target, (
            self.alpha, self.beta, self.gamma, self.smooth, self.focal_gamma, self.focal_alpha, self.region_weight,
            self.voxel_weight, self.per_sample))


class TverskyLoss(RegionVoxelLoss):
    """1 - TI with TI = (I + s) / (I + alpha FP + beta FN + s) (Salehi et al. 2017); beta > alpha
    weights missed voxels over false alarms."""

    def __init__(self, alpha: float = 0.3, beta: float = 0.7, smooth: float = 1.0, per_sample: bool = False):
        super().__init__(alpha=alpha, beta=beta, smooth=smooth, per_sample=per_sample)


class FocalTverskyLoss(RegionVoxelLoss):
    """(1 - TI) ** gamma (Abraham & Khan 2019; gamma < 1 raises the gradient of nearly-solved
    groups, gamma > 1 focuses on the badly segmented ones)."""

    def __init__(self, alpha: float = 0.3, beta: float = 0.7, gamma: float = 0.75, smooth: float = 1.0,
                 per_sample: bool = False):
        super().__init__(alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, per_sample=per_sample)


class FocalLoss(RegionVoxelLoss):
    """The voxel term only: torchvision's ``sigmoid_focal_loss(pred, target, alpha, gamma,
    reduction='mean')`` (Lin et al. 2017); ``alpha=None`` switches the class weight off."""

    def __init__(self, gamma: float = 2.0, alpha=0.25):
        super().__init__(focal_gamma=gamma, focal_alpha=alpha, region_weight=0.0, voxel_weight=1.0)


class FocalTverskyFocalLoss(RegionVoxelLoss):
    """The compound form: region_weight * focal-Tversky + voxel_weight * focal."""

    def __init__(self, region_weight: float = 0.5, voxel_weight: float = 0.5, alpha: float = 0.3, beta: float = 0.7,
                 gamma: float = 0.75, smooth: float = 1.0, focal_gamma: float = 2.0, focal_alpha=0.25,
                 per_sample: bool = False):
        super().__init__(alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, focal_gamma=focal_gamma,
                         focal_alpha=focal_alpha, region_weight=region_weight, voxel_weight=voxel_weight,
                         per_sample=per_sample)


class SoftmaxDiceCELoss(nn.Module):
    """``ce_weight`` * softmax cross-entropy + ``dice_weight`` * mean per-class Dice loss for mutually
    exclusive classes: ``pred`` is ``(N, C, D, H, W)`` logits (2 <= C <= 8), ``target`` the class map
    ``(N, 1, D, H, W)`` or ``(N, D, H, W)``, fp32 or uint8, read by the kernel as it is.  A voxel
    whose label is not an integer in [0, C) is ignored (``ignore_index`` for free, e.g. 255).
    ``class_weights`` (C weights >= 0) are ``F.cross_entropy``'s ``weight``; the Dice mean leaves the
    background class out unless ``include_background``; ``per_sample=True`` takes the Dice sums per
    sample instead of over the batch.  ``classes.softmax_dice_ce_loss_host`` is the definition.

    Two launches forward, one backward, no host sync, fixed-order sums (the same bits on every
    run).  Under data parallelism the loss stays per replica."""

    def __init__(self, ce_weight: float = 0.5, dice_weight: float = 0.5, smooth: float = 1.0, class_weights=None,
                 include_background: bool = False, per_sample: bool = False):
        super().__init__()
        _validate_loss(ce_weight, dice_weight, smooth, class_weights)
        self.ce_weight, self.dice_weight, self.smooth = ce_weight, dice_weight, smooth
        self.class_weights = None if class_weights is None else tuple(float(w) for w in class_weights)
        self.include_background, self.per_sample = bool(include_background), bool(per_sample)

    def forward(self, pred, target):
        return softmax_dice_ce_loss(pred, target, self.ce_weight, self.dice_weight, self.smooth, self.class_weights,
                                    self.include_background, self.per_sample)


# config["loss"] names of utils/trainer.py
LOSSES = {"dice": DiceLoss, "bce_dice": BCEDiceLoss, "tversky": TverskyLoss, "focal_tversky": FocalTverskyLoss,
          "focal": FocalLoss, "focal_tversky_focal": FocalTverskyFocalLoss, "softmax_dice_ce": SoftmaxDiceCELoss}


def create_criterion(loss="dice", loss_args=None):
    """The criterion of a trainer config: ``loss`` a name of ``LOSSES`` (constructed with
    ``loss_args``, a dict) or an ``nn.Module`` instance, used as it is.  Unknown: ValueError."""
    if isinstance(loss, nn.Module):
        if loss_args:
            raise ValueError("loss_args given with a loss module instance")
        return loss
    if not isinstance(loss, str) or loss not in LOSSES:
        raise ValueError(f"unknown loss {loss!r}: one of {sorted(LOSSES)} or an nn.Module")
    return LOSSES[loss](**dict(loss_args or {}))
