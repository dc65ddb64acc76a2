"""Mutually exclusive classes (csrc/classes.hip): host forms, then the device forms.

A *class map* holds one class index per voxel, 0 the background; the network emits ``C`` logit
planes and a voxel belongs to the class of its largest softmax probability.

* ``softmax_dice_ce_loss_host``: the definition of ``utils.losses.SoftmaxDiceCELoss`` in fp64 torch
  on the CPU; ``softmax_dice_ce_loss`` runs it on pcms_softmax_loss_fwd / _bwd.
* ``classes_of``: the class-map label of a resampled label volume through a value table;
  ``resample.resample_device(..., nearest=True, class_values=...)`` forms it from raw NIfTI bytes
  (pcms_resample_classes / pcms_resample_affine_classes), byte for byte.
* ``labels_on_grid``: class probabilities on the training grid -> the class map on the native grid
  (per-class ``resample.resample``, then the first maximum); ``softmax_planes_device`` and
  ``labels_on_grid_device`` are pcms_softmax_planes and pcms_probs_to_labels.
* ``class_overlap``: per-class voxel counts of two class maps; ``class_overlap_device`` is
  pcms_class_overlap.  ``scores_of_counts`` turns them into per-class Dice and IoU.
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence, Tuple

import numpy as np
import torch

from ._args import device_tensor, host_floats
from ._lib import call, query
from .resample import resample

MAX_CLASSES = 8  # the kernels are instantiated for 2..8 logit planes; a value table holds 7 entries


def check_n_classes(n_classes) -> int:
    if isinstance(n_classes, bool) or not isinstance(n_classes, int) or not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"n_classes is an integer in 1..{MAX_CLASSES}, got {n_classes!r}")
    return n_classes


def class_values_of(n_classes: int, class_values=None) -> Tuple[float, ...]:
    """The label-file values of the foreground classes 1 .. n_classes - 1 (default ``(1, ..,
    n_classes - 1)``): ``n_classes - 1`` distinct finite numbers that fp32 holds exactly."""
    n = check_n_classes(n_classes)
    if n < 2:
        raise ValueError("a class table needs n_classes >= 2")
    values = tuple(float(v) for v in (range(1, n) if class_values is None else class_values))
    if len(values) != n - 1 or len(set(values)) != len(values):
        raise ValueError(f"class_values holds {n - 1} distinct values for n_classes={n}, got {values}")
    if any(not math.isfinite(v) or float(np.float32(v)) != v for v in values):
        raise ValueError(f"class_values must be finite and exact in fp32, got {values}")
    return values


# ---- the loss ---------------------------------------------------------------------------------
def _validate_loss(ce_weight, dice_weight, smooth, class_weights, n_classes=None):
    """The rules of pcms_softmax_loss_fwd's argument checks, as ValueError."""
    for k, v in (("ce_weight", ce_weight), ("dice_weight", dice_weight), ("smooth", smooth)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{k} must be a finite number, got {v!r}")
    if smooth < 0:
        raise ValueError(f"smooth must be >= 0, got {smooth}")
    if class_weights is not None:
        w = [float(v) for v in class_weights]
        if not 2 <= len(w) <= MAX_CLASSES or any(not math.isfinite(v) or v < 0 for v in w):
            raise ValueError(f"class_weights holds 2..{MAX_CLASSES} finite weights >= 0, got {class_weights!r}")
        if n_classes is not None and len(w) != n_classes:
            raise ValueError(f"class_weights holds {len(w)} weights for {n_classes} classes")


def _loss_shapes(pred, target):
    """(N, C, nvox) of ``pred`` (N, C, ...) after checking ``target`` (N, 1, ...) or (N, ...)."""
    if pred.dim() < 3 or not 2 <= int(pred.shape[1]) <= MAX_CLASSES:
        raise ValueError(f"pred is (N, C, ...) logits with 2 <= C <= {MAX_CLASSES}, got shape {tuple(pred.shape)}")
    n, c = int(pred.shape[0]), int(pred.shape[1])
    want = (n,) + tuple(pred.shape[2:])
    if tuple(target.shape) not in (want, (n, 1) + tuple(pred.shape[2:])):
        raise ValueError(f"预测值和目标值的形状不匹配: pred.shape={tuple(pred.shape)}, target.shape={tuple(target.shape)} "
                         f"(a class map is {want} or (N, 1, ...))")
    return n, c, int(np.prod(pred.shape[2:], dtype=np.int64))


def softmax_dice_ce_loss_host(pred, target, ce_weight=0.5, dice_weight=0.5, smooth=1.0, class_weights=None,
                              include_background=False, per_sample=False):
    """The definition of ``SoftmaxDiceCELoss`` in fp64 torch on the CPU, differentiable by autograd
    with respect to ``pred`` (N, C, ...): what the kernels are tested against.  ``target`` is a
    class map (N, 1, ...) or (N, ...); a voxel whose label is not an integer in [0, C) is ignored.
    With p = softmax_c(pred), y the one-hot label, over the valid voxels of a group g (the batch, or
    one sample with ``per_sample``):

        I_c = sum p_c y_c,  P_c = sum p_c,  T_c = sum y_c,  dice_c = (2 I_c + s) / (P_c + T_c + s)
        region_g = mean_{c in K} (1 - dice_c),   K = {1..C-1}, or {0..C-1} with include_background
        CE = sum_i w[y_i] (-log p_{y_i}) / sum_i w[y_i] over the batch's valid voxels (0 without one)
        loss = ce_weight * CE + dice_weight * mean_g region_g

    (``dice_c`` is 1 where its denominator is not positive: ``smooth=0`` on an empty group.)"""
    n, C, nvox = _loss_shapes(pred, target)
    _validate_loss(ce_weight, dice_weight, smooth, class_weights, C)
    x = pred.to(device="cpu", dtype=torch.float64).reshape(n, C, nvox)
    t = target.detach().to(device="cpu", dtype=torch.float64).reshape(n, nvox)
    valid = (t >= 0) & (t < C) & (t == torch.floor(t))
    y = torch.where(valid, t, torch.zeros_like(t)).long()
    v = valid.to(torch.float64)
    logp = torch.log_softmax(x, dim=1)
    p = torch.exp(logp) * v[:, None]
    onehot = torch.zeros_like(x).scatter_(1, y[:, None], 1.0) * v[:, None]
    groups = n if per_sample else 1
    pg, og = (a.transpose(0, 1).reshape(C, groups, -1) for a in (p, onehot))
    I, P, T = (pg * og).sum(2), pg.sum(2), og.sum(2)  # (C, groups)
    den = P + T + smooth
    ok = den > 0
    dice = torch.where(ok, (2.0 * I + smooth) / torch.where(ok, den, torch.ones_like(den)), torch.ones_like(den))
    c0 = 0 if include_background else 1
    region = (1.0 - dice[c0:]).mean(0)
    w = torch.ones(C, dtype=torch.float64) if class_weights is None else \
        torch.tensor([float(a) for a in class_weights], dtype=torch.float64)
    wy = w[y] * v
    sw = wy.sum()
    ce = (wy * -logp.gather(1, y[:, None])[:, 0]).sum() / sw if float(sw) > 0 else x.sum() * 0.0
    return ce_weight * ce + dice_weight * region.mean()


class _SoftmaxLossFunction(torch.autograd.Function):
    """pcms_softmax_loss_fwd / _bwd; cfg = (ce_weight, dice_weight, smooth, class_weights or None,
    include_background, per_sample)."""

    @staticmethod
    def forward(ctx, pred, target, cfg):
        if pred.device.type != "cuda":
            raise RuntimeError("pcms_amd losses run on a ROCm device only (no CPU path)")
        wce, wd, smooth, weights, bg, per_sample = cfg
        n, C, nvox = _loss_shapes(pred, target)
        x = pred.detach().contiguous().float()
        t = target.detach().to(device=x.device)
        if t.dtype not in (torch.float32, torch.uint8):  # the kernel reads these two as they are
            t = t.to(torch.float32)
        t = t.contiguous()
        u8 = int(t.dtype == torch.uint8)
        groups = n if per_sample else 1
        rows = query("pcms_softmax_loss_rows", nvox, n)
        if rows < 1:
            raise ValueError(f"pcms_softmax_loss_rows({nvox}, {n}) = {rows}: empty input")
        K = 3 * C + 2
        part = torch.empty(n * rows * K, dtype=torch.float32, device=x.device)
        sums = torch.empty(groups * K, dtype=torch.float64, device=x.device)
        coef = torch.empty(groups * 2 * C + 1, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        host = None if weights is None else host_floats(weights)  # read during the calls: kept in ctx
        wptr = None if host is None else ctypes.addressof(host)
        call("pcms_softmax_loss_fwd", x, t, u8, nvox, n, C, int(per_sample), int(bg), float(smooth), float(wce),
             float(wd), wptr, part, sums, coef, loss)
        ctx.save_for_backward(x, t, coef)
        ctx.cfg = (u8, nvox, n, C, int(per_sample), host)
        ctx.shape, ctx.dtype = pred.shape, pred.dtype
        return loss

    @staticmethod
    def backward(ctx, gout):
        x, t, coef = ctx.saved_tensors
        u8, nvox, n, C, per_sample, host = ctx.cfg
        dx = torch.empty_like(x)
        g = gout.detach().contiguous().float()
        call("pcms_softmax_loss_bwd", x, t, u8, nvox, n, C, per_sample, None if host is None else ctypes.addressof(host),
             coef, g, dx)
        return dx.view(ctx.shape).to(ctx.dtype), None, None


def softmax_dice_ce_loss(pred, target, ce_weight=0.5, dice_weight=0.5, smooth=1.0, class_weights=None,
                         include_background=False, per_sample=False):
    """``softmax_dice_ce_loss_host`` on the GPU (pcms_softmax_loss_fwd / _bwd): two launches
    forward, one backward, no host synchronisation, the same bits on every run.  ``target`` is read
    as it is when fp32 or uint8 (any other dtype is converted to fp32 first)."""
    n, C, _ = _loss_shapes(pred, target)
    _validate_loss(ce_weight, dice_weight, smooth, class_weights, C)
    weights = None if class_weights is None else tuple(float(v) for v in class_weights)
    return _SoftmaxLossFunction.apply(pred, target, (ce_weight, dice_weight, smooth, weights, bool(include_background),
                                                     bool(per_sample)))


# ---- class-map labels --------------------------------------------------------------------------
def classes_of(values, class_values: Sequence[float]) -> np.ndarray:
    """A resampled label volume -> its class map, fp32: ``j + 1`` where ``float32(value) ==
    class_values[j]`` (the first such j), 0 everywhere else -- values the table does not name are
    background."""
    v = np.asarray(values).astype(np.float32)
    table = [np.float32(c) for c in class_values]
    if not 1 <= len(table) <= MAX_CLASSES - 1 or not all(np.isfinite(table)):
        raise ValueError(f"class_values holds 1..{MAX_CLASSES - 1} finite values, got {tuple(class_values)!r}")
    out = np.zeros(v.shape, dtype=np.float32)
    for j in reversed(range(len(table))):
        out[v == table[j]] = np.float32(j + 1)
    return out


# ---- prediction ----------------------------------------------------------------------------------
def labels_on_grid(probs, native_shape: Sequence[int]):
    """Class probabilities (C, D, H, W) on the training grid -> ``(uint8 class map, float32
    probabilities (C, ...))`` on the ``native_shape`` grid: ``resample.resample`` of every class
    plane (``predict.mask_on_grid``'s geometry), then ``np.argmax`` over the classes -- the first
    maximum wins, so a voxel past the volume's edge (every plane 0) is background."""
    probs = np.asarray(probs)
    if probs.ndim != 4 or not 1 <= probs.shape[0] <= MAX_CLASSES:
        raise ValueError(f"labels_on_grid takes (C, D, H, W) probabilities with C <= {MAX_CLASSES}, got {probs.shape}")
    native = np.stack([resample(p.astype(np.float32), tuple(int(v) for v in native_shape)) for p in probs], axis=0)
    return np.argmax(native, axis=0).astype(np.uint8), native


def softmax_planes_device(logits: torch.Tensor) -> torch.Tensor:
    """(B, C, ...) fp32 logits on the GPU -> class-major probabilities (C, B, ...): pcms_softmax_planes."""
    if not isinstance(logits, torch.Tensor) or logits.device.type != "cuda":
        raise RuntimeError("softmax_planes_device needs a tensor on the GPU: pcms_amd has no CPU fallback")
    if logits.dim() < 3 or not 2 <= int(logits.shape[1]) <= MAX_CLASSES or logits.numel() == 0:
        raise ValueError(f"logits are (B, C, ...) with 2 <= C <= {MAX_CLASSES}, got shape {tuple(logits.shape)}")
    x = logits.detach().float().contiguous()
    B, C = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((C, B) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    call("pcms_softmax_planes", x, B, C, x[0, 0].numel(), out)
    return out


def labels_on_grid_device(probs: torch.Tensor, native_shape: Sequence[int], return_probability: bool = False):
    """``labels_on_grid`` on the GPU, byte for byte (pcms_probs_to_labels): ``(uint8 class map,
    fp32 (C, ...) probabilities or None)`` on the native grid, on the current stream."""
    probs = device_tensor(probs, torch.float32, 4, "labels_on_grid_device")
    if int(probs.shape[0]) > MAX_CLASSES:
        raise ValueError(f"labels_on_grid_device takes at most {MAX_CLASSES} class planes, got {probs.shape[0]}")
    native = tuple(int(v) for v in native_shape)
    labels = torch.empty(native, dtype=torch.uint8, device=probs.device)
    planes = torch.empty((int(probs.shape[0]),) + native, dtype=torch.float32, device=probs.device) \
        if return_probability else None
    call("pcms_probs_to_labels", probs, int(probs.shape[0]), *probs.shape[1:], labels, planes, *native)
    return labels, planes


# ---- per-class overlap ---------------------------------------------------------------------------
def class_overlap(pred, ref, n_classes: int) -> np.ndarray:
    """``counts[c] = (|pred == c|, |ref == c|, |pred == c and ref == c|)`` for ``c < n_classes``,
    int64 (n_classes, 3), of two class maps of one shape."""
    n = check_n_classes(n_classes)
    p, r = np.asarray(pred), np.asarray(ref)
    if p.shape != r.shape or p.size == 0:
        raise ValueError(f"class_overlap takes two non-empty class maps of one shape, got {p.shape} and {r.shape}")
    return np.array([[np.count_nonzero(p == c), np.count_nonzero(r == c), np.count_nonzero((p == c) & (r == c))]
                     for c in range(n)], dtype=np.int64)


def class_overlap_device(pred: torch.Tensor, ref: torch.Tensor, n_classes: int) -> torch.Tensor:
    """``class_overlap`` of two uint8 class maps on the GPU (pcms_class_overlap): an int64
    (n_classes, 3) device tensor, exact, on the current stream."""
    n = check_n_classes(n_classes)
    for m in (pred, ref):
        if not isinstance(m, torch.Tensor) or m.device.type != "cuda":
            raise RuntimeError("class_overlap_device needs uint8 tensors on the GPU: pcms_amd has no CPU fallback -- "
                               "use class_overlap on the host")
    if pred.dtype != torch.uint8 or ref.dtype != torch.uint8 or pred.shape != ref.shape or pred.numel() == 0:
        raise ValueError(f"class_overlap_device takes two non-empty uint8 class maps of one shape, got {pred.dtype} "
                         f"{tuple(pred.shape)} and {ref.dtype} {tuple(ref.shape)}")
    counts = torch.empty((n, 3), dtype=torch.int64, device=pred.device)
    call("pcms_class_overlap", pred.contiguous(), ref.contiguous(), pred.numel(), n, counts)
    return counts


def scores_of_counts(counts) -> Tuple[list, list]:
    """Per-class ``(dice, iou)`` lists of a ``class_overlap`` table: ``2|X∩Y| / (|X| + |Y|)`` and
    ``|X∩Y| / |X∪Y|``; a class absent from both maps scores 1.0."""
    dice, iou = [], []
    for a, b, both in np.asarray(counts, dtype=np.int64).tolist():
        dice.append(1.0 if a + b == 0 else 2.0 * both / (a + b))
        iou.append(1.0 if a + b == 0 else both / (a + b - both))
    return dice, iou
