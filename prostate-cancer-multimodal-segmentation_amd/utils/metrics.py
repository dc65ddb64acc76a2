"""Validation metrics and the evaluation loop (reference
script/validate_model.py:24-95 metrics, :188-274 per-case evaluation).

Binary masks come from ``UNet3D.inference`` (HIP eval forward: BatchNorm from running stats,
``sigmoid > threshold`` in the head kernel); the two overlap scores are small reductions over those
masks, done where the masks live (device tensors, no host round trip per voxel).
"""
from __future__ import annotations

import json
import os
from datetime import datetime
import math
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .. import classes, distance, lesions
from ..data import device_batch, get_dataloader


def calculate_dice_score(pred: torch.Tensor, target: torch.Tensor) -> float:
    """2|X∩Y| / (|X| + |Y| + 1e-8) over all voxels (validate_model.py:24-50)."""
    p, t = pred.reshape(-1).float(), target.reshape(-1).float()
    inter = (p * t).sum()
    return float((2.0 * inter) / (p.sum() + t.sum() + 1e-8))


def calculate_iou(pred: torch.Tensor, target: torch.Tensor) -> float:
    """|X∩Y| / (|X∪Y| + 1e-8) (validate_model.py:53-80)."""
    p, t = pred.reshape(-1).float(), target.reshape(-1).float()
    inter = (p * t).sum()
    union = p.sum() + t.sum() - inter
    return float(inter / (union + 1e-8))


def calculate_class_scores(pred, target, n_classes: int) -> Dict:
    """Per-class overlap of two class maps of one shape: ``{"dice": [..], "iou": [..]}``, one entry
    per class ``c < n_classes`` -- ``2|X∩Y| / (|X| + |Y|)`` and ``|X∩Y| / |X∪Y|`` of ``pred == c``
    against ``target == c``, a class absent from both maps scoring 1.0 -- plus ``mean_dice`` /
    ``mean_iou`` over the foreground classes ``1 .. n_classes - 1``.  CUDA tensors are counted on
    the device (pcms_class_overlap: exact integer counts), numpy arrays by the host form; a CPU
    tensor raises, as everywhere in pcms_amd."""
    if isinstance(pred, np.ndarray) and isinstance(target, np.ndarray):
        counts = classes.class_overlap(pred, target, n_classes)
    elif isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor):
        p, t = (m.to(torch.uint8) if m.device.type == "cuda" else m for m in (pred, target))
        counts = classes.class_overlap_device(p, t, n_classes).cpu().numpy()
    else:
        raise TypeError("pred and target are both CUDA tensors or both numpy arrays, got "
                        f"{type(pred).__name__} and {type(target).__name__}")
    dice, iou = classes.scores_of_counts(counts)
    fg = max(len(dice) - 1, 1)
    return {"dice": dice, "iou": iou, "mean_dice": sum(dice[1:]) / fg, "mean_iou": sum(iou[1:]) / fg}


def _as_volume(m):
    """A mask as a (D, H, W) volume: leading dimensions of size 1 (the channel of ``mask[i]`` at
    the Dice call sites) are squeezed away."""
    while m.ndim > 3 and m.shape[0] == 1:
        m = m[0]
    if m.ndim != 3:
        raise ValueError(f"a mask is a (D, H, W) volume, optionally behind dimensions of size 1; got {tuple(m.shape)}")
    return m


def calculate_surface_metrics(pred, target, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> Dict:
    """Boundary metrics of two binary masks (foreground ``!= 0``) in the units of ``spacing =
    (sz, sy, sx)``: ``hd`` (Hausdorff distance), ``hd95`` (its 95th percentile, MedPy's), ``assd``
    (average symmetric surface distance), ``n_a`` / ``n_b`` (surface voxels of pred / target).
    CUDA tensors are scored on the device (distance.surface_metrics_device: exact distance
    transform in HIP), numpy arrays by the host form (distance.surface_metrics); a CPU tensor
    raises, as everywhere in pcms_amd.  Both surfaces empty: 0.0; exactly one empty: inf."""
    if isinstance(pred, np.ndarray) and isinstance(target, np.ndarray):
        return distance.surface_metrics(_as_volume(pred), _as_volume(target), spacing)
    if isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor):
        p, t = ((_as_volume(m) != 0).to(torch.uint8) if m.device.type == "cuda" else m for m in (pred, target))
        return distance.surface_metrics_device(p, t, spacing)
    raise TypeError("pred and target are both CUDA tensors or both numpy arrays, got "
                    f"{type(pred).__name__} and {type(target).__name__}")


def calculate_lesion_metrics(pred, target, spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26,
                             min_iou: float = 0.1) -> Dict:
    """Lesion-level detection scores of two binary masks (foreground ``!= 0``): connected
    components at ``connectivity`` matched one to one at ``min_iou`` (lesions.lesion_metrics has
    the definition and the keys: ``tp`` / ``fp`` / ``fn`` / ``sensitivity`` / ``precision`` / ``f1``
    and the per-lesion tables).  CUDA tensors are scored on the device
    (lesions.lesion_metrics_device), numpy arrays by the host form; a CPU tensor raises."""
    if isinstance(pred, np.ndarray) and isinstance(target, np.ndarray):
        return lesions.lesion_metrics(_as_volume(pred), _as_volume(target), None, spacing, connectivity, min_iou)
    if isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor):
        p, t = ((_as_volume(m) != 0).to(torch.uint8) if m.device.type == "cuda" else m for m in (pred, target))
        return lesions.lesion_metrics_device(p, t, None, spacing, connectivity, min_iou)
    raise TypeError("pred and target are both CUDA tensors or both numpy arrays, got "
                    f"{type(pred).__name__} and {type(target).__name__}")


def calculate_hd95(pred, target, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> float:
    """The 95th-percentile Hausdorff distance (``calculate_surface_metrics``'s ``hd95``)."""
    return calculate_surface_metrics(pred, target, spacing)["hd95"]


def calculate_assd(pred, target, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> float:
    """The average symmetric surface distance (``calculate_surface_metrics``'s ``assd``)."""
    return calculate_surface_metrics(pred, target, spacing)["assd"]


@torch.no_grad()
def evaluate(model, loader: Iterable, threshold: float = 0.5, device=None, surface_metrics: bool = False,
             spacing: Sequence[float] = (1.0, 1.0, 1.0), lesion_metrics: bool = False, min_iou: float = 0.1,
             connectivity: int = 26, n_classes: int = 1) -> Dict:
    """Per-case Dice / IoU of ``model.inference`` masks against binarised labels, and their
    means (the ModelValidator loop, validate_model.py:226-274, one case per batch item).  With
    ``surface_metrics=True`` every case also carries ``hd95`` / ``assd`` / ``hd`` at ``spacing``
    (z, y, x; ``calculate_surface_metrics`` on the device) and the result ``mean_hd95`` /
    ``mean_assd`` over the ``surface_cases`` cases where they are finite.  With
    ``lesion_metrics=True`` every case also carries ``lesion_tp`` / ``lesion_fp`` / ``lesion_fn``
    (``calculate_lesion_metrics`` at ``connectivity`` and ``min_iou``) and the result their sums
    over the cases as ``lesion_tp`` / ``lesion_fp`` / ``lesion_fn``, ``lesion_sensitivity`` =
    tp / (tp + fn), ``lesion_precision`` = tp / (tp + fp), ``lesion_f1`` = 2 tp / (2 tp + fp + fn)
    (nan where the denominator is 0) and ``mean_fp_per_case``.
    ``n_classes > 1`` (a model with that many logit planes, labels that are class maps): the mask
    of a case is the class of its largest logit (pcms_probs_to_labels on the training grid, the
    first maximum on a tie; ``threshold`` is unused); a case carries ``class_dice`` / ``class_iou``
    (``calculate_class_scores``), its ``dice`` / ``iou`` are their means over the foreground
    classes, and the surface and lesion metrics run per foreground class on ``mask == c`` against
    ``label == c`` through the same functions: ``hd95`` / ``assd`` / ``hd`` become lists with one
    entry per foreground class (the means run over the finite (case, class) pairs) and the lesion
    counts are summed over the classes."""
    device = device or next(model.parameters()).device
    model.eval()
    if classes.check_n_classes(n_classes) > 1:
        return _evaluate_classes(model, loader, device, n_classes, surface_metrics, spacing, lesion_metrics, min_iou,
                                 connectivity)
    cases: List[Dict] = []
    for batch in loader:
        batch = device_batch(batch, device)
        x = batch["image"].to(device, non_blocking=True)
        y = batch["label"].to(device, non_blocking=True)
        mask = model.inference(x, threshold=threshold)
        ids = batch.get("case_id", [str(len(cases) + i) for i in range(x.shape[0])])
        for i in range(x.shape[0]):
            cases.append({"case_id": ids[i], "dice": calculate_dice_score(mask[i], y[i]),
                          "iou": calculate_iou(mask[i], y[i])})
            if surface_metrics:
                m = calculate_surface_metrics(mask[i], y[i], spacing)
                cases[-1].update(hd95=m["hd95"], assd=m["assd"], hd=m["hd"])
            if lesion_metrics:
                m = calculate_lesion_metrics(mask[i], y[i], spacing, connectivity, min_iou)
                cases[-1].update(lesion_tp=m["tp"], lesion_fp=m["fp"], lesion_fn=m["fn"])
    n = max(len(cases), 1)
    result = {"cases": cases, "mean_dice": sum(c["dice"] for c in cases) / n,
              "mean_iou": sum(c["iou"] for c in cases) / n}
    if surface_metrics:
        finite = [c for c in cases if math.isfinite(c["hd95"]) and math.isfinite(c["assd"])]
        k = max(len(finite), 1)
        result.update(mean_hd95=sum(c["hd95"] for c in finite) / k, mean_assd=sum(c["assd"] for c in finite) / k,
                      surface_cases=len(finite))
    if lesion_metrics:
        tp, fp, fn = (sum(c[k] for c in cases) for k in ("lesion_tp", "lesion_fp", "lesion_fn"))
        ratio = lambda num, den: num / den if den else float("nan")  # noqa: E731
        result.update(lesion_tp=tp, lesion_fp=fp, lesion_fn=fn, lesion_sensitivity=ratio(tp, tp + fn),
                      lesion_precision=ratio(tp, tp + fp), lesion_f1=ratio(2 * tp, 2 * tp + fp + fn),
                      mean_fp_per_case=fp / n)
    return result


def _evaluate_classes(model, loader, device, n_classes, surface_metrics, spacing, lesion_metrics, min_iou,
                      connectivity) -> Dict:
    """``evaluate`` for ``n_classes > 1`` (its docstring has the keys)."""
    cases: List[Dict] = []
    for batch in loader:
        batch = device_batch(batch, device)
        x = batch["image"].to(device, non_blocking=True)
        y = batch["label"].to(device, non_blocking=True)
        logits = model(x).float().contiguous()
        grid = tuple(logits.shape[2:])
        ids = batch.get("case_id", [str(len(cases) + i) for i in range(x.shape[0])])
        for i in range(x.shape[0]):
            mask, _ = classes.labels_on_grid_device(logits[i], grid)  # softmax is monotone: the same argmax
            lab = _as_volume(y[i]).to(torch.uint8)
            s = calculate_class_scores(mask, lab, n_classes)
            case = {"case_id": ids[i], "dice": s["mean_dice"], "iou": s["mean_iou"], "class_dice": s["dice"],
                    "class_iou": s["iou"]}
            pairs = [((mask == c).to(torch.uint8), (lab == c).to(torch.uint8)) for c in range(1, n_classes)] \
                if surface_metrics or lesion_metrics else []
            if surface_metrics:
                ms = [calculate_surface_metrics(p, t, spacing) for p, t in pairs]
                case.update(hd95=[m["hd95"] for m in ms], assd=[m["assd"] for m in ms], hd=[m["hd"] for m in ms])
            if lesion_metrics:
                ms = [calculate_lesion_metrics(p, t, spacing, connectivity, min_iou) for p, t in pairs]
                case.update(lesion_tp=sum(m["tp"] for m in ms), lesion_fp=sum(m["fp"] for m in ms),
                            lesion_fn=sum(m["fn"] for m in ms))
            cases.append(case)
    n = max(len(cases), 1)
    result = {"cases": cases, "mean_dice": sum(c["dice"] for c in cases) / n,
              "mean_iou": sum(c["iou"] for c in cases) / n,
              "mean_class_dice": [sum(c["class_dice"][k] for c in cases) / n for k in range(n_classes)],
              "mean_class_iou": [sum(c["class_iou"][k] for c in cases) / n for k in range(n_classes)]}
    if surface_metrics:
        finite = [(h, a) for c in cases for h, a in zip(c["hd95"], c["assd"]) if math.isfinite(h) and math.isfinite(a)]
        k = max(len(finite), 1)
        result.update(mean_hd95=sum(h for h, _ in finite) / k, mean_assd=sum(a for _, a in finite) / k,
                      surface_cases=len(finite))
    if lesion_metrics:
        tp, fp, fn = (sum(c[k] for c in cases) for k in ("lesion_tp", "lesion_fp", "lesion_fn"))
        ratio = lambda num, den: num / den if den else float("nan")  # noqa: E731
        result.update(lesion_tp=tp, lesion_fp=fp, lesion_fn=fn, lesion_sensitivity=ratio(tp, tp + fn),
                      lesion_precision=ratio(tp, tp + fp), lesion_f1=ratio(2 * tp, 2 * tp + fp + fn),
                      mean_fp_per_case=fp / n)
    return result


class ModelValidator:
    """script/validate_model.py:98-274: load a checkpoint (either form), run the test loader
    through ``UNet3D.inference`` (HIP eval forward, sigmoid > 0.5 in the head kernel), per-case
    Dice / IoU, and write ``validation_results.json`` to ``config['save_dir']`` with the
    reference's keys (timestamp, avg_dice, avg_iou, case_count, case_results).  With
    ``config['surface_metrics']`` (default False) the cases are also scored by ``hd95`` / ``assd``
    / ``hd`` at ``config['spacing']`` ((z, y, x), default (1, 1, 1)) and the JSON gains
    ``avg_hd95`` and ``avg_assd``.  ``config['n_classes']`` (default 1) with ``config['class_values']``:
    a model of that many logit planes scored per class (``evaluate``'s ``n_classes``); the JSON
    gains ``avg_class_dice`` and ``avg_class_iou``."""

    def __init__(self, config: dict, model=None, test_loader: Optional[Iterable] = None):
        from ..models.unet3d import UNet3D, load_weights
        self.config = config
        self.device = torch.device(config.get("device", "cuda"))
        if model is None:
            model = UNet3D(n_modalities=5, n_classes=config.get("n_classes", 1),
                           precision=config.get("precision", "bf16")).to(self.device)
            if config.get("model_path"):
                load_weights(model, config["model_path"])
        self.model = model
        self.model.eval()
        if test_loader is None and config.get("data_dir"):
            test_loader = get_dataloader(config["data_dir"], batch_size=config.get("batch_size", 1), shuffle=False,
                                         missing_strategy=config.get("handle_missing_modalities", "zero_fill"),
                                         target_size=tuple(config.get("target_size", (128, 128, 128))),
                                         is_training=False, data_type=config.get("data_type", "BPH"),
                                         n_classes=config.get("n_classes", 1), class_values=config.get("class_values"))
        self.test_loader = test_loader

    def validate(self):
        surface = bool(self.config.get("surface_metrics", False))
        r = evaluate(self.model, self.test_loader, threshold=0.5, device=self.device, surface_metrics=surface,
                     spacing=tuple(self.config.get("spacing", (1.0, 1.0, 1.0))),
                     n_classes=self.config.get("n_classes", 1))
        results = {"timestamp": datetime.now().strftime("%Y-%m-%d %H:%M:%S"), "avg_dice": r["mean_dice"],
                   "avg_iou": r["mean_iou"], "case_count": len(r["cases"]), "case_results": r["cases"]}
        if surface:
            results.update(avg_hd95=r["mean_hd95"], avg_assd=r["mean_assd"])
        if "mean_class_dice" in r:
            results.update(avg_class_dice=r["mean_class_dice"], avg_class_iou=r["mean_class_iou"])
        save_dir = self.config.get("save_dir")
        if save_dir:
            os.makedirs(save_dir, exist_ok=True)
            with open(os.path.join(save_dir, "validation_results.json"), "w", encoding="utf-8") as f:
                json.dump(results, f, ensure_ascii=False, indent=2)
        return r["mean_dice"], r["mean_iou"]
