"""Lesion analysis (csrc/lesions.hip): host forms, then device forms.

``component_table`` / ``overlap_pairs`` / ``match_lesions`` / ``lesion_table`` / ``lesion_metrics``
are the host forms of the per-lesion table (voxels, box, centroid, peak probability) and of the
detection scores (one-to-one matching at an IoU threshold); ``component_table_device`` /
``overlap_pairs_device`` / ``lesion_table_device`` / ``lesion_metrics_device`` build the tables in
HIP kernels, on the bytes, and share the host arithmetic; ``ModelPredictor.predict_case(...,
return_lesions=True)`` and ``score_case(..., lesion_metrics=True)`` carry them.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._args import device_tensor, volume3
from ._lib import call, query
from .components import label_components, label_components_device
from .distance import _spacing


# ---- lesion analysis -------------------------------------------------------------
# A lesion candidate is a connected component; its confidence is the component's maximum
# probability; a hit is an overlap of at least ``min_iou`` IoU with a reference lesion.  The host
# forms below define what csrc/lesions.hip computes, on the bytes.
TABLE_CAPACITY = 4096


def _float_keys(prob: np.ndarray) -> np.ndarray:
    """uint32 keys whose unsigned order is the total order of the fp32 values' bits:
    ``bits ^ (sign ? 0xFFFFFFFF : 0x80000000)``, so -0.0 < +0.0 and a positive NaN is above +inf."""
    bits = np.ascontiguousarray(prob, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _decode_peak_keys(packed: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(peak float32, peak_index int32) of ``(key << 32) | ~index`` words."""
    key = (packed >> np.uint64(32)).astype(np.uint32)
    bits = np.where(key >> 31 != 0, key ^ np.uint32(0x80000000), ~key)
    index = (~(packed & np.uint64(0xFFFFFFFF)).astype(np.uint32)).view(np.int32)
    return bits.astype(np.uint32).view(np.float32), index


def component_table(labels: np.ndarray, prob: Optional[np.ndarray] = None) -> dict:
    """One row per component of a canonical label volume (``label_components``' output: 0 on
    background, ``1 + the smallest flat index of the component`` elsewhere), in ascending label
    order, as a dict of arrays: ``label`` int32 (K,), ``voxels`` int32 (K,), ``bbox`` int32 (K, 6)
    = dmin, dmax, hmin, hmax, wmin, wmax (inclusive), ``index_sum`` int64 (K, 3) = the sums of
    d, h and w over the component, and with ``prob`` (fp32, the labels' shape) ``peak`` float32,
    the component's maximum probability, and ``peak_index`` int32, the smallest flat index
    attaining it.  The maximum is taken under the total order of the integer key
    ``bits ^ (sign ? 0xFFFFFFFF : 0x80000000)`` of the float's bits: -0.0 < +0.0, a
    positive-signed NaN is above +inf; that is the definition, not an error.  ValueError for a
    volume that is not canonical: a voxel with a negative label, or with a label ``L > 0`` where
    ``L - 1`` is outside the volume or ``labels.flat[L - 1] != L``.  A volume without foreground
    gives K = 0 and zero-length columns."""
    lab = volume3(labels)
    if lab.dtype.kind not in "iu":
        raise ValueError(f"labels are integers, got {lab.dtype}")
    shape, n = lab.shape, lab.size
    flat = lab.reshape(-1).astype(np.int64)
    fg = np.flatnonzero(flat != 0)
    L = flat[fg]
    if (L < 0).any() or (L > n).any() or (flat[np.clip(L - 1, 0, n - 1)] != L).any():
        raise ValueError("the label volume is not canonical: some voxel's label L is negative, past the volume, "
                         "or labels.flat[L - 1] != L")
    if prob is not None:
        prob = np.asarray(prob)
        if prob.shape != shape or prob.dtype != np.float32:
            raise ValueError(f"prob is float32 of shape {shape}, got {prob.dtype} {prob.shape}")
    K = 0
    table = {"label": np.zeros(0, np.int32), "voxels": np.zeros(0, np.int32), "bbox": np.zeros((0, 6), np.int32),
             "index_sum": np.zeros((0, 3), np.int64)}
    if prob is not None:
        table.update(peak=np.zeros(0, np.float32), peak_index=np.zeros(0, np.int32))
    if fg.size:
        uniq, inverse, counts = np.unique(L, return_inverse=True, return_counts=True)
        K = len(uniq)
        order = np.argsort(inverse, kind="stable")  # the voxels row by row
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        coords = [c[order].astype(np.int64) for c in np.unravel_index(fg, shape)]
        table["label"] = uniq.astype(np.int32)
        table["voxels"] = counts.astype(np.int32)
        table["bbox"] = np.stack([f.reduceat(c, starts) for c in coords for f in (np.minimum, np.maximum)],
                                 axis=1).astype(np.int32)
        table["index_sum"] = np.stack([np.add.reduceat(c, starts) for c in coords], axis=1).astype(np.int64)
        if prob is not None:
            packed = (_float_keys(prob).reshape(-1)[fg].astype(np.uint64) << np.uint64(32)) | \
                (~fg.astype(np.uint32)).astype(np.uint64)
            table["peak"], table["peak_index"] = _decode_peak_keys(np.maximum.reduceat(packed[order], starts))
    assert all(len(v) == K for v in table.values())
    return table


def overlap_pairs(labels_a: np.ndarray, labels_b: np.ndarray, connectivity: int = 26) -> np.ndarray:
    """The overlapping pairs of components of two canonical label volumes on one grid, int64
    (P, 3): rows ``(label_a, label_b, voxels in both)`` sorted by ``(label_a, label_b)``.
    Defined without a hash table, which is how the device computes it: the intersection mask
    ``(labels_a > 0) & (labels_b > 0)`` is labelled at ``connectivity``; ``component_table`` of that
    gives each intersection component's size and root voxel; its pair is ``(labels_a, labels_b)``
    read at the root; rows with the same pair are summed.
    Containment: two voxels adjacent at ``connectivity`` inside the intersection are foreground
    and adjacent on side a, so, a being labelled at a connectivity at least as permissive, they
    carry the same label_a; by induction along a path every intersection component lies inside
    exactly one component of a, and likewise of b, so the labels read at its root are those of
    all of its voxels.  Hence ``connectivity`` must not exceed the connectivity either side was
    labelled at: use the same one for all three."""
    a, b = volume3(labels_a), volume3(labels_b)
    if a.shape != b.shape:
        raise ValueError(f"the label volumes are on different grids: {a.shape} and {b.shape}")
    inter = label_components((a > 0) & (b > 0), connectivity)
    roots = component_table(inter)
    return _sum_pairs(a.reshape(-1)[roots["label"] - 1], b.reshape(-1)[roots["label"] - 1], roots["voxels"])


def _sum_pairs(la, lb, voxels) -> np.ndarray:
    """Rows (la, lb, sum of voxels) over the distinct (la, lb), sorted."""
    if len(voxels) == 0:
        return np.zeros((0, 3), np.int64)
    pairs = np.stack([np.asarray(la, np.int64), np.asarray(lb, np.int64)], axis=1)
    uniq, inverse = np.unique(pairs, axis=0, return_inverse=True)
    total = np.zeros(len(uniq), np.int64)
    np.add.at(total, inverse.reshape(-1), np.asarray(voxels, np.int64))
    return np.concatenate([uniq, total[:, None]], axis=1)


def _ratio(num: int, den: int) -> float:
    return num / den if den else float("nan")


def match_lesions(pred_table: dict, ref_table: dict, pairs: np.ndarray, min_iou: float = 0.1) -> dict:
    """Lesion-level detection scores from two ``component_table``s and ``overlap_pairs(pred
    labels, ref labels)``.  The IoU of a pair is ``inter / (vp + vr - inter)`` in fp64 from the
    exact integers; the candidates are the pairs with ``iou >= min_iou``; sorted by (iou
    descending, ref label ascending, pred label ascending) they are matched greedily one to one.
    Returns ``matches`` (a list of ``(ref_label, pred_label, inter, iou, dice)``, in match order),
    ``tp``, ``fp`` (unmatched predicted components), ``fn`` (unmatched reference components),
    ``sensitivity`` = tp / n_ref, ``precision`` = tp / n_pred, ``f1`` = 2 tp / (n_pred + n_ref)
    (each nan where its denominator is 0), ``n_pred`` and ``n_ref``."""
    vp = {int(k): int(v) for k, v in zip(pred_table["label"], pred_table["voxels"])}
    vr = {int(k): int(v) for k, v in zip(ref_table["label"], ref_table["voxels"])}
    candidates = []
    for lp, lr, inter in np.asarray(pairs, np.int64).reshape(-1, 3).tolist():
        iou = inter / (vp[lp] + vr[lr] - inter)
        if iou >= min_iou:
            candidates.append((-iou, lr, lp, inter))
    candidates.sort()
    used_p, used_r, matches = set(), set(), []
    for neg_iou, lr, lp, inter in candidates:
        if lp in used_p or lr in used_r:
            continue
        used_p.add(lp)
        used_r.add(lr)
        matches.append((lr, lp, inter, -neg_iou, 2.0 * inter / (vp[lp] + vr[lr])))
    tp, n_pred, n_ref = len(matches), len(vp), len(vr)
    return {"matches": matches, "tp": tp, "fp": n_pred - tp, "fn": n_ref - tp,
            "sensitivity": _ratio(tp, n_ref), "precision": _ratio(tp, n_pred), "f1": _ratio(2 * tp, n_pred + n_ref),
            "n_pred": n_pred, "n_ref": n_ref}


def _lesion_rows(table: dict, shape, sp) -> List[dict]:
    """``lesion_table``'s dicts from a component table (host arithmetic in fp64)."""
    K = len(table["label"])
    order = np.lexsort((table["label"], -table["voxels"].astype(np.int64)))  # voxels descending, label ascending
    rows = []
    for r in order.tolist() if K else []:
        voxels = int(table["voxels"][r])
        row = {"label": int(table["label"][r]), "voxels": voxels, "volume": voxels * sp[0] * sp[1] * sp[2],
               "bbox": tuple(int(v) for v in table["bbox"][r]),
               "centroid": tuple(float(s) / voxels for s in table["index_sum"][r].tolist()),
               "confidence": None, "peak_voxel": None}
        if "peak" in table:
            row["confidence"] = float(table["peak"][r])
            row["peak_voxel"] = tuple(int(v) for v in np.unravel_index(int(table["peak_index"][r]), shape))
        rows.append(row)
    return rows


def lesion_table(mask: np.ndarray, prob: Optional[np.ndarray] = None, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                 connectivity: int = 26) -> List[dict]:
    """The lesion candidates of a mask (foreground ``!= 0``), one dict per component at
    ``connectivity``, ordered by (voxels descending, label ascending): ``label``, ``voxels``,
    ``volume`` = ``voxels * sz * sy * sx``, ``bbox`` (dmin, dmax, hmin, hmax, wmin, wmax),
    ``centroid`` = index_sum / voxels as (z, y, x) in fp64, ``confidence`` = the component's peak
    of ``prob`` and ``peak_voxel`` = its (z, y, x); the last two are None without ``prob``."""
    sp = _spacing(spacing)
    lab = label_components(mask, connectivity)
    return _lesion_rows(component_table(lab, prob), lab.shape, sp)


def _lesion_report(tp, tr, pairs, shape, sp, min_iou) -> dict:
    scores = match_lesions(tp, tr, pairs, min_iou)
    matched = {lp: lr for lr, lp, _, _, _ in scores["matches"]}
    pred_rows = _lesion_rows(tp, shape, sp)
    for row in pred_rows:
        row["matched_ref"] = matched.get(row["label"])
    ref_table = {k: v for k, v in tr.items() if k not in ("peak", "peak_index")}
    scores.update(pred_lesions=pred_rows, ref_lesions=_lesion_rows(ref_table, shape, sp))
    return scores


def lesion_metrics(pred: np.ndarray, ref: np.ndarray, prob: Optional[np.ndarray] = None,
                   spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26, min_iou: float = 0.1) -> dict:
    """Lesion-level detection scores of a predicted mask against a reference mask (foreground
    ``!= 0``, same grid): ``match_lesions`` of the two masks' component tables and overlap pairs,
    plus ``pred_lesions`` and ``ref_lesions`` (``lesion_table`` of each; ``prob`` gives the
    predicted lesions their confidence), every predicted lesion carrying ``matched_ref``: the
    label of the reference lesion it was matched to, or None."""
    sp = _spacing(spacing)
    lp, lr = label_components(pred, connectivity), label_components(ref, connectivity)
    if lp.shape != lr.shape:
        raise ValueError(f"the masks are on different grids: {lp.shape} and {lr.shape}")
    return _lesion_report(component_table(lp, prob), component_table(lr), overlap_pairs(lp, lr, connectivity),
                          lp.shape, sp, min_iou)


def _table_enqueue(labels: torch.Tensor, prob: Optional[torch.Tensor], capacity: int):
    """(table bytes as int64, header) with pcms_component_table enqueued on the current stream."""
    nwork = query("pcms_component_table_work_bytes", *labels.shape)
    nbytes = query("pcms_component_table_bytes", int(capacity), int(prob is not None))
    if nwork < 0 or nbytes < 0:
        raise ValueError(f"a volume of shape {tuple(labels.shape)} or a table of {capacity} rows is too large")
    table = torch.empty(nbytes // 8, dtype=torch.int64, device=labels.device)
    header = torch.empty(2, dtype=torch.int32, device=labels.device)
    work = torch.empty(nwork // 4, dtype=torch.int32, device=labels.device)
    call("pcms_component_table", labels, prob, table, int(capacity), header, work, *labels.shape)
    return table, header


def _table_columns(raw: np.ndarray, capacity: int, K: int, with_prob: bool) -> dict:
    """The first K rows of pcms_component_table's bytes (include/pcms_hip.h has the layout)."""
    c = capacity
    col = lambda lo, hi, dtype: raw[lo * c:hi * c].view(dtype)  # noqa: E731
    table = {"label": col(24, 28, np.int32)[:K].copy(), "voxels": col(28, 32, np.int32)[:K].copy(),
             "bbox": col(32, 56, np.int32).reshape(c, 6)[:K].copy(),
             "index_sum": col(0, 24, np.int64).reshape(c, 3)[:K].copy()}
    if with_prob:
        table.update(peak=col(64, 68, np.float32)[:K].copy(), peak_index=col(68, 72, np.int32)[:K].copy())
    return table


def component_table_device(labels: torch.Tensor, prob: Optional[torch.Tensor] = None,
                           capacity: int = TABLE_CAPACITY) -> dict:
    """``component_table`` on the GPU, on the bytes (pcms_component_table): an int32 CUDA label
    volume (``label_components_device``'s) and optionally fp32 probabilities in, the host form's
    dict of numpy arrays out.  The table, the component count and the status travel in one
    device-to-host copy; with more than ``capacity`` components the launches run once more with
    ``capacity`` = that count.  RuntimeError for a label volume that is not canonical (the
    kernel's status word); CPU tensors raise."""
    labels = device_tensor(labels, torch.int32, 3, "component_table_device")
    if prob is not None:
        prob = device_tensor(prob, torch.float32, 3, "component_table_device")
        if prob.shape != labels.shape or prob.device != labels.device:
            raise ValueError(f"prob {tuple(prob.shape)} on {prob.device} is not on the labels' grid "
                             f"{tuple(labels.shape)} on {labels.device}")
    if not isinstance(capacity, (int, np.integer)) or capacity < 1:
        raise ValueError(f"capacity is an integer >= 1, got {capacity!r}")
    capacity = int(capacity)
    with torch.cuda.device(labels.device):
        for _ in range(2):  # the second turn only when the first reported more rows than it had room for
            table, header = _table_enqueue(labels, prob, capacity)
            raw = torch.cat([table.view(torch.uint8), header.view(torch.uint8)]).cpu().numpy()
            status, K = (int(v) for v in raw[-8:].view(np.int32))
            if status != 0:
                raise RuntimeError(f"component_table_device: the label volume is not canonical (status {status})")
            if K <= capacity:
                return _table_columns(raw[:-8], capacity, K, prob is not None)
            capacity = K
    raise RuntimeError(f"component_table_device: {K} components after sizing the table for as many")


def overlap_pairs_device(labels_a: torch.Tensor, labels_b: torch.Tensor, connectivity: int = 26) -> np.ndarray:
    """``overlap_pairs`` on the GPU, exactly: the intersection by a torch ``&``, its labels by
    pcms_components_label, its table by pcms_component_table, the two label volumes read at the
    roots by a torch gather; equal pairs are summed on the host.  CPU tensors raise."""
    a = device_tensor(labels_a, torch.int32, 3, "overlap_pairs_device")
    b = device_tensor(labels_b, torch.int32, 3, "overlap_pairs_device")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"the label volumes are on different grids or devices: {tuple(a.shape)} on {a.device} and "
                         f"{tuple(b.shape)} on {b.device}")
    with torch.cuda.device(a.device):
        inter = ((a > 0) & (b > 0)).to(torch.uint8)
        roots = component_table_device(label_components_device(inter, connectivity))
        if len(roots["label"]) == 0:
            return np.zeros((0, 3), np.int64)
        at = torch.from_numpy(roots["label"].astype(np.int64) - 1).to(a.device)
        both = torch.stack([a.reshape(-1)[at], b.reshape(-1)[at]]).cpu().numpy()
    return _sum_pairs(both[0], both[1], roots["voxels"])


def lesion_table_device(mask: torch.Tensor, prob: Optional[torch.Tensor] = None,
                        spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26) -> List[dict]:
    """``lesion_table`` on the GPU: pcms_components_label, pcms_component_table, then the host
    form's fp64 arithmetic on the bit-equal integer table, so the dicts are equal.  A uint8 CUDA
    mask and optionally fp32 CUDA probabilities in; CPU tensors raise."""
    sp = _spacing(spacing)
    mask = device_tensor(mask, torch.uint8, 3, "lesion_table_device")
    table = component_table_device(label_components_device(mask, connectivity), prob)
    return _lesion_rows(table, tuple(mask.shape), sp)


def lesion_metrics_device(pred: torch.Tensor, ref: torch.Tensor, prob: Optional[torch.Tensor] = None,
                          spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26,
                          min_iou: float = 0.1) -> dict:
    """``lesion_metrics`` on the GPU: labels, tables and overlap pairs from the kernels, matching
    and every fp64 quantity on the host by the host form's own functions, so the result is equal.
    uint8 CUDA masks (and optionally fp32 CUDA probabilities) in; CPU tensors raise."""
    sp = _spacing(spacing)
    pred = device_tensor(pred, torch.uint8, 3, "lesion_metrics_device")
    ref = device_tensor(ref, torch.uint8, 3, "lesion_metrics_device")
    if pred.shape != ref.shape or pred.device != ref.device:
        raise ValueError(f"the masks are on different grids or devices: {tuple(pred.shape)} on {pred.device} and "
                         f"{tuple(ref.shape)} on {ref.device}")
    lp, lr = label_components_device(pred, connectivity), label_components_device(ref, connectivity)
    return _lesion_report(component_table_device(lp, prob), component_table_device(lr),
                          overlap_pairs_device(lp, lr, connectivity), tuple(pred.shape), sp, min_iou)
