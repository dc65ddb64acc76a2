"""Mask post-processing by connected components (csrc/components.hip): host forms, then
device forms.  ``label_components`` / ``filter_components`` / ``fill_holes`` / ``postprocess`` define
what pcms_components_label and pcms_mask_postprocess compute, byte for byte.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from ._args import device_tensor, volume3
from ._lib import call, query


# ---- mask post-processing ----------------------------------------------------------
# Foreground is ``mask != 0``; the flat index of voxel (d, h, w) is ``(d*H + h)*W + w``; two voxels
# are adjacent at ``connectivity`` 6 / 18 / 26 when every index offset is in {-1, 0, 1}, not all are
# zero, and at most 1 / 2 / 3 of them are nonzero.
MAX_KEEP_LARGEST = 8


def _offsets(connectivity: int) -> List[Tuple[int, int, int]]:
    if connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity is 6, 18 or 26, got {connectivity!r}")
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
            if 1 <= (a != 0) + (b != 0) + (c != 0) <= most]


def label_components(mask: np.ndarray, connectivity: int = 26) -> np.ndarray:
    """Connected components of the foreground (``mask != 0``), int32 (D, H, W): 0 on background,
    ``1 + the smallest flat index ((d*H + h)*W + w) of the voxel's component`` on foreground.
    Adjacency at ``connectivity`` 6 / 18 / 26: offsets in {-1, 0, 1}, not all zero, at most
    1 / 2 / 3 of them nonzero.  The label depends on the mask alone, never on a traversal order;
    ranking the distinct labels in ascending order gives ``scipy.ndimage.label``'s numbering.
    Computed by min-propagation over the shifted neighbours plus pointer jumping until nothing
    changes: every voxel carries the flat index of its tree's root; a round takes the minimum
    root over each voxel's neighbours, hangs every root below the smallest root seen by any of
    its voxels, and jumps the pointers until every voxel points at a root again."""
    offsets = _offsets(connectivity)
    fg = volume3(mask) != 0
    D, H, W = fg.shape
    n = fg.size
    big = np.int64(n)  # the background's value: larger than every index, so it never wins a minimum
    fgi = np.flatnonzero(fg)
    root = np.full(n, big, dtype=np.int64)  # root[i]: the root of voxel i's tree, a voxel with root[r] == r
    root[fgi] = fgi
    pad = np.full((D + 2, H + 2, W + 2), big, dtype=np.int64)
    while True:
        pad[1:-1, 1:-1, 1:-1] = root.reshape(fg.shape)
        seen = pad[1:-1, 1:-1, 1:-1].copy()
        for a, b, c in offsets:
            np.minimum(seen, pad[1 + a:1 + a + D, 1 + b:1 + b + H, 1 + c:1 + c + W], out=seen)
        seen = seen.reshape(-1)[fgi]
        mine = root[fgi]
        lower = seen < mine
        if not lower.any():
            break
        np.minimum.at(root, mine[lower], seen[lower])  # a root hangs below a smaller root of its component
        while True:  # pointer jumping
            nxt = root[root[fgi]]
            if np.array_equal(nxt, root[fgi]):
                break
            root[fgi] = nxt
    lab = np.zeros(n, dtype=np.int32)
    lab[fgi] = root[fgi] + 1
    return lab.reshape(fg.shape)


def _check_filter(keep_largest, min_voxels):
    if not isinstance(keep_largest, (int, np.integer)) or not 0 <= keep_largest <= MAX_KEEP_LARGEST:
        raise ValueError(f"keep_largest is an integer in 0..{MAX_KEEP_LARGEST}, got {keep_largest!r}")
    if not isinstance(min_voxels, (int, np.integer)) or not 0 <= min_voxels < 2 ** 31:
        raise ValueError(f"min_voxels is a non-negative 32-bit integer, got {min_voxels!r}")


def filter_components(mask: np.ndarray, keep_largest: int = 0, min_voxels: int = 0,
                      connectivity: int = 26) -> np.ndarray:
    """The foreground (``mask != 0``) components that stay, as a uint8 0 / 1 mask.  All components
    (``label_components`` at ``connectivity``) are ranked by (size descending, label ascending);
    one stays iff ``size >= min_voxels`` and (``keep_largest == 0`` or its rank
    ``< keep_largest``).  Equal sizes resolve to the smaller label.  ``keep_largest`` is in 0..8
    and ``min_voxels >= 0``, else ValueError."""
    _check_filter(keep_largest, min_voxels)
    lab = label_components(mask, connectivity)
    labels, inverse, sizes = np.unique(lab.reshape(-1), return_inverse=True, return_counts=True)
    stay = (sizes >= min_voxels) & (labels != 0)
    if keep_largest:
        comp = np.flatnonzero(labels != 0)
        order = comp[np.lexsort((labels[comp], -sizes[comp]))]  # size descending, then label ascending
        top = np.zeros_like(stay)
        top[order[:keep_largest]] = True
        stay &= top
    return stay[inverse.reshape(-1)].reshape(lab.shape).astype(np.uint8)


def fill_holes(mask: np.ndarray) -> np.ndarray:
    """``mask != 0`` with its enclosed holes filled, uint8: the background is labelled at
    6-connectivity (always 6, the dual of 26 and ``scipy.ndimage.binary_fill_holes``' default) and
    every background component with no voxel on any of the six faces of the volume becomes 1."""
    fg = volume3(mask) != 0
    lab = label_components(~fg, 6)
    faces = np.concatenate([lab[0].ravel(), lab[-1].ravel(), lab[:, 0].ravel(), lab[:, -1].ravel(),
                            lab[:, :, 0].ravel(), lab[:, :, -1].ravel()])
    open_labels = np.unique(faces)
    hole = (lab != 0) & ~np.isin(lab, open_labels)
    return (fg | hole).astype(np.uint8)


def postprocess(mask: np.ndarray, keep_largest: int = 0, min_voxels: int = 0, fill_holes: bool = False,
                connectivity: int = 26) -> np.ndarray:
    """``filter_components`` then (when asked) ``fill_holes``, uint8.  With ``keep_largest == 0``,
    ``min_voxels <= 1`` and ``fill_holes=False`` this is ``(mask != 0)``."""
    _check_filter(keep_largest, min_voxels)
    _offsets(connectivity)
    out = filter_components(mask, keep_largest, min_voxels, connectivity)
    return _fill_holes(out) if fill_holes else out


_fill_holes = fill_holes  # postprocess's keyword of the same name shadows the function there


def _components_work(mask: torch.Tensor) -> torch.Tensor:
    n = query("pcms_components_work_ints", *mask.shape)
    if n < 0:
        raise ValueError(f"a volume of shape {tuple(mask.shape)} is too large to label")
    return torch.empty(n, dtype=torch.int32, device=mask.device)


def _check_status(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"{what}: a labelling kernel ran into its iteration cap (status {status})")


def _postprocess_enqueue(mask: torch.Tensor, keep_largest, min_voxels, fill_holes, connectivity):
    """(out, work) with pcms_mask_postprocess enqueued on the current stream; work[0] is the
    status the caller copies back with the mask."""
    _check_filter(keep_largest, min_voxels)
    _offsets(connectivity)
    out = torch.empty_like(mask)
    work = _components_work(mask)
    call("pcms_mask_postprocess", mask, out, work, int(keep_largest), int(min_voxels), int(bool(fill_holes)),
         int(connectivity), *mask.shape)
    return out, work


def postprocess_device(mask: torch.Tensor, keep_largest: int = 0, min_voxels: int = 0, fill_holes: bool = False,
                       connectivity: int = 26) -> torch.Tensor:
    """``postprocess`` on the GPU, byte for byte: a uint8 CUDA tensor (D, H, W) in, a new uint8
    tensor out, enqueued on the current stream (pcms_mask_postprocess).  The kernels' status word
    is read back at the end; RuntimeError if it is nonzero.  A CPU tensor raises."""
    mask = device_tensor(mask, torch.uint8, 3, "postprocess_device")
    with torch.cuda.device(mask.device):
        out, work = _postprocess_enqueue(mask, keep_largest, min_voxels, fill_holes, connectivity)
        _check_status(int(work[0].item()), "postprocess_device")
    return out


def label_components_device(mask: torch.Tensor, connectivity: int = 26, invert: bool = False) -> torch.Tensor:
    """``label_components`` on the GPU, bit for bit (pcms_components_label): int32 (D, H, W), the
    lesion map.  ``invert=True`` labels the zero voxels instead.  A CPU tensor raises."""
    mask = device_tensor(mask, torch.uint8, 3, "label_components_device")
    _offsets(connectivity)
    with torch.cuda.device(mask.device):
        labels = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
        work = _components_work(mask)
        call("pcms_components_label", mask, int(bool(invert)), int(connectivity), labels, work, *mask.shape)
        _check_status(int(work[0].item()), "label_components_device")
    return labels
