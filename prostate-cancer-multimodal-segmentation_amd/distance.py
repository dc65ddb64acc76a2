"""Surface-distance scoring (csrc/distance.hip): host forms, then device forms.

``surface`` / ``edt_sq`` / ``distance_transform`` / ``surface_metrics`` are the host forms of the
boundary metrics (Hausdorff distance, HD95, ASSD under per-axis spacing); ``surface_device`` /
``distance_transform_device`` / ``surface_metrics_device`` run them in HIP kernels, the distance
transform bit for bit; ``ModelPredictor.score_case`` scores a ``predict_case`` result against a
label file in millimetres.
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence, Tuple

import numpy as np
import torch

from ._args import device_tensor, volume3
from ._lib import call, query


# ---- surface distances -----------------------------------------------------------
# Volumes are (D, H, W) with W fastest; ``spacing = (sz, sy, sx)`` is three finite doubles > 0.
# The host forms below define what csrc/distance.hip computes: the transform bit for bit.
def _spacing(spacing) -> Tuple[float, float, float]:
    try:
        sp = tuple(float(v) for v in spacing)
    except TypeError:
        raise ValueError(f"spacing is three numbers (sz, sy, sx), got {spacing!r}") from None
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0.0 for v in sp):
        raise ValueError(f"spacing is three finite numbers > 0 (sz, sy, sx), got {spacing!r}")
    return sp


def surface(mask: np.ndarray) -> np.ndarray:
    """The surface of the foreground (``mask != 0``), uint8 0 / 1: a voxel is on it iff it is
    foreground and at least one of its six face neighbours is background or lies outside the
    volume -- ``m ^ binary_erosion(m, generate_binary_structure(3, 1))`` with scipy's default
    ``border_value=0`` (MedPy's surface)."""
    fg = volume3(mask) != 0
    pad = np.pad(fg, 1)  # outside the volume: background
    inner = (pad[:-2, 1:-1, 1:-1] & pad[2:, 1:-1, 1:-1] & pad[1:-1, :-2, 1:-1] & pad[1:-1, 2:, 1:-1]
             & pad[1:-1, 1:-1, :-2] & pad[1:-1, 1:-1, 2:])
    return (fg & ~inner).astype(np.uint8)


def _sq_terms(n: int, s: float) -> np.ndarray:
    """fl(fl(k s) fl(k s)) for k = 0 .. n - 1."""
    t = np.arange(n, dtype=np.float64) * np.float64(s)
    return t * t


def edt_sq(feat: np.ndarray, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> np.ndarray:
    """The exact squared Euclidean distance to the nearest feature voxel (``feat != 0``), fp64
    (D, H, W): for every voxel p

        min over feature voxels q of fl(Z(|pd-qd|) + fl(Y(|ph-qh|) + X(|pw-qw|))),
        X(k) = fl(fl(k sx) fl(k sx)), Y and Z alike with sy and sz,

    every operation rounded on its own, and ``+inf`` when there is no feature voxel.  Computed in
    the separable form, which has the same bits (fp64 addition is monotone in each argument and
    X, Y, Z are monotone in k, so both inner minima commute with the outer additions): the
    integer distance along W by a forward and a backward scan, then a minimum over the line
    along H and one along D, one candidate position of the whole volume at a time."""
    sz, sy, sx = _spacing(spacing)
    f = volume3(feat) != 0
    D, H, W = f.shape
    idx = np.arange(W, dtype=np.int64)
    far = np.int64(4 * W)  # farther than any distance on the row
    left = np.maximum.accumulate(np.where(f, idx, -far), axis=2)             # the last feature at or before w
    right = np.minimum.accumulate(np.where(f, idx, far)[:, :, ::-1], axis=2)[:, :, ::-1]  # the first at or after
    g1 = np.minimum(idx - left, right - idx)
    none = g1 >= W
    g = np.where(none, np.inf, _sq_terms(W, sx)[np.where(none, 0, g1)])      # X(g1)
    Y = _sq_terms(H, sy)
    pos = np.arange(H)
    g2 = np.full(f.shape, np.inf)
    for q in range(H):
        np.minimum(g2, Y[np.abs(pos - q)][None, :, None] + g[:, q:q + 1, :], out=g2)
    Z = _sq_terms(D, sz)
    pos = np.arange(D)
    g3 = np.full(f.shape, np.inf)
    for q in range(D):
        np.minimum(g3, Z[np.abs(pos - q)][:, None, None] + g2[q:q + 1], out=g3)
    return g3


def distance_transform(feat: np.ndarray, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                       squared: bool = False) -> np.ndarray:
    """The distance of every voxel to the nearest feature voxel (``feat != 0``) under per-axis
    ``spacing``, fp64: ``sqrt(edt_sq)`` (``edt_sq`` itself with ``squared=True``) --
    ``scipy.ndimage.distance_transform_edt(feat == 0, sampling=spacing)``."""
    sq = edt_sq(feat, spacing)
    return sq if squared else np.sqrt(sq)


def _percentile95(v: np.ndarray) -> float:
    """The 95th percentile of an ascending fp64 vector by linear interpolation, written out
    (``np.percentile(v, 95)``'s default method): every operation rounded on its own."""
    n = len(v)
    pos = (n - 1) * 0.95
    lo = int(math.floor(pos))
    hi = min(lo + 1, n - 1)
    t = pos - lo
    a, b = float(v[lo]), float(v[hi])
    return a + (b - a) * t


def _empty_metrics(n_a: int, n_b: int) -> dict:
    v = 0.0 if n_a == 0 and n_b == 0 else math.inf
    return {"hd": v, "hd95": v, "assd": v, "n_a": n_a, "n_b": n_b}


def surface_metrics(a: np.ndarray, b: np.ndarray, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> dict:
    """Boundary metrics of two masks on one grid, in the units of ``spacing``: with ``Sa`` /
    ``Sb`` their ``surface``, ``da`` the distances ``sqrt(edt_sq(Sb))`` at the voxels of ``Sa``
    and ``db`` the other way round,

    * ``hd``: the Hausdorff distance ``max(max da, max db)``;
    * ``hd95``: the 95th percentile of ``da ++ db`` (MedPy's ``hd95``; ``_percentile95``);
    * ``assd``: ``(mean(da) + mean(db)) / 2``;
    * ``n_a`` / ``n_b``: the surface voxel counts.

    Both surfaces empty: all three are 0.0; exactly one empty: all three are ``inf``."""
    sp = _spacing(spacing)
    sa, sb = surface(a) != 0, surface(b) != 0
    if sa.shape != sb.shape:
        raise ValueError(f"the masks are on different grids: {sa.shape} and {sb.shape}")
    n_a, n_b = int(sa.sum()), int(sb.sum())
    if n_a == 0 or n_b == 0:
        return _empty_metrics(n_a, n_b)
    da = np.sqrt(edt_sq(sb, sp)[sa])
    db = np.sqrt(edt_sq(sa, sp)[sb])
    both = np.sort(np.concatenate([da, db]))
    return {"hd": float(max(da.max(), db.max())), "hd95": _percentile95(both),
            "assd": (float(da.mean()) + float(db.mean())) / 2.0, "n_a": n_a, "n_b": n_b}


def _edt_work_bytes(mask: torch.Tensor) -> int:
    n = query("pcms_edt_work_bytes", *mask.shape)
    if n < 0:
        raise ValueError(f"a volume of shape {tuple(mask.shape)} is too large for the distance kernels "
                         "(at most 2048 per axis)")
    return n


def _edt_work(mask: torch.Tensor) -> torch.Tensor:
    return torch.empty(_edt_work_bytes(mask) // 8, dtype=torch.float64, device=mask.device)


def surface_device(mask: torch.Tensor) -> torch.Tensor:
    """``surface`` on the GPU, byte for byte (pcms_mask_surface): a uint8 CUDA tensor (D, H, W)
    in, a new one out, enqueued on the current stream.  A CPU tensor raises."""
    mask = device_tensor(mask, torch.uint8, 3, "surface_device")
    _edt_work_bytes(mask)  # the size check
    with torch.cuda.device(mask.device):
        out = torch.empty_like(mask)
        call("pcms_mask_surface", mask, out, *mask.shape)
    return out


def _edt_sq_enqueue(feat: torch.Tensor, sp, work: torch.Tensor) -> torch.Tensor:
    out = torch.empty(feat.shape, dtype=torch.float64, device=feat.device)
    host = (ctypes.c_double * 3)(*sp)  # read during the call (kernel arguments)
    call("pcms_edt_sq", feat, ctypes.addressof(host), out, work, *feat.shape)
    return out


def distance_transform_device(mask: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                              squared: bool = False) -> torch.Tensor:
    """``distance_transform`` on the GPU (pcms_edt_sq): fp64 (D, H, W); with ``squared=True``
    equal to ``edt_sq`` bit for bit, else its ``torch.sqrt``.  A CPU tensor raises."""
    sp = _spacing(spacing)
    mask = device_tensor(mask, torch.uint8, 3, "distance_transform_device")
    with torch.cuda.device(mask.device):
        sq = _edt_sq_enqueue(mask, sp, _edt_work(mask))
        return sq if squared else torch.sqrt(sq)


def surface_metrics_device(a: torch.Tensor, b: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> dict:
    """``surface_metrics`` on the GPU: pcms_mask_surface and pcms_edt_sq per mask, then
    pcms_surface_distance_stats per direction.  ``hd``, ``hd95``, ``n_a`` and ``n_b`` equal the
    host form's exactly (order statistics of bit-equal squared distances: they are sorted on the
    device, the two that ``hd95`` interpolates and the statistics come to the host in one copy,
    and the square roots are taken there in fp64); ``assd`` comes from the device's sums of
    square roots and agrees to rounding.  CPU tensors raise."""
    sp = _spacing(spacing)
    a = device_tensor(a, torch.uint8, 3, "surface_metrics_device")
    b = device_tensor(b, torch.uint8, 3, "surface_metrics_device")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"the masks are on different grids or devices: {tuple(a.shape)} on {a.device} and "
                         f"{tuple(b.shape)} on {b.device}")
    with torch.cuda.device(a.device):
        work = _edt_work(a)
        selected, stats = [], torch.empty((2, 3), dtype=torch.float64, device=a.device)
        for k, (m, other) in enumerate(((a, b), (b, a))):
            feat = torch.empty_like(other)
            call("pcms_mask_surface", other, feat, *other.shape)
            sq = _edt_sq_enqueue(feat, sp, work)
            sd = torch.empty_like(sq)
            call("pcms_surface_distance_stats", m, sq, sd, stats[k], work, *m.shape)
            selected.append(sd[sd >= 0])
        n_a, n_b = selected[0].numel(), selected[1].numel()
        if n_a == 0 or n_b == 0:
            return _empty_metrics(n_a, n_b)
        v = torch.sort(torch.cat(selected)).values
        n = n_a + n_b
        pos = (n - 1) * 0.95
        lo = int(math.floor(pos))
        hi = min(lo + 1, n - 1)
        host = torch.cat([v[lo:lo + 1], v[hi:hi + 1], stats.reshape(-1)]).cpu().numpy()
    counts = host[[2, 5]].view(np.int64)
    if (int(counts[0]), int(counts[1])) != (n_a, n_b):
        raise RuntimeError(f"surface_metrics_device: the kernel counted {counts.tolist()} surface voxels, "
                           f"the selection holds {[n_a, n_b]}")
    host = [float(x) for x in host]
    lo_v, hi_v = math.sqrt(host[0]), math.sqrt(host[1])
    return {"hd": math.sqrt(max(host[3], host[6])), "hd95": lo_v + (hi_v - lo_v) * (pos - lo),
            "assd": (host[4] / n_a + host[7] / n_b) / 2.0, "n_a": n_a, "n_b": n_b}
