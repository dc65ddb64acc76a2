"""Intensity normalisation (csrc/intensity.hip): host forms, then device forms.

``normalise`` is the min-max normalisation ``predict.load_multimodal_images`` applies to a channel.
Percentile intensity normalisation: ``intensity_window`` / ``normalise_window`` are the host forms
of a robust window -- two exact order statistics of a volume, the volume clipped to them and scaled
to [0, 1]; ``Normalisation`` names the choice wherever ``normalise`` is taken (``True`` stays
min-max); on the device pcms_volume_window selects the window from the raw bytes and the
``_window`` resampling kernels consume it, bit for bit.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import call, query


def normalise(vol: np.ndarray) -> np.ndarray:
    """Min-max normalisation of one volume to [0, 1] as ``load_multimodal_images`` forms a
    channel, bit for bit: ``v = vol.astype(float32)``, ``lo = v.min()``, ``hi = v.max()``,
    ``den = float32(float64(hi) - float64(lo))``, the result ``(v - lo) / den`` in fp32, or
    zeros when ``den == 0``.  A NaN in the volume makes ``lo``, ``hi`` and every voxel NaN."""
    v = np.asarray(vol).astype(np.float32)
    lo, hi = v.min(), v.max()
    with np.errstate(over="ignore", invalid="ignore"):
        den = np.float32(np.float64(hi) - np.float64(lo))
        if den == 0:
            return np.zeros_like(v)
        return (v - lo) / den


def _window_ppm(lower: float, upper: float) -> Tuple[int, int]:
    """The two percentiles in parts per million, as integers; ValueError unless
    ``0 <= q_lo < q_hi <= 1_000_000``."""
    try:
        q_lo, q_hi = int(round(float(lower) * 10000)), int(round(float(upper) * 10000))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"percentiles are two numbers with 0 <= lower < upper <= 100, got {lower!r}, "
                         f"{upper!r}") from None
    if not 0 <= q_lo < q_hi <= 1_000_000:
        raise ValueError(f"percentiles need 0 <= lower < upper <= 100, got {lower!r}, {upper!r}")
    return q_lo, q_hi


def _window_above(above) -> Optional[float]:
    if above is None:
        return None
    a = float(np.float32(above))
    if not math.isfinite(a):
        raise ValueError(f"above is None or a finite number, got {above!r}")
    return a


def intensity_window(vol: np.ndarray, lower: float = 0.5, upper: float = 99.5, above=None) -> np.ndarray:
    """The robust intensity window ``[lo, hi]`` of one volume, two float32 values: exact order
    statistics, no interpolation.  ``v = vol.astype(float32) + float32(0)`` (the sum folds -0.0
    into +0.0); the selected set is all of ``v``, or ``v[v > float32(above)]`` (never a NaN); ``m``
    is its size and ``m == 0`` gives ``[0, 0]``.  The percentiles become integers,
    ``q = int(round(p * 10000))`` parts per million with ``0 <= q_lo < q_hi <= 1_000_000``
    (ValueError), and so do the ranks: ``r_lo = (q_lo * (m - 1)) // 10**6`` and
    ``r_hi = ceil(q_hi * (m - 1) / 10**6)``.  ``s = np.sort(selected)`` (NaNs last):
    ``lo = s[r_lo]``, ``hi = s[r_hi]``.  ``lower=0, upper=100`` is the minimum and maximum of a
    NaN-free volume.  libpcms_hip's pcms_volume_window is compared with this on the bits."""
    q_lo, q_hi = _window_ppm(lower, upper)
    above = _window_above(above)
    v = np.asarray(vol).astype(np.float32).reshape(-1) + np.float32(0)
    if above is not None:
        with np.errstate(invalid="ignore"):
            v = v[v > np.float32(above)]
    m = int(v.size)
    if m == 0:
        return np.zeros(2, dtype=np.float32)
    r_lo = (q_lo * (m - 1)) // 10 ** 6
    r_hi = -((-q_hi * (m - 1)) // 10 ** 6)
    s = np.sort(v)
    return np.array([s[r_lo], s[r_hi]], dtype=np.float32)


def normalise_window(vol: np.ndarray, lohi) -> np.ndarray:
    """``vol`` clipped to the window ``lohi = (lo, hi)`` and scaled to [0, 1], float32:
    ``den = float32(float64(hi) - float64(lo))``; zeros when ``den == 0``; else ``c`` is ``lo``
    where ``v < lo``, ``hi`` where ``v > hi`` and ``v`` elsewhere -- comparisons, not min / max, so
    a NaN voxel stays NaN -- and the result is ``(c - lo) / den`` in fp32.  With
    ``lohi = (v.min(), v.max())`` of a NaN-free volume this is ``normalise`` bit for bit."""
    v = np.asarray(vol).astype(np.float32)
    lo, hi = (np.float32(x) for x in np.asarray(lohi, dtype=np.float32).reshape(2))
    with np.errstate(over="ignore", invalid="ignore"):
        den = np.float32(np.float64(hi) - np.float64(lo))
        if den == 0:
            return np.zeros_like(v)
        c = np.where(v < lo, lo, np.where(v > hi, hi, v))
        return (c - lo) / den


@dataclasses.dataclass
class Normalisation:
    """How a volume's intensities are brought to [0, 1] before resampling.  ``method``:
    ``"minmax"`` (``normalise``, what the reference's ``load_multimodal_images`` does) or
    ``"percentile"`` (``normalise_window`` of ``intensity_window(vol, lower, upper, above)``: the
    percentile window of the voxels above ``above``, or of all voxels with ``above=None``)."""
    method: str = "minmax"
    lower: float = 0.5
    upper: float = 99.5
    above: Optional[float] = None

    METHODS = ("minmax", "percentile")

    @staticmethod
    def of(x) -> Optional["Normalisation"]:
        """``False`` / ``None``: no normalisation (None); ``True``: min-max; a method name, a
        dict of the fields or an instance."""
        if x is None or isinstance(x, Normalisation):
            return x
        if isinstance(x, (bool, np.bool_, int)):
            return Normalisation() if x else None
        if isinstance(x, str):
            return Normalisation(method=x)
        if isinstance(x, dict):
            return Normalisation(**x)
        raise ValueError(f"normalise is False, True, a method name, a dict or a Normalisation, got {x!r}")

    def __post_init__(self):
        if self.method not in self.METHODS:
            raise ValueError(f"unknown normalisation method {self.method!r}: one of {self.METHODS}")
        self.ppm = _window_ppm(self.lower, self.upper)
        self.lower, self.upper = float(self.lower), float(self.upper)
        self.above = _window_above(self.above)

    def apply(self, vol: np.ndarray) -> np.ndarray:
        """The normalised volume, float32 (the host form of both device paths)."""
        if self.method == "minmax":
            return normalise(vol)
        return normalise_window(vol, intensity_window(vol, self.lower, self.upper, self.above))


def _host_lohi(vol: np.ndarray, norm: Optional[Normalisation]) -> np.ndarray:
    """The (lo, hi) window a volume's histogram values are normalised with: ``norm``'s percentile
    window, or the minimum and maximum (also when ``norm`` is None)."""
    if norm is not None and norm.method == "percentile":
        return intensity_window(vol, norm.lower, norm.upper, norm.above)
    v = np.asarray(vol).astype(np.float32)
    return np.array([v.min(), v.max()], dtype=np.float32)


def _lohi_enqueue(raw, norm: Normalisation, lohi: torch.Tensor) -> str:
    """Enqueue the kernel that leaves ``norm``'s (lo, hi) of the raw volume in the two device
    floats ``lohi``: pcms_volume_minmax or pcms_volume_window.  Returns the suffix of the
    consumers that read it: ``"norm"`` (pcms_resample_linear_norm, pcms_patch_resample_linear
    with lohi) or ``"window"`` (pcms_resample_linear_window, pcms_patch_resample_window)."""
    n = int(np.prod(raw.shape))
    if norm.method == "minmax":
        work = torch.empty(query("pcms_volume_minmax_work_floats", n), dtype=torch.float32, device=lohi.device)
        call("pcms_volume_minmax", *raw.kernel_args(flat=True), lohi, work)
        return "norm"
    nbytes = query("pcms_volume_window_work_bytes", n)
    if nbytes < 0:
        raise ValueError(f"a volume of {n} voxels is outside pcms_volume_window's range")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=lohi.device)
    call("pcms_volume_window", *raw.kernel_args(flat=True), norm.ppm[0], norm.ppm[1], 0 if norm.above is None else 1,
         0.0 if norm.above is None else norm.above, lohi, work)
    return "window"


def _window_device(raw, norm: Optional[Normalisation]) -> torch.Tensor:
    """``_host_lohi`` on the device: two fp32 values from pcms_volume_window or pcms_volume_minmax."""
    lohi = torch.empty(2, dtype=torch.float32, device=raw.data.device)
    _lohi_enqueue(raw, norm if norm is not None and norm.method == "percentile" else Normalisation(), lohi)
    return lohi
