"""Single-case prediction pipeline (reference script/predict.py), on the HIP engine.

* ``load_multimodal_images(case_dir, handle_missing)``: the five modality folders
  ['ADC', 'DWI', 'gaoqing-T2', 'T2 fs', 'T2 not fs'] (predict.py:25), the first ``.nii`` of
  each, per-modality min-max normalisation to [0, 1] (constant image -> zeros, :70-75),
  missing modalities by 'zero_fill' / 'skip' / 'duplicate' (:38-55), stacked (5, D, H, W)
  (:81).  NIfTI through pcms_amd.data's reader (SimpleITK is not a dependency).
* ``preprocess_image``: (1, 5, D, H, W) float32 tensor (:85-100).
* ``ModelPredictor(model_path, device)``: UNet3D(n_modalities=5, n_classes=1) with either
  checkpoint form (:121-145), ``predict`` -> (D, H, W) probabilities from ``UNet3D.predict``
  (sigmoid in the head kernel, :160-170), ``save_prediction`` -> uint8 ``> 0.5`` mask NIfTI
  with the reference image's voxel spacing when one is given (:172-196).  ``saliency`` ->
  (5, D, H, W) input gradient of the summed probabilities (no reference equivalent in
  predict.py; plain autograd through the reference model gives the same quantity).

Case prediction on the training grid: ``predict_case(case_dir)`` takes a case from
its raw NIfTI files to a uint8 mask on the native grid of its reference image, every per-voxel
step in a HIP kernel; ``save_case`` writes it with that image's full geometry.  The host forms
``normalise`` / ``prepare_case`` / ``tta_mean`` / ``mask_on_grid`` define what the kernels
compute, bit for bit.

Scoring: ``surface`` / ``edt_sq`` / ``distance_transform`` / ``surface_metrics`` are
the host forms of the boundary metrics (Hausdorff distance, HD95, ASSD under per-axis spacing);
``surface_device`` / ``distance_transform_device`` / ``surface_metrics_device`` run them in HIP
kernels, the distance transform bit for bit; ``ModelPredictor.score_case`` scores a
``predict_case`` result against a label file in millimetres.

Lesion analysis: ``component_table`` / ``overlap_pairs`` / ``match_lesions`` /
``lesion_table`` / ``lesion_metrics`` are the host forms of the per-lesion table (voxels, box,
centroid, peak probability) and of the detection scores (one-to-one matching at an IoU
threshold); ``component_table_device`` / ``overlap_pairs_device`` / ``lesion_table_device`` /
``lesion_metrics_device`` build the tables in HIP kernels, on the bytes, and share the host
arithmetic; ``predict_case(..., return_lesions=True)`` and ``score_case(..., lesion_metrics=True)``
carry them.

Sliding-window prediction: ``window_starts`` / ``window_grid`` / ``window_weights`` /
``gather_windows`` / ``blend_windows`` / ``sliding_window_predict`` are the host forms of cutting
a volume into fixed-size overlapping windows and blending the windows' probabilities with
centre-weighted weights; ``gather_windows_device`` / ``blend_windows_device`` /
``sliding_window_device`` run them in HIP kernels, bit for bit and independent of the batching;
``predict_case(..., window=...)`` predicts a case at its native resolution through them.

Percentile intensity normalisation: ``intensity_window`` / ``normalise_window`` are
the host forms of a robust window -- two exact order statistics of a volume, the volume clipped to
them and scaled to [0, 1]; ``Normalisation`` names the choice wherever ``normalise`` is taken
(``True`` stays min-max); on the device pcms_volume_window selects the window from the raw bytes
and the ``_window`` resampling kernels consume it, bit for bit.

Modality alignment: ``Alignment`` names how the modalities of a case reach one grid --
through their NIfTI world geometry (``data.world_matrix`` / ``align_affine`` / ``case_affine``) and
optionally a rigid registration; ``joint_histogram`` / ``normalised_mutual_information`` /
``register_rigid`` are the host forms of the similarity and of the search that maximises it;
``joint_histogram_device`` (pcms_joint_histogram, on the counts) / ``register_rigid_device`` /
``register_case_device`` / ``register_dataset`` run them on the GPU; ``prepare_case``,
``prepare_case_device`` and ``predict_case`` take ``align=``.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import data as _data
from .data import read_nifti, read_nifti_header, write_nifti
from .models.unet3d import UNet3D, load_weights

MODALITIES = ["ADC", "DWI", "gaoqing-T2", "T2 fs", "T2 not fs"]


def load_multimodal_images(case_dir: str, handle_missing: str = "zero_fill") -> Tuple[np.ndarray, List[str]]:
    images, reference = [], None
    for modality in MODALITIES:
        mdir = os.path.join(case_dir, modality)
        if not os.path.exists(mdir):
            raise FileNotFoundError(f"modality directory missing: {mdir}")
        files = sorted(f for f in os.listdir(mdir) if f.endswith(".nii"))
        if not files:
            if handle_missing == "zero_fill":
                img = np.zeros_like(reference, dtype=np.float32) if reference is not None else \
                    np.zeros((64, 64, 64), dtype=np.float32)
            elif handle_missing == "duplicate" and reference is not None:
                img = reference.copy()
            else:
                raise FileNotFoundError(f"no .nii file in {mdir}")
        else:
            img = read_nifti(os.path.join(mdir, files[0]))
            if reference is None:
                reference = img
        img = img.astype(np.float32)
        lo, hi = float(img.min()), float(img.max())
        img = (img - lo) / (hi - lo) if hi - lo != 0 else np.zeros_like(img, dtype=np.float32)
        images.append(img.astype(np.float32))
    return np.stack(images, axis=0), list(MODALITIES)


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


_normalise = normalise  # prepare_case's keyword of the same name shadows the function there


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


def _lohi_enqueue(raw, norm: Normalisation, lohi: torch.Tensor) -> str:
    """Enqueue the kernel that leaves ``norm``'s (lo, hi) of the raw volume in the two device
    floats ``lohi``: pcms_volume_minmax or pcms_volume_window.  Returns the suffix of the
    consumers that read it: ``"norm"`` (pcms_resample_linear_norm, pcms_patch_resample_linear
    with lohi) or ``"window"`` (pcms_resample_linear_window, pcms_patch_resample_window)."""
    from ._lib import call, query
    n = int(np.prod(raw.shape))
    if norm.method == "minmax":
        work = torch.empty(query("pcms_volume_minmax_work_floats", n), dtype=torch.float32, device=lohi.device)
        call("pcms_volume_minmax", raw.data, int(raw.code), n, float(raw.slope), float(raw.inter), lohi, work)
        return "norm"
    nbytes = query("pcms_volume_window_work_bytes", n)
    if nbytes < 0:
        raise ValueError(f"a volume of {n} voxels is outside pcms_volume_window's range")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=lohi.device)
    call("pcms_volume_window", raw.data, int(raw.code), n, float(raw.slope), float(raw.inter), norm.ppm[0], norm.ppm[1],
         0 if norm.above is None else 1, 0.0 if norm.above is None else norm.above, lohi, work)
    return "window"


def _case_files(case_dir: str) -> List[Optional[str]]:
    """Per modality the first ``.nii`` of its folder in sorted order, or None."""
    paths = []
    for modality in MODALITIES:
        mdir = os.path.join(case_dir, modality)
        if not os.path.exists(mdir):
            raise FileNotFoundError(f"modality directory missing: {mdir}")
        files = sorted(f for f in os.listdir(mdir) if f.endswith(".nii"))
        paths.append(os.path.join(mdir, files[0]) if files else None)
    return paths


def _case_plan(case_dir: str, target_size, handle_missing: str, align=None):
    """(paths, the grid every channel is formed on, the channel a missing modality copies or
    None for zeros): what ``prepare_case`` and ``prepare_case_device`` decide alike.  With
    ``align`` (an ``Alignment``) ``target_size=None`` is the native grid of the reference file and
    the modalities' shapes may differ."""
    if handle_missing not in ("zero_fill", "skip", "duplicate"):
        raise ValueError(f"unsupported missing-modality strategy: {handle_missing}")
    paths = _case_files(case_dir)
    present = [c for c, p in enumerate(paths) if p is not None]
    if not present or (handle_missing == "skip" and len(present) < len(paths)):
        missing = [m for m, p in zip(MODALITIES, paths) if p is None]
        raise FileNotFoundError(f"no .nii file for {missing} in {case_dir}")
    if target_size is not None:
        grid = tuple(int(v) for v in target_size)
    elif align is not None:
        grid = _shape_of(_case_reference(paths, align))
    else:
        shapes = {p: tuple(read_nifti_header(p)["shape_xyz"][:3][::-1]) for p in paths if p is not None}
        if len(set(shapes.values())) != 1:
            raise ValueError(f"target_size=None needs modalities of one shape, got {sorted(set(shapes.values()))}")
        grid = shapes[paths[present[0]]]
    return paths, grid, present[0] if handle_missing == "duplicate" else None


def _first_volume(a: np.ndarray) -> np.ndarray:
    if a.ndim not in (3, 4):
        raise ValueError(f"unsupported image dimensions: {a.shape}")
    return a if a.ndim == 3 else a[0]


# ---- modality alignment ------------------------------------------------------------
# Geometry lives in data.py (world_matrix, align_affine, case_affine).  Below: the similarity of two
# volumes of different contrast -- the joint histogram of their window-normalised intensities under
# an affine and its normalised mutual information -- and a rigid registration that maximises it.
# The host forms define what csrc/align.hip counts, exactly.
DEFAULT_LEVELS = (((1, 2, 2), (4.0, 2.0, 1.0)), ((1, 1, 1), (0.5, 0.25)))


def _bin_index(v: np.ndarray, bins: int) -> np.ndarray:
    """``fl32(v * float32(bins))`` clamped to ``[0, bins - 1]`` as a float and truncated: for ``v``
    in [0, 1] that is ``min(int(fl32(v * bins)), bins - 1)``; NaNs (never counted) map to 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        b = np.asarray(v, dtype=np.float32) * np.float32(bins)
        b = np.where(b < 0, np.float32(0), np.where(b > np.float32(bins - 1), np.float32(bins - 1), b))
    return np.where(np.isnan(b), np.float32(0), b).astype(np.int64)


def _check_hist_args(bins, stride) -> Tuple[int, Tuple[int, int, int]]:
    if isinstance(bins, bool) or int(bins) != bins or not 2 <= int(bins) <= 64:
        raise ValueError(f"bins is an integer in 2..64, got {bins!r}")
    stride = _data._axes3(stride, "stride")
    if min(stride) < 1:
        raise ValueError(f"every stride is at least 1, got {stride}")
    return int(bins), stride


def joint_histogram(fix: np.ndarray, mov: np.ndarray, A, t, fix_lohi, mov_lohi, bins: int = 32,
                    stride: Sequence[int] = (1, 1, 1)) -> np.ndarray:
    """The joint intensity histogram of a fixed and a moving (D, H, W) volume under the affine
    ``(A, t)`` (fixed array index -> moving array index), int64 ``(bins, bins)``.  For every
    lattice index ``q = (a*sd, b*sh, e*sw)`` inside the fixed volume: ``f`` is
    ``normalise_window(fix, fix_lohi)`` at ``q``; ``m`` is the linear sample
    (``data.resample_affine``'s gather) of ``normalise_window(mov, mov_lohi)`` at
    ``c_a = ((A[a][0]*q_d + A[a][1]*q_h) + A[a][2]*q_w) + t[a]``.  The voxel counts only if
    ``-0.5 <= c_a < n_a - 0.5`` on all three moving axes and neither value is NaN; then
    ``hist[bin(f), bin(m)] += 1`` with ``bin(v) = min(int(fl32(v * float32(bins))), bins - 1)``
    (``_bin_index``).  The sum of the table is the overlap count.  libpcms_hip's
    pcms_joint_histogram is compared with this on the counts."""
    bins, stride = _check_hist_args(bins, stride)
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    fix, mov = _volume(fix), _volume(mov)
    f = normalise_window(fix, fix_lohi)[::stride[0], ::stride[1], ::stride[2]]
    mv = normalise_window(mov, mov_lohi)
    shapes = ((-1, 1, 1), (1, -1, 1), (1, 1, -1))
    q = [np.arange(0, n, s, dtype=np.int64).astype(np.float64).reshape(sh)
         for n, s, sh in zip(fix.shape, stride, shapes)]
    with np.errstate(over="ignore", invalid="ignore"):
        c = [((A[a, 0] * q[0] + A[a, 1] * q[1]) + A[a, 2] * q[2]) + t[a] for a in range(3)]
        inside = np.ones(f.shape, dtype=bool)
        for a in range(3):
            inside = inside & ((c[a] >= -0.5) & (c[a] < mov.shape[a] - 0.5))
    with np.errstate(over="ignore", invalid="ignore"):
        m = _data._sample_at(mv, c, False, 1.0, 0.0)
    ok = inside & ~np.isnan(f) & ~np.isnan(m)
    flat = _bin_index(f, bins)[ok] * bins + _bin_index(m, bins)[ok]
    return np.bincount(flat, minlength=bins * bins).astype(np.int64).reshape(bins, bins)


def normalised_mutual_information(hist) -> float:
    """``(H(X) + H(Y)) / H(X, Y)`` of a joint count table, in fp64 from the counts: with
    ``p = hist / N`` the entropies are ``-sum p log p`` over the non-empty cells of the table and
    of its row and column sums.  1.0 for independent intensities, 2.0 for a one-to-one relation;
    0.0 for an empty table and for a table with a single non-empty cell (``H(X, Y) = 0``: two
    constant images say nothing about their alignment)."""
    h = np.asarray(hist, dtype=np.float64)
    n = float(h.sum())
    if n <= 0.0:
        return 0.0

    def entropy(counts):
        p = counts[counts > 0] / n
        return float(-(p * np.log(p)).sum())

    hxy = entropy(h.reshape(-1))
    if hxy <= 0.0:
        return 0.0
    return (entropy(h.sum(axis=1)) + entropy(h.sum(axis=0))) / hxy


@dataclasses.dataclass
class Alignment:
    """How the modalities of a case are brought onto one grid.  ``mode``: ``"world"`` -- every file
    is resampled through its header geometry (``data.align_affine``) onto the reference file's
    grid -- or ``"register"`` -- each other modality is first registered rigidly to the reference
    (``register_rigid``) and the correction goes into its affine.  ``to``: the reference, a modality
    name or a file path (None: the caller's default; training also takes ``"label"``).  ``bins``,
    ``levels``, ``min_overlap``, ``max_translation_mm`` and ``max_rotation_deg`` are
    ``register_rigid``'s."""
    mode: str = "world"
    to: Optional[str] = None
    bins: int = 32
    levels: tuple = DEFAULT_LEVELS
    min_overlap: float = 0.5
    max_translation_mm: float = 20.0
    max_rotation_deg: float = 10.0

    MODES = ("world", "register")

    @staticmethod
    def of(x) -> Optional["Alignment"]:
        """``None``: no alignment (None); a mode name, a dict of the fields or an instance."""
        if x is None or isinstance(x, Alignment):
            return x
        if isinstance(x, str):
            return Alignment(mode=x)
        if isinstance(x, dict):
            return Alignment(**x)
        raise ValueError(f"align is None, a mode name, a dict or an Alignment, got {x!r}")

    def __post_init__(self):
        if self.mode not in self.MODES:
            raise ValueError(f"unknown alignment mode {self.mode!r}: one of {self.MODES}")
        if self.to is not None and not isinstance(self.to, str):
            raise ValueError(f"Alignment.to is None, a modality name or a file path, got {self.to!r}")
        self.bins = _check_hist_args(self.bins, (1, 1, 1))[0]
        levels = []
        for level in self.levels:
            stride, steps = level
            steps = tuple(float(s) for s in steps)
            if not steps or not all(math.isfinite(s) and s > 0.0 for s in steps):
                raise ValueError(f"the steps of a level are finite numbers > 0, got {level!r}")
            levels.append((_check_hist_args(2, stride)[1], steps))
        if not levels:
            raise ValueError("Alignment.levels holds at least one (stride, steps) level")
        self.levels = tuple(levels)
        self.min_overlap = float(self.min_overlap)
        self.max_translation_mm, self.max_rotation_deg = float(self.max_translation_mm), float(self.max_rotation_deg)
        if not 0.0 <= self.min_overlap <= 1.0 or not self.max_translation_mm >= 0.0 or not self.max_rotation_deg >= 0.0:
            raise ValueError("Alignment: min_overlap lies in [0, 1] and the two limits are not negative")


def _host_lohi(vol: np.ndarray, norm: Optional[Normalisation]) -> np.ndarray:
    """The (lo, hi) window a volume's histogram values are normalised with: ``norm``'s percentile
    window, or the minimum and maximum (also when ``norm`` is None)."""
    if norm is not None and norm.method == "percentile":
        return intensity_window(vol, norm.lower, norm.upper, norm.above)
    v = np.asarray(vol).astype(np.float32)
    return np.array([v.min(), v.max()], dtype=np.float32)


def _pattern_search(evaluate, fix_shape, fix_geometry: dict, mov_geometry: dict, settings: Alignment) -> dict:
    """``register_rigid``'s search over an evaluator ``evaluate(A, t, stride) -> (bins, bins)``
    counts: the host and the device form differ in that evaluator alone."""
    centre = _data.world_centre(fix_geometry, fix_shape)
    seen, count = {}, [0]

    def score(params, stride):
        """NMI of ``params`` on the lattice of ``stride``, or None below the overlap floor."""
        key = (tuple(params), stride)
        if key not in seen:
            A, t = _data.align_affine(fix_geometry, mov_geometry, _data.rigid_world(params, centre))
            hist = np.asarray(evaluate(A, t, stride))
            count[0] += 1
            lattice = int(np.prod([-(-n // s) for n, s in zip(fix_shape, stride)]))
            seen[key] = normalised_mutual_information(hist) if int(hist.sum()) >= settings.min_overlap * lattice \
                else None
        return seen[key]

    def allowed(params):
        return all(abs(v) <= settings.max_translation_mm for v in params[:3]) and \
            all(abs(v) <= settings.max_rotation_deg for v in params[3:])

    params = [0.0] * 6
    fine = settings.levels[-1][0]
    before = score(params, fine)
    for stride, steps in settings.levels:
        best = score(params, stride)
        for step in steps:
            improved = True
            while improved:
                improved = False
                for k in range(6):
                    for sign in (1.0, -1.0):
                        cand = list(params)
                        cand[k] = cand[k] + sign * step
                        if not allowed(cand):
                            continue
                        s = score(cand, stride)
                        if s is not None and (best is None or s > best):
                            params, best, improved = cand, s, True
                            break
    after = score(params, fine)
    return {"params": tuple(float(v) for v in params), "before": 0.0 if before is None else before,
            "after": 0.0 if after is None else after, "evaluations": count[0]}


def register_rigid(fix: np.ndarray, mov: np.ndarray, fix_geometry: dict, mov_geometry: dict, fix_lohi=None,
                   mov_lohi=None, normalise=None, settings=None) -> dict:
    """Rigid registration of a moving volume to a fixed volume of another contrast, both (z, y, x)
    arrays with their ``read_nifti_geometry`` dicts.  Six parameters ``(tz, ty, tx mm; rz, ry, rx
    degrees)`` describe a rigid motion in world millimetres about the fixed volume's centre
    (``data.rigid_world``); it is the ``correction`` of ``data.align_affine(fix_geometry,
    mov_geometry, .)``, whose ``(A, t)`` the similarity ``normalised_mutual_information(
    joint_histogram(fix, mov, A, t, fix_lohi, mov_lohi, bins, stride))`` is evaluated under.
    A deterministic coordinate pattern search maximises it.  ``settings`` (an ``Alignment``, a
    dict of its fields or None for the defaults) holds ``bins``, the limits and ``levels``: per level a
    lattice stride and a list of step sizes, equal in mm and in degrees.  For each step the six
    parameters are swept in order; ``+step`` is tried, then ``-step``, the first strict improvement
    is accepted and the sweep moves to the next parameter; the sweep repeats until none improves.
    A candidate is rejected without comparison when its overlap count is below ``min_overlap`` of
    the lattice size, or when a translation exceeds ``max_translation_mm`` or a rotation
    ``max_rotation_deg`` in absolute value.  A point met twice is evaluated once.
    ``fix_lohi`` / ``mov_lohi``: the windows of the histogram (None: from ``normalise`` --
    the percentile window it names, else the minimum and maximum).
    Returns ``{"params": six floats, "before": the similarity at zero, "after": the similarity at
    the result (both on the last level's lattice; 0.0 below the overlap floor), "evaluations":
    the number of histograms formed}``."""
    settings = Alignment.of(settings) or Alignment()
    norm = Normalisation.of(normalise)
    fix, mov = _volume(fix), _volume(mov)
    fl = _host_lohi(fix, norm) if fix_lohi is None else np.asarray(fix_lohi, dtype=np.float32)
    ml = _host_lohi(mov, norm) if mov_lohi is None else np.asarray(mov_lohi, dtype=np.float32)
    return _pattern_search(lambda A, t, stride: joint_histogram(fix, mov, A, t, fl, ml, settings.bins, stride),
                           fix.shape, fix_geometry, mov_geometry, settings)


def _device_raw(raw, what: str):
    if not isinstance(raw, _data.RawVolume) or raw.data.device.type != "cuda":
        raise RuntimeError(f"{what} needs RawVolumes whose bytes are on a GPU (RawVolume.to(device)): pcms_amd has no "
                           "CPU fallback -- use the host form of the same name without _device")
    itemsize = np.dtype(_data._NIFTI_DTYPES[raw.code]).itemsize
    if raw.data.dtype != torch.uint8 or not raw.data.is_contiguous() or \
            raw.data.numel() != int(np.prod(raw.shape)) * itemsize:
        raise ValueError(f"RawVolume.data must be the {int(np.prod(raw.shape)) * itemsize} contiguous bytes of shape "
                         f"{raw.shape}, datatype {raw.code}")
    return raw


def _device_lohi(lohi, device) -> torch.Tensor:
    if isinstance(lohi, torch.Tensor):
        if lohi.device != device or lohi.dtype != torch.float32 or lohi.numel() != 2 or not lohi.is_contiguous():
            raise ValueError(f"a window is two contiguous fp32 values on {device}")
        return lohi
    return torch.from_numpy(np.asarray(lohi, dtype=np.float32).reshape(2).copy()).to(device)


def _joint_enqueue(fix_raw, mov_raw, A, t, fix_lohi: torch.Tensor, mov_lohi: torch.Tensor, bins: int, stride,
                   work: torch.Tensor) -> torch.Tensor:
    """The int32 (bins, bins) table with pcms_joint_histogram enqueued on the current stream."""
    from ._lib import call
    host = (ctypes.c_double * 12)(*_data.affine12_of(A, t))  # read during the call (kernel arguments)
    hist = torch.empty((bins, bins), dtype=torch.int32, device=fix_raw.data.device)
    call("pcms_joint_histogram", fix_raw.data, int(fix_raw.code), *fix_raw.shape, float(fix_raw.slope),
         float(fix_raw.inter), fix_lohi, mov_raw.data, int(mov_raw.code), *mov_raw.shape, float(mov_raw.slope),
         float(mov_raw.inter), mov_lohi, ctypes.addressof(host), *stride, bins, hist, work)
    return hist


def _joint_work(bins: int, device) -> torch.Tensor:
    from ._lib import query
    return torch.empty(query("pcms_joint_histogram_work_bytes", bins) // 4, dtype=torch.int32, device=device)


def joint_histogram_device(fix_raw, mov_raw, A, t, fix_lohi, mov_lohi, bins: int = 32,
                           stride: Sequence[int] = (1, 1, 1)) -> torch.Tensor:
    """``joint_histogram`` on the GPU, on the counts exactly (pcms_joint_histogram): two
    ``RawVolume``s whose bytes are on one GPU in, a ``torch.int64`` (bins, bins) tensor there out,
    enqueued on the current stream.  ``fix_lohi`` / ``mov_lohi``: two fp32 values each, as device
    tensors (pcms_volume_minmax's or pcms_volume_window's, consumed where they are) or as host
    numbers (uploaded).  Host bytes raise; ValueError for what the entry point rejects."""
    bins, stride = _check_hist_args(bins, stride)
    fix_raw, mov_raw = _device_raw(fix_raw, "joint_histogram_device"), _device_raw(mov_raw, "joint_histogram_device")
    device = fix_raw.data.device
    if mov_raw.data.device != device:
        raise ValueError(f"the two volumes are on different devices: {device} and {mov_raw.data.device}")
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    if not (np.isfinite(A).all() and np.isfinite(t).all()):
        raise ValueError("the affine must be finite")
    with torch.cuda.device(device):
        hist = _joint_enqueue(fix_raw, mov_raw, A, t, _device_lohi(fix_lohi, device), _device_lohi(mov_lohi, device),
                              bins, stride, _joint_work(bins, device))
        return hist.to(torch.int64)


def _window_device(raw, norm: Optional[Normalisation]) -> torch.Tensor:
    """``_host_lohi`` on the device: two fp32 values from pcms_volume_window or pcms_volume_minmax."""
    lohi = torch.empty(2, dtype=torch.float32, device=raw.data.device)
    _lohi_enqueue(raw, norm if norm is not None and norm.method == "percentile" else Normalisation(), lohi)
    return lohi


def register_rigid_device(fix_raw, mov_raw, fix_geometry: dict, mov_geometry: dict, fix_lohi=None, mov_lohi=None,
                          normalise=None, settings=None) -> dict:
    """``register_rigid`` with pcms_joint_histogram as its evaluator: the same Python search, one
    small table read back per evaluation.  The counts are the host form's, so the search takes the
    same path and returns the same parameters, similarities and evaluation count exactly.
    ``fix_raw`` / ``mov_raw``: ``RawVolume``s whose bytes are on one GPU; the windows default to
    pcms_volume_window (a percentile ``normalise``) or pcms_volume_minmax."""
    settings = Alignment.of(settings) or Alignment()
    norm = Normalisation.of(normalise)
    fix_raw, mov_raw = _device_raw(fix_raw, "register_rigid_device"), _device_raw(mov_raw, "register_rigid_device")
    device = fix_raw.data.device
    if mov_raw.data.device != device:
        raise ValueError(f"the two volumes are on different devices: {device} and {mov_raw.data.device}")
    with torch.cuda.device(device):
        fl = _window_device(fix_raw, norm) if fix_lohi is None else _device_lohi(fix_lohi, device)
        ml = _window_device(mov_raw, norm) if mov_lohi is None else _device_lohi(mov_lohi, device)
        work = _joint_work(settings.bins, device)  # one workspace: the evaluations are ordered on the stream

        def evaluate(A, t, stride):
            return _joint_enqueue(fix_raw, mov_raw, A, t, fl, ml, settings.bins, stride, work).cpu().numpy()

        return _pattern_search(evaluate, tuple(fix_raw.shape), fix_geometry, mov_geometry, settings)


def _shape_of(path: str) -> Tuple[int, int, int]:
    return tuple(int(v) for v in read_nifti_header(path)["shape_xyz"][:3][::-1])


def _case_reference(paths: List[Optional[str]], align: Alignment) -> str:
    """The file whose grid an aligned case is formed on: ``align.to`` as a modality name (its file
    must be present) or a file path, else the first present modality's file."""
    if align.to is None:
        return next(p for p in paths if p is not None)
    if align.to in MODALITIES:
        p = paths[MODALITIES.index(align.to)]
        if p is None:
            raise FileNotFoundError(f"the reference modality {align.to!r} has no .nii file")
        return p
    if not os.path.exists(align.to):
        raise FileNotFoundError(f"Alignment.to is neither a modality of {MODALITIES} nor a file: {align.to!r}")
    return align.to


def _fixed_modality(paths: List[Optional[str]], align: Alignment) -> int:
    """The channel the other modalities are registered to: ``align.to`` when it names a present
    modality, else the first present one (a label or another file only lends its grid)."""
    present = [m for m, p in zip(MODALITIES, paths) if p is not None]
    return MODALITIES.index(_data.registration_fixed(MODALITIES, present, align.to))


def _aligned_affines(paths, grid, reference: str, corrections: Optional[dict], fixed: int):
    """Per present channel the ``(A, t)`` of ``data.case_affine`` from ``grid`` through the
    reference file's geometry into the channel's file, with its rigid correction (six parameters
    about the centre of channel ``fixed``'s file) when it has one."""
    ref_geo, ref_shape = _data.read_nifti_geometry(reference), _shape_of(reference)
    out = {}
    for c, p in enumerate(paths):
        if p is None:
            continue
        T = None
        if corrections is not None and corrections.get(MODALITIES[c]) is not None and c != fixed:
            T = _data.rigid_correction(corrections[MODALITIES[c]]["params"], _data.read_nifti_geometry(paths[fixed]),
                                       _shape_of(paths[fixed]))
        pair = _data.align_affine(ref_geo, _data.read_nifti_geometry(p), T)
        out[c] = _data.case_affine(np.eye(3), np.zeros(3), _shape_of(p), grid, (ref_shape, pair))
    return out


def register_case(case_dir_or_files, normalise=True, align="register") -> dict:
    """The host form of ``register_case_device``: ``register_rigid`` of every other present
    modality to the fixed one, ``{modality: result}``."""
    paths, settings = _register_inputs(case_dir_or_files, align)
    fixed = _fixed_modality(paths, settings)
    fix = _first_volume(read_nifti(paths[fixed]))
    geo = _data.read_nifti_geometry(paths[fixed])
    return {MODALITIES[c]: register_rigid(fix, _first_volume(read_nifti(p)), geo, _data.read_nifti_geometry(p),
                                          normalise=normalise, settings=settings)
            for c, p in enumerate(paths) if p is not None and c != fixed}


def _register_inputs(case_dir_or_files, align):
    settings = Alignment.of(align) or Alignment(mode="register")
    if isinstance(case_dir_or_files, dict):
        unknown = [m for m in case_dir_or_files if m not in MODALITIES]
        if unknown:
            raise ValueError(f"unknown modalities {unknown}: the files are keyed by {MODALITIES}")
        paths = [case_dir_or_files.get(m) for m in MODALITIES]
    else:
        paths = _case_files(case_dir_or_files)
    if all(p is None for p in paths):
        raise FileNotFoundError(f"no modality file in {case_dir_or_files!r}")
    return paths, settings


def register_case_device(case_dir_or_files, normalise=True, align="register", device="cuda", raws=None) -> dict:
    """Rigid registration of a case's modalities on the GPU: ``{modality: register_rigid_device's
    result}`` for every present modality but the fixed one -- ``align.to`` when it names a present
    modality, else the first present one.  ``case_dir_or_files``: a case directory
    (``<dir>/<modality>/*.nii``) or a ``{modality: path}`` dict.  The windows follow ``normalise``
    (min-max when it is off).  Each file's bytes go up once (``raws``: channels already there)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"register_case_device needs a GPU, not '{device}': pcms_amd has no CPU fallback -- "
                           "use predict.register_case on the host")
    paths, settings = _register_inputs(case_dir_or_files, align)
    norm = Normalisation.of(normalise)
    fixed = _fixed_modality(paths, settings)
    raws = dict(raws or {})
    with torch.cuda.device(device):
        for c, p in enumerate(paths):
            if p is not None and c not in raws:
                raws[c] = _data.read_nifti_raw(p).to(device)
        geo = _data.read_nifti_geometry(paths[fixed])
        fl = _window_device(raws[fixed], norm)
        return {MODALITIES[c]: register_rigid_device(raws[fixed], raws[c], geo, _data.read_nifti_geometry(p),
                                                     fix_lohi=fl, normalise=norm, settings=settings)
                for c, p in enumerate(paths) if p is not None and c != fixed}


def register_dataset(dataset, device="cuda", normalise=True, align="register") -> dict:
    """``{case_id: {modality: [tz, ty, tx, rz, ry, rx]}}`` for every case of a ``ProstateDataset``
    (or a ``Subset`` of one): ``register_case_device`` of the case's files, JSON-serialisable --
    the ``corrections`` a dataset takes.  Produce it with the ``to`` the dataset will align with:
    the fixed modality is chosen from it (``"label"`` or None: the first present modality)."""
    base = getattr(dataset, "dataset", dataset)
    indices = getattr(dataset, "indices", range(len(base.case_list)))
    out = {}
    for i in indices:
        case = base.case_list[i]
        files = {m: p for m, p in case["modality_files"].items() if m in MODALITIES}
        res = register_case_device(files, normalise, align, device)
        out[case["case_id"]] = {m: [float(v) for v in r["params"]] for m, r in res.items()}
    return out


def prepare_case(case_dir: str, target_size: Optional[Sequence[int]] = (128, 128, 128),
                 handle_missing: str = "zero_fill", normalise=True, align=None,
                 return_alignment: bool = False) -> np.ndarray:
    """The five modalities of a case on one grid, (5, D, H, W) float32: per modality the first
    ``.nii`` in sorted order (volume 0 of a 4-D file), ``normalise``d when asked, else as fp32,
    then ``data.resample(., target_size)`` (linear).  A missing modality is zeros
    ('zero_fill'), the first present modality's channel ('duplicate') or an error ('skip').
    ``target_size=None``: no resampling; the present shapes must agree (ValueError).
    With ``normalise=False`` a channel is the one the default training loader forms for the
    file; with ``normalise=True`` it is ``load_multimodal_images``' channel on the grid.
    ``normalise`` is anything ``Normalisation.of`` accepts: ``"percentile"`` (or a dict / a
    ``Normalisation``) clips every modality to its own percentile window first.
    ``align`` (anything ``Alignment.of`` accepts; None: everything above, unchanged): every present
    modality is resampled by ``data.resample_affine`` under ``data.case_affine`` -- the grid scaled
    onto the reference file's native grid, then ``data.align_affine`` into the modality's file -- so
    the channels show one place in space whatever each file's field of view, spacing and
    orientation; a grid voxel outside a file's field of view reads 0.  The reference is
    ``align.to`` (a modality name or a file path; default: the first present modality's file) and
    ``target_size=None`` is its native grid; the modalities' shapes may differ.  ``"register"``
    first registers every other modality to the fixed one (``register_case``) and puts the
    correction into its affine.  ``return_alignment=True`` returns ``(channels, alignment)``, the
    second as ``CasePrediction.alignment`` carries it."""
    norm = Normalisation.of(normalise)
    align = Alignment.of(align)
    paths, grid, dup = _case_plan(case_dir, target_size, handle_missing, align)
    affines, report = None, None
    if align is not None:
        fixed = _fixed_modality(paths, align)
        if align.mode == "register":
            report = register_case(dict(zip(MODALITIES, paths)), normalise, align)
        affines = _aligned_affines(paths, grid, _case_reference(paths, align), report, fixed)
    chans: List[Optional[np.ndarray]] = []
    for c, p in enumerate(paths):
        if p is None:
            chans.append(None)
            continue
        vol = _first_volume(read_nifti(p))
        vol = norm.apply(vol) if norm is not None else vol.astype(np.float32)
        chans.append(_data.resample(vol, grid) if affines is None else _data.resample_affine(vol, grid, *affines[c]))
    fill = np.zeros(grid, dtype=np.float32) if dup is None else chans[dup]
    x = np.stack([fill if c is None else c for c in chans], axis=0)
    return (x, _alignment_report(paths, align, report)) if return_alignment else x


def _alignment_report(paths, align: Optional["Alignment"], report: Optional[dict]) -> Optional[dict]:
    """``CasePrediction.alignment``: per present modality the six parameters and the similarity
    before and after (zeros and None for header alignment alone and for the fixed modality);
    None without ``align``."""
    if align is None:
        return None
    out = {}
    for m, p in zip(MODALITIES, paths):
        if p is None:
            continue
        r = (report or {}).get(m)
        out[m] = {"params": (0.0,) * 6, "before": None, "after": None} if r is None else \
            {"params": r["params"], "before": r["before"], "after": r["after"]}
    return out


def tta_mean(probs: Sequence[np.ndarray], flips: Sequence[Tuple[int, ...]]) -> np.ndarray:
    """Test-time-augmentation mean, (D, H, W) float32: ``probs[j]`` is the probability volume
    of the input flipped along the axes ``flips[j]`` (out of 0, 1, 2; ``flips[0]`` must be
    ``()``), flipped back and summed in order in fp32, divided by ``float32(k)``."""
    flips = [tuple(int(a) for a in f) for f in flips]
    if len(probs) != len(flips) or not flips or flips[0] != ():
        raise ValueError("tta_mean needs one flip set per volume, the first of them ()")
    acc = np.asarray(probs[0], dtype=np.float32)
    for p, f in zip(probs[1:], flips[1:]):
        acc = acc + np.flip(np.asarray(p, dtype=np.float32), f)
    return acc / np.float32(len(flips))


def mask_on_grid(prob: np.ndarray, native_shape: Sequence[int], threshold: float = 0.5):
    """A probability volume on the training grid -> ``(uint8 mask, float32 probabilities)`` on
    the ``native_shape`` grid: ``data.resample(prob.astype(float32), native_shape)`` and its
    strict ``> float32(threshold)``.  This is the exact inverse geometry of the forward map:
    native index i samples target coordinate ``i * n_tgt / n_nat``.  ``data.resample``'s edge
    rule holds here too: a sample at or past ``n_tgt - 0.5`` is 0, so where the native grid is
    finer than the training grid the trailing fraction of a training voxel reads as
    background."""
    prob_native = _data.resample(np.asarray(prob).astype(np.float32), tuple(int(v) for v in native_shape))
    return (prob_native > np.float32(threshold)).astype(np.uint8), prob_native


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


def _volume(mask) -> np.ndarray:
    mask = np.asarray(mask)
    if mask.ndim != 3 or 0 in mask.shape:
        raise ValueError(f"a mask is a non-empty (D, H, W) volume, got shape {mask.shape}")
    return mask


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
    fg = _volume(mask) != 0
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
    fg = _volume(mask) != 0
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


def _device_mask(mask, what: str) -> torch.Tensor:
    if not isinstance(mask, torch.Tensor) or mask.device.type != "cuda":
        where = mask.device if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise RuntimeError(f"{what} needs a uint8 tensor on the GPU, not '{where}': pcms_amd has no CPU fallback -- "
                           "use the host form of the same name without _device")
    if mask.dtype != torch.uint8 or mask.dim() != 3 or mask.numel() == 0:
        raise ValueError(f"{what} takes a non-empty uint8 (D, H, W) tensor, got {mask.dtype} {tuple(mask.shape)}")
    return mask.contiguous()


def _components_work(mask: torch.Tensor) -> torch.Tensor:
    from ._lib import query
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
    from ._lib import call
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
    mask = _device_mask(mask, "postprocess_device")
    with torch.cuda.device(mask.device):
        out, work = _postprocess_enqueue(mask, keep_largest, min_voxels, fill_holes, connectivity)
        _check_status(int(work[0].item()), "postprocess_device")
    return out


def label_components_device(mask: torch.Tensor, connectivity: int = 26, invert: bool = False) -> torch.Tensor:
    """``label_components`` on the GPU, bit for bit (pcms_components_label): int32 (D, H, W), the
    lesion map.  ``invert=True`` labels the zero voxels instead.  A CPU tensor raises."""
    from ._lib import call
    mask = _device_mask(mask, "label_components_device")
    _offsets(connectivity)
    with torch.cuda.device(mask.device):
        labels = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
        work = _components_work(mask)
        call("pcms_components_label", mask, int(bool(invert)), int(connectivity), labels, work, *mask.shape)
        _check_status(int(work[0].item()), "label_components_device")
    return labels


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
    lab = _volume(labels)
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
    a, b = _volume(labels_a), _volume(labels_b)
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


def _device_volume(t, dtype, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what} needs tensors on the GPU, not '{where}': pcms_amd has no CPU fallback -- "
                           "use the host form of the same name without _device")
    if t.dtype != dtype or t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{what} takes a non-empty {dtype} (D, H, W) tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _table_enqueue(labels: torch.Tensor, prob: Optional[torch.Tensor], capacity: int):
    """(table bytes as int64, header) with pcms_component_table enqueued on the current stream."""
    from ._lib import call, query
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
    labels = _device_volume(labels, torch.int32, "component_table_device")
    if prob is not None:
        prob = _device_volume(prob, torch.float32, "component_table_device")
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
    a = _device_volume(labels_a, torch.int32, "overlap_pairs_device")
    b = _device_volume(labels_b, torch.int32, "overlap_pairs_device")
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
    mask = _device_mask(mask, "lesion_table_device")
    table = component_table_device(label_components_device(mask, connectivity), prob)
    return _lesion_rows(table, tuple(mask.shape), sp)


def lesion_metrics_device(pred: torch.Tensor, ref: torch.Tensor, prob: Optional[torch.Tensor] = None,
                          spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26,
                          min_iou: float = 0.1) -> dict:
    """``lesion_metrics`` on the GPU: labels, tables and overlap pairs from the kernels, matching
    and every fp64 quantity on the host by the host form's own functions, so the result is equal.
    uint8 CUDA masks (and optionally fp32 CUDA probabilities) in; CPU tensors raise."""
    sp = _spacing(spacing)
    pred = _device_mask(pred, "lesion_metrics_device")
    ref = _device_mask(ref, "lesion_metrics_device")
    if pred.shape != ref.shape or pred.device != ref.device:
        raise ValueError(f"the masks are on different grids or devices: {tuple(pred.shape)} on {pred.device} and "
                         f"{tuple(ref.shape)} on {ref.device}")
    lp, lr = label_components_device(pred, connectivity), label_components_device(ref, connectivity)
    return _lesion_report(component_table_device(lp, prob), component_table_device(lr),
                          overlap_pairs_device(lp, lr, connectivity), tuple(pred.shape), sp, min_iou)


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
    fg = _volume(mask) != 0
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
    f = _volume(feat) != 0
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
    from ._lib import query
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
    from ._lib import call
    mask = _device_mask(mask, "surface_device")
    _edt_work_bytes(mask)  # the size check
    with torch.cuda.device(mask.device):
        out = torch.empty_like(mask)
        call("pcms_mask_surface", mask, out, *mask.shape)
    return out


def _edt_sq_enqueue(feat: torch.Tensor, sp, work: torch.Tensor) -> torch.Tensor:
    from ._lib import call
    out = torch.empty(feat.shape, dtype=torch.float64, device=feat.device)
    host = (ctypes.c_double * 3)(*sp)  # read during the call (kernel arguments)
    call("pcms_edt_sq", feat, ctypes.addressof(host), out, work, *feat.shape)
    return out


def distance_transform_device(mask: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                              squared: bool = False) -> torch.Tensor:
    """``distance_transform`` on the GPU (pcms_edt_sq): fp64 (D, H, W); with ``squared=True``
    equal to ``edt_sq`` bit for bit, else its ``torch.sqrt``.  A CPU tensor raises."""
    sp = _spacing(spacing)
    mask = _device_mask(mask, "distance_transform_device")
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
    from ._lib import call
    sp = _spacing(spacing)
    a = _device_mask(a, "surface_metrics_device")
    b = _device_mask(b, "surface_metrics_device")
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


def _flip_masks(flips) -> List[int]:
    """Flip sets (tuples of axes out of 0, 1, 2) as pcms_flip_mean's bit masks, () first."""
    masks = [0]
    for f in flips:
        f = tuple(int(a) for a in f)
        if not f or any(a not in (0, 1, 2) for a in f) or len(set(f)) != len(f):
            raise ValueError(f"a flip set holds distinct axes out of (0, 1, 2), got {f!r}")
        masks.append(sum(1 << a for a in f))
    return masks


# ---- sliding-window prediction --------------------------------------------------
# Fixed-size windows slide over a (D, H, W) grid; the row index of ``window_grid`` is *the* window
# index: entries, batches and the blend's order all follow it.  The host forms below define what
# csrc/window.hip computes, bit for bit: every product, sum and quotient rounds on its own in fp32.
MAX_WINDOW_AXIS = 512  # the blend kernel keeps three weight tables of this length in LDS; host forms agree


def window_starts(n: int, w: int, overlap: float) -> List[int]:
    """The window starts along one axis of ``n`` voxels for windows of ``w``: with
    ``step = max(1, int(w * (1.0 - overlap)))``, ``[0]`` when ``n <= w`` (the window sticks out
    past the volume), else ``ceil((n - w) / step) + 1`` starts ``min(i * step, n - w)``: the last
    window is flush with the end.  ValueError for ``w < 1``, ``n < 1`` or ``overlap`` outside
    ``[0, 1)``."""
    n, w, overlap = int(n), int(w), float(overlap)
    if w < 1 or n < 1 or not 0.0 <= overlap < 1.0:
        raise ValueError(f"window_starts needs n >= 1, w >= 1 and 0 <= overlap < 1, got {n}, {w}, {overlap}")
    step = max(1, int(w * (1.0 - overlap)))
    if n <= w:
        return [0]
    count = -(-(n - w) // step) + 1
    return [min(i * step, n - w) for i in range(count)]


def _three(v, what: str, cast=int) -> tuple:
    try:
        out = tuple(cast(a) for a in v)
    except TypeError:
        raise ValueError(f"{what} is three values (d, h, w), got {v!r}") from None
    if len(out) != 3:
        raise ValueError(f"{what} is three values (d, h, w), got {v!r}")
    return out


def window_grid(shape: Sequence[int], window: Sequence[int], overlap=0.5) -> np.ndarray:
    """All window starts on a (D, H, W) grid, int32 (K, 3): the Cartesian product of the three
    axes' ``window_starts``, d-major, then h, then w.  ``overlap`` is a scalar or one value per
    axis."""
    shape, window = _three(shape, "shape"), _three(window, "window")
    overlap = (float(overlap),) * 3 if np.ndim(overlap) == 0 else _three(overlap, "overlap", float)
    axes = [window_starts(n, w, o) for n, w, o in zip(shape, window, overlap)]
    return np.array([(a, b, c) for a in axes[0] for b in axes[1] for c in axes[2]], dtype=np.int32)


def window_weights(window: Sequence[int], blend: str = "gaussian",
                   sigma_scale: float = 0.125) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The per-axis blend weights of a window, three fp32 vectors (wd, wh, ww): 'gaussian' is
    ``exp(-0.5 * ((i - (w - 1) / 2) / (sigma_scale * w)) ** 2)`` in float64 cast to fp32,
    'constant' is ones.  The weight of window voxel (a, b, c) is
    ``fl32(fl32(wd[a] * wh[b]) * ww[c])``."""
    window = _three(window, "window")
    if any(w < 1 for w in window):
        raise ValueError(f"a window axis is at least 1, got {window}")
    if blend == "constant":
        return tuple(np.ones(w, dtype=np.float32) for w in window)
    if blend != "gaussian" or not float(sigma_scale) > 0.0:
        raise ValueError(f"blend is 'gaussian' (with sigma_scale > 0) or 'constant', got {blend!r}, {sigma_scale!r}")
    out = []
    for w in window:
        i = np.arange(w, dtype=np.float64)
        out.append(np.exp(-0.5 * ((i - (w - 1) / 2) / (float(sigma_scale) * w)) ** 2).astype(np.float32))
    return tuple(out)


def _window_args(starts, window, flips):
    """(starts as int64 (K, 3), window, pcms flip masks): what the four window forms check alike."""
    window = _three(window, "window")
    if any(not 1 <= w <= MAX_WINDOW_AXIS for w in window):
        raise ValueError(f"a window axis is in 1..{MAX_WINDOW_AXIS}, got {window}")
    starts = np.asarray(starts)
    if starts.ndim != 2 or starts.shape[1] != 3 or len(starts) == 0 or starts.dtype.kind not in "iu":
        raise ValueError(f"starts is a non-empty integer (K, 3) array, got {starts.dtype} {starts.shape}")
    return starts.astype(np.int64), window, _flip_masks(flips)


def _check_starts(starts: np.ndarray, shape) -> None:
    if (starts < 0).any() or (starts >= np.asarray(shape, np.int64)).any():
        raise ValueError(f"a window start lies outside the volume {tuple(shape)}")


def gather_windows(x: np.ndarray, starts, window: Sequence[int],
                   flips: Sequence[Tuple[int, ...]] = ()) -> np.ndarray:
    """The windows of a (C, D, H, W) volume as one network batch, float32
    (K * k, C, wd, wh, ww) with ``k = 1 + len(flips)``: entry ``i * k`` is window ``i`` (row ``i``
    of ``starts``), zero where it sticks out past the volume; entry ``i * k + j`` is that window
    flipped along ``flips[j - 1]`` -- the window is flipped, not the volume."""
    starts, window, masks = _window_args(starts, window, flips)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4 or 0 in x.shape:
        raise ValueError(f"gather_windows takes a non-empty (C, D, H, W) volume, got shape {x.shape}")
    _check_starts(starts, x.shape[1:])
    k = len(masks)
    out = np.zeros((len(starts) * k, x.shape[0]) + window, dtype=np.float32)
    for i, s in enumerate(starts.tolist()):
        n = [min(w, dim - a) for w, dim, a in zip(window, x.shape[1:], s)]
        win = out[i * k]
        win[:, :n[0], :n[1], :n[2]] = x[:, s[0]:s[0] + n[0], s[1]:s[1] + n[1], s[2]:s[2] + n[2]]
        for j, f in enumerate(flips, start=1):
            out[i * k + j] = np.flip(win, [1 + int(a) for a in f])
    return out


def _weight_vectors(weights, window) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    if len(weights) != 3:
        raise ValueError("weights are three vectors (wd, wh, ww)")
    weights = tuple(np.asarray(v) for v in weights)
    if any(v.dtype != np.float32 or v.shape != (w,) for v, w in zip(weights, window)):
        raise ValueError(f"weights are three float32 vectors of lengths {window}")
    return weights


def blend_windows(probs: np.ndarray, starts, window: Sequence[int], weights, shape: Sequence[int],
                  flips: Sequence[Tuple[int, ...]] = ()) -> np.ndarray:
    """The weighted blend of window probabilities on the (D, H, W) grid ``shape``, float32.
    ``probs`` is (K * k, wd, wh, ww) in ``gather_windows``' entry order.  In ascending window
    index ``m_i = tta_mean(probs[i*k:(i+1)*k], ((),) + flips)``, then over the part of the window
    inside the volume ``acc = acc + wgt * m_i`` (the product rounded, then the sum) and
    ``wsum = wsum + wgt``, with ``wgt = (wd[a] * wh[b]) * ww[c]`` from ``weights``; the result is
    ``acc / wsum``."""
    starts, window, masks = _window_args(starts, window, flips)
    shape = _three(shape, "shape")
    weights = _weight_vectors(weights, window)
    k = len(masks)
    probs = np.asarray(probs, dtype=np.float32)
    if probs.shape != (len(starts) * k,) + window:
        raise ValueError(f"probs is {(len(starts) * k,) + window}, got {probs.shape}")
    _check_starts(starts, shape)
    wgt = (weights[0][:, None, None] * weights[1][None, :, None]) * weights[2][None, None, :]
    acc = np.zeros(shape, dtype=np.float32)
    wsum = np.zeros(shape, dtype=np.float32)
    all_flips = [()] + [tuple(f) for f in flips]
    for i, s in enumerate(starts.tolist()):
        m = tta_mean(list(probs[i * k:(i + 1) * k]), all_flips)
        n = [min(w, dim - a) for w, dim, a in zip(window, shape, s)]
        box = (slice(s[0], s[0] + n[0]), slice(s[1], s[1] + n[1]), slice(s[2], s[2] + n[2]))
        part = (slice(0, n[0]), slice(0, n[1]), slice(0, n[2]))
        acc[box] = acc[box] + wgt[part] * m[part]
        wsum[box] = wsum[box] + wgt[part]
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / wsum


def _check_sliding(window, overlap, blend, window_batch) -> tuple:
    """The window as a tuple, after the checks every sliding-window driver makes first."""
    window = _three(window, "window")
    window_weights(window, blend)          # a bad window axis or blend
    window_grid(window, window, overlap)   # a bad overlap
    if any(w > MAX_WINDOW_AXIS for w in window):
        raise ValueError(f"a window axis is at most {MAX_WINDOW_AXIS}, got {window}")
    if not isinstance(window_batch, (int, np.integer)) or window_batch < 1:
        raise ValueError(f"window_batch is an integer >= 1, got {window_batch!r}")
    return window


def _batch_plan(K: int, window_batch: int) -> List[Tuple[int, int]]:
    """(first window, windows that count) per ``predict_fn`` call: every call carries
    ``window_batch`` windows, the last one padded with repeats of window K - 1."""
    return [(f, min(window_batch, K - f)) for f in range(0, K, window_batch)]


def sliding_window_predict(predict_fn, x: np.ndarray, window: Sequence[int], overlap=0.5, blend: str = "gaussian",
                           tta_flips: Sequence[Tuple[int, ...]] = (), window_batch: int = 4) -> np.ndarray:
    """Sliding-window prediction on the host, (D, H, W) float32 from a (C, D, H, W) volume:
    ``gather_windows`` over ``window_grid(x.shape[1:], window, overlap)``, ``predict_fn`` --
    ``(N, C, wd, wh, ww) -> (N, 1, wd, wh, ww)`` -- on batches of exactly ``window_batch * k``
    entries (``k = 1 + len(tta_flips)``; the last batch is padded with repeats of the final
    window, whose outputs are dropped), then ``blend_windows`` with ``window_weights(window,
    blend)``."""
    window = _check_sliding(window, overlap, blend, window_batch)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4:
        raise ValueError(f"sliding_window_predict takes a (C, D, H, W) volume, got shape {x.shape}")
    starts = window_grid(x.shape[1:], window, overlap)
    tiles = gather_windows(x, starts, window, tta_flips)
    K, k = len(starts), 1 + len(tta_flips)
    outs = []
    for first, real in _batch_plan(K, int(window_batch)):
        batch = tiles[first * k:(first + real) * k]
        if real < window_batch:
            batch = np.concatenate([batch] + [tiles[(K - 1) * k:]] * (window_batch - real))
        p = np.asarray(predict_fn(batch), dtype=np.float32)
        if p.shape != (window_batch * k, 1) + window:
            raise ValueError(f"predict_fn returned {p.shape}, not {(window_batch * k, 1) + window}")
        outs.append(p[:real * k, 0])
    return blend_windows(np.concatenate(outs), starts, window, window_weights(window, blend), x.shape[1:], tta_flips)


def _device_float(t, ndim: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what} needs tensors on the GPU, not '{where}': pcms_amd has no CPU fallback -- "
                           "use the host form of the same name without _device")
    if t.dtype != torch.float32 or t.dim() != ndim or t.numel() == 0:
        raise ValueError(f"{what} takes a non-empty float32 tensor of {ndim} dimensions, got {t.dtype} "
                         f"{tuple(t.shape)}")
    return t.contiguous()


def _host_ints(values):
    return (ctypes.c_int * len(values))(*values)  # read during the call (kernel arguments)


def _gather_enqueue(x: torch.Tensor, starts_dev: torch.Tensor, B: int, masks, window, out: torch.Tensor) -> None:
    """pcms_window_gather of the B windows at ``starts_dev`` (device int32, B rows) into ``out``."""
    from ._lib import call
    host = _host_ints(masks)
    call("pcms_window_gather", x, *x.shape, starts_dev, int(B), ctypes.addressof(host), len(masks), *window, out)


def gather_windows_device(x: torch.Tensor, starts, window: Sequence[int],
                          flips: Sequence[Tuple[int, ...]] = ()) -> torch.Tensor:
    """``gather_windows`` on the GPU, bit for bit (pcms_window_gather): a float32 CUDA volume
    (C, D, H, W) and the (K, 3) starts (a host array) in, the (K * k, C, wd, wh, ww) batch out,
    enqueued on the current stream.  A CPU tensor raises."""
    starts, window, masks = _window_args(starts, window, flips)
    x = _device_float(x, 4, "gather_windows_device")
    _check_starts(starts, x.shape[1:])
    with torch.cuda.device(x.device):
        starts_dev = torch.from_numpy(starts.astype(np.int32)).to(x.device)
        out = torch.empty((len(starts) * len(masks), x.shape[0]) + window, dtype=torch.float32, device=x.device)
        _gather_enqueue(x, starts_dev, len(starts), masks, window, out)
    return out


def _blend_enqueue(probs: torch.Tensor, starts_dev: torch.Tensor, first: int, B: int, masks, wts: torch.Tensor,
                   window, acc: torch.Tensor, wsum: torch.Tensor) -> None:
    """pcms_window_blend of windows first .. first + B - 1 of the whole table ``starts_dev``."""
    from ._lib import call
    host = _host_ints(masks)
    call("pcms_window_blend", probs, starts_dev, int(first), int(B), ctypes.addressof(host), len(masks), wts, *window,
         acc, wsum, *acc.shape)


def _finish_enqueue(acc: torch.Tensor, wsum: torch.Tensor) -> torch.Tensor:
    from ._lib import call
    prob = torch.empty_like(acc)
    call("pcms_window_finish", acc, wsum, prob, acc.numel())
    return prob


def blend_windows_device(probs: torch.Tensor, starts, window: Sequence[int], weights, shape: Sequence[int],
                         flips: Sequence[Tuple[int, ...]] = (), batch: Optional[int] = None) -> torch.Tensor:
    """``blend_windows`` on the GPU, bit for bit: pcms_window_blend over consecutive batches of
    ``batch`` windows (all K in one launch by default; the bits do not depend on it), then
    pcms_window_finish.  ``probs`` is a float32 CUDA tensor (K * k, wd, wh, ww); ``starts`` and
    ``weights`` are host arrays.  Returns the (D, H, W) float32 CUDA tensor.  A CPU tensor raises."""
    starts, window, masks = _window_args(starts, window, flips)
    shape = _three(shape, "shape")
    weights = _weight_vectors(weights, window)
    probs = _device_float(probs, 4, "blend_windows_device")
    K, k = len(starts), len(masks)
    if tuple(probs.shape) != (K * k,) + window:
        raise ValueError(f"probs is {(K * k,) + window}, got {tuple(probs.shape)}")
    _check_starts(starts, shape)
    batch = K if batch is None else int(batch)
    if batch < 1:
        raise ValueError(f"batch is an integer >= 1, got {batch!r}")
    with torch.cuda.device(probs.device):
        starts_dev = torch.from_numpy(starts.astype(np.int32)).to(probs.device)
        wts = torch.from_numpy(np.concatenate(weights)).to(probs.device)
        acc = torch.zeros(shape, dtype=torch.float32, device=probs.device)
        wsum = torch.zeros(shape, dtype=torch.float32, device=probs.device)
        for first, real in _batch_plan(K, batch):
            _blend_enqueue(probs[first * k:(first + real) * k], starts_dev, first, real, masks, wts, window, acc, wsum)
        return _finish_enqueue(acc, wsum)


def sliding_window_device(predict_fn, x: torch.Tensor, window: Sequence[int], overlap=0.5, blend: str = "gaussian",
                          tta_flips: Sequence[Tuple[int, ...]] = (), window_batch: int = 4) -> torch.Tensor:
    """``sliding_window_predict`` on the GPU: ``x`` is the (1, C, D, H, W) float32 CUDA tensor of
    ``prepare_case_device``; per batch pcms_window_gather forms the ``window_batch * k`` entries
    (the last batch padded with repeats of the final window, so ``predict_fn`` sees one shape
    only), ``predict_fn`` maps them to (N, 1, wd, wh, ww) probabilities on the device, and
    pcms_window_blend accumulates the windows that count; pcms_window_finish divides.  Returns
    the (D, H, W) float32 probabilities on the device; everything is enqueued on the current
    stream.  A CPU tensor raises."""
    window = _check_sliding(window, overlap, blend, window_batch)
    masks = _flip_masks(tta_flips)
    x = _device_float(x, 5, "sliding_window_device")
    if x.shape[0] != 1:
        raise ValueError(f"sliding_window_device takes one case, (1, C, D, H, W), got {tuple(x.shape)}")
    vol, shape = x[0], tuple(x.shape[2:])
    starts = window_grid(shape, window, overlap)
    K, k, wb = len(starts), len(masks), int(window_batch)
    plan = _batch_plan(K, wb)
    padded = np.concatenate([starts] + [starts[-1:]] * (len(plan) * wb - K))
    with torch.cuda.device(x.device):
        starts_dev = torch.from_numpy(padded).to(x.device)
        wts = torch.from_numpy(np.concatenate(window_weights(window, blend))).to(x.device)
        acc = torch.zeros(shape, dtype=torch.float32, device=x.device)
        wsum = torch.zeros(shape, dtype=torch.float32, device=x.device)
        batch = torch.empty((wb * k, vol.shape[0]) + window, dtype=torch.float32, device=x.device)
        for first, real in plan:
            _gather_enqueue(vol, starts_dev[first:first + wb], wb, masks, window, batch)
            probs = predict_fn(batch)
            if not isinstance(probs, torch.Tensor) or tuple(probs.shape) != (wb * k, 1) + window \
                    or probs.device != x.device:
                got = tuple(probs.shape) if isinstance(probs, torch.Tensor) else type(probs).__name__
                raise ValueError(f"predict_fn returned {got}, not a {(wb * k, 1) + window} tensor on {x.device}")
            probs = probs.float().contiguous()
            _blend_enqueue(probs, starts_dev, first, real, masks, wts, window, acc, wsum)
        return _finish_enqueue(acc, wsum)


def prepare_case_device(case_dir: str, target_size: Optional[Sequence[int]] = (128, 128, 128),
                        handle_missing: str = "zero_fill", normalise=True,
                        device="cuda", align=None, return_alignment: bool = False) -> torch.Tensor:
    """``prepare_case`` on the GPU, bit for bit, as the (1, 5, D, H, W) fp32 network input: each
    file's undecoded bytes (``data.read_nifti_raw``) go up once; pcms_volume_minmax and
    pcms_resample_linear_norm form the min-max normalised channel, pcms_volume_window and
    pcms_resample_linear_window the percentile one (the window is computed once per volume and
    read from device memory), ``data.resample_device`` the plain one.  Everything is enqueued on
    the current stream.
    ``align``: ``prepare_case``'s, bit for bit too.  Per present modality one launch under the
    twelve doubles of ``data.case_affine`` -- the host form's own -- fills the channel:
    pcms_patch_resample_linear / pcms_patch_resample_window with one patch at origin 0 that is the
    whole grid (the normalised corners), or pcms_resample_affine_linear without normalisation.
    ``"register"`` runs ``register_case_device`` on the uploaded bytes first (it reads one small
    table back per evaluation).  ``align=None``: nothing new is launched."""
    from ._lib import call
    norm = Normalisation.of(normalise)
    align = Alignment.of(align)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"prepare_case_device needs a GPU, not '{device}': pcms_amd has no CPU fallback -- "
                           "use predict.prepare_case on the host")
    paths, grid, dup = _case_plan(case_dir, target_size, handle_missing, align)
    report = None
    with torch.cuda.device(device):
        x = torch.empty((1, len(paths)) + grid, dtype=torch.float32, device=device)
        lohi = torch.empty(2, dtype=torch.float32, device=device)
        raws = {c: _data.read_nifti_raw(p).to(device) for c, p in enumerate(paths) if p is not None}
        affines = None
        if align is not None:
            if align.mode == "register":
                report = register_case_device(dict(zip(MODALITIES, paths)), normalise, align, device, raws)
            affines = _aligned_affines(paths, grid, _case_reference(paths, align), report,
                                       _fixed_modality(paths, align))
            origin = torch.zeros(3, dtype=torch.int32, device=device)
        for c, raw in raws.items():
            if affines is not None:
                twelve = _data.affine12_of(*affines[c])
                if norm is None:
                    _data.resample_device(raw, grid, out=x[0, c], affine=twelve)
                    continue
                windowed = _lohi_enqueue(raw, norm, lohi) == "window"
                host = (ctypes.c_double * 12)(*twelve)  # read during the call (kernel arguments)
                call("pcms_patch_resample_window" if windowed else "pcms_patch_resample_linear", raw.data,
                     int(raw.code), *raw.shape, float(raw.slope), float(raw.inter), ctypes.addressof(host), lohi, 1.0,
                     0.0, *grid, origin, 1, x[0, c], grid[0] * grid[1] * grid[2], *grid)
                continue
            if norm is None:
                _data.resample_device(raw, grid, out=x[0, c])
                continue
            kind = _lohi_enqueue(raw, norm, lohi)
            call("pcms_resample_linear_" + kind, raw.data, int(raw.code), *raw.shape, float(raw.slope),
                 float(raw.inter), lohi, x[0, c], *grid)
        for c, p in enumerate(paths):
            if p is None and dup is None:
                x[0, c].zero_()
            elif p is None:
                x[0, c].copy_(x[0, dup])
    return (x, _alignment_report(paths, align, report)) if return_alignment else x


@dataclasses.dataclass
class CasePrediction:
    """``ModelPredictor.predict_case``'s result: the uint8 ``mask`` and, when asked for, the fp32
    ``probability`` on the native (z, y, x) grid of ``reference_path``, whose
    ``data.read_nifti_geometry`` is ``geometry``; ``lesions`` is ``lesion_table`` of the mask when
    ``predict_case`` was asked for it; ``alignment``: with ``align``, per present modality
    ``{"params": (tz, ty, tx, rz, ry, rx), "before": .., "after": ..}`` -- the rigid correction
    and the similarity before and after it (zeros and None where nothing was registered) -- else
    None."""
    mask: np.ndarray
    probability: Optional[np.ndarray]
    reference_path: str
    geometry: dict
    lesions: Optional[List[dict]] = None
    alignment: Optional[dict] = None


def preprocess_image(image: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(image)).float().unsqueeze(0)


class ModelPredictor:
    def __init__(self, model_path: str, device: str = "cuda", precision: str = "bf16"):
        self.device = torch.device(device)
        self.model = UNet3D(n_modalities=5, n_classes=1, precision=precision).to(self.device)
        load_weights(self.model, model_path)
        self.model.eval()

    def predict(self, image_tensor: torch.Tensor) -> np.ndarray:
        with torch.no_grad():
            out = self.model.predict(image_tensor.to(self.device))
        return out.squeeze(0).squeeze(0).cpu().numpy()

    def saliency(self, image_tensor: torch.Tensor) -> np.ndarray:
        """Input attribution of one case: d(sum of sigmoid(logits)) / d(input) as a (5, D, H, W)
        float32 array -- which modality and which voxels drive the predicted lesion volume.
        Eval mode (running BatchNorm statistics); no parameter gradient is touched."""
        x = image_tensor.to(self.device).float().detach().requires_grad_(True)
        self.model.eval()
        with torch.enable_grad():
            torch.sigmoid(self.model(x)).sum().backward()
        return x.grad.squeeze(0).float().cpu().numpy()

    def save_prediction(self, prediction: np.ndarray, output_path: str,
                        reference_image_path: Optional[str] = None) -> None:
        spacing = (1.0, 1.0, 1.0)
        if reference_image_path and os.path.exists(reference_image_path):
            spacing = read_nifti_header(reference_image_path)["spacing"][:3]
        write_nifti(output_path, (prediction > 0.5).astype(np.uint8), spacing=spacing)

    def predict_case(self, case_dir: str, target_size: Optional[Sequence[int]] = (128, 128, 128),
                     handle_missing: str = "zero_fill", normalise=True, threshold: float = 0.5,
                     tta_flips: Sequence[Tuple[int, ...]] = (), output_like: Optional[str] = None,
                     return_probability: bool = False, *, keep_largest: int = 0, min_voxels: int = 0,
                     fill_holes: bool = False, connectivity: int = 26,
                     return_lesions: bool = False, window: Optional[Sequence[int]] = None, overlap=0.5,
                     blend: str = "gaussian", window_batch: int = 4, align=None) -> CasePrediction:
        """One case from its raw NIfTI files to a mask on its native grid, on the GPU:
        ``prepare_case_device`` -> the network on the input and on its copies flipped along each
        of ``tta_flips`` (tuples of axes out of 0, 1, 2) in one batch -> pcms_flip_mean
        (``tta_mean``; skipped without flips) -> pcms_prob_to_mask (``mask_on_grid``) -> one copy
        of the mask to the host (and of the probabilities with ``return_probability``).  The
        native grid is that of ``output_like`` (any NIfTI file, e.g. the label) or else of the
        first present modality's file.  ``normalise=False`` feeds the network what the training
        loader feeds it; ``normalise=True`` what ``load_multimodal_images`` would, resampled;
        ``"percentile"`` or a ``Normalisation`` the percentile window, here and with
        ``window``.
        ``keep_largest`` / ``min_voxels`` / ``fill_holes`` / ``connectivity`` (keyword-only): the
        mask goes through pcms_mask_postprocess (``postprocess``) on the device before the copy;
        with their defaults nothing is launched for them.  ``return_lesions=True``: the result's
        ``lesions`` is ``lesion_table`` of the final mask (after any post-processing) at
        ``connectivity``, from pcms_component_table on the device, with the native-grid
        probabilities as ``prob`` and the reference image's pixdim as spacing.
        ``window`` (keyword-only, with ``overlap`` / ``blend`` / ``window_batch``): sliding-window
        prediction.  ``target_size`` then names the grid the windows slide over
        (``None``: the native grid of the modalities) and the probabilities on it come from
        ``sliding_window_device(self.model.predict, ...)``: the network only ever sees batches of
        ``window_batch * (1 + len(tta_flips))`` windows of one shape; everything after the
        probabilities runs as without a window.  ``window=None``: nothing changes and nothing new
        is launched.  ValueError for a window axis under 16 (the network pools four times) or a
        bad ``overlap`` / ``blend`` / ``window_batch``.
        ``align`` (keyword-only): ``prepare_case_device``'s -- the modalities are
        brought onto the reference file's grid through their header geometry (``"world"``) and a
        rigid registration on the device (``"register"``) instead of being stretched onto it.  The
        reference defaults to ``output_like``, else the first present modality's file;
        ``target_size=None`` is its native grid and the modalities' shapes may differ.  The
        result's ``alignment`` reports the corrections.  ``align=None``: nothing changes."""
        from ._lib import call
        align = Alignment.of(align)
        if align is not None and align.to is None and output_like is not None:
            align = dataclasses.replace(align, to=output_like)
        masks = _flip_masks(tta_flips)
        if window is not None:
            window = _check_sliding(window, overlap, blend, window_batch)
            if any(w < 16 for w in window):
                raise ValueError(f"a window axis is at least 16 (the network pools four times), got {window}")
        _check_filter(keep_largest, min_voxels)
        _offsets(connectivity)
        post = keep_largest != 0 or min_voxels > 1 or bool(fill_holes)
        x, alignment = prepare_case_device(case_dir, target_size, handle_missing, normalise, self.device, align,
                                           return_alignment=True)  # raises if none present
        reference = output_like if output_like is not None else \
            next(p for p in _case_files(case_dir) if p is not None) if align is None else \
            _case_reference(_case_files(case_dir), align)
        native = tuple(int(v) for v in read_nifti_header(reference)["shape_xyz"][:3][::-1])
        geometry = _data.read_nifti_geometry(reference)
        grid = tuple(x.shape[2:])
        with torch.no_grad(), torch.cuda.device(self.device):
            if window is not None:
                prob = sliding_window_device(self.model.predict, x, window, overlap, blend, tta_flips, window_batch)
            else:
                batch = torch.cat([x] + [torch.flip(x, dims=[2 + a for a in f]) for f in tta_flips], dim=0)
                probs = self.model.predict(batch).float().contiguous()  # (k, 1, D, H, W)
                if len(masks) > 1:
                    host = (ctypes.c_int * len(masks))(*masks)  # read during the call (kernel arguments)
                    prob = torch.empty(grid, dtype=torch.float32, device=self.device)
                    call("pcms_flip_mean", probs, len(masks), ctypes.addressof(host), prob, *grid)
                else:
                    prob = probs[0, 0]
            mask = torch.empty(native, dtype=torch.uint8, device=self.device)
            prob_native = torch.empty(native, dtype=torch.float32, device=self.device) \
                if return_probability or return_lesions else None
            call("pcms_prob_to_mask", prob, *grid, float(threshold), mask, prob_native, *native)
            if post:
                mask, work = _postprocess_enqueue(mask, keep_largest, min_voxels, fill_holes, connectivity)
                # the status word travels with the mask: one device-to-host copy
                both = torch.cat([mask.reshape(-1), work[:1].view(torch.uint8)]).cpu().numpy()
                _check_status(int.from_bytes(both[-4:].tobytes(), "little", signed=True), "predict_case")
                mask_host = both[:-4].reshape(native)
            else:
                mask_host = mask.cpu().numpy()
            lesions = None
            if return_lesions:
                spacing = tuple(float(v) for v in geometry["pixdim"][1:4])[::-1]
                lesions = lesion_table_device(mask, prob_native, spacing, connectivity)
        return CasePrediction(mask_host, prob_native.cpu().numpy() if return_probability else None, reference,
                              geometry, lesions, alignment)

    def score_case(self, result: CasePrediction, label_path: str, lesion_metrics: bool = False,
                   min_iou: float = 0.1, connectivity: int = 26) -> dict:
        """Score ``result.mask`` against the label file ``label_path`` (binarised with ``!= 0``)
        on the device: ``dice`` and ``iou`` (utils.metrics) and ``surface_metrics_device``'s
        ``hd`` / ``hd95`` / ``assd`` / ``n_a`` / ``n_b`` in millimetres, the spacing being
        ``result.geometry``'s pixdim[1..3] reversed to (z, y, x).  With ``lesion_metrics=True`` the
        dict gains ``"lesions"``: ``lesion_metrics_device`` of mask against label at
        ``connectivity`` and ``min_iou``, in the same spacing, the predicted lesions' confidence
        from ``result.probability`` when the result carries it.  ValueError if the label is not on
        the mask's grid."""
        from .utils.metrics import calculate_dice_score, calculate_iou
        label = _first_volume(read_nifti(label_path)) != 0
        if tuple(label.shape) != tuple(result.mask.shape):
            raise ValueError(f"label of shape {tuple(label.shape)} is not on the grid {tuple(result.mask.shape)} of "
                             "the mask")
        spacing = tuple(float(v) for v in result.geometry["pixdim"][1:4])[::-1]
        with torch.cuda.device(self.device):
            mask = torch.from_numpy(np.ascontiguousarray(result.mask != 0).view(np.uint8)).to(self.device)
            lab = torch.from_numpy(np.ascontiguousarray(label).view(np.uint8)).to(self.device)
            scores = {"dice": calculate_dice_score(mask, lab), "iou": calculate_iou(mask, lab)}
            scores.update(surface_metrics_device(mask, lab, spacing))
            if lesion_metrics:
                prob = None if result.probability is None else \
                    torch.from_numpy(np.ascontiguousarray(result.probability, dtype=np.float32)).to(self.device)
                scores["lesions"] = lesion_metrics_device(mask, lab, prob, spacing, connectivity, min_iou)
        return scores

    def save_case(self, result: CasePrediction, output_path: str) -> None:
        """Write ``result.mask`` as a NIfTI file with the reference image's spacing, qform and
        sform (the reference's ``CopyInformation``); ValueError if the mask is not on that
        image's grid."""
        shape = tuple(int(v) for v in read_nifti_header(result.reference_path)["shape_xyz"][:3][::-1])
        if tuple(result.mask.shape) != shape:
            raise ValueError(f"mask of shape {tuple(result.mask.shape)} is not on the grid {shape} of "
                             f"{result.reference_path}")
        write_nifti(output_path, result.mask.astype(np.uint8), geometry=result.geometry)
