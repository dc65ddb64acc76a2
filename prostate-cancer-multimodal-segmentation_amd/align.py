"""Modality alignment (csrc/align.hip): host forms, then device forms.

``Alignment`` names how the modalities of a case reach one grid -- through their NIfTI world geometry
(``geometry.world_matrix`` / ``align_affine`` / ``case_affine``) and optionally a rigid
registration; ``joint_histogram`` / ``normalised_mutual_information`` / ``register_rigid`` are the
host forms of the similarity and of the search that maximises it; ``joint_histogram_device``
(pcms_joint_histogram, on the counts) / ``register_rigid_device`` / ``register_case_device`` /
``register_dataset`` run them on the GPU; ``predict.prepare_case``, ``prepare_case_device`` and
``predict_case`` take ``align=``.  A case is ``<dir>/<modality>/*.nii`` over ``MODALITIES``.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._args import axes3, host_affine12, volume3
from ._lib import call, query
from .geometry import (affine12_of, align_affine, case_affine, registration_fixed, rigid_correction, rigid_world,
                       world_centre)
from .intensity import Normalisation, _host_lohi, _window_device, normalise_window
from .nifti import _first_volume, _shape_zyx, device_raw, read_nifti, read_nifti_geometry, read_nifti_raw
from .resample import _sample_at


MODALITIES = ["ADC", "DWI", "gaoqing-T2", "T2 fs", "T2 not fs"]


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


# ---- modality alignment ------------------------------------------------------------
# Geometry lives in geometry.py (world_matrix, align_affine, case_affine).  Below: the similarity of
# two volumes of different contrast -- the joint histogram of their window-normalised intensities
# under an affine and its normalised mutual information -- and a rigid registration that maximises
# it.  The host forms define what csrc/align.hip counts, exactly.
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
    stride = axes3(stride, "stride")
    if min(stride) < 1:
        raise ValueError(f"every stride is at least 1, got {stride}")
    return int(bins), stride


def joint_histogram(fix: np.ndarray, mov: np.ndarray, A, t, fix_lohi, mov_lohi, bins: int = 32,
                    stride: Sequence[int] = (1, 1, 1)) -> np.ndarray:
    """The joint intensity histogram of a fixed and a moving (D, H, W) volume under the affine
    ``(A, t)`` (fixed array index -> moving array index), int64 ``(bins, bins)``.  For every
    lattice index ``q = (a*sd, b*sh, e*sw)`` inside the fixed volume: ``f`` is
    ``normalise_window(fix, fix_lohi)`` at ``q``; ``m`` is the linear sample
    (``resample.resample_affine``'s gather) of ``normalise_window(mov, mov_lohi)`` at
    ``c_a = ((A[a][0]*q_d + A[a][1]*q_h) + A[a][2]*q_w) + t[a]``.  The voxel counts only if
    ``-0.5 <= c_a < n_a - 0.5`` on all three moving axes and neither value is NaN; then
    ``hist[bin(f), bin(m)] += 1`` with ``bin(v) = min(int(fl32(v * float32(bins))), bins - 1)``
    (``_bin_index``).  The sum of the table is the overlap count.  libpcms_hip's
    pcms_joint_histogram is compared with this on the counts."""
    bins, stride = _check_hist_args(bins, stride)
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    fix, mov = volume3(fix), volume3(mov)
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
        m = _sample_at(mv, c, False, 1.0, 0.0)
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
    is resampled through its header geometry (``geometry.align_affine``) onto the reference file's
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


def _pattern_search(evaluate, fix_shape, fix_geometry: dict, mov_geometry: dict, settings: Alignment) -> dict:
    """``register_rigid``'s search over an evaluator ``evaluate(A, t, stride) -> (bins, bins)``
    counts: the host and the device form differ in that evaluator alone."""
    centre = world_centre(fix_geometry, fix_shape)
    seen, count = {}, [0]

    def score(params, stride):
        """NMI of ``params`` on the lattice of ``stride``, or None below the overlap floor."""
        key = (tuple(params), stride)
        if key not in seen:
            A, t = align_affine(fix_geometry, mov_geometry, rigid_world(params, centre))
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
    (``geometry.rigid_world``); it is the ``correction`` of ``geometry.align_affine(fix_geometry,
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
    fix, mov = volume3(fix), volume3(mov)
    fl = _host_lohi(fix, norm) if fix_lohi is None else np.asarray(fix_lohi, dtype=np.float32)
    ml = _host_lohi(mov, norm) if mov_lohi is None else np.asarray(mov_lohi, dtype=np.float32)
    return _pattern_search(lambda A, t, stride: joint_histogram(fix, mov, A, t, fl, ml, settings.bins, stride),
                           fix.shape, fix_geometry, mov_geometry, settings)


def _lohi_on(lohi, device) -> torch.Tensor:
    if isinstance(lohi, torch.Tensor):
        if lohi.device != device or lohi.dtype != torch.float32 or lohi.numel() != 2 or not lohi.is_contiguous():
            raise ValueError(f"a window is two contiguous fp32 values on {device}")
        return lohi
    return torch.from_numpy(np.asarray(lohi, dtype=np.float32).reshape(2).copy()).to(device)


def _joint_enqueue(fix_raw, mov_raw, A, t, fix_lohi: torch.Tensor, mov_lohi: torch.Tensor, bins: int, stride,
                   work: torch.Tensor) -> torch.Tensor:
    """The int32 (bins, bins) table with pcms_joint_histogram enqueued on the current stream."""
    host = host_affine12(affine12_of(A, t))  # read during the call: stays in this local until it returns
    hist = torch.empty((bins, bins), dtype=torch.int32, device=fix_raw.data.device)
    call("pcms_joint_histogram", *fix_raw.kernel_args(), fix_lohi, *mov_raw.kernel_args(), mov_lohi,
         ctypes.addressof(host), *stride, bins, hist, work)
    return hist


def _joint_work(bins: int, device) -> torch.Tensor:
    return torch.empty(query("pcms_joint_histogram_work_bytes", bins) // 4, dtype=torch.int32, device=device)


def joint_histogram_device(fix_raw, mov_raw, A, t, fix_lohi, mov_lohi, bins: int = 32,
                           stride: Sequence[int] = (1, 1, 1)) -> torch.Tensor:
    """``joint_histogram`` on the GPU, on the counts exactly (pcms_joint_histogram): two
    ``RawVolume``s whose bytes are on one GPU in, a ``torch.int64`` (bins, bins) tensor there out,
    enqueued on the current stream.  ``fix_lohi`` / ``mov_lohi``: two fp32 values each, as device
    tensors (pcms_volume_minmax's or pcms_volume_window's, consumed where they are) or as host
    numbers (uploaded).  Host bytes raise; ValueError for what the entry point rejects."""
    bins, stride = _check_hist_args(bins, stride)
    fix_raw, mov_raw = device_raw(fix_raw, "joint_histogram_device"), device_raw(mov_raw, "joint_histogram_device")
    device = fix_raw.data.device
    if mov_raw.data.device != device:
        raise ValueError(f"the two volumes are on different devices: {device} and {mov_raw.data.device}")
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    if not (np.isfinite(A).all() and np.isfinite(t).all()):
        raise ValueError("the affine must be finite")
    with torch.cuda.device(device):
        hist = _joint_enqueue(fix_raw, mov_raw, A, t, _lohi_on(fix_lohi, device), _lohi_on(mov_lohi, device),
                              bins, stride, _joint_work(bins, device))
        return hist.to(torch.int64)


def register_rigid_device(fix_raw, mov_raw, fix_geometry: dict, mov_geometry: dict, fix_lohi=None, mov_lohi=None,
                          normalise=None, settings=None) -> dict:
    """``register_rigid`` with pcms_joint_histogram as its evaluator: the same Python search, one
    small table read back per evaluation.  The counts are the host form's, so the search takes the
    same path and returns the same parameters, similarities and evaluation count exactly.
    ``fix_raw`` / ``mov_raw``: ``RawVolume``s whose bytes are on one GPU; the windows default to
    pcms_volume_window (a percentile ``normalise``) or pcms_volume_minmax."""
    settings = Alignment.of(settings) or Alignment()
    norm = Normalisation.of(normalise)
    fix_raw, mov_raw = device_raw(fix_raw, "register_rigid_device"), device_raw(mov_raw, "register_rigid_device")
    device = fix_raw.data.device
    if mov_raw.data.device != device:
        raise ValueError(f"the two volumes are on different devices: {device} and {mov_raw.data.device}")
    with torch.cuda.device(device):
        fl = _window_device(fix_raw, norm) if fix_lohi is None else _lohi_on(fix_lohi, device)
        ml = _window_device(mov_raw, norm) if mov_lohi is None else _lohi_on(mov_lohi, device)
        work = _joint_work(settings.bins, device)  # one workspace: the evaluations are ordered on the stream

        def evaluate(A, t, stride):
            return _joint_enqueue(fix_raw, mov_raw, A, t, fl, ml, settings.bins, stride, work).cpu().numpy()

        return _pattern_search(evaluate, tuple(fix_raw.shape), fix_geometry, mov_geometry, settings)


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
    return MODALITIES.index(registration_fixed(MODALITIES, present, align.to))


def _aligned_affines(paths, grid, reference: str, corrections: Optional[dict], fixed: int):
    """Per present channel the ``(A, t)`` of ``geometry.case_affine`` from ``grid`` through the
    reference file's geometry into the channel's file, with its rigid correction (six parameters
    about the centre of channel ``fixed``'s file) when it has one."""
    ref_geo, ref_shape = read_nifti_geometry(reference), _shape_zyx(reference)
    out = {}
    for c, p in enumerate(paths):
        if p is None:
            continue
        T = None
        if corrections is not None and corrections.get(MODALITIES[c]) is not None and c != fixed:
            T = rigid_correction(corrections[MODALITIES[c]]["params"], read_nifti_geometry(paths[fixed]),
                                       _shape_zyx(paths[fixed]))
        pair = align_affine(ref_geo, read_nifti_geometry(p), T)
        out[c] = case_affine(np.eye(3), np.zeros(3), _shape_zyx(p), grid, (ref_shape, pair))
    return out


def register_case(case_dir_or_files, normalise=True, align="register") -> dict:
    """The host form of ``register_case_device``: ``register_rigid`` of every other present
    modality to the fixed one, ``{modality: result}``."""
    paths, settings = _register_inputs(case_dir_or_files, align)
    fixed = _fixed_modality(paths, settings)
    fix = _first_volume(read_nifti(paths[fixed]))
    geo = read_nifti_geometry(paths[fixed])
    return {MODALITIES[c]: register_rigid(fix, _first_volume(read_nifti(p)), geo, read_nifti_geometry(p),
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
                raws[c] = read_nifti_raw(p).to(device)
        geo = read_nifti_geometry(paths[fixed])
        fl = _window_device(raws[fixed], norm)
        return {MODALITIES[c]: register_rigid_device(raws[fixed], raws[c], geo, read_nifti_geometry(p),
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
