"""Input pipeline feeding ``Trainer.step`` (reference script/data_loader.py).

The reference reads and resamples NIfTI volumes with SimpleITK, which is absent here: the reader
is ``nifti`` (``read_nifti`` / ``read_nifti_raw``), the resampler ``resample`` (``resample`` /
``resample_affine`` / ``resample_deform`` / ``resample_device``), the affines come from
``geometry``; every public name of those modules is also a name of this one.

Dataset semantics follow script/data_loader.py:
  * case discovery from ``<data_dir>/BPH-PCA/<data_type>/ADC/*.nii[.gz]`` (:57-94);
  * per-modality files ``<data_dir>/BPH-PCA/<data_type>/<modality>/<case>.nii[.gz]``, labels
    ``<data_dir>/BPH-PCA/ROI(BPH+PCA)/<data_type>/<case>.nii[.gz]``; cases without a label or
    with an unreadable header are dropped (:96-194);
  * missing modalities: 'skip' drops the case, 'duplicate' copies the first available
    modality (none available: dropped), 'zero_fill' loads zeros of ``target_size``
    (:147-163, :318-333);
  * every modality resampled (linear) to ``target_size`` (D, H, W), label resampled
    (nearest) and binarised ``> 0`` (:240-283, :379-409);
  * batches ``{'image': (N, M, D, H, W) f32, 'label': (N, 1, D, H, W) f32, 'case_id': [..]}``
    from a ``DataLoader`` with ``pin_memory`` (:421-466).
``device_resample=True`` (dataset and loader) moves the resampling to the GPU: samples carry the
files' undecoded first volumes (``read_nifti_raw`` -> ``RawVolume``) and ``assemble_batch``
uploads the bytes and runs ``resample_device`` (libpcms_hip's pcms_resample_linear / _label, the
arithmetic of ``resample`` restated per voxel) into the batch: the same batches bit for bit.
``augment=...`` (dataset, loader, ``Trainer`` config) turns on training-time augmentation: one
3x4 affine per case and epoch (``draw_transform``: flips, rotations, zoom, shift; gain / bias per
modality) under which every volume of the case is resampled -- ``resample_affine`` on the host,
pcms_resample_affine_linear / _label in ``assemble_batch`` -- again the same batches bit for bit.
``Augment.elastic_grid`` / ``elastic_disp`` add a smooth elastic deformation in front of that
affine: one cubic B-spline control grid per case and epoch, ``resample_deform`` on the host,
pcms_resample_deform_linear / _label in ``assemble_batch``, the same batches bit for bit too.
``patches=...`` (``PatchSampling``; dataset, loader, ``Trainer`` config) turns on patch training
for a sliding-window predictor: per case and epoch P crops of the window's shape from the case
grid, a chosen share centred on a lesion voxel -- ``draw_patches`` / ``pick_origins`` /
``resample_patch`` on the host, pcms_foreground_pick / pcms_patch_resample_linear in
``assemble_patch_batch``, the origins chosen and consumed on the device; the same batches bit
for bit once more.
``align=...`` (an ``align.Alignment``; dataset, loader, ``Trainer`` config) places every volume of
a case on the reference file's grid through the files' world geometry instead of stretching it
onto the grid: ``world_matrix`` / ``align_affine`` / ``compose_affine`` / ``case_affine`` on the
host, the same twelve doubles per volume in the existing affine launches on the device, with the
rigid ``corrections`` of ``align.register_dataset`` when given; the same batches bit for bit.
``n_classes=C`` (with ``class_values``; dataset, loader, ``assemble_batch``, ``Trainer`` config;
DESIGN §0t) keeps the label a class map instead of binarising it: ``classes.classes_of`` of the
nearest-resampled label on the host, pcms_resample_classes / pcms_resample_affine_classes on the
device, the same batches byte for byte; ``n_classes=1`` is everything above, untouched.
The reference's SimpleITK ``SetSize`` takes (x, y, z), so its non-cubic outputs come out
axis-reversed; here ``target_size`` is (D, H, W) as documented (:41).
"""
from __future__ import annotations

import ctypes
import dataclasses
import glob
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from ._args import axes3, host_affine12, host_ints
from ._lib import call, query
from .align import Alignment
from .classes import check_n_classes, class_values_of, classes_of
from .geometry import (RIGID_NAMES, affine12_of, align_affine, case_affine, compose_affine,  # noqa: F401
                       compose_transform, registration_fixed, rigid_correction, rigid_world, volume_affine,
                       world_centre, world_matrix)
from .intensity import Normalisation, _lohi_enqueue
from .nifti import (_NIFTI_DTYPES, RawVolume, _shape_zyx, device_raw, read_nifti,  # noqa: F401
                    read_nifti_geometry, read_nifti_header, read_nifti_raw, write_nifti)
from .resample import (MAX_CONTROL_POINTS, _sample_at, field_displacement, resample,  # noqa: F401
                       resample_affine, resample_deform, resample_device)
from .window import gather_windows


DEFAULT_MODALITIES = ["ADC", "DWI", "gaoqing-T2", "T2 fs", "T2 not fs"]


@dataclasses.dataclass
class Augment:
    """Training-time augmentation settings (also accepted as a plain dict of these fields).
    The defaults are all identity: nothing is varied and the transform is exactly the plain
    resampler's."""
    flip_prob: Tuple[float, float, float] = (0.0, 0.0, 0.0)    # per axis (D, H, W)
    rotate_deg: Tuple[float, float, float] = (0.0, 0.0, 0.0)   # max |angle| about the D, H, W axes
    zoom: Tuple[float, float] = (1.0, 1.0)                     # (lo, hi)
    shift_frac: Tuple[float, float, float] = (0.0, 0.0, 0.0)   # max |shift| per axis / output extent
    gain: Tuple[float, float] = (1.0, 1.0)                     # (lo, hi), drawn per modality
    bias: Tuple[float, float] = (0.0, 0.0)                     # (lo, hi), drawn per modality
    # Elastic deformation (``resample_deform``): control points per output axis (D, H, W), all 0
    # (off) or each >= 4 with at most MAX_CONTROL_POINTS in all (a scalar: that count on every
    # axis), and the maximum |control displacement| per axis in output voxels.  Whether the map
    # stays invertible is the user's concern and is not checked: keep elastic_disp[a] well under
    # the control spacing N_a / (elastic_grid[a] - 3).
    elastic_grid: Tuple[int, int, int] = (0, 0, 0)
    elastic_disp: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    @staticmethod
    def of(aug) -> Optional["Augment"]:
        if aug is None or isinstance(aug, Augment):
            return aug
        return Augment(**dict(aug))

    def __post_init__(self):
        for name, n in (("flip_prob", 3), ("rotate_deg", 3), ("shift_frac", 3), ("zoom", 2), ("gain", 2), ("bias", 2),
                        ("elastic_disp", 3)):
            v = getattr(self, name)
            v = (float(v),) * n if np.isscalar(v) and n == 3 else tuple(float(x) for x in v)
            if len(v) != n or not all(np.isfinite(v)):
                raise ValueError(f"Augment.{name} must hold {n} finite numbers, got {getattr(self, name)!r}")
            setattr(self, name, v)
        if not self.zoom[0] > 0.0:
            raise ValueError(f"Augment.zoom must be positive, got {self.zoom!r}")
        if min(self.elastic_disp) < 0.0:
            raise ValueError(f"Augment.elastic_disp must not be negative, got {self.elastic_disp!r}")
        g = self.elastic_grid
        g = (g,) * 3 if np.isscalar(g) else tuple(g)
        if len(g) != 3 or any(isinstance(v, bool) or int(v) != v for v in g):
            raise ValueError(f"Augment.elastic_grid must hold 3 integers, got {self.elastic_grid!r}")
        g = tuple(int(v) for v in g)
        if any(g) and (min(g) < 4 or g[0] * g[1] * g[2] > MAX_CONTROL_POINTS):
            raise ValueError("Augment.elastic_grid must be all 0 (off) or hold three counts >= 4 with a product "
                             f"<= {MAX_CONTROL_POINTS}, got {self.elastic_grid!r}")
        self.elastic_grid = g

    @property
    def elastic(self) -> bool:
        return any(self.elastic_grid)


@dataclasses.dataclass
class Transform:
    """One case's drawn transform: ``L`` (3x3) and ``shift_frac`` (the shift as a fraction of
    the output extent, per axis) shared by every volume of the case, ``gain`` / ``bias`` per
    modality; ``field``: the elastic control grid (fp64 ``(gd, gh, gw, 3)``, output voxels), shared
    by every volume of the case too, or None."""
    L: np.ndarray
    shift_frac: np.ndarray
    gain: Tuple[float, ...]
    bias: Tuple[float, ...]
    field: Optional[np.ndarray] = None

    def affine(self, n_in, n_out, alignment=None) -> Tuple[np.ndarray, np.ndarray]:
        """``case_affine`` of this transform: with ``alignment`` = ``(ref_shape, (A, t))`` the
        volume is placed through the reference file's grid and ``align_affine``."""
        n_out = tuple(int(v) for v in n_out)
        return case_affine(self.L, self.shift_frac * np.array(n_out, dtype=np.float64), n_in, n_out, alignment)

    def affine12(self, n_in, n_out, alignment=None) -> Tuple[float, ...]:
        """``affine`` as the twelve doubles the C entry points take: row-major A, then t."""
        return affine12_of(*self.affine(n_in, n_out, alignment))

    @staticmethod
    def identity(n_modalities: int) -> "Transform":
        """The transform of a case that is not augmented: ``affine`` is the plain resampler's map."""
        return Transform(np.eye(3), np.zeros(3), (1.0,) * int(n_modalities), (0.0,) * int(n_modalities))


def draw_transform(aug, seed: int, epoch: int, case_number: int,
                   n_modalities: int = len(DEFAULT_MODALITIES)) -> Transform:
    """The transform of case ``case_number`` (its index in ``ProstateDataset.case_list`` --
    not a position in a Subset, a rank's shard or a worker) in ``epoch``: a function of
    ``(seed, epoch, case_number)`` alone, so loader topology and a resume do not change it.

    Stream: ``np.random.default_rng([seed, epoch, case_number])``; every draw is one
    ``rng.random()`` (u in [0, 1)), always taken, in this order:
      1-3    flips of D, H, W: flipped iff ``u < flip_prob[a]``;
      4-6    angles about D, H, W: ``rotate_deg[a] * (2u - 1)`` degrees;
      7      zoom: ``lo + (hi - lo) * u``;
      8-10   shifts of D, H, W: ``shift_frac[a] * (2u - 1)`` of the output extent;
      then per modality m = 0 .. n_modalities - 1:  gain_m, bias_m: ``lo + (hi - lo) * u`` each;
      then, only with ``elastic_grid`` on, ``gd*gh*gw*3`` more in C order (kd, kh, kw, component):
      the control displacements ``elastic_disp[c] * (2u - 1)`` (appended, so the draws above are
      those of the same settings without it)."""
    aug = Augment.of(aug)
    rng = np.random.default_rng([int(seed), int(epoch), int(case_number)])
    flips = [rng.random() < p for p in aug.flip_prob]
    angles = [m * (2.0 * rng.random() - 1.0) for m in aug.rotate_deg]
    zoom = aug.zoom[0] + (aug.zoom[1] - aug.zoom[0]) * rng.random()
    shift = np.array([m * (2.0 * rng.random() - 1.0) for m in aug.shift_frac]) + 0.0
    gain, bias = [], []
    for _ in range(int(n_modalities)):
        gain.append(float(aug.gain[0] + (aug.gain[1] - aug.gain[0]) * rng.random()))
        bias.append(float(aug.bias[0] + (aug.bias[1] - aug.bias[0]) * rng.random()))
    field = None
    if aug.elastic:
        u = np.array([rng.random() for _ in range(int(np.prod(aug.elastic_grid)) * 3)]).reshape(aug.elastic_grid + (3,))
        field = np.array(aug.elastic_disp) * (2.0 * u - 1.0) + 0.0
    return Transform(compose_transform(flips, angles, zoom), shift, tuple(gain), tuple(bias), field)


# ---- patch training: foreground-biased crops of the window's shape ---------------------------
MAX_PATCHES = 64        # patches per case: one workgroup of the pick each, one launch per modality


MAX_PATCH_AXIS = 512    # the label patches come out of pcms_window_gather, which caps a window axis


@dataclasses.dataclass
class PatchSampling:
    """Patch training settings (also accepted as a plain dict of these fields): every case
    yields ``patches_per_case`` crops of ``patch_size`` -- the window shape of a sliding-window
    predictor, every axis a multiple of 16 because the network pools four times -- cut from
    ``grid``, the case grid the windows slide over (``None``: the shape of the case's label
    file).  A share ``foreground_prob`` of them is centred on a lesion voxel (``draw_patches``,
    ``pick_origins``).  ``normalise``: every modality is normalised over its whole volume first, as
    ``predict.prepare_case`` does: ``True`` is min-max (and stays ``True``); a method name
    (``"percentile"``), a dict or an ``intensity.Normalisation`` is kept as a ``Normalisation``.
    ``seed`` seeds the patch draws."""
    patch_size: Tuple[int, int, int] = (16, 128, 128)
    patches_per_case: int = 2
    foreground_prob: float = 0.5
    grid: Optional[Tuple[int, int, int]] = None
    normalise: object = False
    seed: int = 0

    @staticmethod
    def of(patches) -> Optional["PatchSampling"]:
        if patches is None or isinstance(patches, PatchSampling):
            return patches
        return PatchSampling(**dict(patches))

    def __post_init__(self):
        self.patch_size = axes3(self.patch_size, "PatchSampling.patch_size")
        if any(w < 16 or w % 16 or w > MAX_PATCH_AXIS for w in self.patch_size):
            raise ValueError("PatchSampling.patch_size: every axis is a multiple of 16 (the network pools four "
                             f"times) up to {MAX_PATCH_AXIS}, got {self.patch_size}")
        p = self.patches_per_case
        if isinstance(p, bool) or int(p) != p or not 1 <= int(p) <= MAX_PATCHES:
            raise ValueError(f"PatchSampling.patches_per_case is an integer in 1..{MAX_PATCHES}, got {p!r}")
        self.patches_per_case = int(p)
        self.foreground_prob = float(self.foreground_prob)
        if not 0.0 <= self.foreground_prob <= 1.0:  # false for NaN
            raise ValueError(f"PatchSampling.foreground_prob lies in [0, 1], got {self.foreground_prob!r}")
        if self.grid is not None:
            self.grid = axes3(self.grid, "PatchSampling.grid")
            if min(self.grid) < 1:
                raise ValueError(f"PatchSampling.grid: every axis is at least 1, got {self.grid}")
        if isinstance(self.normalise, (str, dict)) or dataclasses.is_dataclass(self.normalise):
            self.normalise = Normalisation.of(self.normalise)  # ValueError for an unknown method
        else:
            self.normalise = bool(self.normalise)
        self.seed = int(self.seed)


def _resample_patch(vol: np.ndarray, grid, A, t, origin, patch, gain, bias) -> np.ndarray:
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    grid, patch, origin = axes3(grid, "grid"), axes3(patch, "patch"), axes3(origin, "origin")
    shapes = ((-1, 1, 1), (1, -1, 1), (1, 1, -1))
    idx = [(np.arange(w, dtype=np.int64) + o).reshape(s) for w, o, s in zip(patch, origin, shapes)]
    p = [i.astype(np.float64) for i in idx]
    with np.errstate(over="ignore", invalid="ignore"):
        c = [((A[a, 0] * p[0] + A[a, 1] * p[1]) + A[a, 2] * p[2]) + t[a] for a in range(3)]
    out = _sample_at(vol, c, False, gain, bias)
    on_grid = np.ones(patch, dtype=bool)
    for i, g in zip(idx, grid):
        on_grid = on_grid & ((i >= 0) & (i < g))
    return np.where(on_grid, out, np.float32(0.0))


def resample_patch(vol: np.ndarray, grid, A, t, origin, patch, gain: float = 1.0, bias: float = 0.0,
                   normalise=False) -> np.ndarray:
    """One ``patch`` = (wd, wh, ww) crop of ``resample_affine(vol, grid, A, t, gain=gain,
    bias=bias)`` at ``origin``, bit for bit, formed from the patch's coordinates alone: patch
    index (d, h, w) stands for grid index ``p = (d, h, w) + origin`` (integers, exact in fp64) and
    samples the source at ``c_a = ((A[a][0]*p_d + A[a][1]*p_h) + A[a][2]*p_w) + t[a]``; from the
    coordinate on everything is ``resample_affine``'s (``_sample_at``).  The result is 0 where any
    ``p_a < 0`` or ``p_a >= grid[a]``: a patch that sticks out of the grid is zero-padded, as
    ``window.gather_windows`` pads a window.  ``normalise``: ``vol`` is first replaced by
    ``intensity.normalise(vol)`` (min-max over the whole volume, the corner rule of
    pcms_resample_linear_norm); anything else ``intensity.Normalisation.of`` accepts selects that
    normalisation (``"percentile"``: ``intensity.normalise_window`` at the volume's
    ``intensity.intensity_window``).  libpcms_hip's pcms_patch_resample_linear and
    pcms_patch_resample_window restate this per voxel and are compared with it on the fp32 bits."""
    norm = Normalisation.of(normalise)
    if norm is not None:
        vol = norm.apply(vol)
    return _resample_patch(vol, grid, A, t, origin, patch, gain, bias)


def draw_patches(sampling, seed: int, epoch: int, case_number: int, grid=None) -> Tuple[np.ndarray, np.ndarray]:
    """The patch draws of case ``case_number`` in ``epoch``: ``(rank_u, fallback)``, P doubles and
    a (P, 3) int32 array, a function of ``(sampling, seed, epoch, case_number)`` and the grid
    alone (``grid``: the case grid when ``sampling.grid`` is None -- the label file's shape).

    Stream: ``np.random.default_rng([seed, epoch, case_number, 1])``, a stream of its own, so
    ``draw_transform``'s draws do not move.  Per patch, in order, five ``rng.random()`` values are
    always taken: ``u_mode, u_rank, u_d, u_h, u_w``.  A patch is a foreground patch iff
    ``u_mode < foreground_prob``: its ``rank_u`` is ``u_rank`` (``pick_origins`` turns it into the
    rank of a lesion voxel), every other patch has ``rank_u = -1.0``.  ``fallback`` is the origin
    of a uniformly placed patch, ``int(floor(u_a * (max(G_a - w_a, 0) + 1)))`` per axis: what a
    patch without a rank, or a case without foreground, takes."""
    sampling = PatchSampling.of(sampling)
    grid = sampling.grid if sampling.grid is not None else grid
    if grid is None:
        raise ValueError("draw_patches needs the case grid: PatchSampling.grid is None and no grid was given")
    grid = axes3(grid, "grid")
    rng = np.random.default_rng([int(seed), int(epoch), int(case_number), 1])
    P = sampling.patches_per_case
    rank_u = np.empty(P, dtype=np.float64)
    fallback = np.empty((P, 3), dtype=np.int32)
    for i in range(P):
        u_mode, u_rank = rng.random(), rng.random()
        u = [rng.random() for _ in range(3)]
        rank_u[i] = u_rank if u_mode < sampling.foreground_prob else -1.0
        fallback[i] = [int(np.floor(u[a] * (max(grid[a] - sampling.patch_size[a], 0) + 1))) for a in range(3)]
    return rank_u, fallback


def pick_origins(label_grid: np.ndarray, patch, rank_u, fallback) -> Tuple[np.ndarray, int]:
    """``(origins, T)``: the (P, 3) int32 origins of P patches on ``label_grid`` (D, H, W) and the
    number ``T`` of its voxels ``> 0``.  A patch with ``rank_u >= 0`` on a grid with ``T > 0`` is
    centred on a lesion voxel: ``r = min(T - 1, int(floor(float64(rank_u) * float64(T))))``, the
    voxel ``v`` is the ``r``-th foreground voxel in flat order ``(d*H + h)*W + w``
    (``np.flatnonzero``), and ``o_a = min(max(v_a - w_a // 2, 0), max(G_a - w_a, 0))`` -- so the
    patch contains ``v`` and its label patch is not empty.  Every other patch takes its
    ``fallback`` row.  The device form (pcms_foreground_pick) reads both tables from memory it does
    not trust, and this form states the same rule for what ``draw_patches`` never produces: the
    test for a fallback patch is ``rank_u < 0`` and the cap is ``r = T - 1 unless floor(..) <
    T - 1``, so a NaN rank or a rank of 1 or more selects the last foreground voxel, and a fallback
    entry is clamped into ``[0, max(G_a - w_a, 0)]``."""
    lab = np.asarray(label_grid)
    if lab.ndim != 3 or 0 in lab.shape:
        raise ValueError(f"pick_origins takes a non-empty (D, H, W) label grid, got shape {lab.shape}")
    patch = axes3(patch, "patch")
    if min(patch) < 1:
        raise ValueError(f"a patch axis is at least 1, got {patch}")
    rank_u = np.asarray(rank_u, dtype=np.float64).reshape(-1)
    fallback = np.asarray(fallback).reshape(-1, 3).astype(np.int64)
    if len(rank_u) != len(fallback) or len(rank_u) == 0:
        raise ValueError(f"rank_u holds P >= 1 doubles and fallback P rows, got {len(rank_u)} and {len(fallback)}")
    G = lab.shape
    top = [max(g - w, 0) for g, w in zip(G, patch)]
    fg = np.flatnonzero(lab.reshape(-1) > 0)
    T = int(fg.size)
    origins = np.empty((len(rank_u), 3), dtype=np.int32)
    for i, u in enumerate(rank_u.tolist()):
        if u < 0.0 or T == 0:
            origins[i] = [min(max(int(o), 0), top[a]) for a, o in enumerate(fallback[i])]
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.floor(np.float64(u) * np.float64(T))
        r = int(x) if x < T - 1 else T - 1
        v = np.unravel_index(int(fg[r]), G)
        origins[i] = [min(max(int(v[a]) - patch[a] // 2, 0), top[a]) for a in range(3)]
    return origins, T


def is_raw_batch(batch) -> bool:
    return isinstance(batch, dict) and "raw_images" in batch


def assemble_batch(raw_batch: Dict, target_size: Optional[Tuple[int, int, int]] = None, device=None,
                   class_values=None) -> Dict:
    """A ``device_resample`` loader's batch -> ``{'image': (N, M, D, H, W) f32, 'label':
    (N, 1, D, H, W) f32, 'case_id': [...]}`` on ``device``, equal to the default loader's
    batch: each volume's bytes go up from pinned memory in their native type and one resample
    launch writes its channel plane; ``None`` channels (zero_fill) are zeroed.  Everything is
    enqueued on the current stream.  ``target_size`` defaults to the one the loader recorded.
    A batch of a ``n_classes > 1`` loader carries its ``class_values`` (``class_values=`` here
    overrides them): the label plane then holds class indices (``resample_device``'s ``class_values``)."""
    if "patches" in raw_batch:  # a patch-training loader's batch: the grid and the patch shape ride along
        return assemble_patch_batch(raw_batch, device, class_values)
    target = tuple(int(v) for v in (target_size if target_size is not None else raw_batch["target_size"]))
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise RuntimeError(f"a device_resample batch can only be assembled on a GPU, not on '{device}': "
                           "pcms_amd has no CPU resampling kernel (use the default loader there)")
    images, labels = raw_batch["raw_images"], raw_batch["raw_label"]
    n, m = len(images), len(images[0])
    aug = raw_batch.get("augment")  # per case: the drawn (affines, label affine, gains, biases[, field]), or absent
    # a class-map loader's table, or absent: the binary label
    values = class_values if class_values is not None else raw_batch.get("class_values")
    with torch.cuda.device(device):
        image = torch.empty((n, m) + target, dtype=torch.float32, device=device)
        label = torch.empty((n, 1) + target, dtype=torch.float32, device=device)

        def up(raw):
            return raw if raw.data.device.type == "cuda" else raw.pin_memory().to(device, non_blocking=True)

        for i in range(n):
            field = None if aug is None else aug[i].get("field")
            if field is not None:  # the case's elastic control grid: one upload for its M + 1 launches
                field = (field if field.device.type == "cuda" else field.pin_memory()).to(device, non_blocking=True)
            for c, raw in enumerate(images[i]):
                if raw is None:
                    image[i, c].zero_()
                elif aug is None:
                    resample_device(up(raw), target, out=image[i, c])
                else:
                    resample_device(up(raw), target, out=image[i, c], affine=aug[i]["affine"][c],
                                    gain=aug[i]["gain"][c], bias=aug[i]["bias"][c], field=field)
            # (an elastic field never comes with a class table: the dataset refuses the pair)
            resample_device(up(labels[i]), target, nearest=True, out=label[i, 0],
                            affine=None if aug is None else aug[i]["label_affine"], field=field, class_values=values)
    return {"image": image, "label": label, "case_id": list(raw_batch["case_id"])}


def assemble_patch_batch(raw_batch: Dict, device=None, class_values=None) -> Dict:
    """A patch-training ``device_resample`` batch -> ``{'image': (N*P, M, wd, wh, ww) f32,
    'label': (N*P, 1, wd, wh, ww) f32, 'case_id': [...], 'picks': (N, 3P + 1) int32}`` on
    ``device``, equal to the host loader's batch bit for bit.  Per case: the bytes go up once; one
    pcms_resample_affine_label launch forms the label on the whole grid; pcms_foreground_pick
    chooses the P origins there (``picks``: the origins, then the foreground count) and nothing
    brings them back -- pcms_patch_resample_linear reads them from device memory, once per present
    modality into that channel of the case's P patches (after pcms_volume_minmax with
    ``normalise``, or after pcms_volume_window and through pcms_patch_resample_window when the
    batch's ``"normalise"`` entry selects the percentile window; ``None`` channels are zeroed),
    and one pcms_window_gather cuts the label patches.  Everything is enqueued on the current
    stream, with no host synchronisation.  With the ``class_values`` of a ``n_classes > 1`` loader
    the grid label is a class map (pcms_resample_affine_classes); the origins are still picked on
    ``label > 0``, any foreground class."""
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise RuntimeError(f"a device_resample batch can only be assembled on a GPU, not on '{device}': "
                           "pcms_amd has no CPU resampling kernel (use the default loader there)")
    images, labels, draws = raw_batch["raw_images"], raw_batch["raw_label"], raw_batch["patches"]
    patch = tuple(int(v) for v in raw_batch["patch_size"])
    norm = Normalisation.of(raw_batch["normalise"])
    normalise = norm is not None
    values = class_values if class_values is not None else raw_batch.get("class_values")
    n, m = len(images), len(images[0])
    P = int(draws[0]["rank_u"].numel())
    nwin = patch[0] * patch[1] * patch[2]
    no_flip = host_ints([0])  # read during the calls: stays in this local until the last one returns
    with torch.cuda.device(device):
        image = torch.empty((n * P, m) + patch, dtype=torch.float32, device=device)
        label = torch.empty((n * P, 1) + patch, dtype=torch.float32, device=device)
        picks = torch.empty((n, 3 * P + 1), dtype=torch.int32, device=device)
        lohi = torch.empty(2, dtype=torch.float32, device=device) if normalise else None

        def up(t):
            return t if t.device.type == "cuda" else t.pin_memory().to(device, non_blocking=True)

        for i in range(n):
            d = draws[i]
            grid = tuple(int(v) for v in d["grid"])
            cells = grid[0] * grid[1] * grid[2]
            if int(d["rank_u"].numel()) != P:
                raise ValueError("every case of a batch holds the same number of patches")
            lab = labels[i] if labels[i].data.device.type == "cuda" else labels[i].pin_memory().to(device, True)
            label_grid = resample_device(lab, grid, nearest=True, affine=d["label_affine"], class_values=values)
            work = torch.empty(query("pcms_foreground_pick_work_ints", cells), dtype=torch.int32, device=device)
            call("pcms_foreground_pick", label_grid, cells, *grid, *patch, up(d["rank_u"]), up(d["fallback"]), P,
                 picks[i], work)
            for c, raw in enumerate(images[i]):
                first = image[i * P, c]  # patch p of this channel lies p * m * nwin floats further on
                if raw is None:
                    image[i * P:(i + 1) * P, c].zero_()
                    continue
                raw = raw if raw.data.device.type == "cuda" else raw.pin_memory().to(device, True)
                raw = device_raw(raw, "assemble_patch_batch")
                # the window is formed once per volume and read from device memory by every patch
                windowed = normalise and _lohi_enqueue(raw, norm, lohi) == "window"
                host = host_affine12(d["affine"][c])  # read during the call: stays in this local until it returns
                call("pcms_patch_resample_window" if windowed else "pcms_patch_resample_linear", *raw.kernel_args(),
                     ctypes.addressof(host), lohi, float(d["gain"][c]), float(d["bias"][c]), *grid, picks[i], P, first,
                     m * nwin, *patch)
            call("pcms_window_gather", label_grid, 1, *grid, picks[i], P, ctypes.addressof(no_flip), 1, *patch,
                 label[i * P:(i + 1) * P])
    return {"image": image, "label": label, "case_id": [cid for cid in raw_batch["case_id"] for _ in range(P)],
            "picks": picks}


def device_batch(batch: Dict, device) -> Dict:
    """What every consumer of a loader's batch calls first: a ``device_resample`` batch is
    assembled on ``device`` (``assemble_batch``); any other batch passes through untouched."""
    return assemble_batch(batch, None, device) if is_raw_batch(batch) else batch


class _CollateRaw:
    """Collate of ``device_resample`` samples: raw shapes differ between cases and modalities,
    so the descriptors stay in lists (nothing is stacked); the target size rides along."""

    def __init__(self, target_size, patches=None, class_values=None):
        self.target_size = tuple(int(v) for v in target_size)
        self.patches = PatchSampling.of(patches)
        self.class_values = class_values  # a class-map dataset's table (None: binary labels)

    def __call__(self, samples: List[Dict]) -> Dict:
        batch = {"raw_images": [s["raw_images"] for s in samples], "raw_label": [s["raw_label"] for s in samples],
                 "case_id": [s["case_id"] for s in samples], "target_size": self.target_size}
        if self.class_values is not None:
            batch["class_values"] = self.class_values
        if samples and "augment" in samples[0]:  # an augmenting dataset: each case's drawn transform rides along
            batch["augment"] = [s["augment"] for s in samples]
        if self.patches is not None:  # a patch-training dataset: each case's affines and patch draws (CPU tensors)
            batch["patches"] = [s["patches"] for s in samples]
            batch["patch_size"], batch["normalise"] = self.patches.patch_size, self.patches.normalise
        return batch


def _collate_patches(samples: List[Dict]) -> Dict:
    """Collate of the host loader's patch samples: a sample holds its case's P patches, a batch
    concatenates them -- ``image`` (N*P, M, wd, wh, ww), ``label`` (N*P, 1, ...), ``case_id``
    repeated P times, ``picks`` (N, 3P + 1): each case's origins, then its foreground count."""
    P = samples[0]["image"].shape[0]
    return {"image": torch.cat([s["image"] for s in samples], 0), "label": torch.cat([s["label"] for s in samples], 0),
            "case_id": [s["case_id"] for s in samples for _ in range(P)],
            "picks": torch.stack([s["picks"] for s in samples], 0)}


def _find(base: str, case_id: str) -> Optional[str]:
    for ext in (".nii", ".nii.gz"):
        p = os.path.join(base, case_id + ext)
        if os.path.exists(p):
            return p
    return None


class ProstateDataset(Dataset):
    """script/data_loader.py:9-419 (same constructor, case filtering and sample dicts)."""

    def __init__(self, data_dir: str, modalities: Optional[List[str]] = None, missing_strategy: str = "zero_fill",
                 target_size: Tuple[int, int, int] = (128, 128, 128), is_training: bool = True,
                 data_type: str = "BPH", device_resample: bool = False, augment=None, augment_seed: int = 0,
                 patches=None, align=None, corrections=None, n_classes: int = 1, class_values=None):
        """``augment`` (an ``Augment`` or a dict of its fields; None: off, every sample as
        before): each case is resampled under a transform drawn by ``draw_transform(augment,
        augment_seed, epoch, case index)``, one geometry for all its modalities and its label,
        gain / bias per modality; ``set_epoch`` moves to the next epoch's draws.
        ``patches`` (a ``PatchSampling`` or a dict of its fields; None: off, every sample as
        before): patch training -- a sample is the case's P crops of the patch shape, cut from
        the case grid under that transform (the identity draw without ``augment``) at origins
        drawn by ``draw_patches`` / ``pick_origins``; ``target_size`` is unused, ``set_epoch``
        moves the patch draws too, and an elastic ``augment`` is not supported with it.
        ``align`` (anything ``align.Alignment.of`` accepts; None: off, every sample as before):
        every volume of a case, the label included, is placed on the grid of the reference file
        through its NIfTI world geometry (``case_affine``: the case grid scaled onto the
        reference's native grid, then ``align_affine`` into the volume's file) instead of being
        stretched onto it; a grid voxel outside a file's field of view reads 0.  The reference is
        ``align.to``: ``"label"`` (the default: the label file, whose own map is then the
        identity) or a modality name; with ``patches`` a ``grid`` of None is its shape.  It
        composes with ``augment``, ``patches`` and ``device_resample``, and both kinds of loader
        give the same batches.  ``corrections`` (``align.register_dataset``'s dict ``{case_id:
        {modality: six parameters}}`` or the path of its JSON; needs ``align``): the rigid
        correction of each modality goes into its map.  Training never registers on the fly:
        ``mode="register"`` without ``corrections`` raises.
        ``n_classes`` (default 1: the binary label ``> 0``, every sample as before) with
        ``class_values`` (default ``(1, .., n_classes - 1)``): the label stays a class map --
        ``classes.classes_of`` of the nearest-resampled label file, class ``j + 1`` where its value
        is ``class_values[j]`` and 0 elsewhere -- as fp32 ``(1, D, H, W)``.  Patches are still
        picked on ``label > 0``, any foreground class.  Elastic deformation of a class map is not
        supported (ValueError)."""
        self.n_classes = check_n_classes(n_classes)
        if class_values is not None and self.n_classes == 1:
            raise ValueError("class_values need n_classes > 1")
        self.class_values = class_values_of(self.n_classes, class_values) if self.n_classes > 1 else None
        if missing_strategy not in ("zero_fill", "skip", "duplicate"):
            raise ValueError(f"unsupported missing-modality strategy: {missing_strategy}")
        self.augment = Augment.of(augment)
        self.patches = PatchSampling.of(patches)
        if self.patches is not None and self.augment is not None and self.augment.elastic:
            raise ValueError("patches and Augment.elastic_grid cannot be combined: the patch resampler has no "
                             "deforming form")
        if self.class_values is not None and self.augment is not None and self.augment.elastic:
            raise ValueError("Augment.elastic_grid and n_classes > 1 cannot be combined: the deforming resampler has "
                             "no class-map form")
        self.align = Alignment.of(align)
        if isinstance(corrections, (str, os.PathLike)):
            import json
            with open(corrections) as f:
                corrections = json.load(f)
        if corrections is not None and self.align is None:
            raise ValueError("corrections need align: they are rigid corrections of the header alignment")
        if self.align is not None and self.align.mode == "register" and corrections is None:
            raise ValueError("training does not register on the fly: pass corrections=predict.register_dataset(...) "
                             "(or its JSON file) with align mode 'register'")
        self.corrections = corrections
        self.augment_seed = int(augment_seed)
        self.epoch = 0
        self.data_dir = data_dir
        self.modalities = list(modalities or DEFAULT_MODALITIES)
        self.missing_strategy = missing_strategy
        self.target_size = tuple(int(v) for v in target_size)
        self.is_training = is_training
        self.data_type = data_type
        self.device_resample = bool(device_resample)
        self.case_list = self._filter_cases(self._get_case_list())

    def _root(self, *parts) -> str:
        return os.path.join(self.data_dir, "BPH-PCA", *parts)

    def _get_case_list(self) -> List[str]:
        adc = self._root(self.data_type, "ADC")
        if not os.path.isdir(adc):
            return []
        ids = []
        for p in sorted(glob.glob(os.path.join(adc, "*.nii")) + glob.glob(os.path.join(adc, "*.nii.gz"))):
            name = os.path.basename(p)
            ids.append(name[:-7] if name.endswith(".nii.gz") else name[:-4])
        return ids

    def _filter_cases(self, case_ids: List[str]) -> List[Dict]:
        valid = []
        for cid in case_ids:
            files, missing = {}, []
            for m in self.modalities:
                p = _find(self._root(self.data_type, m), cid)
                if p is None:
                    missing.append(m)
                else:
                    files[m] = p
            label = _find(self._root("ROI(BPH+PCA)", self.data_type), cid)
            if label is None:
                continue
            if missing:
                if self.missing_strategy == "skip":
                    continue
                if self.missing_strategy == "duplicate":
                    avail = [m for m in self.modalities if m not in missing]
                    if not avail:
                        continue
                    for m in missing:
                        files[m] = files[avail[0]]
            try:
                for p in list(files.values()) + [label]:
                    read_nifti_header(p)
            except (ValueError, OSError):
                continue
            valid.append({"case_id": cid, "modality_files": files, "label_path": label,
                          "missing_modalities": missing})
        return valid

    def __len__(self) -> int:
        return len(self.case_list)

    @staticmethod
    def _first_volume(a: np.ndarray) -> np.ndarray:
        if a.ndim == 3:
            return a
        if a.ndim == 4:
            return a[0]
        raise ValueError(f"unsupported image dimensions: {a.shape}")

    def _alignments(self, case: Dict) -> Optional[Dict]:
        """``{modality: (ref_shape, (A, t)), ..., "label": ...}``: the ``alignment`` argument of
        ``Transform.affine`` for every file of the case (``align_affine`` from the reference file,
        with the modality's rigid correction about the centre of the fixed modality's file --
        ``registration_fixed`` -- when ``corrections`` holds one); None without ``align``."""
        if self.align is None:
            return None
        files = case["modality_files"]
        to = self.align.to if self.align.to is not None else "label"
        ref = case["label_path"] if to == "label" else files.get(to)
        if ref is None:
            raise FileNotFoundError(f"case {case['case_id']}: no file for the alignment reference {to!r}")
        ref_geo, ref_shape = read_nifti_geometry(ref), _shape_zyx(ref)
        corr = (self.corrections or {}).get(case["case_id"]) or {}
        fixed = registration_fixed(self.modalities, files, to)
        out = {"label": (ref_shape, align_affine(ref_geo, read_nifti_geometry(case["label_path"])))}
        for m, p in files.items():
            T = None
            if corr.get(m) is not None and m != fixed:
                T = rigid_correction(corr[m], read_nifti_geometry(files[fixed]), _shape_zyx(files[fixed]))
            out[m] = (ref_shape, align_affine(ref_geo, read_nifti_geometry(p), T))
        return out

    def _label_of(self, nearest: np.ndarray) -> np.ndarray:
        """The (D, H, W) fp32 label of a nearest-resampled label volume: ``> 0``, or the class map."""
        if self.class_values is None:
            return (nearest > 0).astype(np.float32)
        return classes_of(nearest, self.class_values)

    def set_epoch(self, epoch: int) -> None:
        """The epoch whose transforms and patch origins ``__getitem__`` draws (no effect without
        ``augment`` or ``patches``).
        Call it before iterating the loader: its worker processes start per iteration and
        take the value along."""
        self.epoch = int(epoch)

    def _augmented(self, idx: int) -> Dict:
        """``__getitem__`` under the case's drawn transform (the identity one when only ``align``
        is on), every volume placed by ``align`` when it is on: every volume resampled by
        ``resample_affine`` (also one already of the target shape), or -- ``device_resample`` --
        handed over undecoded with the twelve doubles and the gain / bias it is to be resampled
        with.  With ``elastic_grid`` on the case's control grid goes along: ``resample_deform``
        here, ``"field"`` in the handed-over dict there."""
        case = self.case_list[idx]
        files = case["modality_files"]
        tf = Transform.identity(len(self.modalities)) if self.augment is None else \
            draw_transform(self.augment, self.augment_seed, self.epoch, idx, len(self.modalities))
        al = self._alignments(case)  # per modality and for "label": (ref_shape, (A, t)), or None
        if self.device_resample:
            raws = [read_nifti_raw(files[m]) if m in files else None for m in self.modalities]
            lab = read_nifti_raw(case["label_path"])
            aug = {"affine": [None if r is None else tf.affine12(r.shape, self.target_size, al and al[m])
                              for m, r in zip(self.modalities, raws)],
                   "label_affine": tf.affine12(lab.shape, self.target_size, al and al["label"]), "gain": tf.gain,
                   "bias": tf.bias}
            if tf.field is not None:  # a CPU tensor, so that the DataLoader's pin_memory handles it
                aug["field"] = torch.from_numpy(np.ascontiguousarray(tf.field))
            return {"raw_images": raws, "raw_label": lab, "case_id": case["case_id"], "augment": aug}
        def sample(vol, alignment, **kw):  # with an elastic field the same gather at the deformed positions
            A, t = tf.affine(vol.shape, self.target_size, alignment)
            if tf.field is None:
                return resample_affine(vol, self.target_size, A, t, **kw)
            return resample_deform(vol, self.target_size, A, t, tf.field, **kw)

        chans = []
        for c, m in enumerate(self.modalities):
            p = files.get(m)
            if p is None:  # zero_fill stays zero: no bias on a channel that is not there
                chans.append(np.zeros(self.target_size, dtype=np.float32))
                continue
            vol = self._first_volume(read_nifti(p)).astype(np.float32)
            chans.append(sample(vol, al and al[m], gain=tf.gain[c], bias=tf.bias[c]))
        lab = self._first_volume(read_nifti(case["label_path"]))
        label = self._label_of(sample(lab, al and al["label"], nearest=True))[None]
        return {"image": torch.from_numpy(np.stack(chans, 0)).float(), "label": torch.from_numpy(label),
                "case_id": case["case_id"]}

    def _patched(self, idx: int) -> Dict:
        """``__getitem__`` of a patch-training dataset: the case's P patches.  One transform per
        case and epoch (``draw_transform``; the identity draw of ``Augment()`` without
        ``augment``) maps every volume onto the case grid; the label is formed on the whole grid
        (``resample_affine(..., nearest=True) > 0``), the origins are picked on it, each modality
        is sampled at the patches' coordinates alone (``resample_patch``) and the label patches
        are ``window.gather_windows`` of the grid label.  ``device_resample``: the volumes are
        handed over undecoded with the twelve doubles per volume and the patch draws as CPU
        tensors, and ``assemble_patch_batch`` does all of that on the GPU."""
        case = self.case_list[idx]
        files = case["modality_files"]
        ps = self.patches
        tf = draw_transform(self.augment if self.augment is not None else Augment(), self.augment_seed, self.epoch,
                            idx, len(self.modalities))
        al = self._alignments(case)  # per modality and for "label": (ref_shape, (A, t)), or None
        if self.device_resample:
            raws = [read_nifti_raw(files[m]) if m in files else None for m in self.modalities]
            lab = read_nifti_raw(case["label_path"])
            grid = ps.grid if ps.grid is not None else tuple(lab.shape) if al is None else al["label"][0]
            rank_u, fallback = draw_patches(ps, ps.seed, self.epoch, idx, grid)
            draws = {"affine": [None if r is None else tf.affine12(r.shape, grid, al and al[m])
                                for m, r in zip(self.modalities, raws)],
                     "label_affine": tf.affine12(lab.shape, grid, al and al["label"]), "gain": tf.gain,
                     "bias": tf.bias, "grid": grid,
                     # CPU tensors, so that the DataLoader's pin_memory handles them
                     "rank_u": torch.from_numpy(rank_u), "fallback": torch.from_numpy(fallback)}
            return {"raw_images": raws, "raw_label": lab, "case_id": case["case_id"], "patches": draws}
        lab = self._first_volume(read_nifti(case["label_path"]))
        grid = ps.grid if ps.grid is not None else tuple(lab.shape) if al is None else al["label"][0]
        rank_u, fallback = draw_patches(ps, ps.seed, self.epoch, idx, grid)
        label_grid = self._label_of(resample_affine(lab, grid, *tf.affine(lab.shape, grid, al and al["label"]),
                                                    nearest=True))
        origins, count = pick_origins(label_grid, ps.patch_size, rank_u, fallback)
        P = ps.patches_per_case
        image = np.zeros((P, len(self.modalities)) + ps.patch_size, dtype=np.float32)
        for c, m in enumerate(self.modalities):
            p = files.get(m)
            if p is None:  # zero_fill stays zero
                continue
            vol = self._first_volume(read_nifti(p)).astype(np.float32)
            if ps.normalise:  # once per volume, not per patch
                vol = Normalisation.of(ps.normalise).apply(vol)
            A, t = tf.affine(vol.shape, grid, al and al[m])
            for k in range(P):
                image[k, c] = _resample_patch(vol, grid, A, t, origins[k], ps.patch_size, tf.gain[c], tf.bias[c])
        label = gather_windows(label_grid[None], origins, ps.patch_size)
        picks = np.concatenate([origins.reshape(-1), np.array([count], dtype=np.int32)]).astype(np.int32)
        return {"image": torch.from_numpy(image), "label": torch.from_numpy(label), "case_id": case["case_id"],
                "picks": torch.from_numpy(picks)}

    def __getitem__(self, idx: int) -> Dict:
        if self.patches is not None:
            return self._patched(idx)
        if self.augment is not None or self.align is not None:
            return self._augmented(idx)
        case = self.case_list[idx]
        if self.device_resample:
            # undecoded volumes for assemble_batch (None: a zero_fill channel); no numpy resampling
            files = case["modality_files"]
            return {"raw_images": [read_nifti_raw(files[m]) if m in files else None for m in self.modalities],
                    "raw_label": read_nifti_raw(case["label_path"]), "case_id": case["case_id"]}
        chans = []
        for m in self.modalities:
            p = case["modality_files"].get(m)
            if p is None:  # zero_fill (duplicate cases have every modality mapped)
                chans.append(np.zeros(self.target_size, dtype=np.float32))
                continue
            vol = self._first_volume(read_nifti(p)).astype(np.float32)
            if vol.shape != self.target_size:
                vol = resample(vol, self.target_size)
            chans.append(vol)
        lab = self._first_volume(read_nifti(case["label_path"]))
        if self.class_values is not None:  # (always through resample: its fp32 values are what the table names)
            label = classes_of(resample(lab, self.target_size, nearest=True), self.class_values)[None]
            return {"image": torch.from_numpy(np.stack(chans, 0)).float(), "label": torch.from_numpy(label),
                    "case_id": case["case_id"]}
        if lab.shape != self.target_size:
            lab = resample(lab, self.target_size, nearest=True)
        label = (lab > 0).astype(np.float32)[None]
        return {"image": torch.from_numpy(np.stack(chans, 0)).float(), "label": torch.from_numpy(label),
                "case_id": case["case_id"]}


def get_dataloader(data_dir: str, batch_size: int = 2, shuffle: bool = True, modalities=None,
                   missing_strategy: str = "zero_fill", target_size=(128, 128, 128), num_workers: int = 0,
                   is_training: bool = True, data_type: str = "BPH", indices=None, rank: int = 0,
                   world_size: int = 1, device_resample: bool = False, augment=None,
                   augment_seed: int = 0, patches=None, align=None, corrections=None, n_classes: int = 1,
                   class_values=None) -> DataLoader:
    """script/data_loader.py:421-466 (pinned host batches; Trainer stages them to the GPU on
    a copy stream one batch ahead).  ``world_size > 1``: each rank iterates its own
    DistributedSampler shard (call ``loader.sampler.set_epoch(epoch)`` every epoch).
    ``device_resample``: the batches carry the files' undecoded volumes (``RawVolume`` lists,
    same cases in the same order); ``assemble_batch`` resamples them on the GPU.
    ``augment`` / ``augment_seed``: training-time augmentation (``ProstateDataset``); call the
    dataset's ``set_epoch(epoch)`` every epoch (through a ``Subset``: ``loader.dataset.dataset``),
    ``Trainer.train`` does.  Both kinds of loader give equal batches with it too.
    ``patches`` (``PatchSampling``): patch training -- a batch concatenates the P patches of each
    of its ``batch_size`` cases, ``image`` (batch_size * P, M, wd, wh, ww), ``label``
    (batch_size * P, 1, ...), ``case_id`` repeated P times, plus ``picks`` (batch_size, 3P + 1):
    the origins and the foreground count per case; ``target_size`` is unused.  Both kinds of
    loader give equal batches here too (``assemble_patch_batch``).
    ``align`` / ``corrections``: the volumes are placed by their world geometry
    (``ProstateDataset``); both kinds of loader give equal batches with it as well.
    ``n_classes`` / ``class_values``: class-map labels (``ProstateDataset``); both kinds of loader
    give equal batches with them too."""
    patches = PatchSampling.of(patches)
    ds = ProstateDataset(data_dir, modalities=modalities, missing_strategy=missing_strategy,
                         target_size=target_size, is_training=is_training, data_type=data_type,
                         device_resample=device_resample, augment=augment, augment_seed=augment_seed,
                         patches=patches, align=align, corrections=corrections, n_classes=n_classes,
                         class_values=class_values)
    collate = _CollateRaw(target_size, patches, ds.class_values) if device_resample else None
    if patches is not None and not device_resample:
        collate = _collate_patches
    if indices is not None:
        ds = torch.utils.data.Subset(ds, indices)
    sampler = None
    if world_size > 1 and not is_training:
        # evaluation: whole batches of the single-process order, batch b on rank b % W (no
        # padding, no duplicates: the (sum, count) of per-batch losses over ranks is the
        # single-process mean)
        return DataLoader(ds, batch_sampler=BatchShard(len(ds), batch_size, rank, world_size),
                          num_workers=num_workers, pin_memory=torch.cuda.is_available(), collate_fn=collate)
    if world_size > 1:
        sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world_size, rank=rank,
                                                                  shuffle=shuffle)
    return DataLoader(ds, batch_size=batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                      num_workers=num_workers, pin_memory=torch.cuda.is_available(), collate_fn=collate)


class BatchShard(torch.utils.data.Sampler):
    """Batches ``b = 0, 1, ...`` of ``range(n)`` in order (``batch_size`` each, the last one
    short), keeping those with ``b % world_size == rank``."""

    def __init__(self, n: int, batch_size: int, rank: int, world_size: int):
        self.n, self.bs, self.rank, self.world = n, batch_size, rank, world_size

    def __iter__(self):
        for b, lo in enumerate(range(0, self.n, self.bs)):
            if b % self.world == self.rank:
                yield list(range(lo, min(self.n, lo + self.bs)))

    def __len__(self):
        nb = -(-self.n // self.bs)
        return max(0, -(-(nb - self.rank) // self.world))

    def set_epoch(self, epoch: int) -> None:  # the evaluation order does not change
        pass


def kfold_indices(n_cases: int, n_splits: int = 5, seed: int = 42):
    """sklearn ``KFold(n_splits, shuffle=True, random_state=seed).split(range(n_cases))``
    restated (the reference's get_kfold_splits, script/data_loader.py:468-497): a legacy
    numpy RandomState(seed) shuffle of arange(n), folds of n // k (+1 for the first n % k),
    each fold's test and train indices in ascending order."""
    if n_splits < 2 or n_splits > n_cases:
        raise ValueError(f"cannot split {n_cases} cases into {n_splits} folds")
    order = np.arange(n_cases)
    np.random.RandomState(seed).shuffle(order)
    sizes = np.full(n_splits, n_cases // n_splits, dtype=int)
    sizes[: n_cases % n_splits] += 1
    splits, cur = [], 0
    for sz in sizes:
        mask = np.zeros(n_cases, dtype=bool)
        mask[order[cur:cur + sz]] = True
        cur += sz
        idx = np.arange(n_cases)
        splits.append((idx[~mask], idx[mask]))
    return splits


def get_kfold_splits(data_dir: str, n_splits: int = 5, modalities=None, missing_strategy: str = "zero_fill",
                     target_size=(128, 128, 128), data_type: str = "BPH"):
    """script/data_loader.py:468-497: K (train_indices, val_indices) pairs over the case list
    scanned from <data_dir>/BPH-PCA/<data_type>/ADC (KFold, shuffle, random_state 42)."""
    ds = ProstateDataset.__new__(ProstateDataset)
    ds.data_dir, ds.data_type = data_dir, data_type
    return kfold_indices(len(ds._get_case_list()), n_splits)
