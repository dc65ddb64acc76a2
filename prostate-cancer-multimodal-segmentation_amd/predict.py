"""Single-case prediction pipeline (reference script/predict.py), on the HIP engine.

* ``load_multimodal_images(case_dir, handle_missing)``: the five modality folders
  ['ADC', 'DWI', 'gaoqing-T2', 'T2 fs', 'T2 not fs'] (predict.py:25), the first ``.nii`` of
  each, per-modality min-max normalisation to [0, 1] (constant image -> zeros, :70-75),
  missing modalities by 'zero_fill' / 'skip' / 'duplicate' (:38-55), stacked (5, D, H, W)
  (:81).  NIfTI through pcms_amd.nifti's reader (SimpleITK is not a dependency).
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

What a case goes through lives with its kernel family, one module per ``csrc/*.hip`` file; every
public name of those modules is also a name of this one:
* ``intensity`` (§0q): min-max and percentile-window normalisation, ``Normalisation``;
* ``align`` (§0r): joint histogram, mutual information, rigid registration, ``Alignment``;
* ``window`` (§0o): sliding windows, their blend, ``tta_mean``;
* ``components`` (§0k): connected components and mask post-processing;
* ``lesions`` (§0n): per-lesion tables and detection scores;
* ``distance`` (§0l): surfaces, the exact distance transform, HD / HD95 / ASSD;
* ``classes`` (§0t): softmax planes, the class map on the native grid, per-class overlap --
  ``ModelPredictor(..., n_classes=C)`` predicts mutually exclusive classes with them.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._args import host_affine12, host_ints
from ._lib import call
from .align import (DEFAULT_LEVELS, MODALITIES, Alignment, _aligned_affines, _case_files,  # noqa: F401
                    _case_reference, _fixed_modality, joint_histogram, joint_histogram_device,
                    normalised_mutual_information, register_case, register_case_device, register_dataset,
                    register_rigid, register_rigid_device)
from .classes import (check_n_classes, class_overlap_device, class_values_of, classes_of,  # noqa: F401
                      labels_on_grid, labels_on_grid_device, scores_of_counts, softmax_planes_device)
from .components import (MAX_KEEP_LARGEST, _check_filter, _check_status, _offsets,  # noqa: F401
                         _postprocess_enqueue, fill_holes, filter_components, label_components,
                         label_components_device, postprocess, postprocess_device)
from .distance import (distance_transform, distance_transform_device, edt_sq, surface,  # noqa: F401
                       surface_device, surface_metrics, surface_metrics_device)
from .geometry import affine12_of
from .intensity import (Normalisation, _lohi_enqueue, intensity_window, normalise,  # noqa: F401
                        normalise_window)
from .lesions import (TABLE_CAPACITY, component_table, component_table_device, lesion_metrics,  # noqa: F401
                      lesion_metrics_device, lesion_table, lesion_table_device, match_lesions, overlap_pairs,
                      overlap_pairs_device)
from .models.unet3d import UNet3D, load_weights
from .nifti import (_first_volume, _shape_zyx, read_nifti, read_nifti_geometry, read_nifti_header, read_nifti_raw,
                    write_nifti)
from .resample import resample, resample_affine, resample_device
from .utils.metrics import calculate_dice_score, calculate_iou
from .window import (MAX_WINDOW_AXIS, _check_sliding, _flip_masks, blend_windows,  # noqa: F401
                     blend_windows_device, gather_windows, gather_windows_device, sliding_window_device,
                     sliding_window_predict, tta_mean, window_grid, window_starts, window_weights)


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
        grid = _shape_zyx(_case_reference(paths, align))
    else:
        shapes = {p: tuple(read_nifti_header(p)["shape_xyz"][:3][::-1]) for p in paths if p is not None}
        if len(set(shapes.values())) != 1:
            raise ValueError(f"target_size=None needs modalities of one shape, got {sorted(set(shapes.values()))}")
        grid = shapes[paths[present[0]]]
    return paths, grid, present[0] if handle_missing == "duplicate" else None


def prepare_case(case_dir: str, target_size: Optional[Sequence[int]] = (128, 128, 128),
                 handle_missing: str = "zero_fill", normalise=True, align=None,
                 return_alignment: bool = False) -> np.ndarray:
    """The five modalities of a case on one grid, (5, D, H, W) float32: per modality the first
    ``.nii`` in sorted order (volume 0 of a 4-D file), ``normalise``d when asked, else as fp32,
    then ``resample.resample(., target_size)`` (linear).  A missing modality is zeros
    ('zero_fill'), the first present modality's channel ('duplicate') or an error ('skip').
    ``target_size=None``: no resampling; the present shapes must agree (ValueError).
    With ``normalise=False`` a channel is the one the default training loader forms for the
    file; with ``normalise=True`` it is ``load_multimodal_images``' channel on the grid.
    ``normalise`` is anything ``Normalisation.of`` accepts: ``"percentile"`` (or a dict / a
    ``Normalisation``) clips every modality to its own percentile window first.
    ``align`` (anything ``Alignment.of`` accepts; None: everything above, unchanged): every present
    modality is resampled by ``resample.resample_affine`` under ``geometry.case_affine`` -- the grid scaled
    onto the reference file's native grid, then ``geometry.align_affine`` into the modality's file -- so
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
        chans.append(resample(vol, grid) if affines is None else resample_affine(vol, grid, *affines[c]))
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


def mask_on_grid(prob: np.ndarray, native_shape: Sequence[int], threshold: float = 0.5):
    """A probability volume on the training grid -> ``(uint8 mask, float32 probabilities)`` on
    the ``native_shape`` grid: ``resample.resample(prob.astype(float32), native_shape)`` and its
    strict ``> float32(threshold)``.  This is the exact inverse geometry of the forward map:
    native index i samples target coordinate ``i * n_tgt / n_nat``.  ``resample.resample``'s edge
    rule holds here too: a sample at or past ``n_tgt - 0.5`` is 0, so where the native grid is
    finer than the training grid the trailing fraction of a training voxel reads as
    background."""
    prob_native = resample(np.asarray(prob).astype(np.float32), tuple(int(v) for v in native_shape))
    return (prob_native > np.float32(threshold)).astype(np.uint8), prob_native


def prepare_case_device(case_dir: str, target_size: Optional[Sequence[int]] = (128, 128, 128),
                        handle_missing: str = "zero_fill", normalise=True,
                        device="cuda", align=None, return_alignment: bool = False) -> torch.Tensor:
    """``prepare_case`` on the GPU, bit for bit, as the (1, 5, D, H, W) fp32 network input: each
    file's undecoded bytes (``nifti.read_nifti_raw``) go up once; pcms_volume_minmax and
    pcms_resample_linear_norm form the min-max normalised channel, pcms_volume_window and
    pcms_resample_linear_window the percentile one (the window is computed once per volume and
    read from device memory), ``resample.resample_device`` the plain one.  Everything is enqueued on
    the current stream.
    ``align``: ``prepare_case``'s, bit for bit too.  Per present modality one launch under the
    twelve doubles of ``geometry.case_affine`` -- the host form's own -- fills the channel:
    pcms_patch_resample_linear / pcms_patch_resample_window with one patch at origin 0 that is the
    whole grid (the normalised corners), or pcms_resample_affine_linear without normalisation.
    ``"register"`` runs ``register_case_device`` on the uploaded bytes first (it reads one small
    table back per evaluation).  ``align=None``: nothing new is launched."""
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
        raws = {c: read_nifti_raw(p).to(device) for c, p in enumerate(paths) if p is not None}
        affines = None
        if align is not None:
            if align.mode == "register":
                report = register_case_device(dict(zip(MODALITIES, paths)), normalise, align, device, raws)
            affines = _aligned_affines(paths, grid, _case_reference(paths, align), report,
                                       _fixed_modality(paths, align))
            origin = torch.zeros(3, dtype=torch.int32, device=device)
        for c, raw in raws.items():
            if affines is not None:
                twelve = affine12_of(*affines[c])
                if norm is None:
                    resample_device(raw, grid, out=x[0, c], affine=twelve)
                    continue
                windowed = _lohi_enqueue(raw, norm, lohi) == "window"
                host = host_affine12(twelve)  # read during the call: stays in this local until it returns
                call("pcms_patch_resample_window" if windowed else "pcms_patch_resample_linear", *raw.kernel_args(),
                     ctypes.addressof(host), lohi, 1.0, 0.0, *grid, origin, 1, x[0, c], grid[0] * grid[1] * grid[2],
                     *grid)
                continue
            if norm is None:
                resample_device(raw, grid, out=x[0, c])
                continue
            kind = _lohi_enqueue(raw, norm, lohi)
            call("pcms_resample_linear_" + kind, *raw.kernel_args(), lohi, x[0, c], *grid)
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
    ``nifti.read_nifti_geometry`` is ``geometry``; ``lesions`` is ``lesion_table`` of the mask when
    ``predict_case`` was asked for it; ``alignment``: with ``align``, per present modality
    ``{"params": (tz, ty, tx, rz, ry, rx), "before": .., "after": ..}`` -- the rigid correction
    and the similarity before and after it (zeros and None where nothing was registered) -- else
    None.  From a predictor of ``n_classes > 1`` the ``mask`` holds class indices, the
    ``probability`` is (C, z, y, x) and every row of ``lesions`` carries its ``"class"``."""
    mask: np.ndarray
    probability: Optional[np.ndarray]
    reference_path: str
    geometry: dict
    lesions: Optional[List[dict]] = None
    alignment: Optional[dict] = None


def preprocess_image(image: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(image)).float().unsqueeze(0)


class ModelPredictor:
    def __init__(self, model_path: str, device: str = "cuda", precision: str = "bf16", n_classes: int = 1,
                 class_values=None):
        """``n_classes > 1``: the network emits that many logit planes and ``predict_case``
        returns a class map; ``class_values`` (default ``(1, .., n_classes - 1)``) are
        the values a label file gives the foreground classes, for ``score_case``."""
        self.device = torch.device(device)
        self.n_classes = check_n_classes(n_classes)
        self.class_values = class_values_of(n_classes, class_values) if n_classes > 1 else None
        self.model = UNet3D(n_modalities=5, n_classes=n_classes, precision=precision).to(self.device)
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
        result's ``alignment`` reports the corrections.  ``align=None``: nothing changes.
        A predictor of ``n_classes > 1``: the logits of the batch go through
        pcms_softmax_planes (class-major), each class's flipped copies through pcms_flip_mean, and
        pcms_probs_to_labels (``classes.labels_on_grid``) gives the class map on the native grid --
        the class of the largest probability, the first one on a tie; ``threshold`` is unused.
        ``keep_largest`` / ``min_voxels`` / ``fill_holes`` run pcms_mask_postprocess once per
        foreground class on ``labels == c``: a removed voxel becomes 0, a filled hole takes the
        class where it was background.  ``return_lesions`` tables every class's components with
        that class's probability plane.  ``window`` raises ValueError there."""
        if self.n_classes > 1:
            if window is not None:
                raise ValueError("sliding-window prediction of n_classes > 1 is not supported: the blend takes one "
                                 "probability plane")
            return self._predict_case_classes(case_dir, target_size, handle_missing, normalise, tta_flips, output_like,
                                              return_probability, keep_largest, min_voxels, fill_holes, connectivity,
                                              return_lesions, align)
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
        geometry = read_nifti_geometry(reference)
        grid = tuple(x.shape[2:])
        with torch.no_grad(), torch.cuda.device(self.device):
            if window is not None:
                prob = sliding_window_device(self.model.predict, x, window, overlap, blend, tta_flips, window_batch)
            else:
                batch = torch.cat([x] + [torch.flip(x, dims=[2 + a for a in f]) for f in tta_flips], dim=0)
                probs = self.model.predict(batch).float().contiguous()  # (k, 1, D, H, W)
                if len(masks) > 1:
                    host = host_ints(masks)  # read during the call: stays in this local until it returns
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

    def _predict_case_classes(self, case_dir, target_size, handle_missing, normalise, tta_flips, output_like,
                              return_probability, keep_largest, min_voxels, fill_holes, connectivity, return_lesions,
                              align) -> CasePrediction:
        """``predict_case`` of a predictor of ``n_classes > 1`` (its docstring has the steps)."""
        align = Alignment.of(align)
        if align is not None and align.to is None and output_like is not None:
            align = dataclasses.replace(align, to=output_like)
        masks = _flip_masks(tta_flips)
        _check_filter(keep_largest, min_voxels)
        _offsets(connectivity)
        post = keep_largest != 0 or min_voxels > 1 or bool(fill_holes)
        x, alignment = prepare_case_device(case_dir, target_size, handle_missing, normalise, self.device, align,
                                           return_alignment=True)  # raises if none present
        reference = output_like if output_like is not None else \
            next(p for p in _case_files(case_dir) if p is not None) if align is None else \
            _case_reference(_case_files(case_dir), align)
        native = tuple(int(v) for v in read_nifti_header(reference)["shape_xyz"][:3][::-1])
        geometry = read_nifti_geometry(reference)
        grid = tuple(x.shape[2:])
        C = self.n_classes
        self.model.eval()
        with torch.no_grad(), torch.cuda.device(self.device):
            batch = torch.cat([x] + [torch.flip(x, dims=[2 + a for a in f]) for f in tta_flips], dim=0)
            probs = softmax_planes_device(self.model(batch))  # (C, k, D, H, W): a class's k volumes are contiguous
            if len(masks) > 1:
                host = host_ints(masks)  # read during the calls: stays in this local until the last one returns
                mean = torch.empty((C,) + grid, dtype=torch.float32, device=self.device)
                for c in range(C):
                    call("pcms_flip_mean", probs[c], len(masks), ctypes.addressof(host), mean[c], *grid)
            else:
                mean = probs[:, 0]
            labels, planes = labels_on_grid_device(mean, native, return_probability or return_lesions)
            if post:
                for c in range(1, C):
                    own = (labels == c).to(torch.uint8)
                    kept, work = _postprocess_enqueue(own, keep_largest, min_voxels, fill_holes, connectivity)
                    _check_status(int(work[0].item()), "predict_case")
                    labels = torch.where((own != 0) & (kept == 0), torch.zeros_like(labels), labels)
                    labels = torch.where((kept != 0) & (labels == 0), torch.full_like(labels, c), labels)
            lesions = None
            if return_lesions:
                spacing = tuple(float(v) for v in geometry["pixdim"][1:4])[::-1]
                lesions = []
                for c in range(1, C):
                    rows = lesion_table_device((labels == c).to(torch.uint8), planes[c], spacing, connectivity)
                    lesions.extend(dict(r, **{"class": c}) for r in rows)
            mask_host = labels.cpu().numpy()
        return CasePrediction(mask_host, planes.cpu().numpy() if return_probability else None, reference, geometry,
                              lesions, alignment)

    def _score_case_classes(self, result: CasePrediction, label_path: str, lesion_metrics: bool, min_iou: float,
                            connectivity: int) -> dict:
        """``score_case`` of a predictor of ``n_classes > 1``."""
        label = classes_of(_first_volume(read_nifti(label_path)), self.class_values).astype(np.uint8)
        if tuple(label.shape) != tuple(result.mask.shape):
            raise ValueError(f"label of shape {tuple(label.shape)} is not on the grid {tuple(result.mask.shape)} of "
                             "the mask")
        spacing = tuple(float(v) for v in result.geometry["pixdim"][1:4])[::-1]
        with torch.cuda.device(self.device):
            mask = torch.from_numpy(np.ascontiguousarray(result.mask, dtype=np.uint8)).to(self.device)
            lab = torch.from_numpy(np.ascontiguousarray(label)).to(self.device)
            dice, iou = scores_of_counts(class_overlap_device(mask, lab, self.n_classes).cpu().numpy())
            per_class = []
            for c in range(1, self.n_classes):
                mc, lc = (mask == c).to(torch.uint8), (lab == c).to(torch.uint8)
                row = {"class": c, "dice": dice[c], "iou": iou[c]}
                row.update(surface_metrics_device(mc, lc, spacing))
                if lesion_metrics:
                    prob = None if result.probability is None else \
                        torch.from_numpy(np.ascontiguousarray(result.probability[c], dtype=np.float32)).to(self.device)
                    row["lesions"] = lesion_metrics_device(mc, lc, prob, spacing, connectivity, min_iou)
                per_class.append(row)
        fg = max(self.n_classes - 1, 1)
        return {"dice": sum(dice[1:]) / fg, "iou": sum(iou[1:]) / fg, "class_dice": dice, "class_iou": iou,
                "classes": per_class}

    def score_case(self, result: CasePrediction, label_path: str, lesion_metrics: bool = False,
                   min_iou: float = 0.1, connectivity: int = 26) -> dict:
        """Score ``result.mask`` against the label file ``label_path`` (binarised with ``!= 0``)
        on the device: ``dice`` and ``iou`` (utils.metrics) and ``surface_metrics_device``'s
        ``hd`` / ``hd95`` / ``assd`` / ``n_a`` / ``n_b`` in millimetres, the spacing being
        ``result.geometry``'s pixdim[1..3] reversed to (z, y, x).  With ``lesion_metrics=True`` the
        dict gains ``"lesions"``: ``lesion_metrics_device`` of mask against label at
        ``connectivity`` and ``min_iou``, in the same spacing, the predicted lesions' confidence
        from ``result.probability`` when the result carries it.  ValueError if the label is not on
        the mask's grid.
        A predictor of ``n_classes > 1``: the label becomes a class map through ``class_values``
        (``classes.classes_of``); ``class_dice`` / ``class_iou`` list every class's score
        (pcms_class_overlap; a class absent from both maps scores 1.0), ``dice`` / ``iou`` are
        their means over the foreground classes, and ``classes`` holds per foreground class the
        scores above, the surface metrics and, when asked, the lesion metrics of ``mask == c``
        against ``label == c``."""
        if self.n_classes > 1:
            return self._score_case_classes(result, label_path, lesion_metrics, min_iou, connectivity)
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
