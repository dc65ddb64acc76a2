"""Resampling (csrc/resample.hip, csrc/deform.hip): host forms, then ``resample_device``.

``resample`` is the reference's ResampleImageFilter set-up -- same origin and direction, output
spacing = size * spacing / target, linear for images, nearest for labels: ITK's index mapping
restated (output index i samples input continuous index i * n_in / n_out); without SimpleITK its
results are parity-unpinned beyond the tests' closed-form cases (identity, integer down-sampling,
constant and linear ramps).  ``resample_affine`` is the same gather under a full 3x4 affine
(training-time augmentation, alignment), ``resample_deform`` adds a cubic B-spline displacement in
front of it.  ``resample_device`` runs all of them on a ``RawVolume`` whose bytes are on the GPU
(pcms_resample_linear / _label, pcms_resample_affine_*, pcms_resample_deform_*), bit for bit, and
with ``class_values`` the class-map labels of csrc/classes.hip.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._args import host_affine12, host_floats
from ._lib import call
from .nifti import RawVolume, device_raw


def _axis_linear(a: np.ndarray, axis: int, n_out: int) -> np.ndarray:
    """ITK linear resampling along one axis: output i samples continuous input index
    c = i * n_in / n_out; neighbours clamped at the border, zero outside [-0.5, n_in - 0.5)."""
    n_in = a.shape[axis]
    if n_in == n_out:
        return a
    c = np.arange(n_out, dtype=np.float64) * (n_in / n_out)
    inside = (c >= -0.5) & (c < n_in - 0.5)
    i0 = np.floor(c).astype(np.int64)
    w = (c - i0).reshape([-1 if d == axis else 1 for d in range(a.ndim)])
    lo = np.clip(i0, 0, n_in - 1)
    hi = np.clip(i0 + 1, 0, n_in - 1)
    out = np.take(a, lo, axis=axis) * (1.0 - w) + np.take(a, hi, axis=axis) * w
    mask = inside.reshape(w.shape)
    return np.where(mask, out, 0.0)


def _axis_nearest(a: np.ndarray, axis: int, n_out: int) -> np.ndarray:
    """ITK nearest neighbour along one axis (index rounded half up)."""
    n_in = a.shape[axis]
    if n_in == n_out:
        return a
    c = np.arange(n_out, dtype=np.float64) * (n_in / n_out)
    idx = np.floor(c + 0.5).astype(np.int64)
    inside = idx < n_in
    out = np.take(a, np.clip(idx, 0, n_in - 1), axis=axis)
    mask = inside.reshape([-1 if d == axis else 1 for d in range(a.ndim)])
    return np.where(mask, out, 0)


def resample(vol: np.ndarray, target: Tuple[int, int, int], nearest: bool = False) -> np.ndarray:
    """Resample a (D, H, W) volume to ``target`` with the reference's ResampleImageFilter
    geometry (script/data_loader.py:258-281 images, linear; :383-406 labels, nearest)."""
    out = vol.astype(np.float64) if not nearest else vol
    f = _axis_nearest if nearest else _axis_linear
    for ax in range(3):
        out = f(out, ax, int(target[ax]))
    return out.astype(np.float32)


def resample_affine(vol: np.ndarray, target: Tuple[int, int, int], A, t, nearest: bool = False,
                    gain: float = 1.0, bias: float = 0.0) -> np.ndarray:
    """``resample`` under a full affine (training-time augmentation): output index (d, h, w)
    samples source axis a at ``c_a = ((A[a][0]*d + A[a][1]*h) + A[a][2]*w) + t[a]`` -- fp64,
    every product and sum a numpy operation of its own, in this order.  A gather over the
    output grid; libpcms_hip's pcms_resample_affine_linear / _label restate it per voxel and
    are compared with it on the fp32 bits.

    Linear: inside iff ``-0.5 <= c_a < n_a - 0.5`` on all three axes (ITK's buffer rule, as
    ``_axis_linear``); there ``i0 = floor(c)``, ``w = c - i0``, neighbours ``i0`` and ``i0 + 1``
    each clamped to ``[0, n - 1]``, the 8 corners lerped ``a*(1-w) + b*w`` along D, then H, then
    W, rounded once to fp32; unless ``gain == 1 and bias == 0`` an inside voxel then becomes
    ``fl32(fl32(r*gain) + bias)`` (``gain`` / ``bias`` as fp32).  Outside voxels are 0.
    ``nearest``: ``k_a = floor(c_a + 0.5)``, 0 where any ``k_a`` is outside ``[0, n_a)``, else the
    voxel's value as fp32 (the loader binarises it ``> 0``).
    With ``A = diag(n_in / n_out)``, ``t = 0`` both forms equal ``resample`` bit for bit."""
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    D, H, W = (int(v) for v in target)
    grid = (np.arange(D, dtype=np.float64).reshape(D, 1, 1), np.arange(H, dtype=np.float64).reshape(1, H, 1),
            np.arange(W, dtype=np.float64).reshape(1, 1, W))
    with np.errstate(over="ignore", invalid="ignore"):  # a far-out coordinate may overflow: it is outside
        c = [((A[a, 0] * grid[0] + A[a, 1] * grid[1]) + A[a, 2] * grid[2]) + t[a] for a in range(3)]
    return _sample_at(vol, c, nearest, gain, bias)


def _sample_at(vol: np.ndarray, c, nearest: bool, gain, bias) -> np.ndarray:
    """The gather of ``resample_affine`` / ``resample_deform`` at the source coordinates ``c``
    (three fp64 arrays of the output shape): inside rule, clamps, lerp tree, intensity step and
    nearest rule as ``resample_affine`` documents them."""
    n_in = vol.shape
    shape = c[0].shape
    with np.errstate(over="ignore", invalid="ignore"):
        if nearest:
            k = [np.floor(c[a] + 0.5) for a in range(3)]
            inside = np.ones(shape, dtype=bool)
            for a in range(3):
                inside &= (k[a] >= 0.0) & (k[a] < float(n_in[a]))
            idx = [np.where(inside, k[a], 0.0).astype(np.int64) for a in range(3)]
            return np.where(inside, vol[idx[0], idx[1], idx[2]], 0).astype(np.float32)
        inside = np.ones(shape, dtype=bool)
        for a in range(3):
            inside &= (c[a] >= -0.5) & (c[a] < n_in[a] - 0.5)
    lo, hi, w = [], [], []
    for a in range(3):
        ca = np.where(inside, c[a], 0.0)
        i0 = np.floor(ca).astype(np.int64)
        w.append(ca - i0)
        lo.append(np.clip(i0, 0, n_in[a] - 1))
        hi.append(np.clip(i0 + 1, 0, n_in[a] - 1))
    v = vol.astype(np.float64)
    vh = []
    for xw in (lo[2], hi[2]):
        vd = [v[lo[0], xh, xw] * (1.0 - w[0]) + v[hi[0], xh, xw] * w[0] for xh in (lo[1], hi[1])]
        vh.append(vd[0] * (1.0 - w[1]) + vd[1] * w[1])
    out = (vh[0] * (1.0 - w[2]) + vh[1] * w[2]).astype(np.float32)
    gain, bias = np.float32(gain), np.float32(bias)
    if not (gain == 1.0 and bias == 0.0):
        out = out * gain + bias  # two fp32 operations
    return np.where(inside, out, np.float32(0.0))


MAX_CONTROL_POINTS = 512  # gd * gh * gw of an elastic field: 12 KB of doubles in the kernels' LDS


def _bspline_axis(n: int, g: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(k, b)`` of one output axis of extent ``n`` under ``g`` control points: the first of
    the four control indices per output index and the (n, 4) uniform cubic B-spline weights,
    one numpy operation per product, sum and division."""
    x = np.arange(n, dtype=np.float64) * (float(g - 3) / float(n))
    f = np.floor(x)
    s = x - f
    r = 1.0 - s
    s2 = s * s
    s3 = s2 * s
    b0 = ((r * r) * r) / 6.0
    b1 = ((3.0 * s3 - 6.0 * s2) + 4.0) / 6.0
    b2 = ((((-3.0 * s3) + 3.0 * s2) + 3.0 * s) + 1.0) / 6.0
    b3 = s3 / 6.0
    return f.astype(np.int64), np.stack([b0, b1, b2, b3], axis=1)


def field_displacement(field: np.ndarray, target: Tuple[int, int, int]) -> List[np.ndarray]:
    """The displacement ``[u_D, u_H, u_W]`` (fp64, output voxels, each of shape ``target``) of
    a control grid ``field[gd][gh][gw][3]``: the uniform cubic B-spline of ``resample_deform``.
    The inner sums depend on (control row, control row, w), then (control row, h, w), so they
    are formed once per such triple -- the same operands in the same order as per voxel."""
    P = np.asarray(field, dtype=np.float64)
    if P.ndim != 4 or P.shape[3] != 3 or min(P.shape[:3]) < 4:
        raise ValueError(f"an elastic field is (gd, gh, gw, 3) with every count >= 4, got {P.shape}")
    D, H, W = (int(v) for v in target)
    (kd, bd), (kh, bh), (kw, bw) = (_bspline_axis(n, g) for n, g in zip((D, H, W), P.shape[:3]))
    u = []
    with np.errstate(over="ignore", invalid="ignore"):  # a non-finite control vector: NaN, outside
        for c in range(3):
            Pc = P[..., c]
            sw = bw[:, 0] * Pc[:, :, kw]                                  # (gd, gh, W)
            for j in (1, 2, 3):
                sw = sw + bw[:, j] * Pc[:, :, kw + j]
            sh = bh[:, 0, None] * sw[:, kh, :]                            # (gd, H, W)
            for j in (1, 2, 3):
                sh = sh + bh[:, j, None] * sw[:, kh + j, :]
            sd = bd[:, 0, None, None] * sh[kd]                            # (D, H, W)
            for j in (1, 2, 3):
                sd = sd + bd[:, j, None, None] * sh[kd + j]
            u.append(sd)
    return u


def resample_deform(vol: np.ndarray, target: Tuple[int, int, int], A, t, field, nearest: bool = False,
                    gain: float = 1.0, bias: float = 0.0) -> np.ndarray:
    """``resample_affine`` with a smooth elastic displacement added to the output index before
    the affine.  ``field`` is one fp64 control grid ``P[gd][gh][gw][3]`` (every count >= 4), a
    uniform cubic B-spline over the output grid's index space.  For output index ``i`` of an
    axis of extent ``N`` with ``g`` control points: ``x = i * ((g - 3) / N)``, ``k = floor(x)``
    (``0 <= k <= g - 4``), ``s = x - k``, ``r = 1 - s``, ``s2 = s*s``, ``s3 = s2*s`` and

        b0 = ((r*r)*r) / 6                     b1 = ((3*s3 - 6*s2) + 4) / 6
        b2 = ((((-3*s3) + 3*s2) + 3*s) + 1) / 6        b3 = s3 / 6

    ``u_c = sum_jd bd[jd] * (sum_jh bh[jh] * (sum_jw bw[jw] * P[kd+jd][kh+jh][kw+jw][c]))`` for
    component c in (D, H, W), every sum left to right from j = 0, every product, sum and
    division a numpy operation of its own.  The voxel samples the source at
    ``c_a = ((A[a][0]*p_d + A[a][1]*p_h) + A[a][2]*p_w) + t[a]`` with ``p_a = index_a + u_a``;
    from there on everything is ``resample_affine``'s, and a zero field gives its result bit
    for bit.  A non-finite control vector gives NaN coordinates, which are outside (0).
    libpcms_hip's pcms_resample_deform_linear / _label restate this per voxel and are compared
    with it on the fp32 bits."""
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    D, H, W = (int(v) for v in target)
    u = field_displacement(field, (D, H, W))
    grid = (np.arange(D, dtype=np.float64).reshape(D, 1, 1), np.arange(H, dtype=np.float64).reshape(1, H, 1),
            np.arange(W, dtype=np.float64).reshape(1, 1, W))
    with np.errstate(over="ignore", invalid="ignore"):
        p = [grid[a] + u[a] for a in range(3)]
        c = [((A[a, 0] * p[0] + A[a, 1] * p[1]) + A[a, 2] * p[2]) + t[a] for a in range(3)]
    return _sample_at(vol, c, nearest, gain, bias)


def resample_device(raw: RawVolume, target: Tuple[int, int, int], nearest: bool = False,
                    out: Optional[torch.Tensor] = None, affine: Optional[Sequence[float]] = None,
                    gain: float = 1.0, bias: float = 0.0, field: Optional[torch.Tensor] = None,
                    class_values: Optional[Sequence[float]] = None) -> torch.Tensor:
    """``resample`` of a volume whose bytes are on the GPU, on the current stream: the linear
    form equals ``resample(vol.astype(float32), target)`` bit for bit, ``nearest=True`` gives
    the binarised label ``resample(vol, target, nearest=True) > 0`` as fp32 {0, 1} (for a
    volume already of the target shape, ``vol > 0``), as ``ProstateDataset.__getitem__`` forms
    them.  Fills ``out`` (a contiguous fp32 (D, H, W) device tensor, e.g. one channel of a
    batch) or returns a new one.  There is no CPU form: host bytes raise.
    ``affine`` (twelve doubles, row-major A then t) selects the augmenting entry points:
    ``resample_affine(vol.astype(float32), target, A, t, gain=gain, bias=bias)`` and, with
    ``nearest``, ``resample_affine(vol, target, A, t, nearest=True) > 0``, bit for bit.
    ``field`` (a contiguous fp64 ``(gd, gh, gw, 3)`` tensor on the volume's device; needs
    ``affine``) selects the deforming entry points: ``resample_deform`` with that control grid
    in place of ``resample_affine``, bit for bit again.
    ``class_values`` (1..7 label-file values; needs ``nearest``, no ``field``) selects the class-map
    entry points pcms_resample_classes / pcms_resample_affine_classes: the same nearest gather,
    then ``classes.classes_of(., class_values)`` in place of ``> 0`` -- class ``j + 1`` where the
    fp32 value is ``class_values[j]``, else 0 -- byte for byte."""
    target = tuple(int(v) for v in target)
    raw = device_raw(raw, "resample_device")
    table = None
    if class_values is not None:
        if not nearest or field is not None:
            raise ValueError("class_values select the class-map label: they need nearest=True and no field (an "
                             "elastic deformation of a class map is not supported)")
        if not 1 <= len(class_values) <= 7:
            raise ValueError(f"class_values holds 1..7 values, got {tuple(class_values)!r}")
        table = host_floats(class_values)  # read during the call: stays in this local until it returns
    if out is None:
        out = torch.empty(target, dtype=torch.float32, device=raw.data.device)
    elif (tuple(out.shape) != target or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != raw.data.device):
        raise ValueError(f"out must be a contiguous fp32 {target} tensor on {raw.data.device}")
    if affine is None:
        if field is not None:
            raise ValueError("field needs affine: the deformation is applied in front of the affine")
        if table is not None:
            call("pcms_resample_classes", *raw.kernel_args(), ctypes.addressof(table), len(class_values), out, *target)
            return out
        call("pcms_resample_label" if nearest else "pcms_resample_linear", *raw.kernel_args(), out, *target)
        return out
    if len(affine) != 12:
        raise ValueError("affine must hold twelve doubles: row-major A[3][3], then t[3]")
    host = host_affine12(affine)  # read during the call: stays in this local until it returns
    if field is not None:
        if (field.dtype != torch.float64 or field.dim() != 4 or field.shape[3] != 3 or not field.is_contiguous()
                or field.device != raw.data.device):
            raise ValueError(f"field must be a contiguous fp64 (gd, gh, gw, 3) tensor on {raw.data.device}")
        grid = tuple(int(v) for v in field.shape[:3])
        if nearest:
            call("pcms_resample_deform_label", *raw.kernel_args(), ctypes.addressof(host), field, *grid, out, *target)
        else:
            call("pcms_resample_deform_linear", *raw.kernel_args(), ctypes.addressof(host), field, *grid, float(gain),
                 float(bias), out, *target)
        return out
    if table is not None:
        call("pcms_resample_affine_classes", *raw.kernel_args(), ctypes.addressof(host), ctypes.addressof(table),
             len(class_values), out, *target)
    elif nearest:
        call("pcms_resample_affine_label", *raw.kernel_args(), ctypes.addressof(host), out, *target)
    else:
        call("pcms_resample_affine_linear", *raw.kernel_args(), ctypes.addressof(host), float(gain), float(bias), out,
             *target)
    return out
