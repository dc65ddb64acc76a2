"""Affine geometry on the host, in fp64 with every product and sum written out (no BLAS: the same
doubles wherever they are formed).

``compose_transform`` / ``volume_affine``: the augmentation transform of a case in the output grid's
index space and one volume's ``(A, t)`` under it.  World geometry: ``world_matrix`` /
``align_affine`` / ``compose_affine`` / ``case_affine`` place every volume of a case on the
reference file's grid through the files' NIfTI geometry; ``rigid_world`` / ``rigid_correction`` are
the rigid corrections ``align.register_rigid`` finds.  ``affine12_of``: the twelve doubles the C
entry points take.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np


def _matmul3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """3x3 product with a fixed order of operations (no BLAS: the same doubles everywhere)."""
    return np.array([[(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(3)] for i in range(3)])


def compose_transform(flips=(False, False, False), rotate_deg=(0.0, 0.0, 0.0), zoom: float = 1.0) -> np.ndarray:
    """The geometric part ``L`` of a transform, in the output grid's index space:
    ``M = R_D(td) . R_H(th) . R_W(tw)`` (rotations about the D, H and W axes),
    ``L = F . M^T / zoom`` with ``F = diag(+-1)`` holding the flips."""
    td, th, tw = (float(np.deg2rad(a)) for a in rotate_deg)
    c, s = np.cos, np.sin
    rd = np.array([[1.0, 0.0, 0.0], [0.0, c(td), -s(td)], [0.0, s(td), c(td)]])
    rh = np.array([[c(th), 0.0, s(th)], [0.0, 1.0, 0.0], [-s(th), 0.0, c(th)]])
    rw = np.array([[c(tw), -s(tw), 0.0], [s(tw), c(tw), 0.0], [0.0, 0.0, 1.0]])
    m = _matmul3(_matmul3(rd, rh), rw)
    f = np.array([-1.0 if b else 1.0 for b in flips])
    return (f[:, None] * m.T) / float(zoom) + 0.0  # + 0.0: no negative zeros


def volume_affine(L, shift, n_in, n_out) -> Tuple[np.ndarray, np.ndarray]:
    """One volume's ``(A, t)`` of a case's transform: with ``S = diag(n_in / n_out)`` and the
    output grid's centre ``C = (n_out - 1) / 2``, ``A = S.L`` and ``t = S.(C - L.C - shift)``
    (``shift`` in output voxels): every volume of a case sees one geometry in output space."""
    L = np.asarray(L, dtype=np.float64).reshape(3, 3)
    shift = np.asarray(shift, dtype=np.float64).reshape(3)
    S = np.array([float(i) / float(o) for i, o in zip(n_in, n_out)])  # numpy's n_in / n_out, as resample
    C = np.array([(float(o) - 1.0) / 2.0 for o in n_out])
    LC = np.array([(L[a, 0] * C[0] + L[a, 1] * C[1]) + L[a, 2] * C[2] for a in range(3)])
    return S[:, None] * L + 0.0, S * ((C - LC) - shift) + 0.0


# ---- world geometry: where a file's grid lies in space -----------------------------
# A world matrix is 4x4 fp64 and maps a file's (x, y, z) voxel index (homogeneous) to millimetres.
# Arrays are (z, y, x), so an array-order affine is P . M . P with P the x<->z swap.  All products
# below are written out (no BLAS): the same doubles wherever they are formed.
def _matmul4(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.array([[((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
                      for j in range(4)] for i in range(4)])


def _affine_inverse4(w: np.ndarray, what: str) -> np.ndarray:
    """The inverse of a 4x4 affine (last row 0 0 0 1) by the adjugate of its 3x3 part; ValueError
    when that part is singular or not finite."""
    m = w[:3, :3]
    c = np.array([[m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3]
                   - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3] for j in range(3)] for i in range(3)])
    det = (m[0, 0] * c[0, 0] + m[0, 1] * c[0, 1]) + m[0, 2] * c[0, 2]
    if not np.isfinite(w).all() or det == 0.0:
        raise ValueError(f"{what}: the world matrix is singular or not finite")
    inv = np.eye(4)
    inv[:3, :3] = c.T / det
    inv[:3, 3] = [-((inv[i, 0] * w[0, 3] + inv[i, 1] * w[1, 3]) + inv[i, 2] * w[2, 3]) for i in range(3)]
    return inv + 0.0


def world_matrix(geometry: dict) -> np.ndarray:
    """The (4, 4) fp64 matrix that maps a file's (x, y, z) voxel index to millimetres, from a
    ``read_nifti_geometry`` dict, formed in fp64 from the header's float32 fields.  Precedence:
    the sform rows (``srow_x/y/z``) when ``sform_code > 0``; else, when ``qform_code > 0``, the
    NIfTI-1 quaternion form -- ``a = sqrt(1 - b^2 - c^2 - d^2)`` (0 when the sum exceeds 1), the
    rotation of (a, b, c, d), its columns scaled by ``pixdim[1..3]``, the third also by ``qfac =
    pixdim[0]`` (-1 only when the field is exactly -1, else +1), the offset ``qoffset_x/y/z``;
    else ``diag(pixdim[1..3])`` with a zero offset."""
    g = geometry
    w = np.eye(4)
    pix = [float(v) for v in g["pixdim"]]
    if int(g["sform_code"]) > 0:
        for i, name in enumerate(("srow_x", "srow_y", "srow_z")):
            w[i, :] = [float(v) for v in g[name]]
        return w
    if int(g["qform_code"]) > 0:
        b, c, d = float(g["quatern_b"]), float(g["quatern_c"]), float(g["quatern_d"])
        a2 = 1.0 - (b * b + c * c + d * d)
        a = float(np.sqrt(a2)) if a2 > 0.0 else 0.0
        r = np.array([[a * a + b * b - c * c - d * d, 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)],
                      [2.0 * (b * c + a * d), a * a + c * c - b * b - d * d, 2.0 * (c * d - a * b)],
                      [2.0 * (b * d - a * c), 2.0 * (c * d + a * b), a * a + d * d - b * b - c * c]])
        qfac = -1.0 if pix[0] == -1.0 else 1.0
        w[:3, :3] = r * np.array([pix[1], pix[2], pix[3] * qfac])
        w[:3, 3] = [float(g["qoffset_x"]), float(g["qoffset_y"]), float(g["qoffset_z"])]
        return w + 0.0
    w[0, 0], w[1, 1], w[2, 2] = pix[1], pix[2], pix[3]
    return w


RIGID_NAMES = ("tz", "ty", "tx", "rz", "ry", "rx")  # millimetres, then degrees


def rigid_world(params, centre_xyz) -> np.ndarray:
    """The (4, 4) rigid motion of six parameters ``(tz, ty, tx mm; rz, ry, rx degrees)`` in world
    millimetres about the world point ``centre_xyz``: ``x -> R (x - c) + c + (tx, ty, tz)`` with
    ``R = R_z(rz) . R_y(ry) . R_x(rx)``, each a right-handed rotation about that world axis."""
    tz, ty, tx, rz, ry, rx = (float(v) for v in params)
    az, ay, ax = (float(np.deg2rad(v)) for v in (rz, ry, rx))
    c, s = np.cos, np.sin
    mz = np.array([[c(az), -s(az), 0.0], [s(az), c(az), 0.0], [0.0, 0.0, 1.0]])
    my = np.array([[c(ay), 0.0, s(ay)], [0.0, 1.0, 0.0], [-s(ay), 0.0, c(ay)]])
    mx = np.array([[1.0, 0.0, 0.0], [0.0, c(ax), -s(ax)], [0.0, s(ax), c(ax)]])
    r = _matmul3(_matmul3(mz, my), mx)
    cen = np.asarray(centre_xyz, dtype=np.float64).reshape(3)
    rc = np.array([(r[i, 0] * cen[0] + r[i, 1] * cen[1]) + r[i, 2] * cen[2] for i in range(3)])
    m = np.eye(4)
    m[:3, :3] = r
    m[:3, 3] = (cen - rc) + np.array([tx, ty, tz])
    return m + 0.0


def world_centre(geometry: dict, shape_zyx) -> np.ndarray:
    """The world position (x, y, z mm) of the centre ``(n - 1) / 2`` of a (z, y, x) grid."""
    w = world_matrix(geometry)
    i = np.array([(float(n) - 1.0) / 2.0 for n in tuple(shape_zyx)[::-1]])
    return np.array([((w[a, 0] * i[0] + w[a, 1] * i[1]) + w[a, 2] * i[2]) + w[a, 3] for a in range(3)])


def rigid_correction(params, ref_geometry: dict, ref_shape) -> np.ndarray:
    """``rigid_world`` of ``params`` about the centre of the reference grid: the ``correction``
    ``align_affine`` takes for a ``align.register_rigid`` result."""
    return rigid_world(params, world_centre(ref_geometry, ref_shape))


def align_affine(ref_geometry: dict, mov_geometry: dict, correction=None) -> Tuple[np.ndarray, np.ndarray]:
    """``(A, t)`` in array order (z, y, x) that takes an array index of the reference file to the
    array index of the same world point in the moving file: ``P . inv(W_mov) . [T] . W_ref . P``
    with ``W`` the ``world_matrix`` of each file, ``P`` the x<->z swap and ``T`` an optional (4, 4)
    rigid ``correction`` in world millimetres (``rigid_correction``: reference world -> moving
    world).  A singular ``W_mov`` raises ValueError.  Without a correction and with two world
    matrices equal element for element the result is exactly ``(I, 0)``.  A reference voxel whose
    image lies outside the moving grid reads 0 in every resampler (the outside rule of
    ``resample_affine``)."""
    w_ref, w_mov = world_matrix(ref_geometry), world_matrix(mov_geometry)
    inv = _affine_inverse4(w_mov, "align_affine")
    if correction is None and np.array_equal(w_ref, w_mov):
        return np.eye(3), np.zeros(3)
    m = w_ref
    if correction is not None:
        T = np.asarray(correction, dtype=np.float64)
        if T.shape != (4, 4) or not np.isfinite(T).all():
            raise ValueError(f"correction is a finite (4, 4) matrix, got {correction!r}")
        m = _matmul4(T, m)
    m = _matmul4(inv, m)
    return m[:3, :3][::-1, ::-1] + 0.0, m[:3, 3][::-1] + 0.0


def compose_affine(first, second) -> Tuple[np.ndarray, np.ndarray]:
    """``(A, t)`` of ``x -> second(first(x))`` for two ``(A, t)`` pairs, in fp64 with every product
    and sum written out: ``A = A2 . A1``, ``t = A2 . t1 + t2``.  An identity ``second`` gives
    ``first`` back exactly."""
    A1, t1 = np.asarray(first[0], dtype=np.float64).reshape(3, 3), np.asarray(first[1], dtype=np.float64).reshape(3)
    A2, t2 = np.asarray(second[0], dtype=np.float64).reshape(3, 3), np.asarray(second[1], dtype=np.float64).reshape(3)
    A = _matmul3(A2, A1)
    t = np.array([((A2[i, 0] * t1[0] + A2[i, 1] * t1[1]) + A2[i, 2] * t1[2]) + t2[i] for i in range(3)])
    return A + 0.0, t + 0.0


def case_affine(L, shift, n_in, n_out, alignment=None) -> Tuple[np.ndarray, np.ndarray]:
    """One volume's ``(A, t)`` from the case grid ``n_out`` into the volume's own array: the one
    function every loader, host or device, forms it with.  Without ``alignment`` it is
    ``volume_affine(L, shift, n_in, n_out)``: the file stretched onto the grid.  ``alignment`` is
    ``(ref_shape, (A, t))``: the case grid is scaled onto the reference file's native grid
    (``volume_affine`` with the reference's shape) and that is composed with the ``align_affine``
    pair into this volume; ``n_in`` then plays no part."""
    if alignment is None:
        return volume_affine(L, shift, n_in, n_out)
    ref_shape, pair = alignment
    return compose_affine(volume_affine(L, shift, tuple(int(v) for v in ref_shape), n_out), pair)


def affine12_of(A, t) -> Tuple[float, ...]:
    """``(A, t)`` as the twelve doubles the C entry points take: row-major A, then t."""
    return tuple(float(v) for v in np.asarray(A).reshape(-1)) + tuple(float(v) for v in np.asarray(t).reshape(-1))


def registration_fixed(modalities: Sequence[str], present, to: Optional[str]) -> str:
    """The modality the others of a case are registered to, and about whose centre their rigid
    corrections turn: ``to`` when it names a present modality, else the first present one in
    ``modalities`` order (a label or any other file only lends its grid)."""
    if to in modalities and to in present:
        return to
    return next(m for m in modalities if m in present)
