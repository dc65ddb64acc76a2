"""Modality alignment, the host forms (no GPU): ``data.world_matrix`` / ``align_affine``
/ ``compose_affine`` / ``case_affine``, ``predict.joint_histogram`` (against a triple Python loop) /
``normalised_mutual_information`` / ``register_rigid``, and their way through ``prepare_case`` and
the host loaders.  The fixtures are written with ``write_nifti(..., geometry=...)``."""
import functools
import json
import os

import numpy as np
import pytest
import torch

MODS = ["ADC", "DWI", "gaoqing-T2", "T2 fs", "T2 not fs"]
REF_SHAPE = (12, 40, 48)            # the T2 series and the label, (z, y, x)
OFFSET = (2, 6, 10)                 # the diffusion series: every second T2 voxel from this index on
COARSE_SHAPE = (5, 16, 18)          # ... so that its last voxel, OFFSET + 2 (n - 1), is inside the T2 grid
TRUE_MOTION = (1.5, -2.0, 1.0, 3.0, 0.0, 0.0)   # tz, ty, tx mm; rz, ry, rx degrees: on the step lattice


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


def _predict():
    import pcms_amd  # noqa: F401
    from pcms_amd import predict
    return predict


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sform_geometry(w):
    """A ``read_nifti_geometry`` dict whose sform is the (4, 4) world matrix ``w``, as a header
    holds it: in float32."""
    w = np.asarray(w, np.float32).astype(np.float64)
    pix = np.sqrt((w[:3, :3] ** 2).sum(axis=0))
    return {"pixdim": (1.0,) + tuple(float(v) for v in pix), "xyzt_units": 2, "qform_code": 0, "sform_code": 1,
            "quatern_b": 0.0, "quatern_c": 0.0, "quatern_d": 0.0, "qoffset_x": 0.0, "qoffset_y": 0.0,
            "qoffset_z": 0.0, "srow_x": tuple(w[0]), "srow_y": tuple(w[1]), "srow_z": tuple(w[2])}


def scaled_world(spacing_zyx, origin_xyz):
    w = np.eye(4)
    w[0, 0], w[1, 1], w[2, 2] = spacing_zyx[::-1]
    w[:3, 3] = origin_xyz
    return w


# spacings and origins are dyadic, so that the analytic maps below are exact in fp64
REF_WORLD = scaled_world((2.0, 0.5, 0.5), (-12.0, -10.0, 4.0))
# voxel j of the coarse grid is voxel OFFSET + 2 j of the reference grid: twice the spacing
COARSE_WORLD = scaled_world((4.0, 1.0, 1.0), tuple(REF_WORLD[:3, 3] + np.array(OFFSET[::-1]) * (0.5, 0.5, 2.0)))
COARSE_A, COARSE_T = np.diag([0.5, 0.5, 0.5]), -np.array(OFFSET, np.float64) / 2.0


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


# ---------------- world_matrix ----------------
def test_world_matrix_sform_wins():
    d = _data()
    w = np.eye(4)
    w[:3, :3] = rot(0, 10.0) @ np.diag([0.5, 0.5, 3.0])
    w[:3, 3] = (-11.0, 7.5, 3.25)
    geo = sform_geometry(w)
    geo.update(qform_code=1, quatern_b=0.5, qoffset_x=99.0)    # a qform that disagrees: the sform has precedence
    got = d.world_matrix(geo)
    assert got.dtype == np.float64 and got.shape == (4, 4)
    assert np.array_equal(got[:3], np.float32(w[:3]).astype(np.float64)) and np.array_equal(got[3], [0, 0, 0, 1])


@pytest.mark.parametrize("qfac", [1.0, -1.0, 0.0])
def test_world_matrix_qform_is_the_rotation_it_was_built_from(qfac):
    d = _data()
    axis, angle = np.array([1.0, 2.0, -2.0]) / 3.0, np.deg2rad(35.0)
    b, c, q = np.sin(angle / 2) * axis
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)     # Rodrigues
    geo = sform_geometry(np.eye(4))
    geo.update(sform_code=0, qform_code=1, quatern_b=float(b), quatern_c=float(c), quatern_d=float(q),
               qoffset_x=-5.0, qoffset_y=6.5, qoffset_z=7.25, pixdim=(qfac, 0.5, 0.75, 3.0))
    exp = np.eye(4)
    exp[:3, :3] = r * np.array([0.5, 0.75, 3.0 * (-1.0 if qfac == -1.0 else 1.0)])
    exp[:3, 3] = (-5.0, 6.5, 7.25)
    assert np.allclose(d.world_matrix(geo), exp, rtol=0, atol=1e-6)       # the header fields are float32


def test_world_matrix_falls_back_to_pixdim(tmp_path):
    d = _data()
    p = str(tmp_path / "plain.nii")
    d.write_nifti(p, np.zeros((3, 4, 5), np.int16), spacing=(0.5, 0.75, 3.0))   # (x, y, z) as the header holds it
    assert np.array_equal(d.world_matrix(d.read_nifti_geometry(p)), np.diag([0.5, 0.75, 3.0, 1.0]))


# ---------------- align_affine ----------------
def test_align_affine_is_exactly_the_identity_for_equal_geometries():
    d = _data()
    w = np.eye(4)
    w[:3, :3] = rot(1, 7.0) @ np.diag([0.6, 0.6, 3.3])
    w[:3, 3] = (1.1, -2.2, 3.3)
    A, t = d.align_affine(sform_geometry(w), sform_geometry(w))
    assert np.array_equal(A, np.eye(3)) and np.array_equal(t, np.zeros(3))
    assert not np.signbit(A).any() and not np.signbit(t).any()


def test_align_affine_of_a_coarser_integer_offset_crop():
    d = _data()
    A, t = d.align_affine(sform_geometry(REF_WORLD), sform_geometry(COARSE_WORLD))
    assert np.array_equal(A, COARSE_A) and np.array_equal(t, COARSE_T)
    B, u = d.align_affine(sform_geometry(COARSE_WORLD), sform_geometry(REF_WORLD))    # and back
    assert np.array_equal(B, np.diag([2.0, 2.0, 2.0])) and np.array_equal(u, np.array(OFFSET, np.float64))


def _direct(w_ref, w_mov, index_zyx, T=None):
    """The moving array index of a reference array index through world coordinates."""
    x = np.float32(w_ref).astype(np.float64) @ np.array(tuple(index_zyx[::-1]) + (1.0,))
    if T is not None:
        x = T @ x
    return np.linalg.solve(np.float32(w_mov).astype(np.float64), x)[:3][::-1]


def test_align_affine_oblique_and_flipped():
    d = _data()
    oblique = np.eye(4)
    oblique[:3, :3] = rot(0, 10.0) @ np.diag([1.25, 1.25, 3.6])
    oblique[:3, 3] = (-20.0, -31.0, 2.0)
    flipped = scaled_world((2.0, 0.5, 0.5), (12.0, -10.0, 4.0))
    flipped[0, 0] = -0.5                                               # x runs right to left
    rng = np.random.default_rng(3)
    for w_mov in (oblique, flipped):
        A, t = d.align_affine(sform_geometry(REF_WORLD), sform_geometry(w_mov))
        for idx in rng.uniform(0, 40, size=(8, 3)):
            assert np.allclose(A @ idx + t, _direct(REF_WORLD, w_mov, idx), rtol=0, atol=1e-9)
    A, _ = d.align_affine(sform_geometry(REF_WORLD), sform_geometry(flipped))
    assert A[2, 2] == -1.0 and A[0, 0] == 1.0
    T = d.rigid_world((1.0, -2.0, 3.0, 4.0, -5.0, 6.0), (3.0, 2.0, 1.0))
    A, t = d.align_affine(sform_geometry(REF_WORLD), sform_geometry(oblique), T)
    for idx in rng.uniform(0, 40, size=(8, 3)):
        assert np.allclose(A @ idx + t, _direct(REF_WORLD, oblique, idx, T), rtol=0, atol=1e-9)


def test_align_affine_rejects_a_singular_moving_geometry():
    d = _data()
    w = REF_WORLD.copy()
    w[:3, 1] = w[:3, 0]
    with pytest.raises(ValueError):
        d.align_affine(sform_geometry(REF_WORLD), sform_geometry(w))
    with pytest.raises(ValueError):
        d.align_affine(sform_geometry(REF_WORLD), sform_geometry(REF_WORLD), np.eye(3))


def test_rigid_world_is_a_rotation_about_the_centre():
    d = _data()
    c = np.array([5.0, -3.0, 2.0])
    T = d.rigid_world((1.5, -2.0, 1.0, 3.0, 0.0, 0.0), c)                # tz ty tx; rz ry rx
    assert np.allclose(T[:3, :3], rot(2, 3.0), atol=1e-15) and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3))
    assert np.allclose(T @ np.append(c, 1.0), np.append(c + (1.0, -2.0, 1.5), 1.0))
    assert np.array_equal(d.rigid_world((0.0,) * 6, c), np.eye(4))


def test_compose_and_case_affine():
    d = _data()
    first = d.volume_affine(d.compose_transform((True, False, False), (3.0, 0.0, -4.0), 1.1), (0.5, 0.0, -1.0),
                            REF_SHAPE, (16, 32, 32))
    A, t = d.compose_affine(first, (np.eye(3), np.zeros(3)))
    assert np.array_equal(A, first[0]) and np.array_equal(t, first[1])
    A, t = d.compose_affine(first, (COARSE_A, COARSE_T))
    p = np.array([3.0, 5.0, 7.0])
    assert np.allclose(A @ p + t, COARSE_A @ (first[0] @ p + first[1]) + COARSE_T, rtol=0, atol=1e-12)
    B, u = d.case_affine(np.eye(3), np.zeros(3), COARSE_SHAPE, (16, 32, 32), (REF_SHAPE, (COARSE_A, COARSE_T)))
    S = np.array(REF_SHAPE) / np.array((16, 32, 32))
    assert np.array_equal(B, np.diag(0.5 * S)) and np.array_equal(u, COARSE_T)
    plain = d.case_affine(np.eye(3), np.zeros(3), COARSE_SHAPE, (16, 32, 32))
    assert np.array_equal(plain[0], d.volume_affine(np.eye(3), np.zeros(3), COARSE_SHAPE, (16, 32, 32))[0])


# ---------------- joint_histogram / NMI ----------------
FIX_SHAPE, MOV_SHAPE = (5, 7, 9), (6, 5, 11)


@functools.lru_cache(maxsize=None)
def _pair():
    rng = np.random.default_rng(21)
    return ((1000.0 * rng.standard_normal(FIX_SHAPE)).astype(np.float32),
            rng.integers(-500, 3000, size=MOV_SHAPE).astype(np.int16))


def loop_histogram(fix, mov, A, t, flohi, mlohi, bins, stride):
    """``joint_histogram`` one voxel at a time, in Python floats (fp64) and np.float32 scalars."""
    p = _predict()
    f = p.normalise_window(fix, flohi)
    m = p.normalise_window(mov, mlohi).astype(np.float64)
    n = mov.shape
    hist = np.zeros((bins, bins), np.int64)

    def bin_of(v):
        return min(int(np.float32(v) * np.float32(bins)), bins - 1)

    for qd in range(0, fix.shape[0], stride[0]):
        for qh in range(0, fix.shape[1], stride[1]):
            for qw in range(0, fix.shape[2], stride[2]):
                c = [((A[a][0] * qd + A[a][1] * qh) + A[a][2] * qw) + t[a] for a in range(3)]
                if not all(-0.5 <= c[a] < n[a] - 0.5 for a in range(3)):
                    continue
                i0 = [int(np.floor(v)) for v in c]
                w = [c[a] - i0[a] for a in range(3)]
                lo = [min(max(i0[a], 0), n[a] - 1) for a in range(3)]
                hi = [min(max(i0[a] + 1, 0), n[a] - 1) for a in range(3)]
                vh = []
                for xw in (lo[2], hi[2]):
                    vd = [m[lo[0], xh, xw] * (1.0 - w[0]) + m[hi[0], xh, xw] * w[0] for xh in (lo[1], hi[1])]
                    vh.append(vd[0] * (1.0 - w[1]) + vd[1] * w[1])
                mv = np.float32(vh[0] * (1.0 - w[2]) + vh[1] * w[2])
                fv = f[qd, qh, qw]
                if np.isnan(fv) or np.isnan(mv):
                    continue
                hist[bin_of(fv), bin_of(mv)] += 1
    return hist


def oblique_affine(shift=(0.3, -0.8, 1.7)):
    d = _data()
    return d.volume_affine(d.compose_transform((False, True, False), (8.0, -5.0, 12.0), 0.9), np.array(shift),
                           MOV_SHAPE, FIX_SHAPE)


@pytest.mark.parametrize("stride", [(1, 1, 1), (1, 2, 2), (2, 3, 1)])
@pytest.mark.parametrize("bins", [2, 8, 32])
def test_joint_histogram_equals_the_triple_loop(bins, stride):
    p = _predict()
    fix, mov = _pair()
    flohi, mlohi = p.intensity_window(fix, 5.0, 95.0), np.float32([mov.min(), mov.max()])
    lattice = int(np.prod([-(-n // s) for n, s in zip(FIX_SHAPE, stride)]))
    for name, (A, t) in {"scaled": (np.diag([1.2, 5 / 7, 11 / 9]), np.zeros(3)), "oblique": oblique_affine(),
                         "far": (np.eye(3), np.array([50.0, 0.0, 0.0]))}.items():
        got = p.joint_histogram(fix, mov, A, t, flohi, mlohi, bins, stride)
        exp = loop_histogram(fix, mov, A, t, flohi, mlohi, bins, stride)
        assert got.dtype == np.int64 and got.shape == (bins, bins)
        assert np.array_equal(got, exp), name
        total = int(got.sum())
        assert {"scaled": total == lattice, "oblique": 0 < total < lattice, "far": total == 0}[name], (name, total)


def test_joint_histogram_edges():
    p = _predict()
    fix, mov = _pair()
    A, t = np.diag([1.2, 5 / 7, 11 / 9]), np.zeros(3)
    full = np.float32([mov.min(), mov.max()])
    sevens = np.full(FIX_SHAPE, 7.0, np.float32)
    h = p.joint_histogram(sevens, np.full(MOV_SHAPE, -2, np.int16), A, t, (7, 7), (-2, -2), 8)
    assert h[0, 0] == 5 * 7 * 9 and h.sum() == 5 * 7 * 9                     # den == 0: everything is 0
    h = p.joint_histogram(sevens, np.full(MOV_SHAPE, 3, np.int16), A, t, (0, 7), (0, 3), 8)
    assert h[7, 7] == 5 * 7 * 9                                               # exactly 1.0: the last bin
    nan = fix.copy()
    nan[1, 2, 3] = np.nan
    a = p.joint_histogram(nan, mov, A, t, (-1000, 1000), full, 8)
    b = p.joint_histogram(fix, mov, A, t, (-1000, 1000), full, 8)
    assert a.sum() == b.sum() - 1
    for bad in (dict(bins=1), dict(bins=65), dict(stride=(0, 1, 1)), dict(stride=(1, 1))):
        with pytest.raises(ValueError):
            p.joint_histogram(fix, mov, A, t, (0, 1), (0, 1), **bad)


def test_normalised_mutual_information_of_hand_tables():
    p = _predict()
    nmi = p.normalised_mutual_information
    assert nmi(np.zeros((2, 2), np.int64)) == 0.0
    assert nmi([[5, 0], [0, 0]]) == 0.0                                      # one cell: H(X, Y) = 0
    assert nmi([[3, 0], [0, 3]]) == pytest.approx(2.0, abs=1e-15)            # one to one
    assert nmi([[1, 1], [1, 1]]) == pytest.approx(1.0, abs=1e-15)            # independent
    # p = [[1/2, 1/4], [0, 1/4]]: H(X) = H(3/4, 1/4), H(Y) = ln 2, H(X, Y) = 3/2 ln 2
    hx = -(0.75 * np.log(0.75) + 0.25 * np.log(0.25))
    assert nmi([[2, 1], [0, 1]]) == pytest.approx((hx + np.log(2.0)) / (1.5 * np.log(2.0)), abs=1e-15)


def test_alignment_of():
    p = _predict()
    assert p.Alignment.of(None) is None
    a = p.Alignment.of("register")
    assert a.mode == "register" and a.bins == 32
    assert a.levels == (((1, 2, 2), (4.0, 2.0, 1.0)), ((1, 1, 1), (0.5, 0.25)))
    assert p.Alignment.of(a) is a and p.Alignment.of({"mode": "world", "to": "T2 fs"}).to == "T2 fs"
    for bad in ("nearest", 3, {"bins": 1}, {"levels": ()}, {"levels": (((1, 1, 0), (1.0,)),)}, {"min_overlap": 2.0}):
        with pytest.raises((ValueError, TypeError)):
            p.Alignment.of(bad)


# ---------------- the registration phantom ----------------
FIX_GRID, FIX_SPACING = (20, 48, 48), (3.0, 1.0, 1.0)
MOV_GRID, MOV_SPACING = (16, 40, 40), (3.6, 1.25, 1.25)


@functools.lru_cache(maxsize=None)
def phantom():
    """(fixed, moving, fixed geometry, moving geometry): sums of Gaussians defined in world
    millimetres; the moving image has another contrast, (1 - v)^2, another grid and the true
    motion TRUE_MOTION about the fixed volume's centre."""
    d = _data()
    w_fix = scaled_world(FIX_SPACING, (-24.0, -24.0, -30.0))
    w_mov = scaled_world(MOV_SPACING, (-25.5, -24.5, -28.0))
    gf, gm = sform_geometry(w_fix), sform_geometry(w_mov)
    rng = np.random.default_rng(5)
    centres = rng.uniform((-16, -16, -20), (16, 16, 20), size=(7, 3))
    sigmas = rng.uniform(4.0, 9.0, size=7)
    amps = rng.uniform(0.4, 1.0, size=7)

    def value(xyz):
        v = sum(a * np.exp(-((xyz - c) ** 2).sum(axis=-1) / (2.0 * s * s)) for a, c, s in zip(amps, centres, sigmas))
        return np.clip(v, 0.0, 1.0)

    def world_points(w, shape):
        z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
        return np.stack([x, y, z, np.ones_like(x)], axis=-1) @ w.T

    T = d.rigid_world(TRUE_MOTION, d.world_centre(gf, FIX_GRID))
    fixed = value(world_points(w_fix, FIX_GRID)[..., :3])
    back = world_points(w_mov, MOV_GRID) @ np.linalg.inv(T).T              # fixed-world point shown by a moving voxel
    moving = (1.0 - value(back[..., :3])) ** 2
    return fixed.astype(np.float32), moving.astype(np.float32), gf, gm


@functools.lru_cache(maxsize=None)
def phantom_result():
    fixed, moving, gf, gm = phantom()
    return _predict().register_rigid(fixed, moving, gf, gm)


def test_register_rigid_recovers_the_phantom_motion():
    res = phantom_result()
    print("register_rigid:", res)
    got, true = np.array(res["params"]), np.array(TRUE_MOTION)
    assert (np.abs(got[:3] - true[:3]) <= 0.5).all(), res
    assert (np.abs(got[3:] - true[3:]) <= 0.5).all(), res
    assert res["after"] > res["before"] > 0.0, res
    assert 0 < res["evaluations"] < 1000
    again = _predict().register_rigid(*phantom())
    assert again == res                                                       # deterministic


def test_register_rigid_respects_its_limits():
    fixed, moving, gf, gm = phantom()
    res = _predict().register_rigid(fixed, moving, gf, gm, settings={"max_translation_mm": 1.0, "max_rotation_deg": 0.0,
                                                                      "levels": (((1, 2, 2), (1.0,)),)})
    assert all(abs(v) <= 1.0 for v in res["params"][:3]) and res["params"][3:] == (0.0, 0.0, 0.0)
    far = sform_geometry(scaled_world(MOV_SPACING, (500.0, -24.5, -28.0)))     # no pose within the limits overlaps
    none = _predict().register_rigid(fixed, moving, gf, far)
    assert none["params"] == (0.0,) * 6 and none["before"] == none["after"] == 0.0


# ---------------- prepare_case ----------------
def coarse_case(root):
    """A case directory: the three T2 series on the reference grid (int16, float32, uint8), DWI and
    ADC as coarser crops of it (COARSE_WORLD)."""
    d = _data()
    rng = np.random.default_rng(17)
    vols = {"ADC": rng.integers(0, 3000, size=COARSE_SHAPE).astype(np.int16),
            "DWI": (300.0 * rng.standard_normal(COARSE_SHAPE)).astype(np.float32),
            "gaoqing-T2": rng.integers(-200, 3000, size=REF_SHAPE).astype(np.int16),
            "T2 fs": (500.0 * rng.standard_normal(REF_SHAPE)).astype(np.float32),
            "T2 not fs": rng.integers(0, 256, size=REF_SHAPE).astype(np.uint8)}
    for m, v in vols.items():
        os.makedirs(os.path.join(root, m))
        geo = sform_geometry(COARSE_WORLD if v.shape == COARSE_SHAPE else REF_WORLD)
        d.write_nifti(os.path.join(root, m, "img.nii"), v, geometry=geo)
    return root, vols


@pytest.mark.parametrize("normalise", [True, "percentile", False])
def test_prepare_case_world_equals_the_analytic_map(tmp_path, normalise):
    d, p = _data(), _predict()
    root, vols = coarse_case(str(tmp_path / "case"))
    norm = p.Normalisation.of(normalise)
    with pytest.raises(ValueError):
        p.prepare_case(root, None, normalise=normalise)                        # shapes differ
    for target in (None, (16, 32, 32)):
        grid = REF_SHAPE if target is None else target
        got, report = p.prepare_case(root, target, normalise=normalise, align={"to": "gaoqing-T2"},
                                     return_alignment=True)
        plain = None if target is None else p.prepare_case(root, target, normalise=normalise)
        assert got.shape == (5,) + grid and got.dtype == np.float32
        S = np.array(REF_SHAPE, np.float64) / np.array(grid, np.float64)
        for c, m in enumerate(MODS):
            vol = norm.apply(vols[m]) if norm is not None else vols[m].astype(np.float32)
            coarse = vols[m].shape == COARSE_SHAPE
            A, t = (np.diag(0.5 * S), COARSE_T) if coarse else (np.diag(S), np.zeros(3))
            exp = d.resample_affine(vol, grid, A, t)
            assert np.array_equal(bits(got[c]), bits(exp)), (m, target)
            if coarse:
                assert not exp[0].any() and exp[4].any()                      # outside the field of view: 0
                assert plain is None or not np.array_equal(got[c], plain[c])
            elif plain is not None:
                assert np.array_equal(bits(got[c]), bits(plain[c]))            # same geometry: today's channel
        assert set(report) == set(MODS) and report["DWI"] == {"params": (0.0,) * 6, "before": None, "after": None}
    assert p.prepare_case(root, (16, 32, 32), normalise=normalise, return_alignment=True)[1] is None


# ---------------- the loaders ----------------
def make_tree(root, same_geometry, cases=2):
    """A training tree.  ``same_geometry``: every file on the label's grid with the label's
    geometry; else ADC and DWI are coarser crops (COARSE_WORLD) and the rest lie on the label's
    grid."""
    d = _data()
    rng = np.random.default_rng(29)
    lab_dir = os.path.join(root, "BPH-PCA", "ROI(BPH+PCA)", "BPH")
    os.makedirs(lab_dir)
    dtypes = {"ADC": np.int16, "DWI": np.float32, "gaoqing-T2": np.int16, "T2 fs": np.uint8, "T2 not fs": np.float32}
    for m in MODS:
        os.makedirs(os.path.join(root, "BPH-PCA", "BPH", m))
    for ci in range(cases):
        for m in MODS:
            coarse = m in ("ADC", "DWI") and not same_geometry
            v = rng.integers(0, 250, size=COARSE_SHAPE if coarse else REF_SHAPE).astype(dtypes[m])
            d.write_nifti(os.path.join(root, "BPH-PCA", "BPH", m, f"p{ci}.nii"), v,
                          geometry=sform_geometry(COARSE_WORLD if coarse else REF_WORLD))
        lab = np.zeros(REF_SHAPE, np.uint8)
        lab[4:8, 16 + ci:24 + ci, 20:28] = 1
        d.write_nifti(os.path.join(lab_dir, f"p{ci}.nii"), lab, geometry=sform_geometry(REF_WORLD))
    return root


AUG = dict(flip_prob=(0.5, 0.5, 0.5), rotate_deg=(10.0, 5.0, 5.0), zoom=(0.9, 1.1), shift_frac=(0.1, 0.1, 0.1),
           gain=(0.9, 1.1), bias=(-5.0, 5.0))
PATCHES = dict(patch_size=(16, 16, 16), patches_per_case=3, foreground_prob=0.7, normalise=True, seed=4)
KINDS = {"plain": {}, "augment": dict(augment=AUG, augment_seed=3), "patches": dict(patches=PATCHES),
         "patches_augment": dict(patches=PATCHES, augment=AUG, augment_seed=3)}
CORRECTIONS = {"p0": {"DWI": [1.0, -0.5, 0.25, 2.0, 0.0, -1.0], "ADC": [0.0, 0.5, 0.0, 0.0, 1.0, 0.0]},
               "p1": {"T2 fs": [0.5, 0.0, 0.0, 0.0, 0.0, 3.0]}}


@pytest.fixture(scope="module")
def same_tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp("align_same")), True)


@pytest.fixture(scope="module")
def coarse_tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp("align_coarse")), False)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_same_geometry_samples_are_bit_identical(same_tree, kind):
    d = _data()
    plain = d.ProstateDataset(same_tree, target_size=(16, 32, 32), **KINDS[kind])
    aligned = d.ProstateDataset(same_tree, target_size=(16, 32, 32), align="world", **KINDS[kind])
    assert len(plain) == len(aligned) == 2
    for i in range(2):
        a, b = plain[i], aligned[i]
        for key in ("image", "label"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (kind, i, key)
        assert a["image"].abs().sum() > 0 and a["label"].sum() > 0


def test_dataset_world_alignment_places_the_coarse_series(coarse_tree):
    d = _data()
    target = (16, 32, 32)
    ds = d.ProstateDataset(coarse_tree, target_size=target, align="world")
    plain = d.ProstateDataset(coarse_tree, target_size=target)
    S = np.array(REF_SHAPE, np.float64) / np.array(target, np.float64)
    for i in range(2):
        s = ds[i]
        files = ds.case_list[i]["modality_files"]
        for c, m in enumerate(MODS):
            vol = d.read_nifti(files[m]).astype(np.float32)
            A, t = (np.diag(0.5 * S), COARSE_T) if m in ("ADC", "DWI") else (np.diag(S), np.zeros(3))
            assert np.array_equal(bits(s["image"][c].numpy()), bits(d.resample_affine(vol, target, A, t))), m
        assert torch.equal(s["label"], plain[i]["label"])                      # the label is the reference
        assert not torch.equal(s["image"][0], plain[i]["image"][0])
        assert torch.equal(s["image"][2:], plain[i]["image"][2:])


def test_dataset_corrections(coarse_tree, tmp_path):
    d = _data()
    target = (16, 32, 32)
    with pytest.raises(ValueError):
        d.ProstateDataset(coarse_tree, corrections=CORRECTIONS)                 # corrections need align
    with pytest.raises(ValueError):
        d.ProstateDataset(coarse_tree, align="register")                        # no registration on the fly
    path = str(tmp_path / "corrections.json")
    with open(path, "w") as f:
        json.dump(CORRECTIONS, f)
    world = d.ProstateDataset(coarse_tree, target_size=target, align="world")
    for corr in (CORRECTIONS, path):
        ds = d.ProstateDataset(coarse_tree, target_size=target, align="register", corrections=corr)
        s, w = ds[0], world[0]
        assert torch.equal(s["image"][2:], w["image"][2:]) and torch.equal(s["label"], w["label"])
        assert not torch.equal(s["image"][1], w["image"][1])
        files = ds.case_list[0]["modality_files"]
        geo = {m: d.read_nifti_geometry(files[m]) for m in MODS}
        T = d.rigid_correction(CORRECTIONS["p0"]["DWI"], geo["ADC"], COARSE_SHAPE)   # ADC: the first present modality
        A, t = d.case_affine(np.eye(3), np.zeros(3), COARSE_SHAPE, target,
                             (REF_SHAPE, d.align_affine(d.read_nifti_geometry(ds.case_list[0]["label_path"]),
                                                        geo["DWI"], T)))
        exp = d.resample_affine(d.read_nifti(files["DWI"]).astype(np.float32), target, A, t)
        assert np.array_equal(bits(s["image"][1].numpy()), bits(exp))
        assert torch.equal(s["image"][0], w["image"][0])    # the fixed modality carries no correction of its own
