"""Elastic deformation, host side (no GPU): ``data.resample_deform`` (the numpy restatement the
device kernels are compared with, and what the default loader runs when ``elastic_grid`` is on),
the field's draws in ``data.draw_transform``, the ``Augment`` settings and the loader plumbing.

The restatement is pinned independently of ``data.py``: with a zero field it is
``resample_affine`` bit for bit; a uniform cubic B-spline reproduces linear functions (which
fixes the knot placement) and constants (partition of unity); and on a linear ramp volume the
result is the ramp at the coordinate that this file computes from the formulas alone."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests.test_augment import AUG, GENERAL_SHAPES, SHAPES, TRANSFORMS, _bits, affine_of
from tests.test_device_loader import TARGET, tree  # noqa: F401  (the synthetic tree fixture)

GRIDS = [(4, 4, 4), (5, 4, 7), (8, 8, 8)]
ELASTIC = dict(AUG, elastic_grid=(5, 5, 5), elastic_disp=(2.0, 2.0, 2.0))
# the fields of the bit-equality tests here and on the GPU: control displacements uniform in
# [-DISP, DISP] output voxels (within the 1.5-3 the coverage conditions are set for)
DISP = 3.0
FIELD_SEED = 16


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


@functools.lru_cache(maxsize=None)
def random_field(grid, seed=FIELD_SEED, disp=DISP):
    f = disp * (2.0 * np.random.default_rng([seed, *grid]).random(tuple(grid) + (3,)) - 1.0)
    f.setflags(write=False)
    return f


def nan_field():
    """random_field((8, 8, 8)) with one NaN control vector, at (3, 3, 3)."""
    f = np.array(random_field((8, 8, 8)))
    f[3, 3, 3, :] = np.nan
    return f


# ---- the issue's formulas, written out per axis (nothing here is taken from data.py) ----
def basis(n, g):
    k, b = [], []
    for i in range(n):
        x = float(i) * (float(g - 3) / float(n))
        f = np.floor(x)
        s = x - f
        r, s2 = 1.0 - s, s * s
        s3 = s2 * s
        k.append(int(f))
        b.append([((r * r) * r) / 6.0, ((3.0 * s3 - 6.0 * s2) + 4.0) / 6.0,
                  ((((-3.0 * s3) + 3.0 * s2) + 3.0 * s) + 1.0) / 6.0, s3 / 6.0])
    return np.array(k), np.array(b)


def displacement(field, target):
    """u_c over the output grid: a dense tensor-product evaluation (up to fp64 rounding)."""
    (kd, bd), (kh, bh), (kw, bw) = (basis(n, g) for n, g in zip(target, field.shape[:3]))
    j = np.arange(4)
    P = field[(kd[:, None] + j)[:, None, None, :, None, None], (kh[:, None] + j)[None, :, None, None, :, None],
              (kw[:, None] + j)[None, None, :, None, None, :]]          # (D, H, W, 4, 4, 4, 3)
    return np.einsum("dhwabcx,da,hb,wc->xdhw", P, bd, bh, bw)


def coords(A, t, target, field):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in target], indexing="ij")
    if field is not None:
        u = displacement(field, target)
        g = [g[a] + u[a] for a in range(3)]
    return [((A[a, 0] * g[0] + A[a, 1] * g[1]) + A[a, 2] * g[2]) + t[a] for a in range(3)]


def coverage(A, t, shape, target, field):
    """(inside share, inside voxels below 0, inside voxels above n - 1, share of the inside voxels
    whose 8-corner cell differs from the affine's alone), on the host form's own coordinates."""
    d = _data()
    u = d.field_displacement(field, target)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in target], indexing="ij")
    p = [g[a] + u[a] for a in range(3)]
    c = [((A[a, 0] * p[0] + A[a, 1] * p[1]) + A[a, 2] * p[2]) + t[a] for a in range(3)]
    c0 = [((A[a, 0] * g[0] + A[a, 1] * g[1]) + A[a, 2] * g[2]) + t[a] for a in range(3)]
    inside = np.ones(target, dtype=bool)
    for a in range(3):
        inside &= (c[a] >= -0.5) & (c[a] < shape[a] - 0.5)
    low = inside & ((c[0] < 0) | (c[1] < 0) | (c[2] < 0))
    high = inside & ((c[0] > shape[0] - 1) | (c[1] > shape[1] - 1) | (c[2] > shape[2] - 1))
    moved = np.zeros(target, dtype=bool)
    for a in range(3):
        moved |= np.floor(c[a]) != np.floor(c0[a])
    return float(inside.mean()), int(low.sum()), int(high.sum()), float(moved[inside].mean())


def _volumes(shape):
    rng = np.random.default_rng(10 + shape[0])
    return (1000.0 * rng.standard_normal(shape)).astype(np.float32), rng.integers(-2, 3, size=shape).astype(np.int16)


# ---------------- resample_deform ----------------
@pytest.mark.parametrize("grid", [(4, 4, 4), (5, 4, 7)])
@pytest.mark.parametrize("shape,target", SHAPES)
def test_zero_field_equals_resample_affine(shape, target, grid):
    d = _data()
    vol, lab = _volumes(shape)
    zero = np.zeros(grid + (3,))
    for transform in TRANSFORMS:
        A, t = affine_of(transform, shape, target)
        assert np.array_equal(_bits(d.resample_deform(vol, target, A, t, zero)), _bits(d.resample_affine(vol, target, A, t)))
        assert np.array_equal(_bits(d.resample_deform(lab, target, A, t, zero, nearest=True)),
                              _bits(d.resample_affine(lab, target, A, t, nearest=True)))


@pytest.mark.parametrize("grid", [(4, 4, 4), (7, 5, 6), (8, 8, 8)])
def test_knot_placement_reproduces_linear_functions(grid):
    """P[m] = m along one axis: a uniform cubic B-spline whose knot m sits at x = m - 1 gives
    u(i) = i (g - 3) / N + 1 -- off by a constant for any other placement."""
    d = _data()
    target = (13, 10, 17)
    for axis in range(3):
        P = np.zeros(grid + (3,))
        m = np.arange(grid[axis], dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(3)])
        P[..., axis] = np.broadcast_to(m, grid)
        u = d.field_displacement(P, target)
        i = np.arange(target[axis], dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(3)])
        exp = np.broadcast_to(i * (grid[axis] - 3) / target[axis] + 1.0, target)
        assert np.allclose(u[axis], exp, rtol=1e-13, atol=1e-13)
        for other in range(3):
            if other != axis:
                assert not u[other].any()


def test_constant_control_grid_is_a_constant_displacement():
    d = _data()
    for grid in GRIDS:
        P = np.empty(grid + (3,))
        P[...] = (1.75, -0.3, 2.0 / 3.0)
        u = d.field_displacement(P, (9, 14, 11))
        for c, v in enumerate((1.75, -0.3, 2.0 / 3.0)):
            assert np.allclose(u[c], v, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("grid", GRIDS)
def test_host_displacement_is_the_formula(grid):
    """The host form's factored sums against the dense tensor-product evaluation of this file."""
    d = _data()
    for target in ((16, 12, 20), (4, 3, 2)):
        u = d.field_displacement(random_field(grid), target)
        exp = displacement(random_field(grid), target)
        for c in range(3):
            assert u[c].shape == target and np.allclose(u[c], exp[c], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("k", range(len(TRANSFORMS)))
def test_ramp_is_sampled_at_the_deformed_coordinate(k):
    """Trilinear interpolation reproduces a linear function: where all 8 corners are unclamped
    the result is the ramp at c, c computed here from the formulas (one fp32 ulp at the ramp's maximum)."""
    d = _data()
    shape, target = SHAPES[0]
    field = random_field(GRIDS[k % 3])
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    ramp = 3.0 * g[0] + 5.0 * g[1] + 7.0 * g[2] + 1.0
    A, t = affine_of(TRANSFORMS[k], shape, target)
    c = coords(A, t, target, field)
    free = np.ones(target, dtype=bool)
    for a in range(3):
        free &= (c[a] >= 1e-9) & (c[a] <= shape[a] - 1.0 - 1e-9)  # clear of the clamp by more than c's rounding
    assert free.sum() > 1000
    got = d.resample_deform(ramp, target, A, t, field)
    exp = 3.0 * c[0] + 5.0 * c[1] + 7.0 * c[2] + 1.0
    ulp = float(np.spacing(np.float32(ramp.max())))
    assert float(np.abs(got.astype(np.float64) - exp)[free].max()) <= ulp
    c0 = coords(A, t, target, None)
    assert max(float(np.abs(c[a] - c0[a]).max()) for a in range(3)) > 0.5  # the field does move the samples


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shape,target", GENERAL_SHAPES)
@pytest.mark.parametrize("k", range(len(TRANSFORMS)))
def test_fields_reach_every_branch(shape, target, k, grid):
    """What the bit-equality tests (here and on the GPU) rely on for each case they use."""
    share, low, high, moved = coverage(*affine_of(TRANSFORMS[k], shape, target), shape, target, random_field(grid))
    print(f"coverage {shape}->{target} transform {k} grid {grid}: inside {share:.3f} low {low} high {high} "
          f"moved {moved:.3f}")
    assert share >= 0.5 and low >= 50 and high >= 50 and moved >= 0.3, (share, low, high, moved)


def test_outside_region_and_nan_control_vector():
    d = _data()
    shape, target = SHAPES[1]
    vol, lab = _volumes(shape)
    vol = np.abs(vol) + 1.0  # no sample is 0: the zeros are the outside
    lab = np.abs(lab) + 1
    A, t = affine_of(((0.0, 0.0, 0.0), 1.0, (False, False, False), (0.0, 0.0, 0.0)), shape, target)
    # a field that pushes the low-D part of the output far outside: the D component of the control planes 0..3
    push = np.zeros((8, 4, 4, 3))
    push[:4, :, :, 0] = -1000.0
    u = d.field_displacement(push, target)[0]
    gone = u <= -target[0] - 1.0  # c_D = (7 / 16) (d + u) < -0.5 there
    assert 0.2 < gone.mean() < 0.8 and not u[13:].any()  # d >= 13 sees the control planes 4..7 only
    for nearest, v in ((False, vol), (True, lab)):
        got = d.resample_deform(v, target, A, t, push, nearest=nearest, **({} if nearest else {"gain": 1.1, "bias": 5.0}))
        assert got.dtype == np.float32 and not _bits(got[gone]).any()
        assert got[13, :, :18].all()  # while the undisplaced end is inside and sampled
    # one NaN control vector: exactly the voxels whose 4x4x4 support holds it are 0, nothing raises
    nan = nan_field()
    hit = np.isnan(d.field_displacement(nan, target)[0])
    (kd, _), (kh, _), (kw, _) = (basis(n, 8) for n in target)
    exp = (kd <= 3)[:, None, None] & (kh <= 3)[None, :, None] & (kw <= 3)[None, None, :]  # k <= 3 <= k + 3
    assert np.array_equal(hit, exp) and 0.1 < hit.mean() < 0.9
    for nearest, v in ((False, vol), (True, lab)):
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # nor a RuntimeWarning
            got = d.resample_deform(v, target, A, t, nan, nearest=nearest)
        assert np.isfinite(got).all() and not _bits(got[hit]).any()
        assert np.array_equal(_bits(got[~hit]), _bits(d.resample_deform(v, target, A, t, random_field((8, 8, 8)),
                                                                       nearest=nearest)[~hit]))


# ---------------- draw_transform ----------------
def _expected_draws(seed, epoch, case, n_modalities=5):
    """draw_transform's documented stream for AUG, from the generator itself."""
    rng = np.random.default_rng([seed, epoch, case])
    flips = [rng.random() < p for p in AUG["flip_prob"]]
    angles = [m * (2.0 * rng.random() - 1.0) for m in AUG["rotate_deg"]]
    zoom = AUG["zoom"][0] + (AUG["zoom"][1] - AUG["zoom"][0]) * rng.random()
    shift = np.array([m * (2.0 * rng.random() - 1.0) for m in AUG["shift_frac"]])
    gb = [(AUG["gain"][0] + (AUG["gain"][1] - AUG["gain"][0]) * rng.random(),
           AUG["bias"][0] + (AUG["bias"][1] - AUG["bias"][0]) * rng.random()) for _ in range(n_modalities)]
    return flips, angles, zoom, shift, tuple(g for g, _ in gb), tuple(b for _, b in gb), rng


def test_stream_is_unchanged_and_the_field_is_appended():
    d = _data()
    for seed, epoch, case in ((3, 5, 7), (11, 0, 2)):
        flips, angles, zoom, shift, gain, bias, rng = _expected_draws(seed, epoch, case)
        L = d.compose_transform(flips, angles, zoom)
        off = d.draw_transform(AUG, seed, epoch, case)
        assert off.field is None
        on = d.draw_transform(ELASTIC, seed, epoch, case)
        for tf in (off, on):  # the first ten draws and the gains / biases
            assert np.array_equal(tf.L, L) and np.array_equal(tf.shift_frac, shift)
            assert tf.gain == gain and tf.bias == bias
        u = np.array([rng.random() for _ in range(5 * 5 * 5 * 3)]).reshape(5, 5, 5, 3)
        assert on.field.shape == (5, 5, 5, 3) and on.field.dtype == np.float64
        assert np.array_equal(on.field, np.array([2.0, 2.0, 2.0]) * (2.0 * u - 1.0))
        assert np.abs(on.field).max() <= 2.0 and np.abs(on.field).max() > 1.5


def test_field_is_a_function_of_seed_epoch_case():
    d = _data()
    aug = dict(AUG, elastic_grid=(4, 5, 6), elastic_disp=(0.0, 1.0, 3.0))
    a, b = d.draw_transform(aug, 3, 5, 7), d.draw_transform(d.Augment(**aug), 3, 5, 7)
    assert a.field.shape == (4, 5, 6, 3) and np.array_equal(a.field, b.field)
    assert np.array_equal(a.field, d.draw_transform(aug, 3, 5, 7, n_modalities=5).field)
    for other in (d.draw_transform(aug, 3, 6, 7), d.draw_transform(aug, 3, 5, 8), d.draw_transform(aug, 4, 5, 7)):
        assert not np.array_equal(other.field, a.field)
    assert not a.field[..., 0].any() and not np.signbit(a.field[..., 0]).any()  # disp 0: +0.0
    assert np.abs(a.field[..., 1]).max() <= 1.0 and 1.0 < np.abs(a.field[..., 2]).max() <= 3.0


def test_elastic_settings_are_checked():
    d = _data()
    for bad in ({"elastic_grid": (4, 0, 4)}, {"elastic_grid": (0, 0, 5)},           # mixed zero
                {"elastic_grid": (4, 3, 4)}, {"elastic_grid": 1}, {"elastic_grid": (4, 4, 2)},  # an entry in 1..3
                {"elastic_grid": (8, 8, 9)}, {"elastic_grid": 9},                  # more than 512 control points
                {"elastic_disp": (1.0, float("nan"), 1.0)}, {"elastic_disp": (1.0, float("inf"), 1.0)},
                {"elastic_disp": (1.0, -0.5, 1.0)}, {"elastic_disp": -1.0}):
        with pytest.raises(ValueError):
            d.Augment(**bad)
    assert d.Augment(elastic_grid=6).elastic_grid == (6, 6, 6)
    assert d.Augment(elastic_grid=8, elastic_disp=1.5).elastic_disp == (1.5, 1.5, 1.5)  # 512 points: allowed
    assert d.Augment(elastic_grid=(4, 4, 32)).elastic_grid == (4, 4, 32)
    assert d.Augment.of({"elastic_grid": [5, 4, 7]}).elastic_grid == (5, 4, 7)
    off = d.Augment()
    assert off.elastic_grid == (0, 0, 0) and off.elastic_disp == (0.0, 0.0, 0.0)
    tf = d.draw_transform(off, 1, 2, 3)
    assert tf.field is None and np.array_equal(tf.L, np.eye(3)) and not tf.shift_frac.any()
    assert d.Transform(np.eye(3), np.zeros(3), (1.0,), (0.0,)).field is None  # the four-argument constructor


# ---------------- loaders ----------------
def _loader(tree, raw=False, **kw):
    kw.setdefault("augment", ELASTIC)
    kw.setdefault("augment_seed", 11)
    return _data().get_dataloader(tree, batch_size=2, shuffle=False, missing_strategy="zero_fill", target_size=TARGET,
                                  device_resample=raw, **kw)


def _same(a, b):
    return (a["case_id"] == b["case_id"] and torch.equal(a["image"].view(torch.int32), b["image"].view(torch.int32))
            and torch.equal(a["label"], b["label"]))


def test_default_loader_returns_resample_deform_of_the_files(tree):
    d = _data()
    ds = d.ProstateDataset(tree, target_size=TARGET, augment=ELASTIC, augment_seed=11)
    affine_only = d.ProstateDataset(tree, target_size=TARGET, augment=AUG, augment_seed=11)
    ds.set_epoch(3)
    affine_only.set_epoch(3)
    for i, case in enumerate(ds.case_list):
        tf = d.draw_transform(ELASTIC, 11, 3, i, 5)
        s = ds[i]
        assert set(s) == {"image", "label", "case_id"} and s["image"].shape == (5,) + TARGET
        for c, m in enumerate(ds.modalities):
            if m not in case["modality_files"]:
                assert not s["image"][c].any()  # zero_fill stays zero
                continue
            vol = ds._first_volume(d.read_nifti(case["modality_files"][m])).astype(np.float32)
            A, t = tf.affine(vol.shape, TARGET)
            exp = d.resample_deform(vol, TARGET, A, t, tf.field, gain=tf.gain[c], bias=tf.bias[c])
            assert np.array_equal(_bits(s["image"][c].numpy()), _bits(exp)), (i, m)
        lab = ds._first_volume(d.read_nifti(case["label_path"]))
        A, t = tf.affine(lab.shape, TARGET)
        exp = (d.resample_deform(lab, TARGET, A, t, tf.field, nearest=True) > 0).astype(np.float32)
        assert np.array_equal(s["label"][0].numpy(), exp)
        other = affine_only[i]  # the same affine without the field: the deformation shows
        assert not torch.equal(s["image"], other["image"]) and not torch.equal(s["label"], other["label"])


def test_every_volume_of_a_case_shares_the_field(tree):
    d = _data()
    ds = d.ProstateDataset(tree, target_size=TARGET, device_resample=True, augment=ELASTIC, augment_seed=11)
    ds.set_epoch(2)
    for i in range(len(ds)):
        s = ds[i]
        tf = d.draw_transform(ELASTIC, 11, 2, i, 5)
        f = s["augment"]["field"]  # one field per case, beside the per-volume affines
        assert isinstance(f, torch.Tensor) and f.dtype == torch.float64 and f.device.type == "cpu"
        assert f.is_contiguous() and tuple(f.shape) == (5, 5, 5, 3) and np.array_equal(f.numpy(), tf.field)
        assert s["augment"]["gain"] == tf.gain and len(s["augment"]["affine"]) == 5
        assert s["augment"]["label_affine"] == tf.affine12(s["raw_label"].shape, TARGET)


def test_workers_and_subset_position_do_not_change_a_sample(tree):
    d = _data()
    runs = []
    for workers in (0, 2):
        ld = _loader(tree, num_workers=workers)
        ld.dataset.set_epoch(1)
        runs.append(list(ld))
    assert len(runs[0]) == len(runs[1]) == 2 and all(_same(a, b) for a, b in zip(*runs))
    full = d.ProstateDataset(tree, target_size=TARGET, augment=ELASTIC, augment_seed=11)
    got = next(iter(_loader(tree, indices=[3, 1])))
    assert got["case_id"] == [full.case_list[3]["case_id"], full.case_list[1]["case_id"]]
    assert torch.equal(got["image"][0], full[3]["image"]) and torch.equal(got["image"][1], full[1]["image"])
    assert torch.equal(got["label"][0], full[3]["label"])


def test_raw_batches_carry_the_field_only_with_elastic_on(tree):
    d = _data()
    b = next(iter(_loader(tree, raw=True)))
    assert d.is_raw_batch(b) and len(b["augment"]) == 2
    for i, a in enumerate(b["augment"]):
        assert np.array_equal(a["field"].numpy(), d.draw_transform(ELASTIC, 11, 0, i, 5).field)
    off = next(iter(_loader(tree, raw=True, augment=AUG)))
    assert all(a.get("field") is None for a in off["augment"])
    assert "augment" not in next(iter(_loader(tree, raw=True, augment=None)))
