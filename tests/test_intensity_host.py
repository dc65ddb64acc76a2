"""Percentile intensity normalisation, the host forms (no GPU): ``predict.intensity_window`` /
``normalise_window`` / ``Normalisation`` and their way through ``data.resample_patch`` and
``PatchSampling``.  ``intensity_window`` is compared with a brute-force restatement
on the order-preserving u32 keys the device kernels select on."""
import numpy as np
import pytest


def _predict():
    import pcms_amd  # noqa: F401
    from pcms_amd import predict
    return predict


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def same_floats(a, b):
    """Equal on the bits, a NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def brute_window(vol, lower, upper, above=None):
    """Sort the u32 keys (every NaN the top key), pick the two ranks, map the keys back."""
    v = np.asarray(vol).astype(np.float32).reshape(-1) + np.float32(0)
    if above is not None:
        with np.errstate(invalid="ignore"):
            v = v[v > np.float32(above)]
    m = v.size
    if m == 0:
        return np.zeros(2, np.float32)
    u = v.view(np.uint32)
    key = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))
    key = np.sort(np.where(np.isnan(v), np.uint32(0xFFFFFFFF), key))
    q_lo, q_hi = int(round(lower * 10000)), int(round(upper * 10000))
    r_lo, r_hi = (q_lo * (m - 1)) // 10 ** 6, -((-q_hi * (m - 1)) // 10 ** 6)
    k = key[[r_lo, r_hi]]
    out = np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)
    return np.where(k == np.uint32(0xFFFFFFFF), np.float32(np.nan), out).astype(np.float32)


def outlier_volume(shape=(20, 64, 64), seed=5):
    """90 % background zeros, tissue in 50..900, one voxel at 30000 (int16)."""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(shape) < 0.9, 0, rng.integers(50, 901, size=shape)).astype(np.int16)
    v[3, 7, 11] = 30000
    return v


VOLUMES = {
    "int16_outlier": lambda: outlier_volume(),
    "float_normal": lambda: (1000.0 * np.random.default_rng(1).standard_normal(70001)).astype(np.float32),
    "constant": lambda: np.full(257, 7, np.uint8),
    "two_values": lambda: np.where(np.arange(4099) % 3 == 0, -2.5, 4.0).astype(np.float32),
    "inf": lambda: np.concatenate([[np.inf, -np.inf], np.random.default_rng(2).standard_normal(255)]).astype(np.float32),
    "zeros_signed": lambda: np.array([-0.0, 0.0, -1.0, 1.0, -0.0, 0.0, 0.0], np.float32),
    "nan": lambda: np.concatenate([[np.nan], np.arange(300.0), [np.nan]]).astype(np.float32),
    "double": lambda: np.random.default_rng(3).standard_normal(1000) * 1e-3,
}


@pytest.mark.parametrize("name", sorted(VOLUMES))
@pytest.mark.parametrize("window", [(0.5, 99.5), (0.0, 100.0), (25.0, 75.0), (49.9999, 50.0)])
@pytest.mark.parametrize("above", [None, 0.0])
def test_intensity_window_matches_the_sorted_keys(name, window, above):
    p = _predict()
    vol = VOLUMES[name]()
    got = p.intensity_window(vol, *window, above=above)
    assert got.dtype == np.float32 and got.shape == (2,)
    assert same_floats(got, brute_window(vol, *window, above=above)), (got, brute_window(vol, *window, above=above))


def test_the_full_window_is_the_minimum_and_maximum():
    p = _predict()
    for name in ("int16_outlier", "float_normal", "constant", "two_values", "inf", "double"):
        v = VOLUMES[name]().astype(np.float32)
        assert np.array_equal(bits(p.intensity_window(v, 0, 100)), bits([v.min(), v.max()])), name


@pytest.mark.parametrize("n", [1, 2, 257, 4099, 70001])
def test_normalise_window_at_min_max_is_normalise(n):
    p = _predict()
    rng = np.random.default_rng(n)
    for vol in ((1000.0 * rng.standard_normal(n)).astype(np.float32), rng.integers(-200, 3000, size=n).astype(np.int16),
                np.full(n, 3.5, np.float32), rng.standard_normal(n) * 1e30):
        exp = p.normalise(vol)
        got = p.normalise_window(vol, p.intensity_window(vol, 0, 100))
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(exp))
        v = vol.astype(np.float32)
        assert np.array_equal(bits(p.normalise_window(vol, (v.min(), v.max()))), bits(exp))


def test_signed_zeros_fold_into_plus_zero():
    p = _predict()
    v = np.array([-0.0, -0.0, -0.0, 1.0], np.float32)
    lohi = p.intensity_window(v, 0, 50)
    assert np.array_equal(bits(lohi), bits([0.0, 0.0]))           # +0.0 on the bits, not -0.0
    v = np.array([-1.0, -0.0, 0.0, -0.0, 2.0], np.float32)
    assert np.array_equal(bits(p.intensity_window(v, 25, 75)), bits([0.0, 0.0]))
    assert np.array_equal(bits(p.intensity_window(v, 0, 100, above=-0.0)), bits([2.0, 2.0]))  # 0 > -0 is false


def test_infinities_are_ordinary_values():
    p = _predict()
    v = np.array([np.inf, 1.0, -np.inf, 2.0, 3.0], np.float32)
    assert np.array_equal(bits(p.intensity_window(v, 0, 100)), bits([-np.inf, np.inf]))
    assert np.array_equal(bits(p.intensity_window(v, 25, 75)), bits([1.0, 3.0]))
    out = p.normalise_window(v, (1.0, 3.0))
    assert np.array_equal(bits(out), bits([1.0, 0.0, 0.0, 0.5, 1.0]))


def test_nans_sort_last_and_stay_nan_through_the_clip():
    p = _predict()
    v = np.array([np.nan, 5.0, 1.0, 3.0, np.nan, 2.0, 4.0], np.float32)
    lohi = p.intensity_window(v, 0, 100)
    assert lohi[0] == 1.0 and np.isnan(lohi[1])
    assert np.array_equal(bits(p.intensity_window(v, 0, 50)), bits([1.0, 4.0]))   # ranks 0 and 3 of 7
    assert np.array_equal(bits(p.intensity_window(v, 0, 100, above=0.0)), bits([1.0, 5.0]))  # above drops the NaNs
    assert np.array_equal(bits(p.intensity_window(v, 0, 100, above=-np.float32(1e30))), bits([1.0, 5.0]))
    out = p.normalise_window(v, (2.0, 4.0))
    assert np.isnan(out[0]) and np.isnan(out[4])
    rest = out[[1, 2, 3, 5, 6]]
    assert np.array_equal(bits(rest), bits([1.0, 0.0, 0.5, 0.0, 1.0])) and rest.min() >= 0 and rest.max() <= 1


def test_empty_and_single_selections():
    p = _predict()
    v = np.array([-3.0, -1.0, 7.0], np.float32)
    assert np.array_equal(bits(p.intensity_window(v, 0.5, 99.5, above=7.0)), bits([0.0, 0.0]))      # m == 0
    assert np.array_equal(bits(p.intensity_window(v, 0.5, 99.5, above=-1.0)), bits([7.0, 7.0]))     # m == 1
    assert np.array_equal(bits(p.intensity_window(np.array([2.5]), 0, 100)), bits([2.5, 2.5]))
    assert np.array_equal(bits(p.normalise_window(v, (7.0, 7.0))), bits([0.0, 0.0, 0.0]))           # den == 0
    assert np.array_equal(bits(p.intensity_window(np.array([np.nan], np.float32), 0, 100, above=0.0)), bits([0, 0]))


@pytest.mark.parametrize("lower,upper", [(-0.1, 99.0), (0.0, 100.1), (50.0, 50.0), (60.0, 40.0), (float("nan"), 99.0),
                                         (10.00001, 10.00002)])
def test_bad_percentiles_raise(lower, upper):
    p = _predict()
    with pytest.raises(ValueError):
        p.intensity_window(np.arange(10), lower, upper)
    with pytest.raises(ValueError):
        p.Normalisation("percentile", lower, upper)


def test_bad_above_and_method_raise():
    p = _predict()
    for above in (float("inf"), float("nan")):
        with pytest.raises(ValueError):
            p.intensity_window(np.arange(10), above=above)
        with pytest.raises(ValueError):
            p.Normalisation("percentile", above=above)
    for bad in ("zscore", "Percentile", ""):
        with pytest.raises(ValueError):
            p.Normalisation.of(bad)
    with pytest.raises(ValueError):
        p.Normalisation.of(3.5)


def test_normalisation_of_every_accepted_form():
    p = _predict()
    N = p.Normalisation
    assert N.of(None) is None and N.of(False) is None
    assert N.of(True) == N("minmax") and N.of("minmax") == N() and N().method == "minmax"
    assert N.of("percentile") == N("percentile", 0.5, 99.5, None)
    assert N.of({"method": "percentile", "lower": 1, "upper": 99, "above": 0}) == N("percentile", 1.0, 99.0, 0.0)
    inst = N("percentile", above=0.0)
    assert N.of(inst) is inst and inst.ppm == (5000, 995000)
    vol = outlier_volume()
    assert np.array_equal(bits(N.of(True).apply(vol)), bits(p.normalise(vol)))
    assert np.array_equal(bits(inst.apply(vol)),
                          bits(p.normalise_window(vol, p.intensity_window(vol, 0.5, 99.5, above=0.0))))


def test_the_window_keeps_tissue_contrast_on_an_outlier_volume():
    """The issue's case: one hot voxel sets min-max's hi; the percentile window of the voxels > 0 does
    not move."""
    p = _predict()
    vol = outlier_volume()
    tissue = (vol > 0) & (vol < 30000)
    assert np.median(p.normalise(vol)[tissue]) < 0.02
    assert 0.45 < np.median(p.Normalisation("percentile", above=0.0).apply(vol)[tissue]) < 0.55


def test_patch_sampling_selects_the_percentile_window():
    """``PatchSampling(normalise="percentile")`` used to be coerced to min-max by ``bool()``."""
    d, p = _data(), _predict()
    ps = d.PatchSampling(patch_size=(16, 16, 16), normalise="percentile")
    assert ps.normalise == p.Normalisation("percentile")
    assert d.PatchSampling(normalise=True).normalise is True and d.PatchSampling().normalise is False
    assert d.PatchSampling.of({"normalise": {"method": "percentile", "above": 0.0}}).normalise == \
        p.Normalisation("percentile", above=0.0)
    with pytest.raises(ValueError):
        d.PatchSampling(normalise="zscore")
    vol = outlier_volume()
    grid, patch, origin = (12, 40, 40), (16, 16, 16), (-2, 7, 13)
    A, t = d.volume_affine(d.compose_transform((True, False, True), (8.0, -5.0, 12.0), 1.15),
                           np.array([0.7, -2.2, 1.4]), vol.shape, grid)
    got = d.resample_patch(vol, grid, A, t, origin, patch, gain=1.25, bias=-0.5, normalise=ps.normalise)
    exp = d._resample_patch(p.normalise_window(vol, p.intensity_window(vol)), grid, A, t, origin, patch, 1.25, -0.5)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(exp))
    minmax = d.resample_patch(vol, grid, A, t, origin, patch, gain=1.25, bias=-0.5, normalise=True)
    assert not np.array_equal(bits(got), bits(minmax))
    assert np.array_equal(bits(minmax), bits(d._resample_patch(p.normalise(vol), grid, A, t, origin, patch, 1.25, -0.5)))
