"""The host forms of the surface-distance metrics (predict.surface / edt_sq / distance_transform /
surface_metrics), no GPU: edt_sq against a brute-force minimum over all feature voxels on the
bits, surface against an explicit six-neighbour loop, the metrics on cases computed by hand, and
all of them against scipy / numpy where scipy imports."""
import functools
import math
import zlib

import numpy as np
import pytest

SHAPES = [(1, 1, 1), (1, 1, 9), (3, 5, 7), (4, 17, 6)]
SPACINGS = [(1.0, 1.0, 1.0), (3.0, 0.5, 0.5), (3.6, 0.3125, 0.3125), (2.2, 0.7, 0.9)]
FEATURES = ["empty", "single", "bernoulli0.02", "bernoulli0.3", "full"]


def _predict():
    import pcms_amd  # noqa: F401
    from pcms_amd import predict
    return predict


@functools.lru_cache(maxsize=None)
def _features(kind, shape):
    rng = np.random.default_rng(zlib.crc32(repr((kind, shape)).encode()))
    f = np.zeros(shape, np.uint8)
    if kind == "single":
        f[tuple(int(rng.integers(0, s)) for s in shape)] = 3  # a feature is != 0
    elif kind.startswith("bernoulli"):
        f = (rng.random(shape) < float(kind[len("bernoulli"):])).astype(np.uint8)
    elif kind == "full":
        f[:] = 1
    return f


def brute_edt_sq(feat, spacing):
    """The definition, one candidate at a time: min over feature voxels q of
    fl(Z(|pd-qd|) + fl(Y(|ph-qh|) + X(|pw-qw|))), every operation rounded on its own."""
    sz, sy, sx = (np.float64(s) for s in spacing)
    d, h, w = (g.astype(np.float64) for g in np.indices(feat.shape))
    best = np.full(feat.shape, np.inf)
    for qd, qh, qw in zip(*np.nonzero(feat)):
        tz, ty, tx = np.abs(d - qd) * sz, np.abs(h - qh) * sy, np.abs(w - qw) * sx
        best = np.minimum(best, tz * tz + (ty * ty + tx * tx))
    return best


def loop_surface(mask):
    D, H, W = mask.shape
    out = np.zeros(mask.shape, np.uint8)
    for d in range(D):
        for h in range(H):
            for w in range(W):
                if mask[d, h, w] == 0:
                    continue
                for dd, dh, dw in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
                    nd, nh, nw = d + dd, h + dh, w + dw
                    if not (0 <= nd < D and 0 <= nh < H and 0 <= nw < W) or mask[nd, nh, nw] == 0:
                        out[d, h, w] = 1
    return out


def _same_bits(got, exp, what):
    assert got.dtype == exp.dtype == np.float64 and got.shape == exp.shape, what
    diff = got.view(np.int64) != exp.view(np.int64)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {got.size} voxels differ"


@pytest.mark.parametrize("kind", FEATURES)
@pytest.mark.parametrize("shape", SHAPES)
def test_edt_sq_equals_brute_force_on_the_bits(shape, kind):
    predict = _predict()
    feat = _features(kind, shape)
    if kind == "empty":
        assert not feat.any()
    elif kind == "single":
        assert int((feat != 0).sum()) == 1
    for spacing in SPACINGS:
        got = predict.edt_sq(feat, spacing)
        _same_bits(got, brute_edt_sq(feat, spacing), f"{kind} {shape} {spacing}")
        if not feat.any():  # "empty", and a Bernoulli draw on a shape too small for one
            assert np.isposinf(got).all()
        else:
            assert np.isfinite(got).all() and (got[feat != 0] == 0).all()
        assert np.array_equal(predict.distance_transform(feat, spacing, squared=True), got)
        assert np.array_equal(predict.distance_transform(feat, spacing), np.sqrt(got))


def test_edt_sq_rejects_bad_arguments():
    predict = _predict()
    feat = _features("full", (3, 5, 7))
    for bad in ((1, 1), (0.0, 1, 1), (1, -1.0, 1), (1, 1, math.nan), (math.inf, 1, 1), 1.0):
        with pytest.raises(ValueError):
            predict.edt_sq(feat, bad)
    with pytest.raises(ValueError):
        predict.edt_sq(feat[0], (1, 1, 1))


def _block_touching_faces(shape):
    m = np.zeros(shape, np.uint8)
    m[:, : shape[1] - 1, 1:] = 1  # touches both D faces, the H = 0 face and the W = W - 1 face
    return m


def test_surface_equals_the_six_neighbour_loop():
    predict = _predict()
    shape = (5, 6, 7)
    solid = np.ones(shape, np.uint8)
    one = np.zeros(shape, np.uint8)
    one[2, 3, 4] = 200
    cases = {"solid": solid, "block": _block_touching_faces(shape), "one voxel": one, "zeros": np.zeros(shape, np.uint8),
             "bernoulli": _features("bernoulli0.3", (4, 17, 6)) * 7, "dense": 1 - _features("bernoulli0.02", (4, 17, 6)),
             "1x1x1": np.ones((1, 1, 1), np.uint8)}
    for name, m in cases.items():
        got = predict.surface(m)
        assert got.dtype == np.uint8 and np.array_equal(got, loop_surface(m)), name
    # a solid volume: exactly its face voxels; the interior is not surface
    s = predict.surface(solid)
    assert int(s.sum()) == solid.size - 3 * 4 * 5 and not s[1:-1, 1:-1, 1:-1].any()
    assert np.array_equal(predict.surface(one), (one != 0).astype(np.uint8))
    assert not predict.surface(cases["zeros"]).any()
    assert predict.surface(cases["block"])[0, 2, 3] == 1  # on a face of the volume


def _cube(shape, lo, size):
    m = np.zeros(shape, np.uint8)
    m[lo[0]:lo[0] + size, lo[1]:lo[1] + size, lo[2]:lo[2] + size] = 1
    return m


def test_surface_metrics_by_hand():
    predict = _predict()
    shape = (8, 9, 12)
    a = _cube(shape, (2, 2, 2), 4)
    same = predict.surface_metrics(a, a.copy(), (3.6, 0.3125, 0.3125))
    assert (same["hd"], same["hd95"], same["assd"]) == (0.0, 0.0, 0.0)
    assert same["n_a"] == same["n_b"] == 4 ** 3 - 2 ** 3
    # the same cube two voxels along W at sx = 0.5: every surface voxel of either finds the other
    # surface within 1.0, the faces at the far ends exactly at 1.0
    b = _cube(shape, (2, 2, 4), 4)
    m = predict.surface_metrics(a, b, (1.0, 1.0, 0.5))
    assert m["hd"] == 1.0 and 0.0 < m["assd"] < 1.0 and m["hd95"] <= 1.0
    assert m["n_a"] == m["n_b"] == 56
    # the empty rules
    z = np.zeros(shape, np.uint8)
    both = predict.surface_metrics(z, z)
    assert (both["hd"], both["hd95"], both["assd"], both["n_a"], both["n_b"]) == (0.0, 0.0, 0.0, 0, 0)
    for x, y in ((a, z), (z, a)):
        one = predict.surface_metrics(x, y)
        assert one["hd"] == one["hd95"] == one["assd"] == math.inf
        assert (one["n_a"], one["n_b"]) == ((56, 0) if x is a else (0, 56))
    with pytest.raises(ValueError):
        predict.surface_metrics(a, a[:-1])
    # single voxels d apart: da = db = [d]; hd = hd95 = assd = d, in millimetres
    p, q = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    p[1, 1, 1] = q[2, 1, 5] = 1
    d = math.sqrt((1 * 3.0) ** 2 + (4 * 0.5) ** 2)
    m = predict.surface_metrics(p, q, (3.0, 0.25, 0.5))
    assert m["hd"] == m["hd95"] == m["assd"] == d and m["n_a"] == m["n_b"] == 1


def test_hd95_interpolates_between_order_statistics():
    predict = _predict()
    from pcms_amd import distance
    # n = 12: pos = 11 * 0.95 = 10.45, between v[10] and v[11]
    v = np.array([0.5 * k * k for k in range(12)])
    pos = 11 * 0.95
    assert pos != math.floor(pos) and math.floor(pos) == 10
    exp = v[10] + (v[11] - v[10]) * (pos - 10)
    assert distance._percentile95(v) == exp and v[10] < exp < v[11]
    assert distance._percentile95(np.array([7.0])) == 7.0
    # n = 21: pos = 19 exactly -- the order statistic itself
    w = np.arange(21, dtype=np.float64) ** 1.5
    assert distance._percentile95(w) == w[19]
    # through surface_metrics: a line of 6 voxels against one voxel at its end; da = 0..5, db = [0]
    a, b = np.zeros((1, 1, 9), np.uint8), np.zeros((1, 1, 9), np.uint8)
    a[0, 0, :6] = 1
    b[0, 0, 0] = 1
    m = predict.surface_metrics(a, b, (1.0, 1.0, 0.7))
    both = np.sort(np.array([0.0] + [math.sqrt((k * 0.7) * (k * 0.7)) for k in range(6)]))
    assert m["hd95"] == distance._percentile95(both) and m["hd"] == both[-1]
    assert m["assd"] == (float(both[1:].mean()) + 0.0) / 2.0


def test_against_scipy_and_numpy():
    ndi = pytest.importorskip("scipy.ndimage")
    predict = _predict()
    from pcms_amd import distance
    compared = 0
    for shape in SHAPES[1:] + [(6, 20, 18)]:
        for kind in ("single", "bernoulli0.02", "bernoulli0.3", "full"):
            feat = _features(kind, shape)
            m = (feat != 0)
            if not m.any():  # scipy's transform is undefined without a feature voxel
                continue
            compared += 1
            assert np.array_equal(predict.surface(feat),
                                  (m ^ ndi.binary_erosion(m, ndi.generate_binary_structure(3, 1))).astype(np.uint8))
            for spacing in SPACINGS:
                exp = ndi.distance_transform_edt(~m, sampling=spacing)
                got = predict.distance_transform(feat, spacing)
                assert np.all(np.abs(got - exp) <= 1e-12 * np.abs(exp)), (shape, kind, spacing)
    assert compared >= 14  # every shape with at least three non-empty feature sets
    rng = np.random.default_rng(5)
    for n in (1, 2, 12, 21, 1000):
        v = np.sort(rng.random(n) * 40.0)
        assert abs(distance._percentile95(v) - np.percentile(v, 95)) <= 1e-12 * np.percentile(v, 95)
    # the whole chain against MedPy's recipe
    a = np.zeros((6, 20, 18), np.uint8)
    b = np.zeros_like(a)
    a[1:5, 4:14, 3:12] = 1
    b[2:6, 6:17, 2:10] = 1
    spacing = (3.6, 0.3125, 0.3125)
    sa, sb = predict.surface(a) != 0, predict.surface(b) != 0
    da = ndi.distance_transform_edt(~sb, sampling=spacing)[sa]
    db = ndi.distance_transform_edt(~sa, sampling=spacing)[sb]
    m = predict.surface_metrics(a, b, spacing)
    assert m["hd"] == pytest.approx(max(da.max(), db.max()), rel=1e-12)
    assert m["hd95"] == pytest.approx(np.percentile(np.hstack([da, db]), 95), rel=1e-12)
    assert m["assd"] == pytest.approx((da.mean() + db.mean()) / 2, rel=1e-12)
