"""predict.py's host forms of the lesion analysis (component_table, overlap_pairs, match_lesions,
lesion_table, lesion_metrics) against plain loops over voxels and hand-made cases (CPU).  The
mask and probability builders here are the ones the GPU tests use; the facts those tests rely on
are asserted at the end."""
import functools
import math

import numpy as np
import pytest

SHAPES = [(1, 1, 1), (1, 1, 257), (3, 5, 7), (9, 17, 33), (24, 40, 48)]
BIG = [(9, 17, 33), (24, 40, 48)]
CASE_SHAPE = (24, 40, 48)
BERNOULLI = {6: 0.30, 18: 0.15, 26: 0.10}  # below each connectivity's percolation threshold


def _predict():
    import pcms_amd  # noqa: F401
    from pcms_amd import predict
    return predict


# ---- masks, probabilities -------------------------------------------------------------------
def _serpentine(shape):
    """A one-voxel-wide 6-connected path through every other row of every other plane: one
    component whose box is the whole volume (up to the last odd row / plane)."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    rows = list(range(0, H, 2))
    m[::2, ::2, :] = 1
    right = True
    for k, d in enumerate(range(0, D, 2)):
        order = rows if k % 2 == 0 else rows[::-1]
        for a, b in zip(order, order[1:]):
            m[d, min(a, b):max(a, b) + 1, W - 1 if right else 0] = 1
            right = not right
        if d + 2 < D:
            m[d:d + 3, order[-1], W - 1 if right else 0] = 1
            right = not right
    return m


@functools.lru_cache(maxsize=None)
def mask(pattern, shape):
    d, h, w = np.indices(shape)
    if pattern == "zeros":
        return np.zeros(shape, np.uint8)
    if pattern == "ones":
        return np.ones(shape, np.uint8)
    if pattern == "checkerboard":
        return ((d + h + w) % 2 == 0).astype(np.uint8)
    if pattern == "serpentine":
        return _serpentine(shape)
    assert pattern.startswith("bernoulli"), pattern
    # seeds at which every one of them has >= 100 components (test_the_masks_are_what_they_claim)
    rng = np.random.default_rng(610 + shape[0])
    return (rng.random(shape) < BERNOULLI[int(pattern[len("bernoulli"):])]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def labels(pattern, shape, connectivity):
    return _predict().label_components(mask(pattern, shape), connectivity)


@functools.lru_cache(maxsize=None)
def prob(shape, seed=0, nan=True):
    """fp32 values out of a handful, so that maxima repeat inside a component: negatives, both
    zeros, both infinities and a positive NaN among them (``nan=False``: 2.0 in its place, for the
    comparisons of dicts, where a NaN would differ from itself)."""
    values = np.array([0.25, 0.5, 0.5, -1.0, 0.0, -0.0, np.inf, -np.inf, np.nan if nan else 2.0, 0.75, -0.125, 0.5],
                      np.float32)
    rng = np.random.default_rng(900 + seed + shape[2])
    p = values[rng.integers(0, len(values), size=shape)]
    if p.size > 64:  # the rare values stay rare: most of the volume is ordinary
        p = np.where(rng.random(shape) < 0.9, rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=shape), p)
    return np.ascontiguousarray(p, np.float32)


def _boxes(shape, rng, count, lo, hi):
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        size = rng.integers(lo, hi + 1, size=3)
        at = [int(rng.integers(0, s - k + 1)) for s, k in zip(shape, size)]
        m[at[0]:at[0] + size[0], at[1]:at[1] + size[1], at[2]:at[2] + size[2]] = 1
    return m


@functools.lru_cache(maxsize=None)
def case_masks():
    """(pred, ref) on CASE_SHAPE: ref is a set of small boxes; pred is ref moved by one voxel with
    some of its boxes missing, some boxes of its own, and a bar that bridges reference lesions."""
    rng = np.random.default_rng(4242)
    ref = _boxes(CASE_SHAPE, rng, 45, 2, 4)
    keep = _boxes(CASE_SHAPE, np.random.default_rng(7), 60, 5, 9)  # where pred follows ref
    pred = np.roll(ref, 1, axis=2) & keep
    pred[:, :, 0] = 0
    pred |= _boxes(CASE_SHAPE, rng, 12, 1, 3)
    pred[12, 20, 4:44] = 1
    return np.ascontiguousarray(pred), np.ascontiguousarray(ref)


# ---- brute force ----------------------------------------------------------------------------
def _key(x):
    bits = int(np.float32(x).view(np.uint32))
    return bits ^ (0xFFFFFFFF if bits >> 31 else 0x80000000)


def _loop_table(lab, p=None):
    rows = {}
    flat = lab.reshape(-1)
    for i in range(flat.size):
        L = int(flat[i])
        if L == 0:
            continue
        d, h, w = np.unravel_index(i, lab.shape)
        row = rows.setdefault(L, {"voxels": 0, "sum": [0, 0, 0], "box": [d, d, h, h, w, w], "peak": None})
        row["voxels"] += 1
        for a, c in enumerate((d, h, w)):
            row["sum"][a] += int(c)
            row["box"][2 * a] = min(row["box"][2 * a], int(c))
            row["box"][2 * a + 1] = max(row["box"][2 * a + 1], int(c))
        if p is not None:
            k = _key(p.reshape(-1)[i])
            if row["peak"] is None or k > row["peak"][0]:  # strict: the first (smallest) index keeps a tie
                row["peak"] = (k, i)
    return rows


def _assert_table(table, lab, p=None):
    rows = _loop_table(lab, p)
    order = sorted(rows)
    assert table["label"].dtype == np.int32 and table["label"].tolist() == order
    assert table["voxels"].dtype == np.int32 and table["voxels"].tolist() == [rows[L]["voxels"] for L in order]
    assert table["bbox"].dtype == np.int32 and table["bbox"].shape == (len(order), 6)
    assert table["bbox"].tolist() == [rows[L]["box"] for L in order]
    assert table["index_sum"].dtype == np.int64 and table["index_sum"].shape == (len(order), 3)
    assert table["index_sum"].tolist() == [rows[L]["sum"] for L in order]
    if p is None:
        assert set(table) == {"label", "voxels", "bbox", "index_sum"}
        return
    assert table["peak"].dtype == np.float32 and table["peak_index"].dtype == np.int32
    assert table["peak_index"].tolist() == [rows[L]["peak"][1] for L in order]
    assert table["peak"].view(np.uint32).tolist() == \
        [int(p.reshape(-1)[rows[L]["peak"][1]].view(np.uint32)) for L in order]


def same_table(got, exp):
    assert set(got) == set(exp)
    for k in exp:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, k
        assert got[k].tobytes() == exp[k].tobytes(), k


# ---- component_table ------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,connectivity", [("ones", 26), ("checkerboard", 6), ("serpentine", 6),
                                                  ("bernoulli6", 6), ("bernoulli18", 18), ("bernoulli26", 26)])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 257), (3, 5, 7), (9, 17, 33)])
def test_component_table_equals_a_loop_over_voxels(shape, pattern, connectivity):
    predict = _predict()
    lab = labels(pattern, shape, connectivity)
    _assert_table(predict.component_table(lab), lab)
    _assert_table(predict.component_table(lab, prob(shape)), lab, prob(shape))


def test_component_table_of_an_empty_volume():
    predict = _predict()
    for p in (None, np.zeros((3, 5, 7), np.float32)):
        t = predict.component_table(np.zeros((3, 5, 7), np.int32), p)
        assert t["label"].shape == (0,) and t["voxels"].shape == (0,) and t["bbox"].shape == (0, 6)
        assert t["index_sum"].shape == (0, 3) and t["index_sum"].dtype == np.int64
        assert ("peak" in t) == (p is not None)
        if p is not None:
            assert t["peak"].shape == (0,) and t["peak"].dtype == np.float32 and t["peak_index"].dtype == np.int32


def test_component_table_rejects_labels_that_are_not_canonical():
    predict = _predict()
    good = labels("bernoulli26", (9, 17, 33), 26)
    predict.component_table(good)
    n = good.size
    zero = np.flatnonzero(good.reshape(-1) == 0)
    at, other = int(zero[9]), int(zero[5])
    for value in (n + 1, 2 ** 31 - 1, -3, other + 1):  # past the volume / negative / naming a background voxel
        bad = good.copy()
        bad.reshape(-1)[at] = value
        with pytest.raises(ValueError):
            predict.component_table(bad)
    shifted = np.where(good > 0, good + 1, 0).astype(np.int32)  # labels that name the voxel after the root
    with pytest.raises(ValueError):
        predict.component_table(shifted)
    with pytest.raises(ValueError):
        predict.component_table(good.astype(np.float32))
    with pytest.raises(ValueError):
        predict.component_table(good, np.zeros(good.shape, np.float64))
    with pytest.raises(ValueError):
        predict.component_table(good, np.zeros((1,) + good.shape[1:], np.float32))


def test_peak_order_ties_zeros_negatives_and_infinities():
    predict = _predict()
    lab = np.zeros((1, 4, 8), np.int32)
    for row in range(4):
        lab[0, row, :] = 1 + row * 8  # four components, one per row
    p = np.zeros((1, 4, 8), np.float32)
    p[0, 0] = [0.5, 0.9, 0.1, 0.9, 0.9, 0.2, 0.3, 0.4]          # the maximum three times: the first wins
    p[0, 1] = [-0.0, -0.0, 0.0, -0.0, 0.0, -1.0, -0.0, -0.0]    # +0.0 is above -0.0
    p[0, 2] = [-3.0, -np.inf, -2.0, -5.0, -2.0, -7.0, -9.0, -4.0]  # all negative
    p[0, 3] = [1.0, np.inf, 2.0, np.inf, -np.inf, 3.0, np.nan, 4.0]  # a positive NaN is above +inf
    t = predict.component_table(lab, p)
    assert t["label"].tolist() == [1, 9, 17, 25]
    assert t["peak_index"].tolist() == [1, 8 + 2, 16 + 2, 24 + 6]
    assert t["peak"][:3].tolist() == [np.float32(0.9), 0.0, -2.0] and not np.signbit(t["peak"][1])
    assert np.isnan(t["peak"][3])
    p[0, 3, 6] = -np.nan  # a negative NaN is below everything
    t = predict.component_table(lab, p)
    assert t["peak_index"][3] == 24 + 1 and t["peak"][3] == np.inf
    p[0, 1] = -0.0
    t = predict.component_table(lab, p)
    assert t["peak_index"][1] == 8 and np.signbit(t["peak"][1]) and t["peak"][1] == 0.0


# ---- overlap_pairs --------------------------------------------------------------------------
def _loop_pairs(la, lb):
    pairs = {}
    for a, b in zip(la.reshape(-1).tolist(), lb.reshape(-1).tolist()):
        if a > 0 and b > 0:
            pairs[(a, b)] = pairs.get((a, b), 0) + 1
    return np.array([[a, b, v] for (a, b), v in sorted(pairs.items())], np.int64).reshape(-1, 3)


@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_overlap_pairs_equal_a_dictionary_over_voxels(connectivity):
    predict = _predict()
    pred, ref = case_masks()
    la, lb = predict.label_components(pred, connectivity), predict.label_components(ref, connectivity)
    got = predict.overlap_pairs(la, lb, connectivity)
    assert got.dtype == np.int64 and np.array_equal(got, _loop_pairs(la, lb))
    empty = predict.overlap_pairs(la, np.zeros_like(lb), connectivity)
    assert empty.shape == (0, 3) and empty.dtype == np.int64
    with pytest.raises(ValueError):
        predict.overlap_pairs(la, lb[:-1], connectivity)


def test_a_pair_that_meets_in_two_places_is_summed():
    predict = _predict()
    a = np.zeros((1, 5, 9), np.uint8)
    a[0, 1:4, 1:8] = 1
    a[0, 2, 2:7] = 0      # a ring
    b = np.zeros_like(a)
    b[0, 0:5, 1] = 1
    b[0, 0:5, 7] = 1
    b[0, 0, 1:8] = 1      # a bracket that crosses the ring's two sides: 3 + 3 voxels, far apart
    la, lb = predict.label_components(a, 26), predict.label_components(b, 26)
    inter = predict.label_components((la > 0) & (lb > 0), 26)
    assert len(np.unique(inter[inter > 0])) == 2
    got = predict.overlap_pairs(la, lb, 26)
    assert got.tolist() == [[int(la.max()), int(lb.max()), 6]] and np.array_equal(got, _loop_pairs(la, lb))


# ---- match_lesions --------------------------------------------------------------------------
def _tables(sizes_p, sizes_r):
    mk = lambda sizes: {"label": np.array(sorted(sizes), np.int32),  # noqa: E731
                        "voxels": np.array([sizes[k] for k in sorted(sizes)], np.int32)}
    return mk(sizes_p), mk(sizes_r)


def test_a_prediction_over_two_references_takes_the_higher_iou():
    predict = _predict()
    tp, tr = _tables({5: 100}, {3: 40, 9: 60})
    pairs = np.array([[5, 3, 30], [5, 9, 50]], np.int64)  # iou 30/110 and 50/110
    m = predict.match_lesions(tp, tr, pairs)
    assert m["matches"] == [(9, 5, 50, 50 / 110, 2 * 50 / 160)]
    assert (m["tp"], m["fp"], m["fn"], m["n_pred"], m["n_ref"]) == (1, 0, 1, 1, 2)
    assert m["sensitivity"] == 0.5 and m["precision"] == 1.0 and m["f1"] == 2 / 3


def test_an_iou_tie_resolves_by_label():
    predict = _predict()
    tp, tr = _tables({4: 10, 8: 10}, {2: 10, 6: 10})
    pairs = np.array([[4, 2, 5], [4, 6, 5], [8, 2, 5], [8, 6, 5]], np.int64)  # all iou 1/3
    m = predict.match_lesions(tp, tr, pairs)
    assert [(r, p) for r, p, *_ in m["matches"]] == [(2, 4), (6, 8)]  # ref ascending, then pred ascending
    assert m["tp"] == 2 and m["fp"] == 0 and m["fn"] == 0 and m["f1"] == 1.0


def test_a_pair_below_min_iou_is_no_match():
    predict = _predict()
    tp, tr = _tables({4: 50}, {2: 50})
    below = np.array([[4, 2, 9]], np.int64)   # 9/91 < 0.1
    at = np.array([[4, 2, 10]], np.int64)     # 10/90 >= 0.1
    m = predict.match_lesions(tp, tr, below)
    assert m["matches"] == [] and (m["tp"], m["fp"], m["fn"]) == (0, 1, 1)
    assert m["sensitivity"] == 0.0 and m["precision"] == 0.0 and m["f1"] == 0.0
    assert predict.match_lesions(tp, tr, at)["tp"] == 1
    assert predict.match_lesions(tp, tr, at, min_iou=0.5)["tp"] == 0
    tp2, tr2 = _tables({4: 10}, {2: 10})
    assert predict.match_lesions(tp2, tr2, np.array([[4, 2, 1]], np.int64), min_iou=1 / 19)["tp"] == 1  # >=


def test_nan_where_there_is_nothing_to_divide_by():
    predict = _predict()
    none = np.zeros((0, 3), np.int64)
    tp, tr = _tables({4: 10}, {})
    m = predict.match_lesions(tp, tr, none)
    assert math.isnan(m["sensitivity"]) and m["precision"] == 0.0 and m["f1"] == 0.0 and m["fp"] == 1
    tp, tr = _tables({}, {2: 10})
    m = predict.match_lesions(tp, tr, none)
    assert math.isnan(m["precision"]) and m["sensitivity"] == 0.0 and m["f1"] == 0.0 and m["fn"] == 1
    tp, tr = _tables({}, {})
    m = predict.match_lesions(tp, tr, none)
    assert all(math.isnan(m[k]) for k in ("sensitivity", "precision", "f1")) and m["tp"] == m["fp"] == m["fn"] == 0


# ---- lesion_table, lesion_metrics -----------------------------------------------------------
def test_lesion_table_rows():
    predict = _predict()
    m = np.zeros((4, 6, 8), np.uint8)
    m[1:3, 1:3, 1:4] = 1   # 12 voxels
    m[3, 5, 5:8] = 1       # 3 voxels
    m[0, 5, 0] = 1         # 1 voxel, the smallest label
    p = np.full(m.shape, 0.25, np.float32)
    p[2, 2, 3] = 0.9
    p[3, 5, 6] = 0.7
    rows = predict.lesion_table(m, p, spacing=(3.0, 0.5, 0.5))
    assert [r["voxels"] for r in rows] == [12, 3, 1]
    big = rows[0]
    assert big["label"] == 1 + np.ravel_multi_index((1, 1, 1), m.shape) and big["volume"] == 12 * 0.75
    assert big["bbox"] == (1, 2, 1, 2, 1, 3) and big["centroid"] == (1.5, 1.5, 2.0)
    assert big["confidence"] == float(np.float32(0.9)) and big["peak_voxel"] == (2, 2, 3)
    assert rows[1]["peak_voxel"] == (3, 5, 6) and rows[2]["peak_voxel"] == (0, 5, 0)
    bare = predict.lesion_table(m)
    assert all(r["confidence"] is None and r["peak_voxel"] is None for r in bare)
    assert [r["label"] for r in bare] == [r["label"] for r in rows]
    # equal sizes: the smaller label first
    two = np.zeros((1, 1, 9), np.uint8)
    two[0, 0, [1, 2, 6, 7]] = 1
    assert [r["label"] for r in predict.lesion_table(two)] == [2, 7]
    assert predict.lesion_table(np.zeros((2, 2, 2), np.uint8)) == []
    with pytest.raises(ValueError):
        predict.lesion_table(m, spacing=(1.0, 0.0, 1.0))


def test_lesion_metrics_on_the_case_masks():
    predict = _predict()
    pred, ref = case_masks()
    p = prob(CASE_SHAPE, nan=False)
    m = predict.lesion_metrics(pred, ref, p, spacing=(3.0, 0.5, 0.5))
    lp, lr = predict.label_components(pred), predict.label_components(ref)
    expect = predict.match_lesions(predict.component_table(lp), predict.component_table(lr),
                                   predict.overlap_pairs(lp, lr))
    for k, v in expect.items():
        assert m[k] == v or (isinstance(v, float) and math.isnan(v) and math.isnan(m[k])), k
    assert m["ref_lesions"] == predict.lesion_table(ref, None, (3.0, 0.5, 0.5))
    bare = [{k: v for k, v in row.items() if k != "matched_ref"} for row in m["pred_lesions"]]
    assert bare == predict.lesion_table(pred, p, (3.0, 0.5, 0.5))
    matched = {row["label"]: row["matched_ref"] for row in m["pred_lesions"]}
    assert {lp_: lr_ for lr_, lp_, *_ in m["matches"]} == {k: v for k, v in matched.items() if v is not None}
    assert m["tp"] + m["fp"] == m["n_pred"] == len(m["pred_lesions"])
    assert m["tp"] + m["fn"] == m["n_ref"] == len(m["ref_lesions"])
    from pcms_amd.utils.metrics import calculate_lesion_metrics
    assert calculate_lesion_metrics(pred[None], ref[None], (3.0, 0.5, 0.5))["matches"] == m["matches"]


# ---- the masks are what they claim ----------------------------------------------------------
def test_the_masks_are_what_they_claim():
    predict = _predict()
    for shape in BIG:
        for connectivity in (6, 18, 26):
            lab = labels(f"bernoulli{connectivity}", shape, connectivity)
            assert len(np.unique(lab[lab > 0])) >= 100, (shape, connectivity)
        board = mask("checkerboard", shape)
        assert len(np.unique(labels("checkerboard", shape, 6))) - 1 == int(board.sum()) >= board.size // 2
        snake = predict.component_table(labels("serpentine", shape, 6))
        assert len(snake["label"]) == 1
        assert snake["bbox"][0].tolist() == [0, (shape[0] - 1) // 2 * 2, 0, (shape[1] - 1) // 2 * 2, 0, shape[2] - 1]
    for shape in SHAPES:
        assert len(predict.component_table(labels("ones", shape, 26))["label"]) == 1
    p = prob(CASE_SHAPE)
    for v in (np.inf, -np.inf):
        assert (p == v).any()
    assert np.isnan(p).any() and (p < 0).any()
    assert (p == 0).any() and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()
    pred, ref = case_masks()
    lp, lr = predict.label_components(pred), predict.label_components(ref)
    pairs = predict.overlap_pairs(lp, lr)
    assert len(pairs) >= 20
    assert np.unique(pairs[:, 0], return_counts=True)[1].max() >= 2  # one prediction over two references
    m = predict.lesion_metrics(pred, ref)
    assert m["tp"] >= 1 and m["fp"] >= 1 and m["fn"] >= 1
    assert len(predict.component_table(lp)["label"]) >= 20
