"""pcms_components_label / pcms_mask_postprocess at the C ABI against predict.py's host forms
(label_components, postprocess), on the bytes: canonical labels are a function of the mask alone,
so there is no tolerance and two runs must agree.  Outputs sit between guard bands and work[0]
(the kernels' iteration-cap status) must read 0 after every call.

The labelling kernel works on 8 x 16 x 32 (D x H x W) tiles: 9x17x33 is one voxel past the tile on
every axis (8 tiles), 24x40x48 has 3 x 3 x 2 tiles, 1x1x257 nine along W."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_predict_ops import _Guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 257), (3, 5, 7), (9, 17, 33), (24, 40, 48)]
BIG = [(9, 17, 33), (24, 40, 48)]
CONNECTIVITIES = (6, 18, 26)
BERNOULLI = {6: 0.30, 18: 0.15, 26: 0.10}  # below each connectivity's percolation threshold


def _predict():
    import pcms_amd  # noqa: F401
    from pcms_amd import predict
    return predict


# ---- masks ---------------------------------------------------------------------------------
def _serpentine(shape):
    """A one-voxel-wide 6-connected path: every other row of every other plane, rows joined at
    alternating W ends, planes joined through the odd plane between them at alternating corners."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    rows = list(range(0, H, 2))
    m[::2, ::2, :] = 1
    right = True  # the walk starts at w = 0, so the first row ends (and joins the next) at w = W - 1
    for k, d in enumerate(range(0, D, 2)):
        order = rows if k % 2 == 0 else rows[::-1]
        for a, b in zip(order, order[1:]):
            m[d, min(a, b):max(a, b) + 1, W - 1 if right else 0] = 1
            right = not right
        if d + 2 < D:  # on through the odd plane where this plane's last row ends
            m[d:d + 3, order[-1], W - 1 if right else 0] = 1
            right = not right
    return m


def _comb(shape):
    """Teeth along W in every other row of every other plane, joined only at w = W - 1 (the far
    end in scan order) by a back plate."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    m[::2, ::2, :] = 1
    m[:, :, W - 1] = 1
    return m


def _box(shape, kind):
    """A hollow box with one-voxel walls one voxel inside the volume ('box'); with a straight
    one-voxel channel from the cavity to the W = 0 face ('channel'); with the wall's first corner
    removed, which touches the cavity diagonally only ('diagonal')."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    m[1:D - 1, 1:H - 1, 1:W - 1] = 1
    m[2:D - 2, 2:H - 2, 2:W - 2] = 0
    if kind == "channel":
        m[D // 2, H // 2, :2] = 0
    if kind == "diagonal":
        m[1, 1, 1] = 0
    return m


@functools.lru_cache(maxsize=None)
def _mask(pattern, shape, seed=0):
    d, h, w = np.indices(shape)
    if pattern == "zeros":
        return np.zeros(shape, np.uint8)
    if pattern == "ones":
        return np.full(shape, 255, np.uint8)  # foreground is != 0
    if pattern == "checkerboard":
        return ((d + h + w) % 2 == 0).astype(np.uint8)
    if pattern == "serpentine":
        return _serpentine(shape)
    if pattern == "comb":
        return _comb(shape)
    if pattern == "giant":
        return (np.random.default_rng(500 + seed).random(shape) < 0.5).astype(np.uint8)
    if pattern.startswith("bernoulli"):
        p = BERNOULLI[int(pattern[len("bernoulli"):])]
        # a seed at which every one of them has >= 100 components, the largest well under half the
        # foreground (test_the_patterns_are_what_they_claim): p sits near the percolation threshold
        rng = np.random.default_rng(610 + seed + shape[0])
        return ((rng.random(shape) < p) * rng.integers(1, 256, size=shape)).astype(np.uint8)
    return _box(shape, pattern)


@functools.lru_cache(maxsize=None)
def _host_labels(pattern, shape, connectivity, invert):
    m = _mask(pattern, shape)
    return _predict().label_components((m == 0) if invert else m, connectivity)


def _components(labels):
    """(count, size of the largest) of a canonical label volume."""
    sizes = np.unique(labels[labels > 0], return_counts=True)[1]
    return len(sizes), int(sizes.max()) if len(sizes) else 0


# ---- device calls --------------------------------------------------------------------------
def _work(shape):
    n = _lib().query("pcms_components_work_ints", *shape)
    assert n >= 2 * int(np.prod(shape))
    return _Guarded(n, torch.int32, 0x5A5A5A5A)


def _device_labels(mask, connectivity, invert):
    """Two runs on fresh buffers; the labels of the first after checking both agree."""
    L = _lib()
    runs = []
    dev = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    for _ in range(2):
        labels, work = _Guarded(mask.size, torch.int32, -7), _work(mask.shape)
        L.call("pcms_components_label", dev, int(invert), connectivity, labels.out, work.out, *mask.shape)
        assert int(work.check()[0]) == 0, "a labelling kernel hit its iteration cap"
        runs.append(labels.check().view(*mask.shape).numpy())
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    return runs[0]


def _device_post(mask, keep, min_voxels, fill, connectivity):
    L = _lib()
    runs = []
    dev = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    before = dev.clone()
    for _ in range(2):
        out, work = _Guarded(mask.size, torch.uint8, 0xAB), _work(mask.shape)
        L.call("pcms_mask_postprocess", dev, out.out, work.out, keep, min_voxels, int(fill), connectivity, *mask.shape)
        assert int(work.check()[0]) == 0, "a labelling kernel hit its iteration cap"
        runs.append(out.check().view(*mask.shape).numpy())
    assert torch.equal(dev, before), "the input mask was written"
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    assert set(np.unique(runs[0])) <= {0, 1}, "an output byte was not written"
    return runs[0]


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    assert np.array_equal(got, exp), f"{what}: {int((got != exp).sum())} of {got.size} voxels differ"


# ---- labels --------------------------------------------------------------------------------
PATTERNS = ["zeros", "ones", "checkerboard", "serpentine", "comb", "giant", "bernoulli6", "bernoulli18",
            "bernoulli26"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_labels_equal_host(shape, pattern):
    mask = _mask(pattern, shape)
    for connectivity in CONNECTIVITIES:
        for invert in (0, 1):
            exp = _host_labels(pattern, shape, connectivity, invert)
            _same(_device_labels(mask, connectivity, invert), exp, f"{pattern} {shape} c{connectivity} inv{invert}")


def test_the_patterns_are_what_they_claim():
    """Host-side facts the cases above rely on, so that none degenerates."""
    for shape in BIG:
        n = int(np.prod(shape))
        for connectivity in CONNECTIVITIES:
            lab = _host_labels(f"bernoulli{connectivity}", shape, connectivity, 0)
            count, largest = _components(lab)
            assert count >= 100 and 2 * largest < int((lab > 0).sum()), (shape, connectivity, count, largest)
        count, largest = _components(_host_labels("giant", shape, 26, 0))
        assert 2 * largest > int(_mask("giant", shape).sum())  # p = 0.5 percolates at 26: one giant component
        board = _mask("checkerboard", shape)
        assert _components(_host_labels("checkerboard", shape, 6, 0)) == (int(board.sum()), 1)
        assert _components(_host_labels("checkerboard", shape, 18, 0))[0] == 1
        assert _components(_host_labels("checkerboard", shape, 26, 0))[0] == 1
        snake = _mask("serpentine", shape)
        assert _components(_host_labels("serpentine", shape, 6, 0)) == (1, int(snake.sum()))
        assert n // 5 <= int(snake.sum()) <= n // 3
        # a path: two ends with one neighbour, every other voxel with two
        pad = np.pad(snake, 1).astype(np.int32)
        nb = sum(np.roll(pad, s, a) for a in range(3) for s in (-1, 1))[1:-1, 1:-1, 1:-1][snake != 0]
        assert sorted(np.unique(nb, return_counts=True)[1].tolist())[0] == 2 and set(np.unique(nb)) == {1, 2}
        comb = _mask("comb", shape)
        assert _components(_host_labels("comb", shape, 6, 0))[0] == 1
        assert _components(_predict().label_components(comb[:, :, :-1], 6))[0] > 10  # the teeth join only there


# ---- post-processing -----------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("shape", BIG)
def test_postprocess_parameter_grid(shape, connectivity):
    predict = _predict()
    pattern = f"bernoulli{connectivity}"
    mask = _mask(pattern, shape)
    binary = (mask != 0).astype(np.uint8)
    for keep in (0, 1, 2, 8):
        for min_voxels in (0, 4):
            filtered = predict.filter_components(mask, keep, min_voxels, connectivity)
            if keep or min_voxels:  # a filtering case removes something and keeps something
                assert filtered.any() and not np.array_equal(filtered, binary)
                assert _components(predict.label_components(filtered, connectivity))[0] >= 1
            for fill in (False, True):
                exp = predict.postprocess(mask, keep, min_voxels, fill, connectivity)
                _same(_device_post(mask, keep, min_voxels, fill, connectivity), exp,
                      f"{pattern} {shape} keep {keep} min {min_voxels} fill {fill}")


@pytest.mark.parametrize("pattern", ["zeros", "ones", "checkerboard", "serpentine", "comb", "giant"])
@pytest.mark.parametrize("shape", SHAPES)
def test_postprocess_patterns(shape, pattern):
    predict = _predict()
    mask = _mask(pattern, shape)
    for connectivity in CONNECTIVITIES:
        for keep, min_voxels, fill in ((1, 4, True), (2, 0, False), (0, 4, False), (0, 1, True), (0, 0, False)):
            exp = predict.postprocess(mask, keep, min_voxels, fill, connectivity)
            _same(_device_post(mask, keep, min_voxels, fill, connectivity), exp,
                  f"{pattern} {shape} c{connectivity} keep {keep} min {min_voxels} fill {fill}")


@pytest.mark.parametrize("shape", [(9, 17, 33), (24, 40, 48), (5, 6, 7)])
def test_hole_filling(shape):
    predict = _predict()
    solid = np.zeros(shape, np.uint8)
    solid[1:shape[0] - 1, 1:shape[1] - 1, 1:shape[2] - 1] = 1
    box, channel, diagonal = (_mask(kind, shape) for kind in ("box", "channel", "diagonal"))
    open_corner = solid.copy()
    open_corner[1, 1, 1] = 0
    for connectivity in CONNECTIVITIES:
        _same(_device_post(box, 0, 0, True, connectivity), solid, f"box {shape}")
        _same(_device_post(channel, 0, 0, True, connectivity), channel, f"channel {shape}")
        # the background is 6-connected whatever the foreground's connectivity: a diagonal leak fills
        _same(_device_post(diagonal, 0, 0, True, connectivity), open_corner, f"diagonal {shape}")
        for m in (box, channel, diagonal):
            _same(_device_post(m, 1, 0, True, connectivity), predict.postprocess(m, 1, 0, True, connectivity), "host")
    assert np.array_equal(predict.fill_holes(box), solid) and np.array_equal(predict.fill_holes(channel), channel)
    assert np.array_equal(predict.fill_holes(diagonal), open_corner)


def test_tie_across_tiles():
    """Two blobs of 8 voxels in different tiles and a smaller third: keep_largest=1 keeps the one
    with the smaller label; moved so that the other comes first in scan order, it keeps that one."""
    predict = _predict()
    shape = (24, 40, 48)
    for first, second in (((1, 1, 1), (20, 30, 40)), ((1, 30, 40), (20, 1, 1)), ((9, 17, 33), (9, 17, 2))):
        mask = np.zeros(shape, np.uint8)
        for d, h, w in (first, second):
            mask[d:d + 2, h:h + 2, w:w + 2] = 1
        mask[12, 20, 20:23] = 1
        flat = [np.ravel_multi_index(c, shape) for c in (first, second)]
        winner = (first, second)[int(np.argmin(flat))]
        tile = [(d // 8, h // 16, w // 32) for d, h, w in (first, second)]
        assert tile[0] != tile[1]
        exp = np.zeros(shape, np.uint8)
        exp[winner[0]:winner[0] + 2, winner[1]:winner[1] + 2, winner[2]:winner[2] + 2] = 1
        for connectivity in CONNECTIVITIES:
            assert np.array_equal(predict.postprocess(mask, 1, 0, False, connectivity), exp)
            _same(_device_post(mask, 1, 0, False, connectivity), exp, f"tie {first} {second} c{connectivity}")
            two = _device_post(mask, 2, 0, False, connectivity)
            assert int(two.sum()) == 16 and not two[12, 20, 20:23].any()


def test_bad_arguments():
    L = _lib()
    lib = L.load()
    S = L.stream()
    shape = (3, 5, 7)
    n = int(np.prod(shape))
    src = torch.ones(n, dtype=torch.uint8, device=DEV)
    out = _Guarded(n, torch.uint8, 0xAB)
    labels = _Guarded(n, torch.int32, -7)
    work = _work(shape)
    m, o, lb, wk = (t.data_ptr() for t in (src, out.out, labels.out, work.out))
    assert lib.pcms_components_work_ints(0, 5, 7) < 0 and lib.pcms_components_work_ints(1025, 1024, 1024) < 0
    for args in [(None, 0, 26, lb, wk, *shape),          # NULL mask
                 (m, 0, 26, None, wk, *shape),           # NULL labels
                 (m, 0, 26, lb, None, *shape),           # NULL work
                 (m, 0, 26, lb + 2, wk, *shape),         # misaligned labels
                 (m, 0, 26, lb, wk + 1, *shape),         # misaligned work
                 (m, 0, 8, lb, wk, *shape),              # no such connectivity
                 (m, 0, 0, lb, wk, *shape),
                 (m, 0, 27, lb, wk, *shape),
                 (m, 0, 26, lb, wk, 0, 5, 7),            # empty volume
                 (m, 0, 26, lb, wk, 3, -5, 7),
                 (m, 0, 26, lb, wk, 1025, 1024, 1024)]:  # more than 2^30 voxels
        assert lib.pcms_components_label(*args, S) < 0, args
    for args in [(None, o, wk, 1, 0, 1, 26, *shape),
                 (m, None, wk, 1, 0, 1, 26, *shape),
                 (m, o, None, 1, 0, 1, 26, *shape),
                 (m, o, wk + 2, 1, 0, 1, 26, *shape),    # misaligned work
                 (m, o, wk, 1, 0, 1, 4, *shape),         # no such connectivity
                 (m, o, wk, -1, 0, 1, 26, *shape),       # keep_largest outside 0..8
                 (m, o, wk, 9, 0, 1, 26, *shape),
                 (m, o, wk, 1, -1, 1, 26, *shape),       # min_voxels < 0
                 (m, o, wk, 1, 0, 1, 26, 3, 5, 0),
                 (m, o, wk, 1, 0, 1, 26, 2048, 2048, 2048),
                 (o, o, wk, 1, 0, 1, 26, *shape),        # out aliases mask
                 (o + 1, o, wk, 1, 0, 1, 26, 1, 1, n - 1)]:  # ... or overlaps it
        assert lib.pcms_mask_postprocess(*args, S) < 0, args
    for g in (out, labels, work):
        g.check(written=False)
    assert bool((src == 1).all())
