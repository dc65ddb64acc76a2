"""predict.py's mask post-processing host forms (label_components, filter_components, fill_holes,
postprocess: the oracle of the device kernels) and the host workspace query.  No GPU."""
import itertools

import numpy as np
import pytest

import pcms_amd  # noqa: F401
from pcms_amd import _lib, predict

CONNECTIVITIES = (6, 18, 26)


def flood_labels(mask, connectivity):
    """1 + the smallest flat index of each foreground voxel's component, by a pure-Python flood
    fill seeded in scan order (the seed of a component is then its smallest index)."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(v != 0 for v in o) <= most]
    D, H, W = mask.shape
    lab = np.zeros(mask.shape, np.int32)
    for seed in range(mask.size):
        d, h, w = np.unravel_index(seed, mask.shape)
        if mask[d, h, w] == 0 or lab[d, h, w]:
            continue
        lab[d, h, w] = seed + 1
        stack = [(d, h, w)]
        while stack:
            cd, ch, cw = stack.pop()
            for a, b, c in offs:
                nd, nh, nw = cd + a, ch + b, cw + c
                if 0 <= nd < D and 0 <= nh < H and 0 <= nw < W and mask[nd, nh, nw] != 0 and not lab[nd, nh, nw]:
                    lab[nd, nh, nw] = seed + 1
                    stack.append((nd, nh, nw))
    return lab


def _tiny_masks():
    rng = np.random.default_rng(11)
    for shape in [(1, 1, 1), (1, 1, 7), (2, 3, 4), (3, 5, 7)]:
        for p in (0.1, 0.25, 0.5, 0.8):
            yield (rng.random(shape) < p).astype(np.uint8) * rng.integers(1, 255, size=shape).astype(np.uint8)
        yield np.zeros(shape, np.uint8)
        yield np.ones(shape, np.uint8)
        d, h, w = np.indices(shape)
        yield ((d + h + w) % 2 == 0).astype(np.uint8)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_label_components_against_flood_fill(connectivity):
    several = 0
    for mask in _tiny_masks():
        got = predict.label_components(mask, connectivity)
        exp = flood_labels(mask, connectivity)
        assert got.dtype == np.int32 and got.shape == mask.shape
        assert np.array_equal(got, exp), (mask.shape, connectivity)
        several += len(np.unique(exp)) > 2
    assert several >= 3  # the masks are not all one blob


def test_checkerboard_depends_on_connectivity():
    d, h, w = np.indices((3, 5, 7))
    board = ((d + h + w) % 2 == 0).astype(np.uint8)
    six = predict.label_components(board, 6)
    assert np.array_equal(six[board != 0], np.flatnonzero(board) + 1)  # every voxel on its own
    for connectivity in (18, 26):
        assert set(np.unique(predict.label_components(board, connectivity))) == {0, 1}


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_label_ranks_are_scipy_labels(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    rng = np.random.default_rng(12)
    for shape, p in [((3, 5, 7), 0.4), ((9, 17, 33), 0.2), ((12, 20, 24), 0.12)]:
        mask = (rng.random(shape) < p).astype(np.uint8)
        lab = predict.label_components(mask, connectivity)
        ref, count = ndi.label(mask, structure)
        distinct = np.unique(lab[lab > 0])
        assert len(distinct) == count
        rank = np.where(lab > 0, np.searchsorted(distinct, lab) + 1, 0)
        assert np.array_equal(rank, ref)


def test_fill_holes_is_scipy_binary_fill_holes():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(13)
    filled_some = False
    for shape, p in [((3, 5, 7), 0.6), ((9, 17, 33), 0.7), ((12, 20, 24), 0.8)]:
        mask = (rng.random(shape) < p).astype(np.uint8)
        got = predict.fill_holes(mask)
        assert got.dtype == np.uint8
        assert np.array_equal(got, ndi.binary_fill_holes(mask).astype(np.uint8))
        filled_some |= bool((got != mask).any())
    assert filled_some


def _box(shape=(7, 8, 9)):
    box = np.zeros(shape, np.uint8)
    box[1:6, 1:7, 1:8] = 1
    box[2:5, 2:6, 2:7] = 0
    return box


def test_fill_holes_box_channel_and_diagonal():
    box = _box()
    solid = box.copy()
    solid[2:5, 2:6, 2:7] = 1
    assert np.array_equal(predict.fill_holes(box), solid)
    channel = box.copy()
    channel[3, 3, :3] = 0  # a straight one-voxel channel to the W = 0 face
    assert np.array_equal(predict.fill_holes(channel), channel)
    diagonal = box.copy()
    diagonal[1, 1, 1] = 0  # the wall's corner: open to the outside, it touches the cavity's corner
    expect = solid.copy()  # (2, 2, 2) diagonally only, and the background is 6-connected: still filled
    expect[1, 1, 1] = 0
    assert np.array_equal(predict.fill_holes(diagonal), expect)
    assert np.array_equal(predict.fill_holes(5 * box), solid)  # foreground is != 0


def test_tie_resolves_to_the_smaller_label():
    mask = np.zeros((3, 5, 7), np.uint8)
    mask[0, 0, 0:3] = 1
    mask[2, 4, 4:7] = 1
    mask[1, 2, 3] = 1
    only_first = np.zeros_like(mask)
    only_first[0, 0, 0:3] = 1
    for connectivity in CONNECTIVITIES:
        assert np.array_equal(predict.filter_components(mask, keep_largest=1, connectivity=connectivity), only_first)
        two = predict.filter_components(mask, keep_largest=2, connectivity=connectivity)
        assert two.sum() == 6 and two[1, 2, 3] == 0
        assert np.array_equal(predict.filter_components(mask, min_voxels=3), two)
        # the rank is over all components: the speck would be third, min_voxels removes nothing more
        assert np.array_equal(predict.postprocess(mask, keep_largest=3, min_voxels=2), two)


def test_identity_parameters():
    rng = np.random.default_rng(14)
    mask = (rng.random((3, 5, 7)) < 0.4) * rng.integers(1, 255, size=(3, 5, 7))
    mask = mask.astype(np.uint8)
    binary = (mask != 0).astype(np.uint8)
    for min_voxels in (0, 1):
        for connectivity in CONNECTIVITIES:
            got = predict.postprocess(mask, 0, min_voxels, False, connectivity)
            assert got.dtype == np.uint8 and np.array_equal(got, binary)
    assert np.array_equal(predict.filter_components(mask), binary)
    assert np.array_equal(predict.postprocess(mask, keep_largest=8, connectivity=26),
                          predict.filter_components(mask, keep_largest=8))


def test_argument_errors():
    mask = np.ones((2, 2, 2), np.uint8)
    for bad in (4, 8, 27, 0, None):
        with pytest.raises(ValueError):
            predict.label_components(mask, bad)
        with pytest.raises(ValueError):
            predict.postprocess(mask, connectivity=bad)
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError):
            predict.filter_components(mask, keep_largest=bad)
        with pytest.raises(ValueError):
            predict.postprocess(mask, keep_largest=bad)
    with pytest.raises(ValueError):
        predict.filter_components(mask, min_voxels=-1)
    with pytest.raises(ValueError):
        predict.label_components(np.ones((2, 2), np.uint8))
    with pytest.raises(ValueError):
        predict.fill_holes(np.ones((2, 0, 2), np.uint8))


def test_device_forms_refuse_cpu_tensors():
    import torch
    mask = torch.ones((2, 2, 2), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        predict.postprocess_device(mask, keep_largest=1)
    with pytest.raises(RuntimeError):
        predict.label_components_device(mask)


def test_workspace_query_without_gpu():
    q = lambda *shape: _lib.query("pcms_components_work_ints", *shape)  # noqa: E731
    assert q(1, 1, 1) > 0
    assert q(24, 384, 384) >= 2 * 24 * 384 * 384
    assert q(0, 4, 4) < 0 and q(4, 0, 4) < 0 and q(4, 4, 0) < 0 and q(-1, 4, 4) < 0
    assert q(1025, 1024, 1024) < 0      # more than 2^30 voxels
    assert q(2048, 2048, 2048) < 0      # 2^33: the product does not wrap into range
