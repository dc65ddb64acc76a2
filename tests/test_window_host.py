"""The host forms of sliding-window prediction (predict.window_starts / window_grid /
window_weights / gather_windows / blend_windows / sliding_window_predict): the window geometry
against its stated properties, the blend against a float64 weighted mean built here by direct
slicing, and the driver against a pointwise function of the whole volume, which pins starts,
padding, un-flip and tail padding without reference to the implementation.

The 1e-6 bar is derived, not measured: at overlap 0.5 at most 8 windows meet at a voxel, so a
voxel sees at most 8 fp32 products, 8 + 8 sums and one quotient; all terms are positive, so the
result carries at most about 13 relative roundings of 2^-24 on a value <= 1: 7.7e-7."""
import math

import numpy as np
import pytest

import pcms_amd  # noqa: F401
from pcms_amd import predict

BAR = 1e-6
FLIP_CASES = [(), ((2,), (0, 1))]


@pytest.mark.parametrize("overlap", [0.0, 0.5, 0.75, 0.95])
@pytest.mark.parametrize("w", [1, 4, 16, 32])
def test_window_starts_properties(w, overlap):
    """n below, at and just past the window, and longer runs; overlap 0.95 makes step 1 for
    every w here (int(32 * 0.05) = 1)."""
    step = max(1, int(w * (1.0 - overlap)))
    if overlap == 0.95:
        assert step == 1
    for n in sorted({1, max(1, w - 1), w, w + 1, w + step, 2 * w + 3, 5 * w + 7, 97}):
        starts = predict.window_starts(n, w, overlap)
        count = 1 if n <= w else math.ceil((n - w) / step) + 1
        assert len(starts) == count, (n, w, overlap)
        assert starts[0] == 0 and starts[-1] == max(0, n - w)
        assert all(b > a for a, b in zip(starts, starts[1:])), (n, w, overlap, starts)
        covered = np.zeros(n, bool)
        for s in starts:
            covered[s:s + w] = True
        assert covered.all(), (n, w, overlap, starts)


def test_window_starts_pinned_and_rejected():
    assert predict.window_starts(23, 16, .5) == [0, 7]
    assert predict.window_starts(37, 16, .5) == [0, 8, 16, 21]
    assert predict.window_starts(51, 32, .5) == [0, 16, 19]
    assert predict.window_starts(12, 16, .5) == [0]
    for n, w, o in ((0, 16, .5), (16, 0, .5), (16, 16, 1.0), (16, 16, -0.1), (16, 16, float("nan"))):
        with pytest.raises(ValueError):
            predict.window_starts(n, w, o)


def test_window_grid_is_the_d_major_product():
    grid = predict.window_grid((23, 37, 51), (16, 16, 32), 0.5)
    assert grid.dtype == np.int32 and grid.shape == (24, 3)
    exp = [(a, b, c) for a in (0, 7) for b in (0, 8, 16, 21) for c in (0, 16, 19)]
    assert grid.tolist() == [list(r) for r in exp]
    per_axis = predict.window_grid((23, 37, 51), (16, 16, 32), (0.0, 0.5, 0.75))
    exp = [(a, b, c) for a in predict.window_starts(23, 16, 0.0) for b in predict.window_starts(37, 16, 0.5)
           for c in predict.window_starts(51, 32, 0.75)]
    assert per_axis.tolist() == [list(r) for r in exp]
    assert predict.window_grid((12, 40, 40), (16, 32, 32), 0.5).tolist() == \
        [[0, 0, 0], [0, 0, 8], [0, 8, 0], [0, 8, 8]]
    with pytest.raises(ValueError):
        predict.window_grid((23, 37), (16, 16, 32), 0.5)


@pytest.mark.parametrize("window", [(16, 16, 32), (5, 8, 17)])
def test_window_weights(window):
    vecs = predict.window_weights(window)
    assert len(vecs) == 3
    for v, w in zip(vecs, window):
        assert v.dtype == np.float32 and v.shape == (w,)
        assert np.array_equal(v, v[::-1])
        assert v.max() == v[w // 2] == v[(w - 1) // 2] and (v > 0).all()
        i = np.arange(w, dtype=np.float64)
        exp = np.exp(-0.5 * ((i - (w - 1) / 2) / (0.125 * w)) ** 2).astype(np.float32)
        assert np.array_equal(v.view(np.int32), exp.view(np.int32))
    wide = predict.window_weights(window, sigma_scale=0.25)
    assert all((a >= b).all() and (a > b).any() for a, b in zip(wide, vecs))
    for v, w in zip(predict.window_weights(window, "constant"), window):
        assert v.dtype == np.float32 and np.array_equal(v, np.ones(w, np.float32))
    with pytest.raises(ValueError):
        predict.window_weights(window, "linear")


def test_gather_windows_entries():
    rng = np.random.default_rng(5)
    x = rng.random((2, 12, 40, 40)).astype(np.float32) + 1.0  # no zero inside the volume
    starts = predict.window_grid(x.shape[1:], (16, 32, 32), 0.5)
    flips = ((2,), (0, 1))
    out = predict.gather_windows(x, starts, (16, 32, 32), flips)
    assert out.shape == (12, 2, 16, 32, 32) and out.dtype == np.float32
    for i, (sd, sh, sw) in enumerate(starts.tolist()):
        win = out[3 * i]
        assert np.array_equal(win[:, :12], x[:, :, sh:sh + 32, sw:sw + 32]) and not win[:, 12:].any()
        assert np.array_equal(out[3 * i + 1], win[:, :, :, ::-1])
        assert np.array_equal(out[3 * i + 2], win[:, ::-1, ::-1, :])
        assert not out[3 * i + 2][:, :4].any()  # the padding is flipped with the window
    with pytest.raises(ValueError):
        predict.gather_windows(x, starts, (16, 32, 32), ((3,),))
    with pytest.raises(ValueError):
        predict.gather_windows(x, np.array([[0, 0, 40]]), (16, 32, 32))


def _blend64(probs, starts, window, weights, shape, flips):
    """The weighted mean in float64, the fp32 weights taken as given."""
    k = 1 + len(flips)
    wgt = np.einsum("a,b,c->abc", *(v.astype(np.float64) for v in weights))
    num, den = np.zeros(shape), np.zeros(shape)
    for i, (sd, sh, sw) in enumerate(np.asarray(starts).tolist()):
        m = probs[i * k].astype(np.float64)
        for j, f in enumerate(flips, start=1):
            m = m + np.flip(probs[i * k + j].astype(np.float64), f)
        m = m / k
        nd, nh, nw = (min(w, n - s) for w, n, s in zip(window, shape, (sd, sh, sw)))
        num[sd:sd + nd, sh:sh + nh, sw:sw + nw] += (wgt * m)[:nd, :nh, :nw]
        den[sd:sd + nd, sh:sh + nh, sw:sw + nw] += wgt[:nd, :nh, :nw]
    return num / den


@pytest.mark.parametrize("blend", ["gaussian", "constant"])
@pytest.mark.parametrize("flips", FLIP_CASES)
def test_blend_windows_against_float64(flips, blend):
    shape, window = (23, 37, 51), (16, 16, 32)
    starts = predict.window_grid(shape, window, 0.5)
    assert len(starts) == 24
    k = 1 + len(flips)
    probs = np.random.default_rng(11 + k).random((24 * k,) + window).astype(np.float32)
    weights = predict.window_weights(window, blend)
    got = predict.blend_windows(probs, starts, window, weights, shape, flips)
    assert got.dtype == np.float32 and got.shape == shape
    exp = _blend64(probs, starts, window, weights, shape, flips)
    err = float(np.abs(got.astype(np.float64) - exp).max())
    print(f"blend {blend} flips {flips}: max abs error {err:.3e}")
    assert err <= BAR
    if flips:  # the un-flip matters
        plain = predict.blend_windows(probs[::k], starts, window, weights, shape)
        assert float(np.abs(plain - got).max()) > 1e-3


def _pointwise(batch):
    batch = np.asarray(batch)
    return np.clip(np.float32(0.25) + np.float32(0.5) * batch[:, :1], 0, 1).astype(np.float32)


@pytest.mark.parametrize("flips", FLIP_CASES)
def test_sliding_window_predict_of_a_pointwise_function(flips):
    """A pointwise predict_fn commutes with cutting, flipping and blending: the blended result is
    the function of the whole volume.  D = 12 is below the window: the padded part is dropped."""
    x = np.random.default_rng(12).random((5, 12, 40, 40)).astype(np.float32)
    x[0, 3:9, 10:30, 5:25] *= 2.0  # part of the volume clips at 1
    window, seen = (16, 32, 32), []

    def fn(batch):
        seen.append(batch.shape)
        return _pointwise(batch)

    exp = _pointwise(x[None])[0, 0].astype(np.float64)
    assert float(exp.max()) == 1.0 and float(exp.min()) < 0.3
    results = {}
    for wb in (1, 3, 4):  # K = 4
        seen.clear()
        got = predict.sliding_window_predict(fn, x, window, 0.5, "gaussian", flips, wb)
        k = 1 + len(flips)
        assert seen == [(wb * k, 5) + window] * math.ceil(4 / wb)
        assert got.dtype == np.float32 and got.shape == x.shape[1:]
        err = float(np.abs(got.astype(np.float64) - exp).max())
        print(f"sliding flips {flips} window_batch {wb}: max abs error {err:.3e}")
        assert err <= BAR
        results[wb] = got.tobytes()
    assert results[1] == results[3] == results[4]
    with pytest.raises(ValueError):
        predict.sliding_window_predict(lambda b: _pointwise(b)[:-1], x, window, 0.5, "gaussian", flips, 2)
    with pytest.raises(ValueError):
        predict.sliding_window_predict(fn, x, window, 1.0)
    with pytest.raises(ValueError):
        predict.sliding_window_predict(fn, x, window, 0.5, "gaussian", (), 0)


def test_device_forms_need_a_gpu():
    import torch
    x = torch.zeros((1, 5, 16, 16, 16))
    w = predict.window_weights((16, 16, 16))
    for call in (lambda: predict.gather_windows_device(x[0], [[0, 0, 0]], (16, 16, 16)),
                 lambda: predict.blend_windows_device(x[0, :1], [[0, 0, 0]], (16, 16, 16), w, (16, 16, 16)),
                 lambda: predict.sliding_window_device(lambda b: b[:, :1], x, (16, 16, 16))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
