"""pcms_window_gather / pcms_window_blend / pcms_window_finish against predict.py's host forms
(gather_windows, blend_windows), on the bits: the kernels restate the host arithmetic operation
for operation, so there is no tolerance.  Buffers a call must fully overwrite are NaN-filled
between two guard bands; the blend's accumulators start from zeros between guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_predict_ops import _Guarded
from tests.test_resample_ops import _same_bits

pytestmark = pytest.mark.gpu

FLIPS3 = ((2,), (0, 1))
FLIPS4 = ((2,), (0, 1), (0, 1, 2))
# name -> (volume, window, overlap)
GEOMETRIES = {
    "clipped": ((23, 37, 51), (16, 16, 32), 0.5),     # 24 windows, the last one clipped on every axis
    "abutting": ((23, 37, 51), (16, 16, 32), 0.0),    # 12 windows, overlap only where the last is clipped
    "scalar": ((23, 37, 51), (16, 16, 18), 0.5),      # ww % 4 != 0: the scalar store path
    "padded": ((12, 40, 40), (16, 32, 32), 0.5),      # the window sticks out past D
    "dense": ((20, 20, 36), (16, 16, 16), 0.75),      # step 4: 2 x 2 x 6 windows, up to 16 at a voxel
}


def _predict():
    import pcms_amd  # noqa: F401
    from pcms_amd import predict
    return predict


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _masks(flips):
    return [0] + [sum(1 << a for a in f) for f in flips]


@functools.lru_cache(maxsize=None)
def _volume(shape, C=5):
    return np.random.default_rng(40 + shape[0]).random((C,) + shape).astype(np.float32) + np.float32(0.5)


@functools.lru_cache(maxsize=None)
def _starts(name):
    shape, window, overlap = GEOMETRIES[name]
    return _predict().window_grid(shape, window, overlap)


def _gather(name, flips, offset=0, first=0, B=None):
    """pcms_window_gather of windows first .. first + B - 1 at the C ABI into a poisoned, guarded
    buffer ``offset`` floats off its 16-byte alignment."""
    L = _lib()
    shape, window, _ = GEOMETRIES[name]
    starts = _starts(name)
    B = len(starts) - first if B is None else B
    x = torch.from_numpy(_volume(shape)).to(DEV)
    sdev = torch.from_numpy(starts[first:first + B].copy()).to(DEV)
    masks = _masks(flips)
    n = B * len(masks) * x.shape[0] * int(np.prod(window))
    out = _Guarded(n + offset)
    assert out.out.data_ptr() % 16 == 0
    host = _ints(*masks)  # read during the call
    L.call("pcms_window_gather", x, *x.shape, sdev, B, ctypes.addressof(host), len(masks), *window,
           out.out.data_ptr() + 4 * offset)
    got = out.check()
    assert torch.isnan(got[:offset]).all(), "the floats before the output were written"
    got = got[offset:]
    assert not torch.isnan(got).any(), "an output element was not written"
    return got.view(B * len(masks), x.shape[0], *window)


@pytest.mark.parametrize("flips", [(), FLIPS3], ids=["k1", "k3"])
@pytest.mark.parametrize("name", ["clipped", "scalar", "padded"])
def test_gather_equals_host(name, flips):
    predict = _predict()
    shape, window, _ = GEOMETRIES[name]
    exp = predict.gather_windows(_volume(shape), _starts(name), window, flips)
    _same_bits(_gather(name, flips), exp, f"gather {name} k {1 + len(flips)}")
    if name == "padded":  # the zero padding, flipped with the window
        k = 1 + len(flips)
        assert not exp[::k, :, 12:].any() and exp[::k, :, :12].all()
        if flips:
            assert not exp[2::k, :, :4].any()


@pytest.mark.parametrize("name", ["clipped", "scalar"])
def test_gather_into_a_misaligned_output(name):
    """out one float past a 16-byte boundary: the scalar store path whatever ww is."""
    predict = _predict()
    shape, window, _ = GEOMETRIES[name]
    exp = predict.gather_windows(_volume(shape), _starts(name), window, FLIPS3)
    _same_bits(_gather(name, FLIPS3, offset=1), exp, f"gather {name} misaligned")


def test_gather_of_a_batch_and_the_python_form():
    predict = _predict()
    shape, window, _ = GEOMETRIES["clipped"]
    exp = predict.gather_windows(_volume(shape), _starts("clipped"), window, FLIPS3)
    _same_bits(_gather("clipped", FLIPS3, first=5, B=3), exp[15:24], "gather windows 5..7")
    got = predict.gather_windows_device(torch.from_numpy(_volume(shape)).to(DEV), _starts("clipped"), window, FLIPS3)
    _same_bits(got.cpu(), exp, "gather_windows_device")


@functools.lru_cache(maxsize=None)
def _probs(name, k):
    _, window, _ = GEOMETRIES[name]
    return np.random.default_rng(60 + k).random((len(_starts(name)) * k,) + window).astype(np.float32)


@pytest.mark.parametrize("blend", ["gaussian", "constant"])
@pytest.mark.parametrize("flips", [(), FLIPS4], ids=["k1", "k4"])
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_blend_and_finish_equal_host_for_every_batching(name, flips, blend):
    """blend_windows_device (pcms_window_blend per batch, pcms_window_finish) for B = 1, 3 and K
    windows per launch: each equal to the host form on the bits, hence to one another."""
    predict = _predict()
    shape, window, _ = GEOMETRIES[name]
    starts, k = _starts(name), 1 + len(flips)
    probs = _probs(name, k)
    weights = predict.window_weights(window, blend)
    exp = predict.blend_windows(probs, starts, window, weights, shape, flips)
    assert np.isfinite(exp).all()
    dev = torch.from_numpy(probs).to(DEV)
    for batch in (1, 3, len(starts)):
        got = predict.blend_windows_device(dev, starts, window, weights, shape, flips, batch=batch)
        _same_bits(got.cpu(), exp, f"blend {name} {blend} k {k} batch {batch}")


def test_dense_overlap_meets_many_windows():
    """The geometry the name promises: some voxel of 'dense' lies in 2 x 2 x 4 windows."""
    shape, window, _ = GEOMETRIES["dense"]
    count = np.zeros(shape, int)
    for sd, sh, sw in _starts("dense").tolist():
        count[sd:sd + 16, sh:sh + 16, sw:sw + 16] += 1
    assert count.max() == 16 and count.min() == 1


def test_blend_at_the_c_abi_writes_inside_the_volume_only():
    """acc / wsum between guard bands, reused across two launches (windows 0..1, then 2..3) on the
    geometry whose windows stick out; prob poisoned before the finish."""
    L = _lib()
    predict = _predict()
    shape, window, _ = GEOMETRIES["padded"]
    starts, flips = _starts("padded"), FLIPS3
    k, n, masks = 3, int(np.prod(shape)), _ints(*_masks(FLIPS3))
    probs = _probs("padded", k)
    weights = predict.window_weights(window)
    dev = torch.from_numpy(probs).to(DEV)
    sdev = torch.from_numpy(starts).to(DEV)
    wts = torch.from_numpy(np.concatenate(weights)).to(DEV)
    acc, wsum, prob = _Guarded(n, fill=0.0), _Guarded(n, fill=0.0), _Guarded(n)
    for first in (0, 2):
        L.call("pcms_window_blend", dev[first * k:(first + 2) * k], sdev, first, 2, ctypes.addressof(masks), k, wts,
               *window, acc.out, wsum.out, *shape)
    L.call("pcms_window_finish", acc.out, wsum.out, prob.out, n)
    acc.check(), wsum.check()
    got = prob.check()
    assert not torch.isnan(got).any(), "an output element was not written"
    _same_bits(got.view(*shape), predict.blend_windows(probs, starts, window, weights, shape, flips), "blend C ABI")


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4099])
@pytest.mark.parametrize("offsets", [(0, 0, 0), (1, 1, 1), (3, 3, 3), (0, 1, 0), (2, 2, 1)])
def test_finish_alignments(n, offsets):
    """The three pointers 16-byte aligned, off the boundary alike (scalar head, vector body,
    scalar tail) and off it differently (all scalar)."""
    L = _lib()
    rng = np.random.default_rng(n)
    acc, wsum = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32) + np.float32(0.25)
    bufs = []
    for src, off in ((acc, offsets[0]), (wsum, offsets[1])):
        t = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
        t[off:off + n] = torch.from_numpy(src).to(DEV)
        bufs.append((t, t.data_ptr() + 4 * off))
    prob = _Guarded(n + 4)
    L.call("pcms_window_finish", bufs[0][1], bufs[1][1], prob.out.data_ptr() + 4 * offsets[2], n)
    got = prob.check()
    o = offsets[2]
    assert torch.isnan(got[:o]).all() and torch.isnan(got[o + n:]).all(), "written outside the n elements"
    _same_bits(got[o:o + n], acc / wsum, f"finish n {n} offsets {offsets}")


def test_bad_arguments():
    L = _lib()
    lib = L.load()
    S = L.stream()
    x = torch.zeros(5 * 8 * 8 * 8, device=DEV)
    starts = torch.zeros(6, dtype=torch.int32, device=DEV)
    wts = torch.ones(48, device=DEV)
    out, acc, wsum, prob = _Guarded(4096), _Guarded(512), _Guarded(512), _Guarded(512)
    xp, sp, wp, o, a, w, p = (t.data_ptr() for t in (x, starts, wts, out.out, acc.out, wsum.out, prob.out))
    f1, f2 = _ints(0), _ints(0, 4)
    F1, F2 = ctypes.addressof(f1), ctypes.addressof(f2)
    bad = [_ints(1), _ints(0, 8), _ints(0, -1), _ints(*[0] * 9)]

    def gather(x=xp, C=1, D=8, H=8, W=8, starts=sp, B=2, fm=F1, k=1, wd=4, wh=4, ww=4, out=o):
        return lib.pcms_window_gather(x, C, D, H, W, starts, B, fm, k, wd, wh, ww, out, S)

    def blend(probs=xp, starts=sp, first=0, B=2, fm=F1, k=1, wts=wp, wd=4, wh=4, ww=4, acc=a, wsum=w, D=8, H=8, W=8):
        return lib.pcms_window_blend(probs, starts, first, B, fm, k, wts, wd, wh, ww, acc, wsum, D, H, W, S)

    for kw in [dict(x=None), dict(starts=None), dict(fm=None), dict(out=None),            # NULL pointers
               dict(x=xp + 2), dict(starts=sp + 2), dict(out=o + 1),                      # misaligned pointers
               dict(C=0), dict(D=0), dict(H=-1), dict(W=0), dict(B=0), dict(wd=0), dict(wh=0), dict(ww=-4),
               dict(k=0), dict(k=9, fm=ctypes.addressof(bad[3])),                         # k outside 1..8
               dict(fm=ctypes.addressof(bad[0])),                                         # flipmask[0] != 0
               dict(k=2, fm=ctypes.addressof(bad[1])), dict(k=2, fm=ctypes.addressof(bad[2])),
               dict(wd=513), dict(wh=513), dict(ww=516)]:                                 # a window axis above 512
        assert gather(**kw) < 0, kw
    for kw in [dict(probs=None), dict(starts=None), dict(fm=None), dict(wts=None), dict(acc=None), dict(wsum=None),
               dict(probs=xp + 2), dict(starts=sp + 1), dict(wts=wp + 3), dict(acc=a + 2), dict(wsum=w + 1),
               dict(first=-1), dict(B=0), dict(D=0), dict(H=0), dict(W=-2), dict(wd=0), dict(wh=-1), dict(ww=0),
               dict(k=0), dict(k=9, fm=ctypes.addressof(bad[3])), dict(fm=ctypes.addressof(bad[0])),
               dict(k=2, fm=ctypes.addressof(bad[1])), dict(k=2, fm=ctypes.addressof(bad[2])),
               dict(wd=513), dict(wh=513), dict(ww=513)]:
        assert blend(**kw) < 0, kw
    for args in [(None, w, p, 8), (a, None, p, 8), (a, w, None, 8), (a + 2, w, p, 8), (a, w + 1, p, 8),
                 (a, w, p + 3, 8), (a, w, p, 0), (a, w, p, -4)]:
        assert lib.pcms_window_finish(*args, S) < 0, args
    for g in (out, acc, wsum, prob):
        g.check(written=False)
    # the same tables accept a good call: k = 2 with a W flip
    assert gather(k=2, fm=F2) == 0 and blend(B=1, k=2, fm=F2, acc=a, wsum=w) == 0
    torch.cuda.synchronize()
