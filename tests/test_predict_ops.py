"""pcms_volume_minmax / pcms_resample_linear_norm / pcms_flip_mean / pcms_prob_to_mask at the C
ABI against predict.py's host forms (normalise, tta_mean, mask_on_grid over data.resample), on
the bits: the kernels restate the host arithmetic operation for operation, so there is no
tolerance.  Outputs are NaN-filled (0xAB-filled for the byte mask) between two guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_resample_ops import CODES, GUARD, SHAPES, _decode, _same_bits, _typed_source

pytestmark = pytest.mark.gpu


def _mods():
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    return data, predict


def _code(dtype):
    return {np.dtype(v): k for k, v in _mods()[0]._NIFTI_DTYPES.items()}[np.dtype(dtype)]


class _Guarded:
    """n elements of ``dtype`` filled with ``fill`` between two guard bands."""

    def __init__(self, n, dtype=torch.float32, fill=float("nan")):
        self.n = n
        self.buf = torch.empty(GUARD + n + GUARD, dtype=dtype, device=DEV)
        self.buf[:GUARD] = 77
        self.buf[GUARD:GUARD + n] = fill
        self.buf[GUARD + n:] = 99
        self.before = self.buf.clone()
        self.out = self.buf[GUARD:GUARD + n]

    def check(self, written=True):
        torch.cuda.synchronize()
        got, ref = self.buf.view(torch.uint8), self.before.view(torch.uint8)
        e = self.buf.element_size()
        assert torch.equal(got[:GUARD * e], ref[:GUARD * e]) and torch.equal(got[-GUARD * e:], ref[-GUARD * e:]), \
            "guard overwritten"
        if not written:
            assert torch.equal(got, ref), "a rejected call wrote its output"
        return self.out.clone().cpu()


def _upload(src, offset=0):
    """src's bytes on the device, ``offset`` elements into a 16-byte-aligned allocation."""
    flat = np.ascontiguousarray(src).reshape(-1)
    pad = np.zeros(offset, flat.dtype)
    dev = torch.from_numpy(np.concatenate([pad, flat]).view(np.uint8).copy()).to(DEV)
    assert dev.data_ptr() % 16 == 0
    return dev, dev.data_ptr() + offset * flat.dtype.itemsize


def _minmax(src, slope=1.0, inter=0.0, offset=0):
    L = _lib()
    keep, ptr = _upload(src, offset)
    n = src.size
    nwork = L.query("pcms_volume_minmax_work_floats", n)
    assert nwork >= 2 and nwork % 2 == 0
    lohi, work = _Guarded(2), _Guarded(nwork)
    L.call("pcms_volume_minmax", ptr, _code(src.dtype), n, float(slope), float(inter), lohi.out, work.out)
    work.check()
    return lohi.check().numpy()


def _host_minmax(src, slope=1.0, inter=0.0):
    v = _decode(src, slope, inter).astype(np.float32)
    return np.array([v.min(), v.max()], np.float32)


def _same_lohi(got, exp, what):
    assert got.dtype == exp.dtype == np.float32
    assert np.array_equal(got.view(np.int32), exp.view(np.int32)), (what, got, exp)


@pytest.mark.parametrize("code", CODES)
def test_minmax_every_datatype(code):
    """Sizes around the 256-thread workgroup and the 16-byte vector, one element, two workgroups
    (4099) and many (70001); the pointer element-aligned but off the 16-byte boundary."""
    for n in (1, 255, 256, 257, 4099, 70001):
        src = _typed_source(code, (n,), 500 + code + n)
        _same_lohi(_minmax(src), _host_minmax(src), f"datatype {code} n {n}")
    src = _typed_source(code, (4099,), 600 + code)
    _same_lohi(_minmax(src, offset=1), _host_minmax(src), f"datatype {code} offset 1")
    _same_lohi(_minmax(src[:7], offset=1), _host_minmax(src[:7]), f"datatype {code} offset 1, all head")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 70001])
@pytest.mark.parametrize("where", ["first", "last"])
def test_minmax_extreme_at_the_ends(n, where):
    src = np.random.default_rng(n).integers(-1000, 1000, size=n).astype(np.int16)
    at = 0 if where == "first" else n - 1
    for extreme in (-30000, 30000):
        s = src.copy()
        s[at] = extreme
        exp = _host_minmax(s)
        assert extreme in exp
        _same_lohi(_minmax(s), exp, f"n {n} {where} {extreme}")
        _same_lohi(_minmax(s, offset=3), exp, f"n {n} {where} {extreme} offset 3")


def test_minmax_negative_slope_and_nan():
    """A negative scl_slope: the minimum comes from the raw maximum.  A NaN anywhere (vector body,
    head, tail, element 0) gives NaN for both, as numpy's min / max do."""
    src = np.random.default_rng(7).integers(-3000, 3000, size=4099).astype(np.int16)
    exp = _host_minmax(src, -0.37, 12.5)
    assert exp[0] == np.float32(src.max() * -0.37 + 12.5)
    _same_lohi(_minmax(src, -0.37, 12.5), exp, "negative slope")
    _same_lohi(_minmax(src, 0.0, 2.0), _host_minmax(src, 0.0, 2.0), "slope 0 means 1")
    for dtype in (np.float32, np.float64):
        for at in (0, 1, 2000, 4098):
            f = (100.0 * np.random.default_rng(8).standard_normal(4099)).astype(dtype)
            f[at] = np.nan
            got = _minmax(f, offset=1)
            assert np.isnan(got).all() and np.isnan(_host_minmax(f)).all(), (dtype, at, got)


def _norm(src, target, slope=1.0, inter=0.0):
    L = _lib()
    keep, ptr = _upload(src)
    n = src.size
    lohi = torch.empty(2, device=DEV)
    work = torch.empty(L.query("pcms_volume_minmax_work_floats", n), device=DEV)
    L.call("pcms_volume_minmax", ptr, _code(src.dtype), n, float(slope), float(inter), lohi, work)
    out = _Guarded(int(np.prod(target)))
    L.call("pcms_resample_linear_norm", ptr, _code(src.dtype), *src.shape, float(slope), float(inter), lohi, out.out,
           *target)
    got = out.check()
    assert not torch.isnan(got).any(), "an output element was not written"
    return got.view(*target)


def _norm_oracle(src, target, slope=1.0, inter=0.0):
    data, predict = _mods()
    return data.resample(predict.normalise(_decode(src, slope, inter)), target)


def _norm_source(kind, shape):
    rng = np.random.default_rng(700 + shape[0] * 31 + shape[1] * 7 + shape[2])
    if kind == "int16":
        return rng.integers(-3000, 3000, size=shape).astype(np.int16)
    if kind == "uint8":
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    return (1000.0 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("kind", ["int16", "uint8", "float32"])
@pytest.mark.parametrize("shape,target", SHAPES)
def test_norm_shapes(shape, target, kind):
    src = _norm_source(kind, shape)
    exp = _norm_oracle(src, target)
    if src.size > 1:  # not the den == 0 form: the values spread over [0, 1]
        assert float(exp.max()) > 0.5
    _same_bits(_norm(src, target), exp, f"norm {kind} {shape}->{target}")


@pytest.mark.parametrize("shape,target", SHAPES)
def test_norm_scaled_and_constant(shape, target):
    src = _norm_source("int16", shape)
    for slope, inter in ((0.5, -3.0), (-0.37, 12.5)):
        _same_bits(_norm(src, target, slope, inter), _norm_oracle(src, target, slope, inter),
                   f"norm scaled {slope} {inter} {shape}->{target}")
    zeros = np.zeros(shape, np.int16)
    got = _norm(zeros, target)
    _same_bits(got, _norm_oracle(zeros, target), f"norm zeros {shape}->{target}")
    assert not got.any()
    const = np.full(shape, 37, np.uint8)  # den == 0 with lo != 0
    _same_bits(_norm(const, target), np.zeros(target, np.float32), f"norm constant {shape}->{target}")


FLIP_SETS = [(), (2,), (0, 1), (0, 1, 2)]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_flip_mean(k):
    L = _lib()
    _, predict = _mods()
    shape = (5, 7, 9)
    probs = np.random.default_rng(800).random((4,) + shape).astype(np.float32)
    flips = FLIP_SETS[:k]
    masks = (ctypes.c_int * k)(*(sum(1 << a for a in f) for f in flips))
    out = _Guarded(int(np.prod(shape)))
    L.call("pcms_flip_mean", torch.from_numpy(probs[:k].copy()).to(DEV), k, ctypes.addressof(masks), out.out, *shape)
    exp = predict.tta_mean(list(probs[:k]), flips)
    if k > 1:
        assert not np.array_equal(exp, probs[:k].mean(0, dtype=np.float32))  # the flips matter
    _same_bits(out.check().view(*shape), exp, f"flip mean k {k}")


# target -> native, both directions of every shape pair (identity once).  A one-voxel native grid
# is left out: its mask is all 0 or all 1, which the fraction condition below rules out
MASK_PAIRS = [(a, b) for a, b in SHAPES] + [(b, a) for a, b in SHAPES if a != b and np.prod(a) > 1]


@functools.lru_cache(maxsize=None)
def _prob_case(shape):
    return np.random.default_rng(900 + shape[0] * 31 + shape[1] * 7 + shape[2]).random(shape).astype(np.float32)


@pytest.mark.parametrize("with_prob", [False, True])
@pytest.mark.parametrize("threshold", [0.5, 0.3])
@pytest.mark.parametrize("tgt,native", MASK_PAIRS)
def test_prob_to_mask(tgt, native, threshold, with_prob):
    L = _lib()
    _, predict = _mods()
    prob = _prob_case(tgt)
    exp_mask, exp_prob = predict.mask_on_grid(prob, native, threshold)
    assert 0.05 <= float(exp_mask.mean()) <= 0.95, float(exp_mask.mean())  # no constant mask can pass
    n = int(np.prod(native))
    mask = _Guarded(n, torch.uint8, 0xAB)
    native_prob = _Guarded(n) if with_prob else None
    L.call("pcms_prob_to_mask", torch.from_numpy(prob).to(DEV), *tgt, float(threshold), mask.out,
           native_prob.out if with_prob else None, *native)
    got = mask.check().view(*native).numpy()
    assert set(np.unique(got)) <= {0, 1}, "a mask byte was not written"
    assert np.array_equal(got, exp_mask), f"{int((got != exp_mask).sum())} of {n} mask voxels differ"
    if with_prob:
        _same_bits(native_prob.check().view(*native), exp_prob, f"prob {tgt}->{native}")


def test_bad_arguments():
    L = _lib()
    lib = L.load()
    S = L.stream()
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    lohi, work, out = _Guarded(2), _Guarded(8), _Guarded(64)
    mask = _Guarded(64, torch.uint8, 0xAB)
    s, lh, wk, o, m = (t.data_ptr() for t in (src, lohi.out, work.out, out.out, mask.out))
    assert lib.pcms_volume_minmax_work_floats(0) < 0
    for args in [(s, 3, 8, 1.0, 0.0, lh, wk),        # no such datatype code
                 (s, 32, 8, 1.0, 0.0, lh, wk),       # complex64: not a scalar type
                 (s, 4, 0, 1.0, 0.0, lh, wk),        # empty volume
                 (s, 4, -5, 1.0, 0.0, lh, wk),       # negative length
                 (None, 4, 8, 1.0, 0.0, lh, wk),     # NULL source
                 (s, 4, 8, 1.0, 0.0, None, wk),      # NULL lohi
                 (s, 4, 8, 1.0, 0.0, lh, None),      # NULL work
                 (s + 1, 4, 8, 1.0, 0.0, lh, wk)]:   # int16 source at an odd address
        assert lib.pcms_volume_minmax(*args, S) < 0, args
    for args in [(s, 3, 1, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1),
                 (s, 4, 0, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, lh, o, 1, -1, 1),
                 (None, 4, 1, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, None, o, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, lh, None, 1, 1, 1),
                 (s + 1, 4, 1, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1)]:
        assert lib.pcms_resample_linear_norm(*args, S) < 0, args
    probs = torch.zeros(4 * 8, device=DEV)
    p = probs.data_ptr()

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    for k, fm in [(0, ints(0)), (9, ints(*[0] * 9)), (2, ints(1, 0)), (2, ints(0, 8)), (2, ints(0, -1)), (1, None)]:
        assert lib.pcms_flip_mean(p, k, None if fm is None else ctypes.addressof(fm), o, 2, 2, 2, S) < 0, (k, fm)
    assert lib.pcms_flip_mean(None, 1, ctypes.addressof(ints(0)), o, 2, 2, 2, S) < 0
    assert lib.pcms_flip_mean(p, 1, ctypes.addressof(ints(0)), None, 2, 2, 2, S) < 0
    assert lib.pcms_flip_mean(p, 1, ctypes.addressof(ints(0)), o, 2, 0, 2, S) < 0
    for args in [(None, 2, 2, 2, 0.5, m, o, 2, 2, 2), (p, 2, 2, 2, 0.5, None, o, 2, 2, 2),
                 (p, 0, 2, 2, 0.5, m, o, 2, 2, 2), (p, 2, 2, 2, 0.5, m, o, 2, 2, -3),
                 (p, 2, 2, 2, 0.5, m, o + 2, 2, 2, 2)]:   # the optional fp32 output misaligned
        assert lib.pcms_prob_to_mask(*args, S) < 0, args
    for g in (lohi, work, out, mask):
        g.check(written=False)
