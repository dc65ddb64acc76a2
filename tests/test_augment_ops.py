"""pcms_resample_affine_linear / pcms_resample_affine_label at the C ABI against the host
restatement ``data.resample_affine`` (the oracle), compared on the fp32 bits: the kernels
restate its fp64 arithmetic operation for operation, so there is no tolerance.  Outputs are
written into a NaN-filled plane between two guard bands, as tests/test_resample_ops.py does."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_augment import GENERAL_SHAPES, SHAPES, TRANSFORMS, affine_of, bands
from tests.test_gpu_ops import DEV, _lib
from tests.test_resample_ops import (CODES, GUARD, _data, _decode, _label_case, _linear_case, _same_bits,
                                     _typed_source)
from tests.test_resample_ops import _run as _run_plain

pytestmark = pytest.mark.gpu


def _host12(A, t):
    return (ctypes.c_double * 12)(*[float(v) for v in np.asarray(A).reshape(-1)], *[float(v) for v in t])


def _oracle(src, target, A, t, nearest, slope=1.0, inter=0.0, gain=1.0, bias=0.0):
    d = _data()
    vol = _decode(src, slope, inter)
    if nearest:
        return (d.resample_affine(vol, target, A, t, nearest=True) > 0).astype(np.float32)
    return d.resample_affine(vol.astype(np.float32), target, A, t, gain=gain, bias=bias)


def _run(src, target, A, t, nearest, slope=1.0, inter=0.0, gain=1.0, bias=0.0):
    """The entry point on ``src``'s bytes, into a NaN-filled plane between two guard bands."""
    L = _lib()
    code = {np.dtype(v): k for k, v in _data()._NIFTI_DTYPES.items()}[src.dtype]
    raw = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).view(np.uint8).copy()).to(DEV)
    n = int(np.prod(target))
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV)
    buf[:GUARD] = 12345.678
    buf[GUARD + n:] = -8765.4321
    guard = torch.cat([buf[:GUARD], buf[GUARD + n:]]).clone().view(torch.int32)
    out = buf[GUARD:GUARD + n]
    host = _host12(A, t)
    if nearest:
        L.call("pcms_resample_affine_label", raw, code, *src.shape, float(slope), float(inter),
               ctypes.addressof(host), out, *target)
    else:
        L.call("pcms_resample_affine_linear", raw, code, *src.shape, float(slope), float(inter),
               ctypes.addressof(host), float(gain), float(bias), out, *target)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), "an output element was not written"
    assert torch.equal(torch.cat([buf[:GUARD], buf[GUARD + n:]]).view(torch.int32), guard), "guard overwritten"
    return out.clone().view(*target).cpu()


@functools.lru_cache(maxsize=None)
def _identity(shape, target):
    return _data().volume_affine(np.eye(3), np.zeros(3), shape, target)


@pytest.mark.parametrize("shape,target", SHAPES)
def test_identity(shape, target):
    A, t = _identity(shape, target)
    src = _linear_case(shape)
    got = _run(src, target, A, t, False)
    _same_bits(got, _oracle(src, target, A, t, False), f"identity linear {shape}->{target}")
    assert torch.equal(got.view(torch.int32), _run_plain(src, target, False).view(torch.int32)), "pcms_resample_linear"
    lab = _label_case(shape)
    _same_bits(_run(lab, target, A, t, True), _oracle(lab, target, A, t, True), f"identity label {shape}->{target}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_single_axis_flips(axis):
    d = _data()
    shape, target = SHAPES[0]
    A, t = d.volume_affine(d.compose_transform(flips=[a == axis for a in range(3)]), np.zeros(3), shape, target)
    src, lab = _linear_case(shape), _label_case(shape)
    got = _run(src, target, A, t, False)
    _same_bits(got, _oracle(src, target, A, t, False), f"flip {axis} linear")
    _same_bits(got, np.flip(_oracle(src, target, *_identity(shape, target), False), axis), f"flip {axis} vs np.flip")
    _same_bits(_run(lab, target, A, t, True), _oracle(lab, target, A, t, True), f"flip {axis} label")


@pytest.mark.parametrize("shape,target", GENERAL_SHAPES)
@pytest.mark.parametrize("k", range(len(TRANSFORMS)))
def test_general_transforms(shape, target, k):
    A, t = affine_of(TRANSFORMS[k], shape, target)
    share, low, high = bands(A, t, shape, target)  # outside voxels, the lower and the upper clamp are in play
    assert 0.5 <= share <= 0.9 and low >= 100 and high >= 100, (share, low, high)
    src, lab = _linear_case(shape), _label_case(shape)
    exp = _oracle(src, target, A, t, False)
    assert abs(float((exp == 0).mean()) - (1.0 - share)) < 1e-9  # no sample is 0: the zeros are the outside
    _same_bits(_run(src, target, A, t, False), exp, f"linear {shape}->{target} transform {k}")
    exp = _oracle(lab, target, A, t, True)
    assert 0.1 < float(exp.mean()) < 0.5
    _same_bits(_run(lab, target, A, t, True), exp, f"label {shape}->{target} transform {k}")


@pytest.mark.parametrize("code", CODES)
def test_every_datatype(code):
    shape, target = GENERAL_SHAPES[1]
    A, t = affine_of(TRANSFORMS[3], shape, target)
    src = _typed_source(code, shape, 300 + code)
    _same_bits(_run(src, target, A, t, False), _oracle(src, target, A, t, False), f"linear datatype {code}")
    exp = _oracle(src, target, A, t, True)
    assert 0.1 < float(exp.mean()) < 0.9
    _same_bits(_run(src, target, A, t, True), exp, f"label datatype {code}")


@pytest.mark.parametrize("slope,inter,lo,hi", [(0.5, -3.0, 0, 13), (0.0, 2.0, -5, 3)])
def test_scaled_int16(slope, inter, lo, hi):
    shape, target = GENERAL_SHAPES[1]
    A, t = affine_of(TRANSFORMS[3], shape, target)
    rng = np.random.default_rng(400)
    src = rng.integers(-3000, 3000, size=shape).astype(np.int16)
    _same_bits(_run(src, target, A, t, False, slope, inter), _oracle(src, target, A, t, False, slope, inter),
               f"linear int16 slope {slope} inter {inter}")
    lab = rng.integers(lo, hi, size=shape).astype(np.int16)
    exp = _oracle(lab, target, A, t, True, slope, inter)
    assert not np.array_equal(exp, _oracle(lab, target, A, t, True)) and 0.1 < float(exp.mean()) < 0.9
    _same_bits(_run(lab, target, A, t, True, slope, inter), exp, f"label int16 slope {slope} inter {inter}")


def test_gain_and_bias():
    shape, target = GENERAL_SHAPES[0]
    A, t = affine_of(TRANSFORMS[3], shape, target)
    src = _linear_case(shape)
    plain = _oracle(src, target, A, t, False)
    exp = _oracle(src, target, A, t, False, gain=1.1, bias=-3.0)
    assert not np.array_equal(exp, plain) and np.array_equal(exp == 0, plain == 0)
    got = _run(src, target, A, t, False, gain=1.1, bias=-3.0)
    _same_bits(got, exp, "gain 1.1 bias -3")
    outside = torch.from_numpy(plain == 0)
    assert int(outside.sum()) > 1000 and not got[outside].view(torch.int32).any(), "outside voxels must stay +0.0"
    _same_bits(_run(src, target, A, t, False, gain=1.0, bias=2.5), _oracle(src, target, A, t, False, bias=2.5), "bias only")


@pytest.mark.parametrize("nearest", [False, True])
def test_writes_one_channel_plane(nearest):
    L = _lib()
    shape, target = GENERAL_SHAPES[1]
    A, t = affine_of(TRANSFORMS[3], shape, target)
    src = _label_case(shape) if nearest else _linear_case(shape)
    code = 4 if nearest else 16
    raw = torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).to(DEV)
    batch = torch.full((2, 5) + target, 7.5, device=DEV)
    host = _host12(A, t)
    if nearest:
        L.call("pcms_resample_affine_label", raw, code, *shape, 1.0, 0.0, ctypes.addressof(host), batch[1, 3], *target)
    else:
        L.call("pcms_resample_affine_linear", raw, code, *shape, 1.0, 0.0, ctypes.addressof(host), 1.0, 0.0,
               batch[1, 3], *target)
    torch.cuda.synchronize()
    got = batch.cpu()
    _same_bits(got[1, 3].contiguous(), _oracle(src, target, A, t, nearest), "channel plane")
    got[1, 3] = 7.5
    assert bool((got == 7.5).all()), "another channel was written"


def test_resample_device_takes_the_affine():
    d = _data()
    shape, target = GENERAL_SHAPES[1]
    A, t = affine_of(TRANSFORMS[2], shape, target)
    a12 = tuple(A.reshape(-1)) + tuple(t)
    src, lab = _linear_case(shape), _label_case(shape)

    def raw(a, code):
        return d.RawVolume(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(DEV), code, shape, 1.0, 0.0)

    _same_bits(d.resample_device(raw(src, 16), target, affine=a12, gain=0.9, bias=4.0).cpu(),
               _oracle(src, target, A, t, False, gain=0.9, bias=4.0), "resample_device linear")
    _same_bits(d.resample_device(raw(lab, 4), target, nearest=True, affine=a12).cpu(),
               _oracle(lab, target, A, t, True), "resample_device label")
    with pytest.raises(ValueError):
        d.resample_device(raw(src, 16), target, affine=a12[:9])


def test_bad_arguments():
    L = _lib()
    lib = L.load()
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    out = torch.zeros(64, device=DEV)
    s, o = src.data_ptr(), out.data_ptr()
    ident = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    m = ctypes.addressof(ident)
    bad = {}
    for name, pos, v in (("nan", 4, float("nan")), ("inf", 0, float("inf")), ("ninf_t", 11, float("-inf"))):
        arr = (ctypes.c_double * 12)(*ident)
        arr[pos] = v
        bad[name] = arr
    cases = [(s, 3, 1, 1, 1, 1.0, 0.0, m, o, 1, 1, 1),      # no such datatype code
             (s, 32, 1, 1, 1, 1.0, 0.0, m, o, 1, 1, 1),     # complex64: not a scalar type
             (s, 4, 0, 1, 1, 1.0, 0.0, m, o, 1, 1, 1),      # empty source
             (s, 4, 1, 1, -2, 1.0, 0.0, m, o, 1, 1, 1),     # negative source extent
             (s, 4, 1, 1, 1, 1.0, 0.0, m, o, 1, 0, 1),      # empty target
             (None, 4, 1, 1, 1, 1.0, 0.0, m, o, 1, 1, 1),   # NULL source
             (s, 4, 1, 1, 1, 1.0, 0.0, m, None, 1, 1, 1),   # NULL output
             (s + 1, 4, 1, 1, 1, 1.0, 0.0, m, o, 1, 1, 1),  # int16 source at an odd address
             (s, 4, 1, 1, 1, 1.0, 0.0, None, o, 1, 1, 1)]   # NULL matrix
    cases += [(s, 4, 1, 1, 1, 1.0, 0.0, ctypes.addressof(a), o, 1, 1, 1) for a in bad.values()]  # NaN / inf entries
    for args in cases:
        assert lib.pcms_resample_affine_label(*args, L.stream()) != 0, args
        assert lib.pcms_resample_affine_linear(*args[:8], 1.0, 0.0, *args[8:], L.stream()) != 0, args
    good = (s, 4, 1, 1, 1, 1.0, 0.0, m)
    for gain, bias in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan")), (1.0, float("-inf")), (1e39, 0.0)):
        assert lib.pcms_resample_affine_linear(*good, gain, bias, o, 1, 1, 1, L.stream()) != 0, (gain, bias)
    assert lib.pcms_resample_affine_linear(*good, 1.0, 0.0, o, 1, 1, 1, L.stream()) == 0  # the list above is what fails
    assert lib.pcms_resample_affine_label(*good, o, 1, 1, 1, L.stream()) == 0
    torch.cuda.synchronize()
    assert not out.any()  # nothing but the two good 1-voxel launches (a zero source) wrote
