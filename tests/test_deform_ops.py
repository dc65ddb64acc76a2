"""pcms_resample_deform_linear / pcms_resample_deform_label at the C ABI against the host
restatement ``data.resample_deform`` (the oracle), compared on the fp32 bits: the kernels restate
its fp64 arithmetic operation for operation, so there is no tolerance.  Outputs are written into
a NaN-filled plane between two guard bands, as tests/test_resample_ops.py does.  The fields are
tests/test_deform.py's, whose coverage conditions (outside voxels, both clamp bands, most samples
moved to another 8-corner cell) are asserted here again for every case compared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_augment import GENERAL_SHAPES, SHAPES, TRANSFORMS, affine_of
from tests.test_augment_ops import _host12
from tests.test_augment_ops import _run as _run_affine
from tests.test_deform import GRIDS, coverage, nan_field, random_field
from tests.test_gpu_ops import DEV, _lib
from tests.test_resample_ops import CODES, GUARD, _data, _decode, _label_case, _linear_case, _same_bits, _typed_source

pytestmark = pytest.mark.gpu


def _oracle(src, target, A, t, field, nearest, slope=1.0, inter=0.0, gain=1.0, bias=0.0):
    d = _data()
    vol = _decode(src, slope, inter)
    if nearest:
        return (d.resample_deform(vol, target, A, t, field, nearest=True) > 0).astype(np.float32)
    return d.resample_deform(vol.astype(np.float32), target, A, t, field, gain=gain, bias=bias)


def _run(src, target, A, t, field, nearest, slope=1.0, inter=0.0, gain=1.0, bias=0.0):
    """The entry point on ``src``'s bytes, into a NaN-filled plane between two guard bands."""
    L = _lib()
    code = {np.dtype(v): k for k, v in _data()._NIFTI_DTYPES.items()}[src.dtype]
    raw = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).view(np.uint8).copy()).to(DEV)
    dev_field = torch.from_numpy(np.array(field, dtype=np.float64)).to(DEV)
    n = int(np.prod(target))
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV)
    buf[:GUARD] = 12345.678
    buf[GUARD + n:] = -8765.4321
    guard = torch.cat([buf[:GUARD], buf[GUARD + n:]]).clone().view(torch.int32)
    out = buf[GUARD:GUARD + n]
    host = _host12(A, t)
    if nearest:
        L.call("pcms_resample_deform_label", raw, code, *src.shape, float(slope), float(inter),
               ctypes.addressof(host), dev_field, *field.shape[:3], out, *target)
    else:
        L.call("pcms_resample_deform_linear", raw, code, *src.shape, float(slope), float(inter),
               ctypes.addressof(host), dev_field, *field.shape[:3], float(gain), float(bias), out, *target)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), "an output element was not written"
    assert torch.equal(torch.cat([buf[:GUARD], buf[GUARD + n:]]).view(torch.int32), guard), "guard overwritten"
    return out.clone().view(*target).cpu()


@functools.lru_cache(maxsize=None)
def _affine(k, shape, target):
    return affine_of(TRANSFORMS[k], shape, target)


@pytest.mark.parametrize("shape,target", SHAPES)
def test_zero_field(shape, target):
    """Equal to the host form and to pcms_resample_affine_*; (3, 13, 9) -> (94, 46, 66) is more
    than one grid-stride pass, (1, 1, 1) -> (4, 3, 2) the smallest case."""
    A, t = _affine(3, shape, target)
    zero = np.zeros((5, 4, 7, 3))
    src, lab = _linear_case(shape), _label_case(shape)
    got = _run(src, target, A, t, zero, False)
    _same_bits(got, _oracle(src, target, A, t, zero, False), f"zero field linear {shape}->{target}")
    assert torch.equal(got.view(torch.int32), _run_affine(src, target, A, t, False).view(torch.int32)), "affine_linear"
    got = _run(lab, target, A, t, zero, True)
    _same_bits(got, _oracle(lab, target, A, t, zero, True), f"zero field label {shape}->{target}")
    assert torch.equal(got.view(torch.int32), _run_affine(lab, target, A, t, True).view(torch.int32)), "affine_label"


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shape,target", GENERAL_SHAPES)
@pytest.mark.parametrize("k", range(len(TRANSFORMS)))
def test_general_transforms_and_fields(shape, target, k, grid):
    A, t = _affine(k, shape, target)
    field = random_field(grid)
    share, low, high, moved = coverage(A, t, shape, target, field)
    assert share >= 0.5 and low >= 50 and high >= 50 and moved >= 0.3, (share, low, high, moved)
    src, lab = _linear_case(shape), _label_case(shape)
    exp = _oracle(src, target, A, t, field, False)
    assert abs(float((exp == 0).mean()) - (1.0 - share)) < 1e-9  # no sample is 0: the zeros are the outside
    _same_bits(_run(src, target, A, t, field, False), exp, f"linear {shape}->{target} transform {k} grid {grid}")
    exp = _oracle(lab, target, A, t, field, True)
    assert 0.1 < float(exp.mean()) < 0.5
    _same_bits(_run(lab, target, A, t, field, True), exp, f"label {shape}->{target} transform {k} grid {grid}")


@pytest.mark.parametrize("grid", [(4, 4, 4), (8, 8, 8)])
def test_more_than_one_pass(grid):
    """285,384 output voxels: more than the 1024 x 256 threads of the largest launch, so some
    threads take a second voxel; the (8, 8, 8) grid is six rounds of the copy into LDS."""
    shape, target = SHAPES[2]
    # a flip of D: the far end of the output (d >= 86, the second pass) samples the volume's near end
    A, t = affine_of(((0.0, 0.0, 10.0), 1.0, (True, False, False), (0.0, 0.0, 0.0)), shape, target)
    assert int(np.prod(target)) > 1024 * 256 and 86 * target[1] * target[2] <= 1024 * 256
    field = random_field(grid)
    src, lab = _linear_case(shape), _label_case(shape)
    exp = _oracle(src, target, A, t, field, False)
    assert 0.5 < float((exp != 0).mean()) < 0.95 and float((exp[86:] != 0).mean()) > 0.5
    _same_bits(_run(src, target, A, t, field, False), exp, f"linear {shape}->{target} grid {grid}")
    _same_bits(_run(lab, target, A, t, field, True), _oracle(lab, target, A, t, field, True),
               f"label {shape}->{target} grid {grid}")


def test_smallest_case():
    shape, target = SHAPES[5]
    field = random_field((4, 4, 4))
    A, t = _affine(1, shape, target)
    src, lab = _linear_case(shape), _label_case(shape)
    exp = _oracle(src, target, A, t, field, False)
    n_in, n_affine = int((exp != 0).sum()), int((_data().resample_affine(src, target, A, t) != 0).sum())
    assert 0 < n_in < exp.size and n_in != n_affine  # inside and outside voxels, and the field shows
    _same_bits(_run(src, target, A, t, field, False), exp, "linear (1, 1, 1) -> (4, 3, 2)")
    _same_bits(_run(lab, target, A, t, field, True), _oracle(lab, target, A, t, field, True), "label (1, 1, 1) -> (4, 3, 2)")


@pytest.mark.parametrize("code", CODES)
def test_every_datatype(code):
    shape, target = GENERAL_SHAPES[1]
    A, t = _affine(3, shape, target)
    field = random_field((5, 4, 7))
    src = _typed_source(code, shape, 300 + code)
    _same_bits(_run(src, target, A, t, field, False), _oracle(src, target, A, t, field, False), f"linear datatype {code}")
    exp = _oracle(src, target, A, t, field, True)
    assert 0.1 < float(exp.mean()) < 0.9
    _same_bits(_run(src, target, A, t, field, True), exp, f"label datatype {code}")


@pytest.mark.parametrize("slope,inter,lo,hi", [(0.5, -3.0, 0, 13), (0.0, 2.0, -5, 3)])
def test_scaled_int16(slope, inter, lo, hi):
    shape, target = GENERAL_SHAPES[1]
    A, t = _affine(3, shape, target)
    field = random_field((5, 4, 7))
    rng = np.random.default_rng(400)
    src = rng.integers(-3000, 3000, size=shape).astype(np.int16)
    _same_bits(_run(src, target, A, t, field, False, slope, inter), _oracle(src, target, A, t, field, False, slope, inter),
               f"linear int16 slope {slope} inter {inter}")
    lab = rng.integers(lo, hi, size=shape).astype(np.int16)
    exp = _oracle(lab, target, A, t, field, True, slope, inter)
    assert not np.array_equal(exp, _oracle(lab, target, A, t, field, True)) and 0.1 < float(exp.mean()) < 0.9
    _same_bits(_run(lab, target, A, t, field, True, slope, inter), exp, f"label int16 slope {slope} inter {inter}")


def test_gain_and_bias():
    shape, target = GENERAL_SHAPES[0]
    A, t = _affine(3, shape, target)
    field = random_field((8, 8, 8))
    src = _linear_case(shape)
    plain = _oracle(src, target, A, t, field, False)
    exp = _oracle(src, target, A, t, field, False, gain=1.1, bias=-3.0)
    assert not np.array_equal(exp, plain) and np.array_equal(exp == 0, plain == 0)
    got = _run(src, target, A, t, field, False, gain=1.1, bias=-3.0)
    _same_bits(got, exp, "gain 1.1 bias -3")
    outside = torch.from_numpy(plain == 0)
    assert int(outside.sum()) > 1000 and not got[outside].view(torch.int32).any(), "outside voxels must stay +0.0"
    _same_bits(_run(src, target, A, t, field, False, gain=1.0, bias=2.5),
               _oracle(src, target, A, t, field, False, bias=2.5), "bias only")


def test_nan_control_vector():
    """A NaN coordinate is outside: exact +0.0 wherever the NaN vector is in a voxel's support."""
    d = _data()
    shape, target = GENERAL_SHAPES[1]
    A, t = _affine(3, shape, target)
    field = nan_field()
    hit = torch.from_numpy(np.isnan(d.field_displacement(field, target)[0]))
    assert 0.1 < float(hit.float().mean()) < 0.9
    src, lab = _linear_case(shape), np.abs(_label_case(shape)) + 1
    for nearest, v in ((False, src), (True, lab)):
        got = _run(v, target, A, t, field, nearest, **({} if nearest else {"gain": 1.1, "bias": -3.0}))
        exp = _oracle(v, target, A, t, field, nearest, **({} if nearest else {"gain": 1.1, "bias": -3.0}))
        assert exp[~hit.numpy()].any()
        _same_bits(got, exp, f"NaN control vector, nearest={nearest}")
        assert not got[hit].view(torch.int32).any()


@pytest.mark.parametrize("nearest", [False, True])
def test_writes_one_channel_plane(nearest):
    L = _lib()
    shape, target = GENERAL_SHAPES[1]
    A, t = _affine(3, shape, target)
    field = random_field((5, 4, 7))
    src = _label_case(shape) if nearest else _linear_case(shape)
    code = 4 if nearest else 16
    raw = torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).to(DEV)
    dev_field = torch.from_numpy(np.array(field)).to(DEV)
    batch = torch.full((2, 5) + target, 7.5, device=DEV)
    host = _host12(A, t)
    if nearest:
        L.call("pcms_resample_deform_label", raw, code, *shape, 1.0, 0.0, ctypes.addressof(host), dev_field, 5, 4, 7,
               batch[1, 3], *target)
    else:
        L.call("pcms_resample_deform_linear", raw, code, *shape, 1.0, 0.0, ctypes.addressof(host), dev_field, 5, 4, 7,
               1.0, 0.0, batch[1, 3], *target)
    torch.cuda.synchronize()
    got = batch.cpu()
    _same_bits(got[1, 3].contiguous(), _oracle(src, target, A, t, field, nearest), "channel plane")
    got[1, 3] = 7.5
    assert bool((got == 7.5).all()), "another channel was written"


def test_resample_device_takes_the_field():
    d = _data()
    shape, target = GENERAL_SHAPES[1]
    A, t = _affine(2, shape, target)
    a12 = tuple(A.reshape(-1)) + tuple(t)
    field = random_field((5, 4, 7))
    dev_field = torch.from_numpy(np.array(field)).to(DEV)
    src, lab = _linear_case(shape), _label_case(shape)

    def raw(a, code):
        return d.RawVolume(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(DEV), code, shape, 1.0, 0.0)

    _same_bits(d.resample_device(raw(src, 16), target, affine=a12, gain=0.9, bias=4.0, field=dev_field).cpu(),
               _oracle(src, target, A, t, field, False, gain=0.9, bias=4.0), "resample_device linear")
    _same_bits(d.resample_device(raw(lab, 4), target, nearest=True, affine=a12, field=dev_field).cpu(),
               _oracle(lab, target, A, t, field, True), "resample_device label")
    for bad in (dev_field.float(), dev_field.cpu(), dev_field[..., :2].contiguous(), dev_field.permute(3, 0, 1, 2),
                dev_field.reshape(-1)):
        with pytest.raises(ValueError):
            d.resample_device(raw(src, 16), target, affine=a12, field=bad)
    with pytest.raises(ValueError):
        d.resample_device(raw(src, 16), target, field=dev_field)  # no affine


def test_bad_arguments():
    L = _lib()
    lib = L.load()
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    out = torch.zeros(64, device=DEV)
    field = torch.zeros(512 * 3 + 1, dtype=torch.float64, device=DEV)
    s, o, f = src.data_ptr(), out.data_ptr(), field.data_ptr()
    ident = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    m = ctypes.addressof(ident)
    bad = []
    for pos, v in ((4, float("nan")), (0, float("inf")), (11, float("-inf"))):
        arr = (ctypes.c_double * 12)(*ident)
        arr[pos] = v
        bad.append(arr)
    g = (f, 4, 4, 4)
    cases = [(s, 3, 1, 1, 1, 1.0, 0.0, m, *g, o, 1, 1, 1),      # no such datatype code
             (s, 32, 1, 1, 1, 1.0, 0.0, m, *g, o, 1, 1, 1),     # complex64: not a scalar type
             (s, 4, 0, 1, 1, 1.0, 0.0, m, *g, o, 1, 1, 1),      # empty source
             (s, 4, 1, 1, -2, 1.0, 0.0, m, *g, o, 1, 1, 1),     # negative source extent
             (s, 4, 1, 1, 1, 1.0, 0.0, m, *g, o, 1, 0, 1),      # empty target
             (None, 4, 1, 1, 1, 1.0, 0.0, m, *g, o, 1, 1, 1),   # NULL source
             (s, 4, 1, 1, 1, 1.0, 0.0, m, *g, None, 1, 1, 1),   # NULL output
             (s + 1, 4, 1, 1, 1, 1.0, 0.0, m, *g, o, 1, 1, 1),  # int16 source at an odd address
             (s, 4, 1, 1, 1, 1.0, 0.0, None, *g, o, 1, 1, 1)]   # NULL matrix
    cases += [(s, 4, 1, 1, 1, 1.0, 0.0, ctypes.addressof(a), *g, o, 1, 1, 1) for a in bad]  # NaN / inf entries
    cases += [(s, 4, 1, 1, 1, 1.0, 0.0, m, *fg, o, 1, 1, 1) for fg in (
        (None, 4, 4, 4), (f + 4, 4, 4, 4),                        # NULL field, field not 8-byte aligned
        (f, 3, 4, 4), (f, 4, 0, 4), (f, 4, 4, -1), (f, 1, 1, 1),  # a count below 4
        (f, 8, 8, 9), (f, 4, 4, 33), (f, 65536, 65536, 4),        # more than 512 points (one product wraps an int)
        (f, 2 ** 31 - 1, 4, 4))]
    for args in cases:
        assert lib.pcms_resample_deform_label(*args, L.stream()) != 0, args
        assert lib.pcms_resample_deform_linear(*args[:12], 1.0, 0.0, *args[12:], L.stream()) != 0, args
    good = (s, 4, 1, 1, 1, 1.0, 0.0, m)
    for gain, bias in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan")), (1.0, float("-inf")), (1e39, 0.0)):
        assert lib.pcms_resample_deform_linear(*good, *g, gain, bias, o, 1, 1, 1, L.stream()) != 0, (gain, bias)
    for fg in (g, (f, 8, 8, 8), (f + 8, 4, 4, 32)):  # the list above is what fails
        assert lib.pcms_resample_deform_linear(*good, *fg, 1.0, 0.0, o, 1, 1, 1, L.stream()) == 0
        assert lib.pcms_resample_deform_label(*good, *fg, o, 1, 1, 1, L.stream()) == 0
    torch.cuda.synchronize()
    assert not out.any()  # nothing but the good 1-voxel launches (a zero source) wrote
