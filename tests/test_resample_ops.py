"""pcms_resample_linear / pcms_resample_label at the C ABI: the device resampler of a NIfTI
volume against the loader's own ``data.resample`` on the host (the oracle), compared on the
fp32 bits -- the kernels restate its fp64 arithmetic operation for operation, so there is no
tolerance.  Sources are formed as ``read_nifti`` + ``ProstateDataset.__getitem__`` form them:
images ``resample(vol.astype(float32), target)``, labels ``resample(vol, target, nearest=True) > 0``
with ``vol`` the decoded (scaled when the header says so) volume."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib

pytestmark = pytest.mark.gpu

GUARD = 1024
# source -> target: mixed up- and down-sampling; all up-sampling (600 outside zeros); fp64
# coordinates that differ from exact rational ones on all three axes (61,419 outside zeros);
# an identity axis beside non-dyadic ones; identity; one voxel
SHAPES = [((20, 18, 24), (32, 32, 16)), ((7, 9, 5), (16, 12, 20)), ((3, 13, 9), (94, 46, 66)),
          ((13, 17, 11), (13, 40, 8)), ((8, 6, 4), (8, 6, 4)), ((1, 1, 1), (4, 3, 2))]
OUTSIDE = {((7, 9, 5), (16, 12, 20)): 600, ((3, 13, 9), (94, 46, 66)): 61419}
CODES = [2, 4, 8, 16, 64, 256, 512, 768, 1024, 1280]


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


def _decode(src, slope, inter):
    """read_nifti's rule."""
    if slope not in (0.0, 1.0) or inter != 0.0:
        return src.astype(np.float64) * (slope if slope != 0.0 else 1.0) + inter
    return src


def _oracle(src, target, nearest, slope=1.0, inter=0.0):
    d = _data()
    vol = _decode(src, slope, inter)
    if nearest:
        return (d.resample(vol, target, nearest=True) > 0).astype(np.float32)
    return d.resample(vol.astype(np.float32), target)


def _run(src, target, nearest, slope=1.0, inter=0.0):
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
    L.call("pcms_resample_label" if nearest else "pcms_resample_linear", raw, code, *src.shape, float(slope),
           float(inter), out, *target)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), "an output element was not written"
    assert torch.equal(torch.cat([buf[:GUARD], buf[GUARD + n:]]).view(torch.int32), guard), "guard overwritten"
    return out.clone().view(*target).cpu()


def _same_bits(got, exp, what):
    exp = torch.from_numpy(np.ascontiguousarray(exp))
    assert got.shape == exp.shape and got.dtype == exp.dtype == torch.float32, what
    diff = got.view(torch.int32) != exp.view(torch.int32)
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (
        f"{what}: {int(diff.sum())} of {diff.numel()} voxels differ, max |d| = {float((got - exp).abs().max())}")


@functools.lru_cache(maxsize=None)
def _linear_case(shape):
    rng = np.random.default_rng(100 + shape[0] * 31 + shape[1] * 7 + shape[2])
    return (1000.0 * rng.standard_normal(shape)).astype(np.float32)  # the lerps are not exact


@functools.lru_cache(maxsize=None)
def _label_case(shape):
    rng = np.random.default_rng(200 + shape[0] * 31 + shape[1] * 7 + shape[2])
    lab = rng.integers(-2, 3, size=shape).astype(np.int16)
    if lab.size >= 4:
        lab.reshape(-1)[:4] = (-2, -1, 1, 2)  # negatives and positives present whatever the draw
    else:
        lab[...] = 1
    return lab


@pytest.mark.parametrize("shape,target", SHAPES)
def test_linear_shapes(shape, target):
    src = _linear_case(shape)
    exp = _oracle(src, target, False)
    if (shape, target) in OUTSIDE:  # the zeros past the volume's far edge are in play (no sample is 0)
        assert int((exp == 0).sum()) == OUTSIDE[(shape, target)]
    _same_bits(_run(src, target, False), exp, f"linear {shape}->{target}")


@pytest.mark.parametrize("shape,target", SHAPES)
def test_label_shapes(shape, target):
    src = _label_case(shape)
    exp = _oracle(src, target, True)
    if src.size > 1:  # a wrong index shows: neither class dominates
        assert 0.2 < float(exp.mean()) < 0.5, float(exp.mean())
    _same_bits(_run(src, target, True), exp, f"label {shape}->{target}")


def _typed_source(code, shape, seed):
    """Values representable in the type, spread over its range (64-bit integers beyond 2^24,
    where the fp32 rounding of a sample matters), about a third of them not positive."""
    dt = np.dtype(_data()._NIFTI_DTYPES[code])
    rng = np.random.default_rng(seed)
    if dt.kind == "f":
        a = (1000.0 * rng.standard_normal(shape)).astype(dt)
        if dt.itemsize == 8:
            a += rng.standard_normal(shape) * 1e-7  # not fp32-representable
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True)
        if dt.itemsize == 8:
            assert (np.abs(a.astype(np.float64)) > 2.0 ** 24).mean() > 0.5
    if dt.kind != "i":  # unsigned and float draws: plant zeros so the label has a background
        a[rng.random(shape) < 0.35] = 0
    return a


@pytest.mark.parametrize("code", CODES)
def test_every_datatype(code):
    shape, target = (7, 9, 5), (16, 12, 20)
    src = _typed_source(code, shape, 300 + code)
    _same_bits(_run(src, target, False), _oracle(src, target, False), f"linear datatype {code}")
    exp = _oracle(src, target, True)
    assert 0.1 < float(exp.mean()) < 0.9
    _same_bits(_run(src, target, True), exp, f"label datatype {code}")


@pytest.mark.parametrize("slope,inter,lo,hi", [(0.5, -3.0, 0, 13), (0.0, 2.0, -5, 3)])
def test_scaled_int16(slope, inter, lo, hi):
    """scl_slope / scl_inter by read_nifti's rule (slope 0 means 1; the product and the sum round
    separately); the label's sign is that of the scaled value, not of the raw one."""
    shape, target = (7, 9, 5), (16, 12, 20)
    rng = np.random.default_rng(400)
    src = rng.integers(-3000, 3000, size=shape).astype(np.int16)
    _same_bits(_run(src, target, False, slope, inter), _oracle(src, target, False, slope, inter),
               f"linear int16 slope {slope} inter {inter}")
    lab = rng.integers(lo, hi, size=shape).astype(np.int16)
    exp = _oracle(lab, target, True, slope, inter)
    assert not np.array_equal(exp, _oracle(lab, target, True)) and 0.1 < float(exp.mean()) < 0.9
    _same_bits(_run(lab, target, True, slope, inter), exp, f"label int16 slope {slope} inter {inter}")


@pytest.mark.parametrize("nearest", [False, True])
def test_writes_one_channel_plane(nearest):
    L = _lib()
    shape, target = (7, 9, 5), (16, 12, 20)
    src = _label_case(shape) if nearest else _linear_case(shape)
    code = 4 if nearest else 16
    raw = torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).to(DEV)
    batch = torch.full((2, 5) + target, 7.5, device=DEV)
    L.call("pcms_resample_label" if nearest else "pcms_resample_linear", raw, code, *shape, 1.0, 0.0, batch[1, 3],
           *target)
    torch.cuda.synchronize()
    got = batch.cpu()
    _same_bits(got[1, 3].contiguous(), _oracle(src, target, nearest), "channel plane")
    got[1, 3] = 7.5
    assert bool((got == 7.5).all()), "another channel was written"


def test_bad_arguments():
    L = _lib()
    lib = L.load()
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    out = torch.zeros(64, device=DEV)
    s, o = src.data_ptr(), out.data_ptr()
    for fn in (lib.pcms_resample_linear, lib.pcms_resample_label):
        for args in [(s, 3, 1, 1, 1, 1.0, 0.0, o, 1, 1, 1),      # no such datatype code
                     (s, 32, 1, 1, 1, 1.0, 0.0, o, 1, 1, 1),     # complex64: not a scalar type
                     (s, 4, 0, 1, 1, 1.0, 0.0, o, 1, 1, 1),      # empty source
                     (s, 4, 1, 1, -2, 1.0, 0.0, o, 1, 1, 1),     # negative source extent
                     (s, 4, 1, 1, 1, 1.0, 0.0, o, 1, 0, 1),      # empty target
                     (None, 4, 1, 1, 1, 1.0, 0.0, o, 1, 1, 1),   # NULL source
                     (s, 4, 1, 1, 1, 1.0, 0.0, None, 1, 1, 1),   # NULL output
                     (s + 1, 4, 1, 1, 1, 1.0, 0.0, o, 1, 1, 1)]:  # int16 source at an odd address
            assert fn(*args, L.stream()) != 0, args
