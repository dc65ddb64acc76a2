"""pcms_joint_histogram at the C ABI against predict.joint_histogram, on the counts exactly: the
kernel restates the host arithmetic operation for operation and counts in integers, so there is no
tolerance.  The table is filled with 0xFF bytes between two guard bands (no count can be
0xFFFFFFFF: a lattice holds fewer than 2^31 voxels); the workspace is handed over filled with 0xFF
bytes too, so a call that relies on a zeroed workspace fails."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_predict_ops import _Guarded, _code, _mods, _upload
from tests.test_resample_ops import CODES, _decode, _typed_source

pytestmark = pytest.mark.gpu

SMALL = ((5, 7, 9), (6, 5, 11))
LARGE = ((19, 33, 37), (17, 29, 41))       # a lattice of 23199 voxels: 23 workgroups of 1024
STRIDES = [(1, 1, 1), (1, 2, 2), (2, 3, 1)]


def _affine(kind, fix_shape, mov_shape):
    """``scaled``: the fixed grid stretched onto the moving one, everything inside; ``oblique``:
    flipped, rotated, zoomed out and shifted, part of the lattice outside; ``far``: all outside."""
    d = _mods()[0]
    if kind == "scaled":
        return d.volume_affine(np.eye(3), np.zeros(3), mov_shape, fix_shape)
    if kind == "oblique":
        return d.volume_affine(d.compose_transform((False, True, False), (8.0, -5.0, 12.0), 0.9),
                               np.array([0.3, -0.8, 1.7]), mov_shape, fix_shape)
    return np.eye(3), np.array([0.0, 500.0, 0.0])


def _minmax(vol):
    v = np.asarray(vol).astype(np.float32)
    return np.array([v.min(), v.max()], np.float32)


def _device_hist(fix, mov, A, t, flohi, mlohi, bins=32, stride=(1, 1, 1), fscale=(1.0, 0.0), mscale=(1.0, 0.0),
                 offset=0, fill=0xFF, work=None):
    """The table of the entry point on the two sources' bytes, each ``offset`` elements into a
    16-byte-aligned allocation; the workspace ``fill``-filled between guards."""
    L = _lib()
    keep_f, fptr = _upload(fix, offset)
    keep_m, mptr = _upload(mov, offset)
    nbytes = L.query("pcms_joint_histogram_work_bytes", bins)
    assert nbytes == 8 * bins * bins * 4
    hist = _Guarded(bins * bins, torch.int32, -1)
    work = _Guarded(nbytes, torch.uint8, fill) if work is None else work
    host = (ctypes.c_double * 12)(*np.asarray(A, np.float64).reshape(-1).tolist(), *np.asarray(t, np.float64).tolist())
    L.call("pcms_joint_histogram", fptr, _code(fix.dtype), *fix.shape, float(fscale[0]), float(fscale[1]),
           torch.from_numpy(np.asarray(flohi, np.float32)).to(DEV), mptr, _code(mov.dtype), *mov.shape,
           float(mscale[0]), float(mscale[1]), torch.from_numpy(np.asarray(mlohi, np.float32)).to(DEV),
           ctypes.addressof(host), *stride, bins, hist.out, work.out)
    work.check()
    got = hist.check().numpy()
    assert (got >= 0).all(), "a bin was not written"
    return got.astype(np.int64).reshape(bins, bins)


def _host_hist(fix, mov, A, t, flohi, mlohi, bins=32, stride=(1, 1, 1), fscale=(1.0, 0.0), mscale=(1.0, 0.0)):
    return _mods()[1].joint_histogram(_decode(fix, *fscale), _decode(mov, *mscale), A, t, flohi, mlohi, bins, stride)


def _check(fix, mov, kind, what, flohi=None, mlohi=None, expect=None, **kw):
    A, t = _affine(kind, fix.shape, mov.shape)
    scales = {k: kw[k] for k in ("fscale", "mscale") if k in kw}
    flohi = _minmax(_decode(fix, *scales.get("fscale", (1.0, 0.0)))) if flohi is None else flohi
    mlohi = _minmax(_decode(mov, *scales.get("mscale", (1.0, 0.0)))) if mlohi is None else mlohi
    host_kw = {k: v for k, v in kw.items() if k in ("bins", "stride", "fscale", "mscale")}
    exp = _host_hist(fix, mov, A, t, flohi, mlohi, **host_kw)
    got = _device_hist(fix, mov, A, t, flohi, mlohi, **kw)
    assert np.array_equal(got, exp), f"{what}: {int((got != exp).sum())} bins differ, sums {got.sum()} / {exp.sum()}"
    stride = kw.get("stride", (1, 1, 1))
    lattice = int(np.prod([-(-n // s) for n, s in zip(fix.shape, stride)]))
    total = int(exp.sum())
    want = {"scaled": total == lattice, "oblique": 0 < total < lattice, "far": total == 0}[kind] if expect is None \
        else expect(total, lattice)
    assert want, (what, kind, total, lattice)
    return got


@functools.lru_cache(maxsize=None)
def _mr_pair(shapes):
    """An MR-like fixed volume (int16, two thirds background zero: bin (0, .) is hot) and a float32
    moving volume."""
    rng = np.random.default_rng(70 + shapes[0][0])
    fix = rng.integers(0, 3000, size=shapes[0]).astype(np.int16)
    fix[rng.random(shapes[0]) < 0.66] = 0
    mov = (1000.0 * rng.standard_normal(shapes[1])).astype(np.float32)
    mov[rng.random(shapes[1]) < 0.5] = mov.min()
    return fix, mov


@pytest.mark.parametrize("code", CODES)
def test_every_fixed_datatype(code):
    for shapes in (SMALL, LARGE):
        fix = _typed_source(code, shapes[0], 700 + code)
        mov = _mr_pair(shapes)[1]
        for kind, stride in (("oblique", (1, 1, 1)), ("scaled", (2, 3, 1))):
            _check(fix, mov, kind, f"fixed datatype {code} {shapes[0]} {kind}", stride=stride, offset=1)
    _check(fix, mov, "oblique", f"fixed datatype {code} scaled values", fscale=(-0.37, 12.5), offset=1)


@pytest.mark.parametrize("code", CODES)
def test_every_moving_datatype(code):
    for shapes in (SMALL, LARGE):
        fix = _mr_pair(shapes)[0]
        mov = _typed_source(code, shapes[1], 800 + code)
        for kind, stride in (("oblique", (1, 1, 1)), ("scaled", (1, 2, 2))):
            _check(fix, mov, kind, f"moving datatype {code} {shapes[1]} {kind}", stride=stride, offset=1)
    _check(fix, mov, "oblique", f"moving datatype {code} scaled values", mscale=(0.5, -3.0), offset=1)


@pytest.mark.parametrize("bins", [2, 8, 32, 64])
@pytest.mark.parametrize("stride", STRIDES)
def test_bins_strides_and_windows(bins, stride):
    predict = _mods()[1]
    for shapes in (SMALL, LARGE):
        fix, mov = _mr_pair(shapes)
        for kind in ("scaled", "oblique", "far"):
            got = _check(fix, mov, kind, f"min-max {shapes} {kind}", bins=bins, stride=stride, offset=1)
            if kind == "far":
                assert not got.any()
        pf, pm = predict.intensity_window(fix, 10.0, 90.0, above=0.0), predict.intensity_window(mov, 10.0, 90.0)
        assert fix.min() < pf[0] < pf[1] < fix.max() and mov.min() <= pm[0] < pm[1] < mov.max()
        _check(fix, mov, "oblique", f"percentile {shapes}", flohi=pf, mlohi=pm, bins=bins, stride=stride)


def test_constant_volumes_the_last_bin_and_a_zero_denominator():
    fix, mov = np.full(SMALL[0], 7.0, np.float32), np.full(SMALL[1], 3, np.int16)
    n = int(np.prod(SMALL[0]))
    everything = lambda total, lattice: total == lattice  # noqa: E731
    # constant volumes under their own min-max window: den == 0, the whole count in bin (0, 0)
    got = _check(fix, mov, "scaled", "constants", bins=8)
    assert got[0, 0] == n and got.sum() == n
    # a value of exactly 1.0 falls in the last bin
    got = _check(fix, mov, "scaled", "exactly one", flohi=(0, 7), mlohi=(0, 3), bins=8)
    assert got[7, 7] == n and got.sum() == n
    # den == 0 with lo != 0 on one side only
    rng = np.random.default_rng(9)
    varied = rng.integers(0, 100, size=SMALL[1]).astype(np.int16)
    got = _check(fix, varied, "scaled", "den 0, fixed side", flohi=(37, 37), bins=8, expect=everything)
    assert got[0].sum() == n
    got = _check(_mr_pair(SMALL)[0], mov, "scaled", "den 0, moving side", mlohi=(37, 37), bins=8, expect=everything)
    assert got[:, 0].sum() == n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_voxels_are_excluded(dtype):
    rng = np.random.default_rng(31)
    fix = (100.0 * rng.standard_normal(LARGE[0])).astype(dtype)
    mov = (100.0 * rng.standard_normal(LARGE[1])).astype(dtype)
    lohi = np.float32([-250, 250])
    clean = _check(fix, mov, "scaled", "no NaN", flohi=lohi, mlohi=lohi)
    fix[3, 4, 5] = np.nan
    one = _check(fix, mov, "scaled", "a NaN in the fixed volume", flohi=lohi, mlohi=lohi,
                 expect=lambda total, lattice: total == lattice - 1)
    assert one.sum() == clean.sum() - 1
    mov[::2, 7, 7] = np.nan                                      # every lattice voxel whose corners touch one is out
    some = _check(fix, mov, "scaled", "NaNs in the moving volume", flohi=lohi, mlohi=lohi, offset=1,
                  expect=lambda total, lattice: 0 < total < lattice - 1)
    assert some.sum() < one.sum()
    # a NaN window (the min-max of a volume that holds one): every value is a NaN, nothing counts
    none = _check(fix, mov, "scaled", "a NaN window", flohi=np.float32([np.nan, np.nan]), mlohi=lohi,
                  expect=lambda total, lattice: total == 0)
    assert not none.any()


def test_under_a_capped_grid():
    """23199 lattice voxels on one and on two workgroups: every thread makes many trips."""
    L = _lib()
    fix, mov = _mr_pair(LARGE)
    old = L.query("pcms_stream_grid_cap", 1)
    try:
        _check(fix, mov, "oblique", "one workgroup", bins=64, offset=1)
        L.query("pcms_stream_grid_cap", 2)
        for stride in STRIDES:
            _check(fix, mov, "oblique", f"two workgroups stride {stride}", stride=stride)
        _check(fix, mov, "scaled", "two workgroups, everything inside", bins=8)
    finally:
        L.query("pcms_stream_grid_cap", old)
    assert L.query("pcms_stream_grid_cap", -1) == old


def test_stable_from_run_to_run_and_ignores_the_workspace():
    L = _lib()
    fix, mov = _mr_pair(LARGE)
    A, t = _affine("oblique", *LARGE)
    fl, ml = _minmax(fix), _minmax(mov)
    work = _Guarded(L.query("pcms_joint_histogram_work_bytes", 32), torch.uint8, 0xFF)
    runs = [_device_hist(fix, mov, A, t, fl, ml, work=work),          # 0xFF bytes
            _device_hist(fix, mov, A, t, fl, ml, work=work),          # what the first run left there
            _device_hist(fix, mov, A, t, fl, ml, fill=0x00), _device_hist(fix, mov, A, t, fl, ml, fill=0x5A)]
    for r in runs[1:]:
        assert r.tobytes() == runs[0].tobytes()
    assert np.array_equal(runs[0], _host_hist(fix, mov, A, t, fl, ml))


def test_the_wrapper_equals_the_host_form():
    data, predict = _mods()
    fix, mov = _mr_pair(LARGE)
    A, t = _affine("oblique", *LARGE)
    raws = [data.RawVolume(torch.from_numpy(v.reshape(-1).view(np.uint8).copy()), _code(v.dtype), v.shape, 1.0, 0.0)
            for v in (fix, mov)]
    with pytest.raises(RuntimeError):
        predict.joint_histogram_device(raws[0], raws[1], A, t, _minmax(fix), _minmax(mov))     # host bytes
    dev = [r.to(DEV) for r in raws]
    got = predict.joint_histogram_device(dev[0], dev[1], A, t, _minmax(fix), _minmax(mov), 16, (1, 2, 2))
    assert got.dtype == torch.int64 and tuple(got.shape) == (16, 16) and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), predict.joint_histogram(fix, mov, A, t, _minmax(fix), _minmax(mov), 16,
                                                                     (1, 2, 2)))
    lohi = torch.from_numpy(_minmax(mov)).to(DEV)                                              # device windows
    again = predict.joint_histogram_device(dev[0], dev[1], A, t, torch.from_numpy(_minmax(fix)).to(DEV), lohi, 16,
                                           (1, 2, 2))
    assert torch.equal(got, again)
    with pytest.raises(ValueError):
        predict.joint_histogram_device(dev[0], dev[1], A, t, _minmax(fix), _minmax(mov), 65)


def test_bad_arguments():
    L = _lib()
    lib, S = L.load(), L.stream()
    assert lib.pcms_joint_histogram_work_bytes(1) < 0 and lib.pcms_joint_histogram_work_bytes(65) < 0
    assert lib.pcms_joint_histogram_work_bytes(-4) < 0 and lib.pcms_joint_histogram_work_bytes(2) == 128
    assert lib.pcms_joint_histogram_work_bytes(64) == 8 * 64 * 64 * 4
    src = torch.zeros(4 * 4 * 4 * 8 + 16, dtype=torch.uint8, device=DEV)
    lohi = torch.tensor([0.0, 1.0, 0.0, 1.0], device=DEV)
    hist = _Guarded(64 * 64 + 4, torch.int32, -1)
    work = _Guarded(8 * 64 * 64 * 4 + 16, torch.uint8, 0xFF)
    sp, lp, hp, wp = src.data_ptr(), lohi.data_ptr(), hist.out.data_ptr(), work.out.data_ptr()
    good = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    nan = (ctypes.c_double * 12)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1, 0, 0, 0)
    inf = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, float("-inf"), 0)
    GA = ctypes.addressof(good)

    def run(fix=sp, fcode=4, F=(4, 4, 4), flohi=lp, mov=sp, mcode=4, M=(4, 4, 4), mlohi=lp + 8, aff=GA,
            stride=(1, 1, 1), bins=8, hist=hp, work=wp):
        return lib.pcms_joint_histogram(fix, fcode, *F, 1.0, 0.0, flohi, mov, mcode, *M, 1.0, 0.0, mlohi, aff, *stride,
                                        bins, hist, work, S)

    for kw in [dict(bins=1), dict(bins=65), dict(bins=0), dict(bins=-8),
               dict(stride=(0, 1, 1)), dict(stride=(1, -1, 1)), dict(stride=(1, 1, 0)),
               dict(F=(2048, 2048, 512)), dict(F=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)),   # 2^31 voxels and beyond
               dict(F=(4096, 4096, 256), stride=(1, 1, 2)),                                  # ... after the stride too
               dict(F=(0, 4, 4)), dict(F=(4, -1, 4)), dict(M=(4, 4, 0)), dict(M=(-4, 4, 4)),
               dict(fix=None), dict(mov=None), dict(flohi=None), dict(mlohi=None), dict(aff=None), dict(hist=None),
               dict(work=None),
               dict(fix=sp + 1), dict(mov=sp + 1), dict(fcode=16, fix=sp + 2), dict(mcode=64, mov=sp + 4),
               dict(flohi=lp + 2), dict(mlohi=lp + 1), dict(hist=hp + 2), dict(work=wp + 2),
               dict(fcode=3), dict(mcode=32), dict(fcode=0), dict(mcode=-1),
               dict(aff=ctypes.addressof(nan)), dict(aff=ctypes.addressof(inf))]:
        assert run(**kw) < 0, kw
    hist.check(written=False)
    work.check(written=False)
    # the same tables accept a good call, also with element-aligned pointers off the 16-byte boundary
    assert run() == 0 and run(fix=sp + 2, mov=sp + 6, hist=hp + 4, work=wp + 4, fcode=512, mcode=4) == 0
    assert run(F=(4, 4, 4), stride=(5, 7, 9), bins=64) == 0 and run(fcode=2, fix=sp + 1, mcode=256, mov=sp + 3) == 0
    torch.cuda.synchronize()
    hist.check()
