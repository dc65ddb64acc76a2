"""pcms_volume_window / pcms_resample_linear_window / pcms_patch_resample_window at the C ABI
against predict.py's host forms (intensity_window, normalise_window over data.resample and
data.resample_patch), on the bits: the select is exact and the consumers restate the host
arithmetic operation for operation, so there is no tolerance (a selected NaN is compared as a NaN,
not on its payload).  Outputs are NaN-filled between two guard bands; the select's workspace is
handed over filled with 0xFF bytes, so a call that relies on a zeroed workspace fails."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_predict_ops import _Guarded, _code, _minmax, _mods, _upload
from tests.test_resample_ops import CODES, SHAPES, _decode, _same_bits, _typed_source

pytestmark = pytest.mark.gpu

WINDOWS = [(0.5, 99.5), (25.0, 75.0), (0.0, 100.0), (49.9999, 50.0)]   # the last: ppm_hi - ppm_lo == 1


def _ppm(p):
    return int(round(p * 10000))


def _window(src, lower=0.5, upper=99.5, above=None, slope=1.0, inter=0.0, offset=0, fill=0xFF, work=None):
    """lohi of the entry point on ``src``'s bytes; the workspace ``fill``-filled between guards."""
    L = _lib()
    keep, ptr = _upload(src, offset)
    n = src.size
    nbytes = L.query("pcms_volume_window_work_bytes", n)
    assert nbytes > 0 and nbytes % 8 == 0
    lohi = _Guarded(2)
    work = _Guarded(nbytes, torch.uint8, fill) if work is None else work
    assert work.out.data_ptr() % 8 == 0
    L.call("pcms_volume_window", ptr, _code(src.dtype), n, float(slope), float(inter), _ppm(lower), _ppm(upper),
           0 if above is None else 1, 0.0 if above is None else float(above), lohi.out, work.out)
    work.check()
    return lohi.check().numpy()


def _host(src, lower=0.5, upper=99.5, above=None, slope=1.0, inter=0.0):
    return _mods()[1].intensity_window(_decode(src, slope, inter), lower, upper, above)


def _same_lohi(got, exp, what):
    assert got.dtype == exp.dtype == np.float32 and got.shape == exp.shape == (2,)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), (what, got, exp)
    assert np.array_equal(got[~nan].view(np.int32), exp[~nan].view(np.int32)), (what, got, exp)


def _check(src, what, windows=WINDOWS, **kw):
    for lower, upper in windows:
        _same_lohi(_window(src, lower, upper, **kw), _host(src, lower, upper, **{k: v for k, v in kw.items()
                                                                                  if k in ("above", "slope", "inter")}),
                   f"{what} window ({lower}, {upper}) {kw}")


@pytest.mark.parametrize("code", CODES)
def test_window_every_datatype(code):
    """Sizes around the 256-thread workgroup and the 16-byte vector, one and two elements, two
    workgroups (4099) and many (70001); the pointer element-aligned but off the 16-byte boundary,
    with a body and as seven head elements alone."""
    for n in (1, 2, 255, 256, 257, 4099, 70001):
        src = _typed_source(code, (n,), 500 + code + n)
        _check(src, f"datatype {code} n {n}", windows=[(0.5, 99.5)])
    src = _typed_source(code, (4099,), 600 + code)
    _check(src, f"datatype {code} offset 1", windows=[(0.5, 99.5), (25.0, 75.0)], offset=1)
    _check(src[:7], f"datatype {code} offset 1, all head", windows=[(0.5, 99.5), (0.0, 100.0)], offset=1)
    _check(src, f"datatype {code} above", windows=[(0.5, 99.5)], above=0.0)


def test_window_scaled_sources():
    """A negative scl_slope turns the order round; slope 0 means 1."""
    src = np.random.default_rng(7).integers(-3000, 3000, size=4099).astype(np.int16)
    _check(src, "negative slope", slope=-0.37, inter=12.5)
    _check(src, "negative slope, above", slope=-0.37, inter=12.5, above=100.0)
    _check(src, "slope 0", slope=0.0, inter=2.0)
    exp = _host(src, 0, 100, slope=-0.37, inter=12.5)
    assert exp[0] == np.float32(src.max() * -0.37 + 12.5)


def _f32_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def _distribution(name):
    rng = np.random.default_rng(40 + len(name))
    n = 4099
    if name == "all_equal":
        return np.full(n, 3.25, np.float32)
    if name == "all_zero":
        return np.zeros(n, np.int16)
    if name == "two_values":
        return np.where(rng.random(n) < 0.3, -2.5, 4.0).astype(np.float32)
    if name == "mostly_one_value":
        v = np.where(rng.random(n) < 0.9, 0, rng.integers(50, 901, size=n)).astype(np.int16)
        v[1234] = 30000
        return v
    if name == "last_digit":  # keys equal down to the last pass, all 256 digits of it present
        return _f32_bits(np.float32(1000.0).view(np.uint32) & np.uint32(0xFFFFFF00) | rng.integers(0, 256, size=n))
    if name == "last_digit_negative":
        return _f32_bits(np.float32(-1000.0).view(np.uint32) & np.uint32(0xFFFFFF00) | rng.integers(0, 256, size=n))
    if name == "around_zero":   # both signed zeros, the smallest denormals and normals of both signs
        v = rng.standard_normal(n).astype(np.float32)
        v[rng.random(n) < 0.2] = -0.0
        v[rng.random(n) < 0.2] = 0.0
        v[:8] = _f32_bits([1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0, 0x80000000])
        return v
    if name == "signed_zeros_only":
        return np.where(rng.random(n) < 0.5, -0.0, 0.0).astype(np.float32)
    if name == "infinities":
        v = (1000.0 * rng.standard_normal(n)).astype(np.float32)
        v[[0, 5, 2000, n - 1]] = (np.inf, -np.inf, np.inf, -np.inf)
        return v
    raise KeyError(name)


@pytest.mark.parametrize("name", ["all_equal", "all_zero", "two_values", "mostly_one_value", "last_digit",
                                  "last_digit_negative", "around_zero", "signed_zeros_only", "infinities"])
def test_window_distributions_that_break_a_radix_select(name):
    src = _distribution(name)
    _check(src, name, offset=1)
    _check(src, name + " above 0", windows=[(0.5, 99.5), (0.0, 100.0)], above=0.0)
    if name == "signed_zeros_only":  # +0.0 on the bits, whichever zero sits at the rank
        assert np.array_equal(_window(src, 49.0, 51.0).view(np.int32), np.zeros(2, np.int32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("at", [0, 1, 2000, 4098], ids=["element0", "head", "body", "tail"])
def test_window_nan_orders_last(dtype, at):
    f = (100.0 * np.random.default_rng(8).standard_normal(4099)).astype(dtype)
    f[at] = np.nan
    exp = _host(f, 0, 100)
    assert np.isnan(exp[1]) and not np.isnan(exp[0])
    _same_lohi(_window(f, 0, 100, offset=1), exp, f"nan at {at}")
    _check(f, f"nan at {at}", windows=[(0.5, 99.5), (25.0, 75.0)], offset=1)
    _check(f, f"nan at {at} above", windows=[(0.0, 100.0)], above=-1e30, offset=1)   # above never keeps a NaN
    f[::3] = np.nan                                                                 # a third NaN: hi is one
    exp = _host(f, 25, 75)
    assert np.isnan(exp[1]) and not np.isnan(exp[0])
    _same_lohi(_window(f, 25, 75), exp, "a third NaN")


@pytest.mark.parametrize("code", [2, 4, 16, 64, 1280])
def test_full_window_is_the_minmax_pair(code):
    for n in (1, 257, 4099, 70001):
        src = _typed_source(code, (n,), 900 + code + n)
        got = _window(src, 0, 100)
        mm = _minmax(src)
        assert np.array_equal((got + np.float32(0)).view(np.int32), (mm + np.float32(0)).view(np.int32)), (code, n)
        _same_lohi(got, _host(src, 0, 100), f"full window {code} {n}")


def test_above_selects_nothing_one_voxel_and_everything():
    src = np.random.default_rng(12).integers(-500, 3000, size=4099).astype(np.int16)
    src[77] = 3001                                     # the only voxel above 3000
    for above, m in ((3001.0, 0), (3000.0, 1), (-501.0, src.size)):
        assert int((src > above).sum()) == m
        for lower, upper in WINDOWS:
            got = _window(src, lower, upper, above=above, offset=1)
            _same_lohi(got, _host(src, lower, upper, above=above), f"above {above}")
            if m == 0:
                assert np.array_equal(got.view(np.int32), np.zeros(2, np.int32))
            if m == 1:
                assert np.array_equal(got, np.float32([3001, 3001]))


def test_window_under_a_capped_grid():
    """n = 70001 on two workgroups: every thread makes many trips through the vector body."""
    L = _lib()
    old = L.query("pcms_stream_grid_cap", 2)
    try:
        for code in (2, 4, 16, 64):
            src = _typed_source(code, (70001,), 1300 + code)
            _check(src, f"capped grid datatype {code}", windows=[(0.5, 99.5), (25.0, 75.0)], offset=1)
            _check(src, f"capped grid datatype {code} above", windows=[(0.5, 99.5)], above=0.0)
        _check(_distribution("mostly_one_value"), "capped grid, mostly one value")
    finally:
        L.query("pcms_stream_grid_cap", old)
    assert L.query("pcms_stream_grid_cap", -1) == old


def test_window_is_stable_from_run_to_run_and_ignores_the_workspace():
    for src in (_typed_source(4, (70001,), 1400), _typed_source(16, (70001,), 1401), _distribution("mostly_one_value")):
        n = src.size
        work = _Guarded(_lib().query("pcms_volume_window_work_bytes", n), torch.uint8, 0xFF)
        runs = [_window(src, work=work),             # 0xFF bytes
                _window(src, work=work),             # what the first run left there
                _window(src, fill=0x00), _window(src, fill=0x5A), _window(src)]
        for r in runs[1:]:
            assert np.array_equal(r.view(np.int32), runs[0].view(np.int32)), runs
        _same_lohi(runs[0], _host(src), "run stability")


# ---------------- the consumers ----------------
def _inside_pair(vol):
    """A (lo, hi) strictly inside the data range: the quartiles."""
    s = np.sort(np.asarray(vol, np.float32).reshape(-1))
    return np.array([s[s.size // 4], s[(3 * s.size) // 4]], np.float32)


def _resample_window(src, target, lohi, slope=1.0, inter=0.0):
    L = _lib()
    keep, ptr = _upload(src)
    out = _Guarded(int(np.prod(target)))
    L.call("pcms_resample_linear_window", ptr, _code(src.dtype), *src.shape, float(slope), float(inter),
           torch.from_numpy(np.asarray(lohi, np.float32)).to(DEV), out.out, *target)
    got = out.check()
    assert not torch.isnan(got).any(), "an output element was not written"
    return got.view(*target)


def _consumer_source(kind, shape):
    rng = np.random.default_rng(1700 + shape[0] * 31 + shape[1] * 7 + shape[2])
    if kind == "int16":
        return rng.integers(-3000, 3000, size=shape).astype(np.int16)
    if kind == "uint8":
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    return (1000.0 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("kind", ["int16", "uint8", "float32"])
@pytest.mark.parametrize("shape,target", SHAPES)
def test_resample_window_shapes(shape, target, kind):
    data, predict = _mods()
    src = _consumer_source(kind, shape)
    for slope, inter in ((1.0, 0.0), (-0.37, 12.5)):
        vol = np.asarray(_decode(src, slope, inter)).astype(np.float32)
        lohi = _inside_pair(vol)
        if src.size > 1:  # both sides of the clip are hit
            assert (vol < lohi[0]).any() and (vol > lohi[1]).any() and lohi[0] < lohi[1]
        exp = data.resample(predict.normalise_window(vol, lohi), target)
        assert exp.min() >= 0 and exp.max() <= 1 and (src.size == 1 or exp.max() > 0.5)
        _same_bits(_resample_window(src, target, lohi, slope, inter), exp, f"window {kind} {shape}->{target} x{slope}")
    pair = np.float32([37, 37])                                  # den == 0 with lo != 0
    _same_bits(_resample_window(src, target, pair), np.zeros(target, np.float32), f"den 0 {kind} {shape}->{target}")


def test_resample_window_reads_the_select_from_device_memory():
    """pcms_volume_window -> pcms_resample_linear_window with nothing in between, and a NaN voxel."""
    L = _lib()
    data, predict = _mods()
    shape, target = (20, 18, 24), (32, 32, 16)
    src = _consumer_source("float32", shape)
    src[3, 4, 5] = np.nan
    src[7, 7, 7] = 1e9
    keep, ptr = _upload(src)
    lohi = torch.full((2,), float("nan"), device=DEV)
    work = torch.full((L.query("pcms_volume_window_work_bytes", src.size),), 0xFF, dtype=torch.uint8, device=DEV)
    out = _Guarded(int(np.prod(target)))
    L.call("pcms_volume_window", ptr, 16, src.size, 1.0, 0.0, 5000, 995000, 0, 0.0, lohi, work)
    L.call("pcms_resample_linear_window", ptr, 16, *shape, 1.0, 0.0, lohi, out.out, *target)
    got = out.check().view(*target)
    exp = data.resample(predict.Normalisation("percentile").apply(src), target)
    assert np.isnan(exp).any() and np.nanmin(exp) >= 0.0 and 0.9 < np.nanmax(exp) <= 1.0
    nan = torch.from_numpy(np.isnan(exp))
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(torch.int32), torch.from_numpy(exp)[~nan].view(torch.int32))


SRC_SHAPE, GRID = (11, 29, 23), (12, 40, 40)
ORIGINS = [(0, 0, 0), (0, 24, 24), (0, 7, 13), (-4, 33, -6)]
DTYPES = {"u8": (np.uint8, 1.0, 0.0), "i16": (np.int16, 1.0, 0.0), "f32": (np.float32, 1.0, 0.0),
          "f64_scaled": (np.float64, 0.5, -3.0)}


@functools.lru_cache(maxsize=None)
def _patch_source(kind):
    dtype = DTYPES[kind][0]
    rng = np.random.default_rng(len(kind) + 150)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=SRC_SHAPE).astype(dtype)
    if dtype == np.int16:
        return rng.integers(-500, 3000, size=SRC_SHAPE).astype(dtype)
    return (1000.0 * rng.standard_normal(SRC_SHAPE)).astype(dtype)


@functools.lru_cache(maxsize=None)
def _affine(which):
    d = _mods()[0]
    if which == "identity":
        return d.volume_affine(np.eye(3), np.zeros(3), SRC_SHAPE, GRID)
    return d.volume_affine(d.compose_transform((True, False, True), (8.0, -5.0, 12.0), 1.15),
                           np.array([0.7, -2.2, 1.4]), SRC_SHAPE, GRID)


def _run_patches(kind, which, patch, gain=1.0, bias=0.0, stride_mul=1, offset=0, den0=False):
    """(got (P, wd, wh, ww), expected): pcms_patch_resample_window into a poisoned, guarded buffer
    ``offset`` floats off its alignment, patches ``stride_mul`` D H W floats apart; lohi is the
    volume's (25, 75) percentile window, or a den == 0 pair."""
    (d, predict), L = _mods(), _lib()
    src = _patch_source(kind)
    _, slope, inter = DTYPES[kind]
    vol = np.asarray(_decode(src, slope, inter)).astype(np.float32)
    A, t = _affine(which)
    norm = predict.Normalisation("percentile", 25.0, 75.0)
    lohi = np.float32([37, 37]) if den0 else predict.intensity_window(vol, 25.0, 75.0)
    if not den0:
        assert vol.min() < lohi[0] < lohi[1] < vol.max()
    raw = torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).to(DEV)
    P, nwin = len(ORIGINS), int(np.prod(patch))
    stride = stride_mul * nwin
    out = _Guarded((P - 1) * stride + nwin + offset)
    assert out.out.data_ptr() % 16 == 0
    host = (ctypes.c_double * 12)(*A.reshape(-1).tolist(), *t.tolist())  # read during the call
    L.call("pcms_patch_resample_window", raw, _code(src.dtype), *src.shape, float(slope), float(inter),
           ctypes.addressof(host), torch.from_numpy(lohi).to(DEV), float(gain), float(bias), *GRID,
           torch.tensor(ORIGINS, dtype=torch.int32, device=DEV), P, out.out.data_ptr() + 4 * offset, stride, *patch)
    flat = out.check()
    assert torch.isnan(flat[:offset]).all(), "the floats before the output were written"
    flat = flat[offset:]
    got = torch.stack([flat[p * stride:p * stride + nwin] for p in range(P)]).view(P, *patch)
    assert not torch.isnan(got).any(), "an output element was not written"
    for p in range(P - 1):
        assert torch.isnan(flat[p * stride + nwin:(p + 1) * stride]).all(), "written between two patches"
    if den0:
        exp = np.stack([d._resample_patch(np.zeros_like(vol), GRID, A, t, o, patch, gain, bias) for o in ORIGINS])
    else:
        exp = np.stack([d.resample_patch(vol, GRID, A, t, o, patch, gain=gain, bias=bias, normalise=norm)
                        for o in ORIGINS])
    return got, exp


@pytest.mark.parametrize("which", ["identity", "flip_rot_zoom"])
@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_window_patches_equal_host(kind, which):
    for patch, gain, bias in (((16, 16, 16), 1.0, 0.0), ((16, 16, 18), 1.25, -3.5)):
        got, exp = _run_patches(kind, which, patch, gain, bias)
        assert np.count_nonzero(exp) > exp.size // 4 and not exp[3, :4].any()
        _same_bits(got, exp, f"window patch {kind} {which} {patch} gain {gain} bias {bias}")
    got, exp = _run_patches(kind, which, (16, 16, 16), 1.25, -3.5, den0=True)
    _same_bits(got, exp, f"window patch den 0 {kind} {which}")


@pytest.mark.parametrize("patch", [(16, 16, 16), (16, 16, 18)], ids=["vector", "scalar"])
def test_window_patch_stride_and_misaligned_output(patch):
    for stride_mul, offset in ((5, 0), (1, 1), (5, 3)):
        got, exp = _run_patches("i16", "flip_rot_zoom", patch, 1.25, -3.5, stride_mul, offset)
        _same_bits(got, exp, f"window patch stride x{stride_mul} offset {offset} {patch}")


# ---------------- rejections ----------------
def test_window_bad_arguments():
    L = _lib()
    lib, S = L.load(), L.stream()
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    nbytes = L.query("pcms_volume_window_work_bytes", 8)
    lohi, work, out = _Guarded(2), _Guarded(nbytes + 8, torch.uint8, 0xFF), _Guarded(64)
    s, lh, wk, o = (t.data_ptr() for t in (src, lohi.out, work.out, out.out))
    assert lib.pcms_volume_window_work_bytes(0) < 0 and lib.pcms_volume_window_work_bytes(-3) < 0
    assert lib.pcms_volume_window_work_bytes(2 ** 31) < 0 and lib.pcms_volume_window_work_bytes(2 ** 31 - 1) == nbytes

    def select(src=s, code=4, n=8, lo=5000, hi=995000, use=0, above=0.0, lohi=lh, work=wk):
        return lib.pcms_volume_window(src, code, n, 1.0, 0.0, lo, hi, use, above, lohi, work, S)

    for kw in [dict(code=3), dict(code=32), dict(n=0), dict(n=-5), dict(n=2 ** 31),
               dict(src=None), dict(lohi=None), dict(work=None),
               dict(src=s + 1), dict(lohi=lh + 2), dict(work=wk + 4),
               dict(lo=-1), dict(hi=1000001), dict(lo=500000, hi=500000), dict(lo=600000, hi=400000),
               dict(use=1, above=float("inf")), dict(use=1, above=float("-inf")), dict(use=1, above=float("nan"))]:
        assert select(**kw) < 0, kw
    for args in [(s, 3, 1, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1),
                 (s, 4, 0, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, lh, o, 1, -1, 1),
                 (None, 4, 1, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, None, o, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, lh, None, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, lh + 2, o, 1, 1, 1),
                 (s, 4, 1, 1, 1, 1.0, 0.0, lh, o + 2, 1, 1, 1),
                 (s + 1, 4, 1, 1, 1, 1.0, 0.0, lh, o, 1, 1, 1)]:
        assert lib.pcms_resample_linear_window(*args, S) < 0, args
    for g in (lohi, work, out):
        g.check(written=False)
    # the same tables accept a good call; an above that is not used may be anything
    assert select() == 0 and select(above=float("nan")) == 0 and select(lo=0, hi=1, use=1, above=-1.0) == 0
    torch.cuda.synchronize()
    assert lohi.check().tolist() == [0.0, 0.0]


def test_window_patch_bad_arguments():
    L = _lib()
    lib, S = L.load(), L.stream()
    src = torch.zeros(4 * 4 * 4 * 8 + 8, dtype=torch.uint8, device=DEV)
    origins = torch.zeros(65 * 3, dtype=torch.int32, device=DEV)
    lohi = torch.zeros(4, device=DEV)
    out = _Guarded(2 * 512 + 8)
    sp, op, lp, o = src.data_ptr(), origins.data_ptr(), lohi.data_ptr(), out.out.data_ptr()
    good = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    nan = (ctypes.c_double * 12)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1, 0, 0, 0)
    inf = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, float("inf"), 0)
    GA = ctypes.addressof(good)

    def run(src=sp, code=4, Si=(4, 4, 4), slope=1.0, inter=0.0, aff=GA, lohi=lp, gain=1.0, bias=0.0, G=(8, 8, 8),
            origins=op, P=2, out=o, stride=512, D=8, H=8, W=8):
        return lib.pcms_patch_resample_window(src, code, *Si, slope, inter, aff, lohi, gain, bias, *G, origins, P, out,
                                              stride, D, H, W, S)

    for kw in [dict(src=None), dict(out=None), dict(aff=None), dict(origins=None), dict(lohi=None),
               dict(src=sp + 1), dict(code=16, src=sp + 2), dict(code=64, src=sp + 4),
               dict(out=o + 2), dict(origins=op + 2), dict(lohi=lp + 2),
               dict(code=3), dict(code=0),
               dict(Si=(0, 4, 4)), dict(Si=(4, -1, 4)), dict(Si=(4, 4, 0)), dict(D=0), dict(H=-8), dict(W=0),
               dict(G=(0, 8, 8)), dict(G=(8, -1, 8)), dict(G=(8, 8, 0)),
               dict(aff=ctypes.addressof(nan)), dict(aff=ctypes.addressof(inf)),
               dict(gain=float("nan")), dict(bias=float("inf")),
               dict(P=0), dict(P=65), dict(P=-3),
               dict(stride=511), dict(stride=0), dict(stride=-512)]:
        assert run(**kw) < 0, kw
    out.check(written=False)
    assert run() == 0 and run(out=o + 4, stride=513, code=2) == 0   # the same tables accept a good call
    torch.cuda.synchronize()
    out.check()
