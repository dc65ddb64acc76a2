"""pcms_mask_surface / pcms_edt_sq / pcms_surface_distance_stats at the C ABI against predict.py's
host forms (surface, edt_sq), on the bits: the kernels restate the host arithmetic operation for
operation, so the transform has no tolerance and two runs must agree.  Outputs sit between guard
bands.

The H and D passes give a 256-thread workgroup a slab of 32 adjacent w and 8 line positions per
step, the H pass a chunk of 64 positions: 9x65x33 is one voxel past that on every axis.  W = 257
takes the 16-bit W pass (a byte up to 255).  The further shapes take the other kernels: 130 planes
of fp64 and 520 rows of 16-bit integers need the 64 KiB line buffer, 260 planes and 1030 rows
halve the slab."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_predict_ops import _Guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 257), (3, 5, 7), (9, 65, 33), (24, 40, 48)]
SPACINGS = [(1.0, 1.0, 1.0), (3.0, 0.5, 0.5), (3.6, 0.3125, 0.3125), (2.2, 0.7, 0.9)]
CORNERS = [f"corner{c}" for c in range(8)]
PATTERNS = ["zeros", "ones", *CORNERS, "bernoulli0.02", "bernoulli0.3", "plane0", "plane1", "plane2", "last"]
# (shape, why): the kernels the shapes above do not reach
OTHER_PATHS = [((3, 9, 300), "16-bit integers through all three passes"),
               ((130, 3, 5), "D pass: 64 KiB of lines"),
               ((260, 2, 40), "D pass: slab of 16"),
               ((1, 520, 257), "H pass, 16-bit: 64 KiB of lines"),
               ((1, 1030, 3), "H pass, bytes: 64 KiB of lines"),
               ((1, 1030, 260), "H pass, 16-bit: slab of 16")]


def _predict():
    import pcms_amd  # noqa: F401
    from pcms_amd import predict
    return predict


@functools.lru_cache(maxsize=None)
def _mask(pattern, shape):
    D, H, W = shape
    d, h, w = np.indices(shape)
    m = np.zeros(shape, np.uint8)
    if pattern == "ones":
        m[:] = 255  # foreground is != 0
    elif pattern.startswith("corner"):
        c = int(pattern[len("corner"):])
        m[(D - 1) * (c >> 2 & 1), (H - 1) * (c >> 1 & 1), (W - 1) * (c & 1)] = 1
    elif pattern.startswith("bernoulli"):
        rng = np.random.default_rng(700 + D + 3 * H + 7 * W)
        m = ((rng.random(shape) < float(pattern[len("bernoulli"):])) * rng.integers(1, 256, size=shape)).astype(np.uint8)
    elif pattern.startswith("plane"):
        axis = int(pattern[len("plane"):])
        m[(d, h, w)[axis] == shape[axis] // 2] = 1
    elif pattern == "last":  # features in the last row, plane and column only: the three edges at the far corner
        m[((d == D - 1).astype(int) + (h == H - 1) + (w == W - 1)) >= 2] = 1
    elif pattern == "box":  # hollow, one-voxel walls one voxel inside the volume
        m[1:D - 1, 1:H - 1, 1:W - 1] = 1
        m[2:D - 2, 2:H - 2, 2:W - 2] = 0
    elif pattern == "values":  # every nonzero byte value is foreground
        m = (h % 6 != 0).astype(np.uint8) * (1 + (d * 31 + h * 17 + w) % 255).astype(np.uint8)
    else:
        assert pattern == "zeros", pattern
    return m


@functools.lru_cache(maxsize=None)
def _host_edt(pattern, shape, spacing):
    return _predict().edt_sq(_mask(pattern, shape), spacing)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _work(shape):
    n = _lib().query("pcms_edt_work_bytes", *shape)
    assert n >= int(np.prod(shape)) and n % 8 == 0
    return _Guarded(n, torch.uint8, 0x5A)


def _spacing(sp):
    return (ctypes.c_double * 3)(*sp)


def _device_edt(mask, spacing):
    """Two runs on fresh buffers; the first after checking that both agree on the bits."""
    L = _lib()
    dev = _dev(mask)
    before = dev.clone()
    runs = []
    for _ in range(2):
        out, work = _Guarded(mask.size, torch.float64), _work(mask.shape)
        sp = _spacing(spacing)
        L.call("pcms_edt_sq", dev, ctypes.addressof(sp), out.out, work.out, *mask.shape)
        work.check()
        runs.append(out.check().view(*mask.shape).numpy())
    assert torch.equal(dev, before), "the input was written"
    assert np.array_equal(runs[0].view(np.int64), runs[1].view(np.int64)), "two runs differ"
    return runs[0]


def _same_bits(got, exp, what):
    assert got.dtype == exp.dtype == np.float64 and got.shape == exp.shape, what
    diff = got.view(np.int64) != exp.view(np.int64)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {got.size} voxels differ"


# ---- the transform ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_edt_sq_equals_host_on_the_bits(shape, pattern):
    mask = _mask(pattern, shape)
    for spacing in SPACINGS:
        got = _device_edt(mask, spacing)
        _same_bits(got, _host_edt(pattern, shape, spacing), f"{pattern} {shape} {spacing}")
        if pattern == "zeros":
            assert np.isposinf(got).all()


@pytest.mark.parametrize("shape,why", OTHER_PATHS)
def test_edt_sq_other_kernel_paths(shape, why):
    for pattern, spacing in (("bernoulli0.02", SPACINGS[2]), ("corner7", SPACINGS[3])):
        _same_bits(_device_edt(_mask(pattern, shape), spacing), _host_edt(pattern, shape, spacing),
                   f"{why}: {pattern} {shape}")


def test_the_patterns_are_what_they_claim():
    for shape in SHAPES:
        assert not _mask("zeros", shape).any() and _mask("ones", shape).all()
        corners = {int(np.flatnonzero(_mask(c, shape))[0]) for c in CORNERS}
        assert all(int(_mask(c, shape).sum()) == 1 for c in CORNERS)
        assert len(corners) == 2 ** sum(s > 1 for s in shape)
        last = np.argwhere(_mask("last", shape))
        assert len(last) and all(sum(int(i == s - 1) for i, s in zip(p, shape)) >= 2 for p in last)
    for shape in SHAPES[3:]:
        sparse, dense = ((_mask(f"bernoulli{p}", shape) != 0).mean() for p in ("0.02", "0.3"))
        assert 0 < sparse < 0.05 < 0.2 < dense < 0.4
        for axis in range(3):
            assert int(_mask(f"plane{axis}", shape).sum()) == int(np.prod(shape)) // shape[axis]
    # a far corner alone: the longest walks, nothing prunes them
    far = _host_edt("corner7", (24, 40, 48), SPACINGS[0])
    assert far[0, 0, 0] == 23 ** 2 + 39 ** 2 + 47 ** 2


# ---- the surface -----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS + ["box", "values"])
@pytest.mark.parametrize("shape", SHAPES)
def test_surface_equals_host(shape, pattern):
    L = _lib()
    mask = _mask(pattern, shape)
    exp = _predict().surface(mask)
    dev = _dev(mask)
    before = dev.clone()
    runs = []
    for _ in range(2):
        out = _Guarded(mask.size, torch.uint8, 0xAB)
        L.call("pcms_mask_surface", dev, out.out, *shape)
        runs.append(out.check().view(*shape).numpy())
    assert torch.equal(dev, before) and np.array_equal(runs[0], runs[1])
    assert np.array_equal(runs[0], exp), f"{pattern} {shape}: {int((runs[0] != exp).sum())} bytes differ"
    if pattern == "values" and min(shape) > 4:
        assert len(np.unique(mask)) > 50 and 0 < int(exp.sum()) < int((mask != 0).sum())
    if pattern == "box" and min(shape) > 4:
        assert np.array_equal(exp, mask)  # one-voxel walls: all surface


# ---- the statistics --------------------------------------------------------------------------
def _ellipsoid(shape, centre, radii):
    d, h, w = np.indices(shape)
    return ((((d - centre[0]) / radii[0]) ** 2 + ((h - centre[1]) / radii[1]) ** 2
             + ((w - centre[2]) / radii[2]) ** 2) <= 1.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pair(kind):
    if kind == "ellipsoids":
        shape = (24, 40, 48)
        return _ellipsoid(shape, (11, 18, 22), (7, 12, 15)), _ellipsoid(shape, (13, 22, 27), (6, 13, 12))
    shape = (9, 65, 33) if kind == "bernoulli small" else (24, 40, 48)
    rng = np.random.default_rng(len(kind))
    return tuple((rng.random(shape) < 0.4).astype(np.uint8) * np.uint8(k) for k in (1, 9))


@pytest.mark.parametrize("kind", ["ellipsoids", "bernoulli small", "bernoulli"])
@pytest.mark.parametrize("spacing", SPACINGS[1:3])
def test_surface_distance_stats(kind, spacing):
    L = _lib()
    predict = _predict()
    a, b = _pair(kind)
    shape = a.shape
    for x, y in ((a, b), (b, a)):
        sx, sy = predict.surface(x) != 0, predict.surface(y)
        assert sx.any() and sy.any(), "both surfaces are non-empty"
        sq = predict.edt_sq(sy, spacing)
        exp_sd = np.where(sx, sq, -1.0)
        exp_sum = math.fsum(np.sqrt(sq[sx]).tolist())
        dx, dsq = _dev(x), _dev(sq)
        runs = []
        for _ in range(2):
            sd, stats, work = _Guarded(x.size, torch.float64), _Guarded(3, torch.float64), _work(shape)
            L.call("pcms_surface_distance_stats", dx, dsq, sd.out, stats.out, work.out, *shape)
            work.check()
            runs.append((sd.check().view(*shape).numpy(), stats.check().numpy()))
        (sd0, st0), (sd1, st1) = runs
        _same_bits(sd0, exp_sd, f"{kind} {spacing}")
        assert np.array_equal(sd0.view(np.int64), sd1.view(np.int64))
        assert np.array_equal(st0.view(np.int64), st1.view(np.int64)), "the statistics differ between two runs"
        count, mx, total = int(st0.view(np.int64)[0]), float(st0[1]), float(st0[2])
        print(f"{kind} {spacing}: count {count} max {mx!r} sum {total!r} (fsum {exp_sum!r}, "
              f"rel {abs(total - exp_sum) / exp_sum:.3e})")
        assert count == int(sx.sum()) and count <= 2 ** 20
        assert mx == float(sq[sx].max())
        assert abs(total - exp_sum) <= 1e-9 * exp_sum


def test_surface_distance_stats_without_a_surface():
    """No surface voxel in a: count 0, max -1.0 (the largest of an all -1.0 output), sum 0.0."""
    L = _lib()
    shape = (3, 5, 7)
    n = int(np.prod(shape))
    sd, stats, work = _Guarded(n, torch.float64), _Guarded(3, torch.float64), _work(shape)
    L.call("pcms_surface_distance_stats", torch.zeros(n, dtype=torch.uint8, device=DEV),
           torch.ones(n, dtype=torch.float64, device=DEV), sd.out, stats.out, work.out, *shape)
    work.check()
    assert bool((sd.check() == -1.0).all())
    st = stats.check().numpy()
    assert int(st.view(np.int64)[0]) == 0 and st[1] == -1.0 and st[2] == 0.0


# ---- rejections ------------------------------------------------------------------------------
def test_bad_arguments():
    L = _lib()
    lib = L.load()
    S = L.stream()
    shape = (3, 5, 7)
    n = int(np.prod(shape))
    src = torch.ones(n, dtype=torch.uint8, device=DEV)
    sq = torch.ones(n, dtype=torch.float64, device=DEV)
    surf = _Guarded(n, torch.uint8, 0xAB)
    out, sd, stats = _Guarded(n, torch.float64), _Guarded(n, torch.float64), _Guarded(3, torch.float64)
    work = _work(shape)
    m, q, sf, o, d, st, wk = (t.data_ptr() for t in (src, sq, surf.out, out.out, sd.out, stats.out, work.out))
    good = _spacing((3.0, 0.5, 0.5))
    sp = ctypes.addressof(good)
    assert lib.pcms_edt_work_bytes(0, 5, 7) < 0 and lib.pcms_edt_work_bytes(3, -5, 7) < 0
    assert lib.pcms_edt_work_bytes(2049, 5, 7) < 0 and lib.pcms_edt_work_bytes(3, 5, 2049) < 0  # an axis past 2048
    assert lib.pcms_edt_work_bytes(2048, 2048, 2048) < 0                                          # too many voxels
    assert lib.pcms_edt_work_bytes(2048, 3, 2048) > 0
    for args in [(None, sf, *shape), (m, None, *shape), (m, sf, 0, 5, 7), (m, sf, 3, 5, -7), (m, sf, 3, 2049, 7),
                 (sf, sf, *shape),                       # out aliases mask
                 (sf + 1, sf, 1, 1, n - 1)]:             # ... or overlaps it
        assert lib.pcms_mask_surface(*args, S) < 0, args
    bad_spacings = [(0.0, 1.0, 1.0), (1.0, -0.5, 1.0), (1.0, 1.0, math.nan), (math.inf, 1.0, 1.0), (1.0, -math.inf, 1.0)]
    keep = [_spacing(b) for b in bad_spacings]
    for args in [(None, sp, o, wk, *shape), (m, None, o, wk, *shape), (m, sp, None, wk, *shape),
                 (m, sp, o, None, *shape),
                 (m, sp, o + 4, wk, *shape),             # misaligned out
                 (m, sp, o, wk + 4, *shape),             # misaligned work
                 (m, sp, o, wk, 0, 5, 7), (m, sp, o, wk, 3, 5, 0), (m, sp, o, wk, 3, 5, 2049),
                 (m, sp, o, wk, 2048, 2048, 2048),
                 (o, sp, o, wk, *shape),                 # out overlaps feat
                 (o + 7, sp, o, wk, 1, 1, 1),
                 (wk, sp, o, wk, *shape),                # work overlaps feat
                 (m, sp, o, o + 8, *shape),              # work overlaps out
                 *[(m, ctypes.addressof(k), o, wk, *shape) for k in keep]]:
        assert lib.pcms_edt_sq(*args, S) < 0, args
    for args in [(None, q, d, st, wk, *shape), (m, None, d, st, wk, *shape), (m, q, None, st, wk, *shape),
                 (m, q, d, None, wk, *shape), (m, q, d, st, None, *shape),
                 (m, q + 4, d, st, wk, *shape), (m, q, d + 4, st, wk, *shape), (m, q, d, st + 4, wk, *shape),
                 (m, q, d, st, wk + 4, *shape),
                 (m, q, d, st, wk, 3, 0, 7), (m, q, d, st, wk, 2049, 5, 7),
                 (m, d, d, st, wk, *shape),              # sd_sq_out aliases sq_b
                 (d, q, d, st, wk, *shape),              # ... overlaps mask_a
                 (m, q, d, d + 8, wk, *shape),           # stats inside sd_sq_out
                 (m, q, d, st, d, *shape),               # work over sd_sq_out
                 (m, st, d, st, wk, 1, 1, 1)]:           # stats over sq_b
        assert lib.pcms_surface_distance_stats(*args, S) < 0, args
    for g in (surf, out, sd, stats, work):
        g.check(written=False)
    assert bool((src == 1).all()) and bool((sq == 1).all())
