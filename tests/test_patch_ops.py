"""pcms_foreground_pick / pcms_patch_resample_linear at the C ABI against data.py's host forms
(pick_origins, resample_patch), on the bits: the kernels restate the host rules operation for
operation, so there is no tolerance.  Outputs are poisoned (NaN for floats, a sentinel for ints)
between two guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib
from tests.test_predict_ops import _Guarded
from tests.test_resample_ops import _decode, _same_bits

pytestmark = pytest.mark.gpu

POISON = -123456


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


# ---------------- pick ----------------
# below one chunk; a ragged tail with n % 4 == 1; 262 chunks, so the scan takes two passes
VOLUMES = [(5, 7, 11), (17, 33, 65), (16, 260, 257)]
PATCHES = {(5, 7, 11): (4, 4, 8), (17, 33, 65): (16, 16, 32), (16, 260, 257): (16, 128, 128)}


def _patterns(shape):
    n = int(np.prod(shape))
    rng = np.random.default_rng(n)
    first, last = np.zeros(n, np.float32), np.zeros(n, np.float32)
    first[0], last[n - 1] = 1.0, 0.5
    blob = np.zeros(shape, np.float32)
    blob[shape[0] // 3:shape[0] // 3 + 3, shape[1] // 2:shape[1] // 2 + 5, 1:shape[2] - 1] = 3.0
    return {"first": first.reshape(shape), "last": last.reshape(shape), "all": np.ones(shape, np.float32),
            "none": -np.ones(shape, np.float32), "bernoulli": (rng.random(shape) < 0.01).astype(np.float32),
            "blob": blob}


def _ranks(label, chunk):
    """Ranks 0 and T - 1 and, for the first few chunk boundaries, the last voxel before and the
    first one after, as (r + 0.5) / T."""
    flat = label.reshape(-1) > 0
    T = int(flat.sum())
    if T == 0:
        return [0.0, 0.5, np.nextafter(1.0, 0.0)]
    rs = {0, T - 1}
    prefix = np.cumsum([int(flat[k:k + chunk].sum()) for k in range(0, flat.size, chunk)])[:-1]
    for p in [int(p) for p in prefix if 0 < p < T][:4] + [int(p) for p in prefix if 0 < p < T][-2:]:
        rs |= {p - 1, p}
    return [(r + 0.5) / T for r in sorted(rs)]


def _pick(label, patch, rank_u, fallback, offset=0):
    """pcms_foreground_pick on ``label`` placed ``offset`` floats off a 16-byte boundary."""
    L = _lib()
    n = label.size
    dev = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    assert dev.data_ptr() % 16 == 0
    dev[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(label).reshape(-1)).to(DEV)
    P = len(rank_u)
    rank = torch.from_numpy(np.asarray(rank_u, np.float64)).to(DEV)
    fb = torch.from_numpy(np.ascontiguousarray(fallback, dtype=np.int32)).to(DEV)
    nwork = L.query("pcms_foreground_pick_work_ints", n)
    assert nwork == -(-n // L.query("pcms_foreground_pick_chunk")) + 1
    picks = _Guarded(3 * P + 1, dtype=torch.int32, fill=POISON)
    work = _Guarded(nwork, dtype=torch.int32, fill=POISON)
    L.call("pcms_foreground_pick", dev.data_ptr() + 4 * offset, n, *label.shape, *patch, rank, fb, P, picks.out,
           work.out)
    work.check()
    got = picks.check().numpy()
    assert (got != POISON).all(), "a pick was not written"
    return got[:3 * P].reshape(P, 3), int(got[3 * P])


def _mixed(ranks, shape, patch, P, seed):
    """P ranks cycling through ``ranks``, every third patch a uniform one, and P fallback rows."""
    rng = np.random.default_rng(seed)
    rank_u = [-1.0 if i % 3 == 2 else ranks[(i - i // 3) % len(ranks)] for i in range(P)]
    fallback = np.stack([rng.integers(0, max(g - w, 0) + 1, size=P) for g, w in zip(shape, patch)], 1).astype(np.int32)
    return rank_u, fallback


@pytest.mark.parametrize("shape", VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_pick_equals_host(shape):
    d = _data()
    chunk = _lib().query("pcms_foreground_pick_chunk")
    assert chunk > 0 and chunk % 4 == 0
    assert (int(np.prod(shape)) > 256 * chunk) == (shape == VOLUMES[2])
    patch = PATCHES[shape]
    for name, label in _patterns(shape).items():
        ranks = _ranks(label, chunk)
        assert len(ranks) <= 43  # 64 patches with every third one uniform hold them all
        for P in (64, 1):
            rank_u, fallback = _mixed(ranks if P > 1 else ranks[-1:], shape, patch, P, len(name))
            exp, T = d.pick_origins(label, patch, rank_u, fallback)
            got, count = _pick(label, patch, rank_u, fallback)
            assert count == T == int((label > 0).sum()), (name, P)
            assert np.array_equal(got, exp), (name, P, np.argwhere(got != exp)[:4].tolist())


def test_pick_with_a_misaligned_label():
    """label one float past a 16-byte boundary: every voxel a load of its own."""
    d = _data()
    shape, patch = VOLUMES[1], PATCHES[VOLUMES[1]]
    label = _patterns(shape)["bernoulli"]
    rank_u, fallback = _mixed(_ranks(label, _lib().query("pcms_foreground_pick_chunk")), shape, patch, 64, 5)
    exp, T = d.pick_origins(label, patch, rank_u, fallback)
    for offset in (1, 3):
        got, count = _pick(label, patch, rank_u, fallback, offset=offset)
        assert count == T and np.array_equal(got, exp), offset


def test_pick_does_not_trust_its_tables():
    """A NaN rank and a rank of 2.0 land on the last foreground voxel, a fallback row out of range
    is clamped: the host form after the same clamps."""
    d = _data()
    shape, patch = VOLUMES[1], PATCHES[VOLUMES[1]]
    last = np.nextafter(1.0, 0.0)
    top = np.array([max(g - w, 0) for g, w in zip(shape, patch)])
    wild = np.array([[-5, 1000, 7], [2 ** 31 - 1, -2 ** 31, 0], [3, 3, 3], [0, 0, 99], [1, 17, 33]], np.int32)
    for name in ("bernoulli", "none"):
        label = _patterns(shape)[name]
        got, count = _pick(label, patch, [float("nan"), 2.0, 1.0, -1.0, -7.5], wild)
        exp, T = d.pick_origins(label, patch, [last, last, last, -1.0, -1.0], np.clip(wild, 0, top))
        assert count == T and np.array_equal(got, exp), (name, got.tolist(), exp.tolist())


def test_pick_bad_arguments():
    L = _lib()
    lib, S = L.load(), L.stream()
    label = torch.zeros(8 * 8 * 8 + 4, device=DEV)
    rank = torch.zeros(65, dtype=torch.float64, device=DEV)
    fb = torch.zeros(65 * 3, dtype=torch.int32, device=DEV)
    picks, work = _Guarded(3 * 65 + 1, dtype=torch.int32, fill=POISON), _Guarded(64, dtype=torch.int32, fill=POISON)
    lp, rp, fp, pp, wp = (t.data_ptr() for t in (label, rank, fb, picks.out, work.out))

    def pick(label=lp, n=512, G=(8, 8, 8), w=(4, 4, 4), rank=rp, fb=fp, P=2, picks=pp, work=wp):
        return lib.pcms_foreground_pick(label, n, *G, *w, rank, fb, P, picks, work, S)

    for kw in [dict(P=0), dict(P=65), dict(P=-1),                                            # P outside 1..64
               dict(n=511), dict(n=513), dict(n=0), dict(G=(8, 8, 0), n=0), dict(G=(-8, 8, 8)),
               dict(n=2 ** 31, G=(2048, 1024, 1024)), dict(n=2 ** 32, G=(4096, 1024, 1024)),   # n >= 2^31
               dict(w=(0, 4, 4)), dict(w=(4, -1, 4)), dict(w=(4, 4, 0)),                      # a patch axis below 1
               dict(label=None), dict(rank=None), dict(fb=None), dict(picks=None), dict(work=None),
               dict(label=lp + 2), dict(rank=rp + 4), dict(fb=fp + 2), dict(picks=pp + 1), dict(work=wp + 2)]:
        assert pick(**kw) < 0, kw
    assert L.query("pcms_foreground_pick_work_ints", 0) < 0 and L.query("pcms_foreground_pick_work_ints", 2 ** 31) < 0
    assert L.query("pcms_foreground_pick_work_ints", 2 ** 31 - 1) == -(-(2 ** 31 - 1) // L.query(
        "pcms_foreground_pick_chunk")) + 1
    picks.check(written=False), work.check(written=False)
    assert pick(P=64) == 0 and pick(label=lp + 4) == 0   # the same tables accept a good call
    torch.cuda.synchronize()


# ---------------- patch resample ----------------
SRC_SHAPE, GRID = (11, 29, 23), (12, 40, 40)
ORIGINS = [(0, 0, 0), (0, 24, 24), (0, 7, 13)]
DTYPES = {"u8": (np.uint8, 1.0, 0.0), "i16": (np.int16, 1.0, 0.0), "f32": (np.float32, 1.0, 0.0),
          "f64_scaled": (np.float64, 0.5, -3.0)}


@functools.lru_cache(maxsize=None)
def _source(kind):
    dtype = DTYPES[kind][0]
    rng = np.random.default_rng(len(kind) + 50)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=SRC_SHAPE).astype(dtype)
    if dtype == np.int16:
        return rng.integers(-500, 3000, size=SRC_SHAPE).astype(dtype)
    return (1000.0 * rng.standard_normal(SRC_SHAPE)).astype(dtype)   # the lerps are not exact


@functools.lru_cache(maxsize=None)
def _affine(which):
    d = _data()
    if which == "identity":
        A, t = d.volume_affine(np.eye(3), np.zeros(3), SRC_SHAPE, GRID)
    else:
        A, t = d.volume_affine(d.compose_transform((True, False, True), (8.0, -5.0, 12.0), 1.15),
                               np.array([0.7, -2.2, 1.4]), SRC_SHAPE, GRID)
    return A, t


def _run(kind, which, origins, patch, normalise=False, gain=1.0, bias=0.0, stride_mul=1, offset=0, grid=GRID):
    """(got (P, wd, wh, ww), expected): pcms_patch_resample_linear into a poisoned, guarded buffer
    ``offset`` floats off its alignment, patches ``stride_mul`` D H W floats apart."""
    d, L = _data(), _lib()
    src = _source(kind)
    _, slope, inter = DTYPES[kind]
    vol = np.asarray(_decode(src, slope, inter)).astype(np.float32)
    A, t = _affine(which)
    code = {np.dtype(v): k for k, v in d._NIFTI_DTYPES.items()}[src.dtype]
    raw = torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).to(DEV)
    P, nwin = len(origins), int(np.prod(patch))
    stride = stride_mul * nwin
    total = (P - 1) * stride + nwin
    out = _Guarded(total + offset)
    assert out.out.data_ptr() % 16 == 0
    lohi = torch.tensor([float(vol.min()), float(vol.max())], dtype=torch.float32, device=DEV) if normalise else None
    odev = torch.tensor(origins, dtype=torch.int32, device=DEV)
    host = (ctypes.c_double * 12)(*A.reshape(-1).tolist(), *t.tolist())  # read during the call
    L.call("pcms_patch_resample_linear", raw, code, *src.shape, float(slope), float(inter), ctypes.addressof(host),
           lohi, float(gain), float(bias), *grid, odev, P, out.out.data_ptr() + 4 * offset, stride, *patch)
    flat = out.check()
    assert torch.isnan(flat[:offset]).all(), "the floats before the output were written"
    flat = flat[offset:]
    got = torch.stack([flat[p * stride:p * stride + nwin] for p in range(P)]).view(P, *patch)
    assert not torch.isnan(got).any(), "an output element was not written"
    for p in range(P - 1):
        assert torch.isnan(flat[p * stride + nwin:(p + 1) * stride]).all(), "written between two patches"
    exp = np.stack([d.resample_patch(vol, grid, A, t, o, patch, gain=gain, bias=bias, normalise=normalise)
                    for o in origins])
    return got, exp


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "lohi"])
@pytest.mark.parametrize("which", ["identity", "flip_rot_zoom"])
@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_patches_equal_host(kind, which, normalise):
    for patch, gain, bias in (((16, 16, 16), 1.0, 0.0), ((16, 16, 18), 1.25, -3.5), ((16, 16, 16), 0.75, 2.0)):
        got, exp = _run(kind, which, ORIGINS, patch, normalise, gain, bias)
        assert np.count_nonzero(exp) > exp.size // 4
        _same_bits(got, exp, f"patch {kind} {which} norm {normalise} {patch} gain {gain} bias {bias}")


def test_patches_equal_the_slice_of_the_whole_grid_launch():
    """The invariant itself on the device: pcms_resample_affine_linear onto the grid, sliced."""
    d = _data()
    src = _source("i16")
    A, t = _affine("flip_rot_zoom")
    raw = d.RawVolume(torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).to(DEV), 4, SRC_SHAPE, 1.0, 0.0)
    whole = d.resample_device(raw, GRID, affine=tuple(A.reshape(-1)) + tuple(t), gain=1.25, bias=-3.5).cpu()
    got, _ = _run("i16", "flip_rot_zoom", ORIGINS, (8, 16, 16), gain=1.25, bias=-3.5)
    for p, o in enumerate(ORIGINS):
        assert torch.equal(got[p].view(torch.int32), whole[o[0]:o[0] + 8, o[1]:o[1] + 16, o[2]:o[2] + 16].view(torch.int32))


@pytest.mark.parametrize("patch", [(16, 16, 16), (16, 16, 18)], ids=["vector", "scalar"])
def test_patch_stride_and_misaligned_output(patch):
    """Patches 5 D H W floats apart (a channel of a (P, 5, D, H, W) batch) and out one float past
    a 16-byte boundary: nothing between the patches or before the first is written."""
    for stride_mul, offset in ((5, 0), (1, 1), (5, 3)):
        got, exp = _run("i16", "flip_rot_zoom", ORIGINS, patch, True, 1.25, -3.5, stride_mul, offset)
        _same_bits(got, exp, f"patch stride x{stride_mul} offset {offset} {patch}")


def test_origins_out_of_range_give_zeros():
    """Origins are device memory and are not trusted: a patch partly or wholly outside the grid is
    zero there, whatever the origin, and the guard bands stay intact."""
    origins = [(-4, -5, -6), (5, 33, 30), (100, 0, 0), (0, 0, -18), (-2 ** 31, 2 ** 31 - 1, 0),
               (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (0, 7, 13)]
    for patch in ((16, 16, 16), (16, 16, 18)):
        got, exp = _run("i16", "flip_rot_zoom", origins, patch, False, 1.25, -3.5)
        _same_bits(got, exp, f"patch out of range {patch}")
        assert not exp[2:6].any() and exp[0].any() and exp[1].any() and not exp[0, :4].any() and not exp[1, 7:].any()
    got, exp = _run("u8", "identity", origins, (16, 16, 16), True)
    _same_bits(got, exp, "patch out of range, normalised")


def test_patch_bad_arguments():
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

    def run(src=sp, code=4, Si=(4, 4, 4), slope=1.0, inter=0.0, aff=GA, lohi=None, gain=1.0, bias=0.0, G=(8, 8, 8),
            origins=op, P=2, out=o, stride=512, D=8, H=8, W=8):
        return lib.pcms_patch_resample_linear(src, code, *Si, slope, inter, aff, lohi, gain, bias, *G, origins, P, out,
                                              stride, D, H, W, S)

    for kw in [dict(src=None), dict(out=None), dict(aff=None), dict(origins=None),             # NULL pointers
               dict(src=sp + 1), dict(code=16, src=sp + 2), dict(code=64, src=sp + 4),           # misaligned for the type
               dict(out=o + 2), dict(origins=op + 2), dict(lohi=lp + 2),
               dict(code=3), dict(code=0),                                                       # unknown datatype
               dict(Si=(0, 4, 4)), dict(Si=(4, -1, 4)), dict(Si=(4, 4, 0)), dict(D=0), dict(H=-8), dict(W=0),
               dict(G=(0, 8, 8)), dict(G=(8, -1, 8)), dict(G=(8, 8, 0)),
               dict(aff=ctypes.addressof(nan)), dict(aff=ctypes.addressof(inf)),
               dict(gain=float("nan")), dict(bias=float("inf")),
               dict(P=0), dict(P=65), dict(P=-3),                                                # P outside 1..64
               dict(stride=511), dict(stride=0), dict(stride=-512)]:                             # stride below D H W
        assert run(**kw) < 0, kw
    out.check(written=False)
    assert run() == 0 and run(lohi=lp, out=o + 4, stride=513, code=2) == 0   # the same tables accept a good call
    torch.cuda.synchronize()
    out.check()
