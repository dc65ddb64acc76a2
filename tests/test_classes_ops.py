"""The kernels of csrc/classes.hip against their host forms (pcms_amd.classes).

Loss (``SoftmaxDiceCELoss``) against the fp64 definition ``classes.softmax_dice_ce_loss_host`` and
its autograd gradient, at the shapes of tests/test_region_loss_ops.py (N = 2):
* (5, 6, 7): 210 voxels per plane, not a multiple of 4 -- the scalar path, less than one trip;
* (4, 6, 8): 192 per plane, the 16-byte path alone;
* (16, 16, 9): 2304 per plane, also with ``pcms_stream_grid_cap`` at 1 and 3: many trips per
  thread (cap 1), several rows per sample (cap 3, and no cap).
About 5 % of the labels are 255 (ignored) and sample 1 has no voxel of class 2.  Bars: those of
tests/test_region_loss_ops.py, unchanged -- |loss - ref| <= 1e-6 max(1, |ref|) and
close(dx, ref_grad, 1e-5).  Every case prints its two figures (``pytest -s``) before it asserts.

Softmax planes: |p - p64| <= 1e-6 absolute and every voxel's classes sum to 1 within 1e-6 -- expf
at <= 1 ulp, one rounding of x - m, C - 1 additions and one division, on values <= 1.

Everything else is compared byte for byte with its host form."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _lib, close
from tests.test_stream_regimes import grid_cap

pytestmark = pytest.mark.gpu

GOUT = 0.7
SHAPES = [(5, 6, 7), (4, 6, 8), (16, 16, 9)]
# (shape, cap): cap 0 leaves the switch alone
CASES = [(s, 0) for s in SHAPES] + [((16, 16, 9), 1), ((16, 16, 9), 3)]
WEIGHTS = {2: (0.3, 1.7), 3: (0.2, 1.0, 2.5), 4: (0.2, 1.0, 2.5, 0.6)}


@functools.lru_cache(maxsize=None)
def inputs(shape, C, scale):
    g = torch.Generator().manual_seed(31 + shape[0] + 7 * C + int(scale))
    x = torch.randn(2, C, *shape, generator=g) * scale
    t = torch.randint(0, C, (2, 1) + shape, generator=g).float()
    t[1][t[1] == 2] = 0.0                                   # a sample without class 2
    t[torch.rand(t.shape, generator=g) < 0.05] = 255.0      # ignored voxels
    return x, t


def params(per_sample, weighted, C):
    return dict(ce_weight=0.4, dice_weight=0.6, smooth=1.0, class_weights=WEIGHTS[C] if weighted else None,
                include_background=False, per_sample=per_sample)


@functools.lru_cache(maxsize=None)
def reference(shape, C, scale, per_sample, weighted):
    """(loss, dL/dx at gout) of the fp64 definition; computed once per (input, parameters)."""
    from pcms_amd import classes
    x, t = inputs(shape, C, scale)
    xr = x.double().requires_grad_(True)
    ref = classes.softmax_dice_ce_loss_host(xr, t, **params(per_sample, weighted, C))
    ref.backward(torch.tensor(GOUT, dtype=torch.float64))
    return ref.item(), xr.grad


def run(crit, x, t, gout=GOUT):
    xd = x.to(DEV).requires_grad_(True)
    loss = crit(xd, t.to(DEV))
    loss.backward(torch.tensor(gout, device=DEV))
    torch.cuda.synchronize()
    return loss.detach().cpu(), xd.grad.cpu()


def check(what, loss, dx, ref, ref_dx):
    assert torch.isfinite(loss) and torch.isfinite(dx).all(), what
    scale = ref_dx.abs().max().item() + 1e-12
    print(f"\nFIGURE {what}: loss {loss.item():.9g} ref {ref:.12g} err {abs(loss.item() - ref):.3e}; "
          f"grad rel err {(dx.double() - ref_dx).abs().max().item() / scale:.3e}")
    assert abs(loss.item() - ref) <= 1e-6 * max(1.0, abs(ref)), (what, loss.item(), ref)
    close(dx, ref_dx, 1e-5, what)


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("shape,cap", CASES)
def test_softmax_loss_against_fp64(shape, cap, C, per_sample, u8, weighted, scale):
    from pcms_amd.utils import losses
    x, t = inputs(shape, C, scale)
    ref, ref_dx = reference(shape, C, scale, per_sample, weighted)
    nvox = x[0, 0].numel()
    with grid_cap(cap) as L:
        rows = L.query("pcms_softmax_loss_rows", nvox, 2)
        if cap:
            assert rows == min(cap, -(-nvox // 2048))
            if cap == 1:
                assert nvox // 4 > 256, "no thread takes a second trip"
        elif shape == (16, 16, 9):
            assert rows > 1, "one row per sample"
        loss, dx = run(losses.SoftmaxDiceCELoss(**params(per_sample, weighted, C)), x,
                       t.to(torch.uint8) if u8 else t)
    ignored = (t == 255).expand_as(x)
    assert ignored.any() and (dx[ignored] == 0).all(), "an ignored voxel has a gradient"
    check(f"C{C} {shape} cap{cap} per_sample={per_sample} u8={u8} weighted={weighted} x{scale:g}", loss, dx, ref, ref_dx)


@pytest.mark.parametrize("per_sample", [False, True])
def test_two_runs_same_bits(per_sample):
    from pcms_amd.utils import losses
    x, t = inputs((16, 16, 9), 3, 1.0)
    crit = losses.SoftmaxDiceCELoss(**params(per_sample, True, 3))
    (l0, d0), (l1, d1) = run(crit, x, t), run(crit, x, t)
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32))


@pytest.mark.parametrize("u8", [False, True])
def test_all_ignored_target(u8):
    """No valid voxel: CE = 0, every Dice sum empty, so the loss is dice_weight * region of empty
    sums (the host definition's value), and dx == 0 exactly."""
    from pcms_amd import classes
    from pcms_amd.utils import losses
    x, _ = inputs((5, 6, 7), 3, 1.0)
    t = torch.full((2, 1, 5, 6, 7), 255.0)
    for kw in (dict(smooth=1.0), dict(smooth=0.0), dict(smooth=1.0, include_background=True, per_sample=True)):
        ref = classes.softmax_dice_ce_loss_host(x.double(), t, **kw).item()
        loss, dx = run(losses.SoftmaxDiceCELoss(**kw), x, t.to(torch.uint8) if u8 else t)
        assert loss.item() == ref == 0.0, (kw, loss.item(), ref)
        assert (dx == 0).all()


def test_module_api():
    from pcms_amd.utils import losses
    x, t = inputs((4, 6, 8), 3, 1.0)
    crit = losses.create_criterion("softmax_dice_ce", {"per_sample": True})
    assert isinstance(crit, losses.SoftmaxDiceCELoss)
    base_loss, base_dx = run(crit, x, t)
    # a (N, D, H, W) target, an int64 one, a non-contiguous pred: the same bits
    for tt in (t[:, 0], t.long()):
        loss, dx = run(crit, x, tt)
        assert torch.equal(loss, base_loss) and torch.equal(dx, base_dx)
    xt = x.to(DEV).transpose(2, 4).contiguous().transpose(2, 4).requires_grad_(True)
    assert not xt.is_contiguous()
    loss = crit(xt, t.to(DEV))
    loss.backward(torch.tensor(GOUT, device=DEV))
    assert torch.equal(loss.detach().cpu(), base_loss) and torch.equal(xt.grad.cpu(), base_dx)
    with pytest.raises(ValueError, match="形状不匹配"):
        crit(x.to(DEV), t.to(DEV)[:, :, :2])
    with pytest.raises(ValueError):
        crit(x.to(DEV)[:, :1], t.to(DEV))  # one logit plane
    with pytest.raises(RuntimeError, match="ROCm device only"):
        crit(x, t)


@pytest.mark.parametrize("C", [2, 3, 5, 8])
@pytest.mark.parametrize("shape,cap", [((5, 6, 7), 0), ((4, 6, 8), 0), ((16, 16, 9), 1)])
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_softmax_planes(shape, cap, C, scale):
    from pcms_amd import classes
    g = torch.Generator().manual_seed(5 + C)
    x = torch.randn(3, C, *shape, generator=g) * scale
    with grid_cap(cap):  # (cap 1: one block, several trips per thread)
        p = classes.softmax_planes_device(x.to(DEV)).cpu()
    assert p.shape == (C, 3) + shape, "class-major"
    p64 = torch.softmax(x.double(), dim=1).transpose(0, 1)
    err, one = (p.double() - p64).abs().max().item(), (p.double().sum(0) - 1.0).abs().max().item()
    print(f"\nFIGURE softmax planes C{C} {shape} x{scale:g}: |p - p64| {err:.3e}, |sum - 1| {one:.3e}")
    assert err <= 1e-6 and one <= 1e-6


@pytest.mark.parametrize("tgt,native", [((3, 5, 7), (4, 9, 6)), ((6, 6, 6), (6, 6, 6)), ((3, 5, 7), (6, 9, 6))])
def test_probs_to_labels_byte_equal(tgt, native):
    from pcms_amd import classes
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 3, *tgt, generator=g) * 2
    x[0, 2, : tgt[0] // 2 + 1] = x[0, 1, : tgt[0] // 2 + 1]   # planes 1 and 2 equal there: the first one wins
    probs = classes.softmax_planes_device(x.to(DEV))[:, 0].contiguous()
    labels, planes = classes.labels_on_grid_device(probs, native, return_probability=True)
    only, none = classes.labels_on_grid_device(probs, native)
    want, want_planes = classes.labels_on_grid(probs.cpu().numpy(), native)
    tie = (want_planes[1] == want_planes[2]) & (want_planes[1] > want_planes[0])
    assert tie.any() and not (want[tie] == 2).any(), "the tie rule is not exercised"
    assert none is None and np.array_equal(only.cpu().numpy(), want)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(planes.cpu().numpy().view(np.int32), want_planes.view(np.int32))
    if native[0] == 2 * tgt[0]:  # the last native slice samples d = n - 0.5: outside, every plane 0, class 0
        assert (want_planes[:, -1] == 0).all() and (want[-1] == 0).all()


def _raw(dtype, code, shape, slope, inter, seed):
    from pcms_amd.nifti import RawVolume
    rng = np.random.default_rng(seed)
    arr = rng.integers(0, 10, size=shape).astype(dtype)
    return RawVolume(torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()), code, shape, slope, inter)


@pytest.mark.parametrize("slope,inter", [(1.0, 0.0), (0.5, 1.0)])
@pytest.mark.parametrize("dtype,code", [(np.uint8, 2), (np.int16, 4)])
@pytest.mark.parametrize("target", [(4, 9, 6), (5, 6, 7)])
def test_resample_classes_byte_equal(target, dtype, code, slope, inter):
    from pcms_amd import classes
    from pcms_amd.resample import resample, resample_device
    raw = _raw(dtype, code, (5, 6, 7), slope, inter, 3)
    want = classes.classes_of(resample(raw.numpy(), target, nearest=True), (2, 5))
    assert set(np.unique(want)) == {0.0, 1.0, 2.0}
    got = resample_device(raw.to(DEV), target, nearest=True, class_values=(2, 5))
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("slope,inter", [(1.0, 0.0), (0.5, 1.0)])
@pytest.mark.parametrize("dtype,code", [(np.uint8, 2), (np.int16, 4)])
def test_resample_affine_classes_byte_equal(dtype, code, slope, inter):
    from pcms_amd import classes
    from pcms_amd.resample import resample_affine, resample_device
    raw = _raw(dtype, code, (5, 6, 7), slope, inter, 4)
    target = (6, 8, 9)
    c, s = np.cos(0.5), np.sin(0.5)   # a rotation about the D axis, off centre: part of the grid is outside
    A = np.array([[0.8, 0.0, 0.0], [0.0, 0.75 * c, -0.75 * s], [0.0, 0.75 * s, 0.75 * c]])
    t = np.array([0.2, 1.5, -1.0])
    nearest = resample_affine(raw.numpy(), target, A, t, nearest=True)
    want = classes.classes_of(nearest, (2, 5))
    assert set(np.unique(want)) == {0.0, 1.0, 2.0} and (want == 0).sum() > (nearest == 0).sum() > 0
    got = resample_device(raw.to(DEV), target, nearest=True, affine=list(A.reshape(-1)) + list(t), class_values=(2, 5))
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    # a one-hot table: the binary label of one value
    one = resample_device(raw.to(DEV), target, nearest=True, affine=list(A.reshape(-1)) + list(t), class_values=(5,))
    assert np.array_equal(one.cpu().numpy(), classes.classes_of(nearest, (5,)))
    with pytest.raises(ValueError, match="nearest"):
        resample_device(raw.to(DEV), target, class_values=(2, 5))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_class_overlap_exact(n):
    from pcms_amd import classes
    rng = np.random.default_rng(n)
    buf = rng.choice(np.array([0, 0, 0, 1, 2, 3, 255], dtype=np.uint8), size=(2, n + 1))
    for off in (0, 1):  # 4-byte aligned maps, and maps one byte past a boundary
        p, r = buf[0, off:off + n], buf[1, off:off + n]
        want = classes.class_overlap(p, r, 3)
        dev = torch.from_numpy(buf).to(DEV)
        got = [classes.class_overlap_device(dev[0, off:off + n], dev[1, off:off + n], 3).cpu().numpy() for _ in range(2)]
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want) and np.array_equal(got[1], want)
    with grid_cap(1):
        assert np.array_equal(classes.class_overlap_device(dev[0, :n], dev[1, :n], 3).cpu().numpy(),
                              classes.class_overlap(buf[0, :n], buf[1, :n], 3))


def test_bad_arguments_launch_nothing():
    """The C checks: a negative code, outputs untouched."""
    L = _lib()
    lib = L.load()
    S = L.stream()
    x, t = inputs((4, 6, 8), 3, 1.0)
    xd, td = x.to(DEV), t.to(DEV)
    nvox, N, C = 192, 2, 3
    rows = L.query("pcms_softmax_loss_rows", nvox, N)
    K = 3 * C + 2
    part = torch.zeros(N * rows * K, device=DEV)
    sums = torch.zeros(N * K, dtype=torch.float64, device=DEV)
    coef, loss, dx = torch.zeros(N * 2 * C + 1, device=DEV), torch.zeros((), device=DEV), torch.zeros_like(xd)
    neg = (ctypes.c_float * 3)(1.0, -1.0, 1.0)
    good = dict(x=xd.data_ptr(), t=td.data_ptr(), u8=0, nvox=nvox, N=N, C=C, ps=1, bg=0, smooth=1.0, wce=0.5, wd=0.5,
                w=None, part=part.data_ptr(), sums=sums.data_ptr(), coef=coef.data_ptr(), loss=loss.data_ptr())

    def fwd(**kw):
        a = dict(good, **kw)
        return lib.pcms_softmax_loss_fwd(a["x"], a["t"], a["u8"], a["nvox"], a["N"], a["C"], a["ps"], a["bg"],
                                         a["smooth"], a["wce"], a["wd"], a["w"], a["part"], a["sums"], a["coef"],
                                         a["loss"], S)

    def bwd(**kw):
        a = dict(good, **kw)
        return lib.pcms_softmax_loss_bwd(a["x"], a["t"], a["u8"], a["nvox"], a["N"], a["C"], a["ps"], a["w"],
                                         a["coef"], None, dx.data_ptr(), S)

    bad = [dict(x=None), dict(t=None), dict(N=0), dict(N=70000), dict(nvox=0), dict(nvox=1 << 31), dict(C=1), dict(C=9),
           dict(x=xd.data_ptr() + 2), dict(t=td.data_ptr() + 2), dict(w=ctypes.addressof(neg)), dict(smooth=-1.0),
           dict(wce=float("nan")), dict(wd=float("inf")), dict(part=None), dict(sums=None), dict(coef=None),
           dict(loss=None), dict(sums=sums.data_ptr() + 4)]
    for kw in bad:
        assert fwd(**kw) < 0, kw
        if not set(kw) & {"smooth", "wce", "wd", "part", "sums", "loss"}:
            assert bwd(**kw) < 0, kw
    assert L.query("pcms_softmax_loss_rows", 0, 1) < 0 and L.query("pcms_softmax_loss_rows", 10, 0) < 0

    probs = torch.zeros(3 * 192, device=DEV)
    assert lib.pcms_softmax_planes(None, 1, 3, 192, probs.data_ptr(), S) < 0
    assert lib.pcms_softmax_planes(xd.data_ptr(), 1, 3, 192, None, S) < 0
    assert lib.pcms_softmax_planes(xd.data_ptr(), 1, 1, 192, probs.data_ptr(), S) < 0
    assert lib.pcms_softmax_planes(xd.data_ptr(), 1, 9, 192, probs.data_ptr(), S) < 0
    assert lib.pcms_softmax_planes(xd.data_ptr(), 0, 3, 192, probs.data_ptr(), S) < 0
    assert lib.pcms_softmax_planes(xd.data_ptr(), 1, 3, 0, probs.data_ptr(), S) < 0
    assert lib.pcms_softmax_planes(xd.data_ptr(), 1, 3, 192, xd.data_ptr() + 64, S) < 0  # overlapping

    labels = torch.zeros(192, dtype=torch.uint8, device=DEV)
    native = torch.zeros(3 * 192, device=DEV)
    for a in [(None, 3, 4, 6, 8, labels.data_ptr(), None, 4, 6, 8), (xd.data_ptr(), 3, 4, 6, 8, None, None, 4, 6, 8),
              (xd.data_ptr(), 0, 4, 6, 8, labels.data_ptr(), None, 4, 6, 8),
              (xd.data_ptr(), 9, 4, 6, 8, labels.data_ptr(), None, 4, 6, 8),
              (xd.data_ptr(), 3, 0, 6, 8, labels.data_ptr(), None, 4, 6, 8),
              (xd.data_ptr(), 3, 4, 6, 8, labels.data_ptr(), native.data_ptr(), 4, 6, 0),
              (xd.data_ptr(), 3, 4, 6, 8, labels.data_ptr(), native.data_ptr() + 2, 4, 6, 8)]:
        assert lib.pcms_probs_to_labels(*a, S) < 0, a

    raw = _raw(np.int16, 4, (4, 6, 8), 1.0, 0.0, 1).to(DEV)
    out = torch.zeros(4, 6, 8, device=DEV)
    table = (ctypes.c_float * 8)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0)
    nan = (ctypes.c_float * 2)(1.0, float("nan"))
    twelve = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    T, A = ctypes.addressof(table), ctypes.addressof(twelve)
    src = raw.data.data_ptr()
    for a in [(None, 4, 4, 6, 8, 1.0, 0.0, T, 2), (src, 3, 4, 6, 8, 1.0, 0.0, T, 2), (src, 4, 0, 6, 8, 1.0, 0.0, T, 2),
              (src, 4, 4, 6, 8, 1.0, 0.0, None, 2), (src, 4, 4, 6, 8, 1.0, 0.0, T, 0), (src, 4, 4, 6, 8, 1.0, 0.0, T, 8),
              (src, 4, 4, 6, 8, 1.0, 0.0, ctypes.addressof(nan), 2), (src + 1, 4, 4, 6, 8, 1.0, 0.0, T, 2)]:
        assert lib.pcms_resample_classes(*a, out.data_ptr(), 4, 6, 8, S) < 0, a
        assert lib.pcms_resample_affine_classes(*a[:7], A, *a[7:], out.data_ptr(), 4, 6, 8, S) < 0, a
    assert lib.pcms_resample_classes(src, 4, 4, 6, 8, 1.0, 0.0, T, 2, None, 4, 6, 8, S) < 0
    assert lib.pcms_resample_affine_classes(src, 4, 4, 6, 8, 1.0, 0.0, None, T, 2, out.data_ptr(), 4, 6, 8, S) < 0

    counts = torch.zeros(9, dtype=torch.int64, device=DEV)
    for a in [(None, labels.data_ptr(), 192, 3, counts.data_ptr()), (labels.data_ptr(), None, 192, 3, counts.data_ptr()),
              (labels.data_ptr(), labels.data_ptr(), 192, 3, None), (labels.data_ptr(), labels.data_ptr(), 0, 3, counts.data_ptr()),
              (labels.data_ptr(), labels.data_ptr(), 192, 0, counts.data_ptr()),
              (labels.data_ptr(), labels.data_ptr(), 192, 9, counts.data_ptr()),
              (labels.data_ptr(), labels.data_ptr(), 192, 3, counts.data_ptr() + 4)]:
        assert lib.pcms_class_overlap(*a, S) < 0, a

    torch.cuda.synchronize()
    for buf in (part, sums, coef, loss, dx, probs, labels, native, out, counts):
        assert not buf.ne(0).any().item(), "a refused call wrote something"
