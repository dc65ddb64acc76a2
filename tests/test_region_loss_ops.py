"""The region + voxel loss kernels (csrc/losses.hip) against their fp64 definition
``losses.region_voxel_loss_host``.

Shapes are the smallest at which each path can go wrong (N = 2, C = 2):
* (5, 6, 7): 210 per group, not a multiple of 4 -- per sample the odd groups are 16-byte misaligned
  (scalar path), the even ones take the vector path with a 2-element remainder; less than one trip
  per thread;
* (4, 6, 8): 192 per group, the vector path alone;
* (16, 16, 9): 2304 per group, also with ``pcms_stream_grid_cap`` at 1 and 3: the two-vectors-in-
  flight main loop plus its tail (cap 1), several rows per group (cap 3, and no cap).

Bars: those of tests/test_gpu_ops.py::test_loss, whose error shape this shares (fp32 per voxel,
fp64 sums): |loss - ref| <= 1e-6 max(1, |ref|) and close(dx, ref_grad, 1e-5).  Every case prints
its two figures (``pytest -s``) before it asserts.  Measured on the MI355X: loss error at most
4.4e-8 at logits of standard deviation 3 and 5.9e-7 at 30 (losses near 9), gradient error at most
3.6e-7 of the largest element."""
import functools

import pytest
import torch

from tests.test_gpu_ops import DEV, _lib, close
from tests.test_stream_regimes import grid_cap

pytestmark = pytest.mark.gpu

GOUT = 0.7
SHAPES = [(5, 6, 7), (4, 6, 8), (16, 16, 9)]
PARAMS = {
    "ftv_focal_per_sample": dict(alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0, focal_gamma=2.0, focal_alpha=0.25,
                                 region_weight=1.0, voxel_weight=1.0, per_sample=True),
    "ftv43_focal_noalpha_batch": dict(alpha=0.3, beta=0.7, gamma=4.0 / 3.0, smooth=1.0, focal_gamma=2.0,
                                      focal_alpha=None, region_weight=0.5, voxel_weight=0.5, per_sample=False),
    "dice_like_batch": dict(alpha=0.5, beta=0.5, gamma=1.0, smooth=0.5, region_weight=1.0, voxel_weight=0.0,
                            per_sample=False),
    "tversky_tiny_smooth_focal1_per_sample": dict(alpha=0.3, beta=0.7, gamma=1.0, smooth=1e-5, focal_gamma=1.0,
                                                  focal_alpha=0.25, region_weight=1.0, voxel_weight=1.0,
                                                  per_sample=True),
}
# (shape, cap): cap 0 leaves the switch alone
CASES = [(s, 0) for s in SHAPES] + [((16, 16, 9), 1), ((16, 16, 9), 3)]


@functools.lru_cache(maxsize=None)
def inputs(shape, scale):
    g = torch.Generator().manual_seed(17 + shape[0] + int(scale))
    x = torch.randn(2, 2, *shape, generator=g) * scale
    t = (torch.rand(x.shape, generator=g) < 0.1).float()
    t[1, 0] = 0.0  # a group without a lesion
    return x, t


@functools.lru_cache(maxsize=None)
def reference(shape, scale, name):
    """(loss, dL/dx at gout) of the fp64 definition; computed once per (input, parameters)."""
    from pcms_amd.utils import losses
    x, t = inputs(shape, scale)
    xr = x.double().requires_grad_(True)
    ref = losses.region_voxel_loss_host(xr, t, **PARAMS[name])
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


@pytest.mark.parametrize("scale", [3.0, 30.0])
@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("shape,cap", CASES)
def test_region_loss_against_fp64(shape, cap, name, scale):
    from pcms_amd.utils import losses
    x, t = inputs(shape, scale)
    ref, ref_dx = reference(shape, scale, name)
    kw = PARAMS[name]
    with grid_cap(cap) as L:
        groups, nvox = (4, x[0, 0].numel()) if kw["per_sample"] else (1, x.numel())
        rows = L.query("pcms_region_loss_rows", nvox, groups)
        if cap:
            assert rows == min(cap, -(-nvox // 2048))
            if cap == 1:
                assert nvox // 4 > 256, "the vector main loop (two trips' worth of vectors) does not run"
        elif shape == (16, 16, 9):
            assert rows > 1, "one row per group"
        loss, dx = run(losses.RegionVoxelLoss(**kw), x, t)
    check(f"{name} {shape} cap{cap} x{scale:g}", loss, dx, ref, ref_dx)


def test_tversky_half_half_is_dice():
    """TverskyLoss(0.5, 0.5, smooth=0.5) and DiceLoss(1.0) on test_loss's input: one fp64 value."""
    from pcms_amd.utils import losses
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 1, 9, 10, 11, generator=g) * 3
    t = (torch.rand(x.shape, generator=g) < 0.3).float()
    xr = x.double().requires_grad_(True)
    p = torch.sigmoid(xr).reshape(-1)
    tt = t.double().reshape(-1)
    ref = 1 - (2 * (p * tt).sum() + 1) / (p.sum() + tt.sum() + 1)
    ref.backward(torch.tensor(GOUT, dtype=torch.float64))
    for what, crit in (("tversky", losses.TverskyLoss(0.5, 0.5, smooth=0.5)), ("dice", losses.DiceLoss(1.0))):
        loss, dx = run(crit, x, t)
        check(what, loss, dx, ref.item(), xr.grad)


@pytest.mark.parametrize("name", ["ftv_focal_per_sample", "ftv43_focal_noalpha_batch"])
def test_two_runs_same_bits(name):
    from pcms_amd.utils import losses
    x, t = inputs((16, 16, 9), 3.0)
    crit = losses.RegionVoxelLoss(**PARAMS[name])
    (l0, d0), (l1, d1) = run(crit, x, t), run(crit, x, t)
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32))


def test_per_sample_is_the_mean_of_per_sample_calls():
    from pcms_amd.utils import losses
    x, t = inputs((5, 6, 7), 3.0)
    ref, ref_dx = reference((5, 6, 7), 3.0, "ftv_focal_per_sample")
    crit = losses.RegionVoxelLoss(**PARAMS["ftv_focal_per_sample"])
    parts = [run(crit, x[n:n + 1], t[n:n + 1], GOUT / 2) for n in range(2)]  # d mean / d loss_n = 1/2
    loss = torch.stack([p[0] for p in parts]).double().mean().float()
    check("mean of per-sample calls", loss, torch.cat([p[1] for p in parts]), ref, ref_dx)


def test_module_api():
    from pcms_amd.utils import losses
    x, t = inputs((5, 6, 7), 3.0)
    crit = losses.FocalTverskyFocalLoss(per_sample=True)
    base_loss, base_dx = run(crit, x, t)
    # a uint8 target, a non-contiguous pred: what the fp32 contiguous call gives, bit for bit
    xd = x.to(DEV)
    loss = crit(xd, t.to(DEV).to(torch.uint8))
    assert torch.equal(loss.cpu(), base_loss)
    xt = xd.transpose(2, 4).contiguous().transpose(2, 4).requires_grad_(True)
    assert not xt.is_contiguous()
    loss = crit(xt, t.to(DEV))
    loss.backward(torch.tensor(GOUT, device=DEV))
    assert torch.equal(loss.detach().cpu(), base_loss) and torch.equal(xt.grad.cpu(), base_dx)
    # bf16 pred: the fp32 call on the rounded logits; the gradient comes back in bf16
    xb = x.to(torch.bfloat16)
    want_loss, want_dx = run(crit, xb.float(), t)
    xbd = xb.to(DEV).requires_grad_(True)
    loss = crit(xbd, t.to(DEV))
    loss.backward(torch.tensor(GOUT, device=DEV))
    assert loss.dtype == torch.float32 and torch.equal(loss.detach().cpu(), want_loss)
    assert xbd.grad.dtype == torch.bfloat16 and torch.equal(xbd.grad.cpu(), want_dx.to(torch.bfloat16))
    with pytest.raises(ValueError, match="形状不匹配"):
        crit(xd, t.to(DEV)[:, :1])
    with pytest.raises(RuntimeError, match="ROCm device only"):
        crit(x, t)


def test_bad_arguments_launch_nothing():
    """The C checks: a negative code, outputs untouched."""
    L = _lib()
    lib = L.load()
    x, t = inputs((4, 6, 8), 3.0)
    xd, td = x.to(DEV), t.to(DEV)
    nvox, groups = 192, 4
    rows = L.query("pcms_region_loss_rows", nvox, groups)
    part = torch.zeros(groups * rows * 4, device=DEV)
    sums = torch.zeros(groups * 4, dtype=torch.float64, device=DEV)
    coef, loss, dx = torch.zeros(groups * 2, device=DEV), torch.zeros((), device=DEV), torch.zeros_like(xd)
    good = dict(x=xd.data_ptr(), t=td.data_ptr(), nvox=nvox, groups=groups, alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0,
                focal_gamma=2.0, use_alpha=1, focal_alpha=0.25, wr=1.0, wv=1.0, part=part.data_ptr(),
                sums=sums.data_ptr(), coef=coef.data_ptr(), loss=loss.data_ptr())

    def fwd(**kw):
        a = dict(good, **kw)
        return lib.pcms_region_loss_fwd(a["x"], a["t"], a["nvox"], a["groups"], a["alpha"], a["beta"], a["gamma"],
                                        a["smooth"], a["focal_gamma"], a["use_alpha"], a["focal_alpha"], a["wr"],
                                        a["wv"], a["part"], a["sums"], a["coef"], a["loss"], L.stream())

    def bwd(**kw):
        a = dict(good, **kw)
        return lib.pcms_region_loss_bwd(a["x"], a["t"], a["nvox"], a["groups"], a["focal_gamma"], a["use_alpha"],
                                        a["focal_alpha"], a["wv"], a["coef"], None, dx.data_ptr(), L.stream())

    bad = [dict(x=None), dict(t=None), dict(groups=0), dict(nvox=0), dict(groups=2, nvox=1 << 30), dict(alpha=-0.1),
           dict(beta=-0.1), dict(smooth=-1.0), dict(gamma=0.0), dict(focal_gamma=0.5), dict(focal_gamma=-1.0),
           dict(focal_alpha=1.5), dict(focal_alpha=-0.5), dict(part=None), dict(sums=None), dict(coef=None),
           dict(loss=None), dict(x=xd.data_ptr() + 2)]
    for kw in bad:
        assert fwd(**kw) < 0, kw
    for kw in bad:
        if not set(kw) & {"alpha", "beta", "smooth", "gamma", "part", "sums", "loss"}:
            assert bwd(**kw) < 0, kw
    assert fwd(focal_alpha=7.0, use_alpha=0) == 0  # off: the value is not looked at
    torch.cuda.synchronize()
    assert dx.abs().max().item() == 0.0
    assert L.query("pcms_region_loss_rows", 0, 1) < 0 and L.query("pcms_region_loss_rows", 10, 0) < 0
