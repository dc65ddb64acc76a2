"""The definition of the imbalance-aware losses (``losses.region_voxel_loss_host``, fp64 torch on
the CPU), the constructors' parameter checks and the trainer's loss table.  No GPU."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pcms_amd  # noqa: F401
from pcms_amd.utils import losses
from pcms_amd.utils.trainer import BaseTrainer


def loss_input():
    """The input of tests/test_gpu_ops.py::test_loss."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 1, 9, 10, 11, generator=g) * 3
    t = (torch.rand(x.shape, generator=g) < 0.3).float()
    return x.double(), t.double()


def test_half_half_tversky_is_the_reference_dice():
    x, t = loss_input()
    p = torch.sigmoid(x).reshape(-1)
    dice = 1 - (2 * (p * t.reshape(-1)).sum() + 1) / (p.sum() + t.sum() + 1)
    got = losses.region_voxel_loss_host(x, t, alpha=0.5, beta=0.5, smooth=0.5, gamma=1.0)
    assert got.dtype == torch.float64
    assert abs(got.item() - dice.item()) <= 1e-12


def test_voxel_term_is_bce_and_torchvision_focal():
    x, t = loss_input()
    got = losses.region_voxel_loss_host(x, t, region_weight=0.0, voxel_weight=1.0, focal_gamma=0.0)
    assert abs(got.item() - F.binary_cross_entropy_with_logits(x, t).item()) <= 1e-12
    # torchvision.ops.sigmoid_focal_loss(x, t, alpha=0.25, gamma=2, reduction="mean"), inline
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    focal = ((0.25 * t + 0.75 * (1 - t)) * ce * (1 - p_t) ** 2).mean()
    got = losses.region_voxel_loss_host(x, t, region_weight=0.0, voxel_weight=1.0, focal_gamma=2.0, focal_alpha=0.25)
    assert abs(got.item() - focal.item()) <= 1e-12
    # the compound form is the weighted sum of its parts
    a = losses.region_voxel_loss_host(x, t, alpha=0.3, beta=0.7, gamma=0.75, per_sample=True)
    both = losses.region_voxel_loss_host(x, t, alpha=0.3, beta=0.7, gamma=0.75, per_sample=True, focal_gamma=2.0,
                                         focal_alpha=0.25, region_weight=0.5, voxel_weight=0.25)
    assert abs(both.item() - (0.5 * a.item() + 0.25 * focal.item())) <= 1e-12


def test_per_sample_is_the_mean_over_sample_channel_volumes():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 4, 5, 6, generator=g, dtype=torch.float64) * 2
    t = (torch.rand(x.shape, generator=g) < 0.2).double()
    kw = dict(alpha=0.3, beta=0.7, gamma=4.0 / 3.0, smooth=1.0)
    whole = losses.region_voxel_loss_host(x, t, per_sample=True, **kw)
    parts = [losses.region_voxel_loss_host(x[n, c][None, None], t[n, c][None, None], **kw)
             for n in range(2) for c in range(3)]
    assert abs(whole.item() - torch.stack(parts).mean().item()) <= 1e-12


@pytest.mark.parametrize("per_sample", [False, True])
def test_gradcheck(per_sample):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 2, 3, 3, 3, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    t = (torch.rand(x.shape, generator=g) < 0.3).double()
    for kw in (dict(alpha=0.3, beta=0.7, gamma=0.75, focal_gamma=2.0, focal_alpha=0.25, region_weight=1.0,
                    voxel_weight=1.0),
               dict(alpha=0.3, beta=0.7, gamma=4.0 / 3.0, focal_gamma=1.0, region_weight=0.5, voxel_weight=0.5),
               dict(alpha=0.5, beta=0.5, smooth=0.5)):
        assert torch.autograd.gradcheck(
            lambda v: losses.region_voxel_loss_host(v, t, per_sample=per_sample, **kw), (x,))


def test_empty_and_clamped_groups_are_finite():
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, 2, 3, 4, 5, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    t = (torch.rand(x.shape, generator=g) < 0.3).double()
    t[0, 1] = 0.0  # an empty group
    # alpha = 0 on the empty group: D = s, TI = 1 exactly, 1 - TI = 0 -- the clamped branch, where
    # a gamma < 1 has an infinite derivative
    for kw in (dict(alpha=0.0, beta=1.0, gamma=0.75), dict(alpha=0.3, beta=0.7, gamma=0.75),
               dict(alpha=0.0, beta=1.0, gamma=2.0, smooth=0.0)):
        xr = x.detach().clone().requires_grad_(True)
        loss = losses.region_voxel_loss_host(xr, t, per_sample=True, focal_gamma=2.0, focal_alpha=0.25,
                                             voxel_weight=1.0, **kw)
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(xr.grad).all(), kw
    # the clamped group contributes nothing, neither to the loss nor to the gradient
    xr = x.detach().clone().requires_grad_(True)
    loss = losses.region_voxel_loss_host(xr, t, per_sample=True, alpha=0.0, beta=1.0, gamma=0.75)
    loss.backward()
    assert xr.grad[0, 1].abs().max().item() == 0.0 and xr.grad[0, 0].abs().max().item() > 0.0
    # saturated logits
    xs = (x.detach() * 40).requires_grad_(True)
    loss = losses.region_voxel_loss_host(xs, t, per_sample=True, alpha=0.3, beta=0.7, gamma=0.75, focal_gamma=2.0,
                                         focal_alpha=0.25, voxel_weight=1.0)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(xs.grad).all()


BAD = [dict(alpha=-0.1), dict(beta=-1.0), dict(smooth=-1e-3), dict(gamma=0.0), dict(gamma=-1.0),
       dict(focal_gamma=0.5), dict(focal_gamma=-2.0), dict(focal_alpha=1.5), dict(focal_alpha=-0.25),
       dict(alpha=float("nan")), dict(smooth=float("inf")), dict(region_weight=float("nan")),
       dict(voxel_weight=float("inf")), dict(gamma="1")]


@pytest.mark.parametrize("kw", BAD, ids=[str(k) for k in BAD])
def test_invalid_parameters_raise(kw):
    with pytest.raises(ValueError):
        losses.RegionVoxelLoss(**kw)
    x, t = loss_input()
    with pytest.raises(ValueError):
        losses.region_voxel_loss_host(x, t, **kw)


def test_named_constructors_validate_and_carry_their_defaults():
    for make in (lambda: losses.TverskyLoss(alpha=-1.0), lambda: losses.FocalTverskyLoss(gamma=0.0),
                 lambda: losses.FocalLoss(gamma=0.5), lambda: losses.FocalLoss(alpha=2.0),
                 lambda: losses.FocalTverskyFocalLoss(focal_gamma=0.3), lambda: losses.TverskyLoss(smooth=-1.0)):
        with pytest.raises(ValueError):
            make()
    tv = losses.TverskyLoss()
    assert (tv.alpha, tv.beta, tv.gamma, tv.smooth, tv.voxel_weight, tv.per_sample) == (0.3, 0.7, 1.0, 1.0, 0.0, False)
    ft = losses.FocalTverskyLoss(per_sample=True)
    assert (ft.alpha, ft.beta, ft.gamma, ft.per_sample) == (0.3, 0.7, 0.75, True)
    fl = losses.FocalLoss()
    assert (fl.focal_gamma, fl.focal_alpha, fl.region_weight, fl.voxel_weight) == (2.0, 0.25, 0.0, 1.0)
    assert losses.FocalLoss(alpha=None).focal_alpha is None
    cf = losses.FocalTverskyFocalLoss()
    assert (cf.region_weight, cf.voxel_weight, cf.gamma, cf.focal_gamma, cf.focal_alpha) == (0.5, 0.5, 0.75, 2.0, 0.25)


def test_shape_mismatch_and_cpu_tensors_raise():
    x = torch.zeros(1, 1, 2, 2, 2)
    with pytest.raises(ValueError, match="形状不匹配"):
        losses.TverskyLoss()(x, torch.zeros(1, 1, 2, 2, 3))
    with pytest.raises(ValueError, match="形状不匹配"):
        losses.region_voxel_loss_host(x, torch.zeros(1, 1, 2, 2, 3))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        losses.FocalTverskyLoss()(x, x)


def _criterion(config):
    """BaseTrainer._create_criterion on a stub: no model, no device."""
    return BaseTrainer._create_criterion(types.SimpleNamespace(config=config))


def test_trainer_loss_table():
    assert type(_criterion({})) is losses.DiceLoss
    assert type(_criterion({"loss": "dice"})) is losses.DiceLoss
    assert type(_criterion({"loss": "bce_dice"})) is losses.BCEDiceLoss
    for name, cls in (("tversky", losses.TverskyLoss), ("focal_tversky", losses.FocalTverskyLoss),
                      ("focal", losses.FocalLoss), ("focal_tversky_focal", losses.FocalTverskyFocalLoss)):
        assert type(_criterion({"loss": name})) is cls
        assert losses.LOSSES[name] is cls
    c = _criterion({"loss": "focal_tversky", "loss_args": {"gamma": 1.5, "per_sample": True}})
    assert (c.gamma, c.per_sample, c.alpha) == (1.5, True, 0.3)
    c = _criterion({"loss": "focal", "loss_args": {"alpha": None}})
    assert c.focal_alpha is None
    mod = nn.BCEWithLogitsLoss()
    assert _criterion({"loss": mod}) is mod
    for bad in ("Dice", "tversky_focal", "", None, 3):
        with pytest.raises(ValueError):
            _criterion({"loss": bad})
    with pytest.raises(ValueError):
        _criterion({"loss": "tversky", "loss_args": {"alpha": -1.0}})
