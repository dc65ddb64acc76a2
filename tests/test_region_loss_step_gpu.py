"""The imbalance-aware losses inside the training step: ``UNet3D(5, 2, precision="fp32")`` at
(2, 5, 16, 16, 16), train mode, ``FocalTverskyFocalLoss(per_sample=True)``.  (Two samples: the
bottleneck of a 16^3 input is one voxel, and a train-mode BatchNorm needs more than one value per
channel -- one sample raises, here as in torch.)"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = (16, 16, 16)


def batch(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 5, *SHAPE, generator=g)
    y = (torch.rand(2, 2, *SHAPE, generator=g) < 0.1).float()
    y[0, 1] = 0.0  # a channel without a lesion
    return x, y


def model():
    from pcms_amd.models.unet3d import UNet3D
    torch.manual_seed(0)
    return UNet3D(n_modalities=5, n_classes=2, precision="fp32").cuda().train()


def test_criterion_backward_is_the_engine_backward_of_its_dx():
    """``criterion(model(x), y).backward()`` leaves the flat gradient that a second forward on the
    same state followed by ``logits.backward(dx)`` leaves, bit for bit, with dx the criterion's
    gradient on a detached leaf copy of the logits: the engine's backward is linear in dlogits and
    the step is deterministic."""
    from pcms_amd.optim import FlatAdam
    from pcms_amd.utils.losses import FocalTverskyFocalLoss
    x, y = batch(3)
    x, y = x.cuda(), y.cuda()
    m = model()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-5)
    eng = m.engine()
    crit = FocalTverskyFocalLoss(per_sample=True)
    bn0 = eng.flat_bn.clone()
    opt.zero_grad()
    loss = crit(m(x), y)
    loss.backward()
    g1 = eng.flat_g.clone()
    assert math.isfinite(loss.item()) and torch.isfinite(g1).all() and g1.abs().max().item() > 0
    eng.flat_bn.copy_(bn0)  # the BatchNorm running buffers the first forward moved
    opt.zero_grad()
    logits = m(x)
    leaf = logits.detach().clone().requires_grad_(True)
    loss2 = crit(leaf, y)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach())
    logits.backward(leaf.grad)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat_g.view(torch.int32), g1.view(torch.int32))


def test_trainer_steps_with_a_named_loss():
    from pcms_amd.utils.losses import FocalTverskyFocalLoss
    from pcms_amd.utils.trainer import Trainer
    cfg = {"device": "cuda", "learning_rate": 1e-3, "batch_size": 2, "num_epochs": 1, "precision": "fp32",
           "loss": "focal_tversky_focal", "loss_args": {"per_sample": True, "region_weight": 0.6, "voxel_weight": 0.4}}
    batches = [dict(zip(("image", "label"), batch(s))) for s in (3, 4, 5)]
    tr = Trainer(cfg, train_loader=batches, model=model())
    assert type(tr.criterion) is FocalTverskyFocalLoss
    assert (tr.criterion.per_sample, tr.criterion.region_weight, tr.criterion.voxel_weight) == (True, 0.6, 0.4)
    p0 = tr.model.engine().flat_p.clone()
    losses = [tr.step(b) for b in batches]
    assert all(math.isfinite(v) and v > 0 for v in losses), losses
    p1 = tr.model.engine().flat_p
    assert torch.isfinite(p1).all() and not torch.equal(p0, p1)
