"""Elastic deformation through the ``device_resample`` loader on the GPU: ``data.assemble_batch``
uploads each case's control grid once and runs the deforming entry points for the case's volumes,
and its batches must be the default loader's (``data.resample_deform`` on the host) bit for bit --
through a one-epoch ``Trainer.train`` as well.  The tree is tests/test_device_loader.py's."""
import numpy as np
import pytest
import torch

from tests.test_augment import AUG
from tests.test_deform import ELASTIC
from tests.test_device_loader import TARGET, tree  # noqa: F401  (the synthetic tree fixture)

pytestmark = pytest.mark.gpu


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


def _loader(tree, strategy, raw, epoch=0, augment=ELASTIC):
    ld = _data().get_dataloader(tree, batch_size=2, shuffle=False, missing_strategy=strategy, target_size=TARGET,
                                device_resample=raw, augment=augment, augment_seed=11)
    ld.dataset.set_epoch(epoch)
    return ld


def _equal(got, ref):
    return (got["case_id"] == ref["case_id"]
            and torch.equal(got["image"].cpu().view(torch.int32), ref["image"].cpu().view(torch.int32))
            and torch.equal(got["label"].cpu(), ref["label"].cpu()))


@pytest.mark.parametrize("strategy", ["zero_fill", "duplicate"])
def test_assembled_batches_equal_the_default_loader(tree, strategy):
    d = _data()
    epochs = []
    for epoch in (0, 1):
        n, batches = 0, []
        for ref, raw in zip(_loader(tree, strategy, False, epoch), _loader(tree, strategy, True, epoch)):
            assert all(a["field"].shape == (5, 5, 5, 3) for a in raw["augment"])
            got = d.assemble_batch(raw, TARGET, "cuda")
            assert _equal(got, ref)
            if strategy == "zero_fill" and "c2" in ref["case_id"]:  # the missing DWI: one fill, still zero
                assert not got["image"][ref["case_id"].index("c2"), 1].any()
            n += ref["image"].shape[0]
            batches.append(got)
        assert n == 4
        epochs.append(batches)
    for a, b in zip(*epochs):  # the next epoch draws other transforms and fields
        assert not torch.equal(a["image"], b["image"]) and not torch.equal(a["label"], b["label"])
    # with elastic off the augmenting path gives today's augmented batches: the affine host form's,
    # which the deformed ones differ from
    for ref, raw, deformed in zip(_loader(tree, strategy, False, augment=AUG), _loader(tree, strategy, True, augment=AUG),
                                  epochs[0]):
        assert all(a.get("field") is None for a in raw["augment"])
        got = d.assemble_batch(raw, TARGET, "cuda")
        assert _equal(got, ref)
        assert not torch.equal(got["image"], deformed["image"]) and not torch.equal(got["label"], deformed["label"])


def _train(tree, raw):
    from pcms_amd.utils.trainer import Trainer
    cfg = {"device": "cuda", "learning_rate": 1e-3, "batch_size": 2, "num_epochs": 1, "loss": "bce_dice",
           "precision": "bf16", "data_dir": tree, "validation": False, "target_size": TARGET,
           "device_resample": raw, "augment": ELASTIC, "augment_seed": 11}
    torch.manual_seed(0)
    tr = Trainer(cfg)
    ds = tr.train_loader.dataset
    assert ds.device_resample == raw and ds.augment.elastic_grid == (5, 5, 5)
    losses = []
    train_epoch = tr.train_epoch

    def recorded():
        losses.append(train_epoch())
        return losses[-1]

    tr.train_epoch = recorded
    torch.manual_seed(1)  # the shuffled order of the train loader
    tr.train()
    eng = tr.model.engine()
    torch.cuda.synchronize()
    return losses, eng.flat_p.clone(), eng.flat_bn.clone()


def test_trainer_one_epoch_bit_identical_on_both_loaders(tree):
    """bf16 build, one epoch of 2 batches of 2 (batch 2 assembled on the copy stream under step
    1): equal losses and final weights / BN buffers on the two loaders."""
    a = _train(tree, False)
    b = _train(tree, True)
    assert len(a[0]) == 1 and a[0] == b[0], (a[0], b[0])
    assert all(np.isfinite(v) for v in a[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
