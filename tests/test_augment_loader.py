"""Augmentation through the ``device_resample`` loader on the GPU: ``data.assemble_batch`` runs
the affine entry points with the transform each sample carries, and its batches must be the
default loader's augmented batches (``data.resample_affine`` on the host) bit for bit -- through
a two-epoch ``Trainer.train`` as well.  The tree is tests/test_device_loader.py's: int16 / uint8
/ float32 files, a .nii.gz, a 4-D and a big-endian file, scaled headers, a missing modality."""
import numpy as np
import pytest
import torch

from tests.test_augment import AUG
from tests.test_device_loader import TARGET, tree  # noqa: F401  (the synthetic tree fixture)

pytestmark = pytest.mark.gpu


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


def _loader(tree, strategy, raw, epoch=0, augment=AUG):
    ld = _data().get_dataloader(tree, batch_size=2, shuffle=False, missing_strategy=strategy, target_size=TARGET,
                                device_resample=raw, augment=augment, augment_seed=11)
    ld.dataset.set_epoch(epoch)
    return ld


@pytest.mark.parametrize("strategy", ["zero_fill", "duplicate"])
def test_assembled_batches_equal_the_default_loader(tree, strategy):
    d = _data()
    epochs = []
    for epoch in (0, 1):
        n, batches = 0, []
        for ref, raw in zip(_loader(tree, strategy, False, epoch), _loader(tree, strategy, True, epoch)):
            got = d.assemble_batch(raw, TARGET, "cuda")
            assert got["case_id"] == ref["case_id"]
            assert torch.equal(got["image"].cpu().view(torch.int32), ref["image"].view(torch.int32))
            assert torch.equal(got["label"].cpu(), ref["label"])
            if strategy == "zero_fill" and "c2" in ref["case_id"]:  # the missing DWI: one fill, still zero
                assert not got["image"][ref["case_id"].index("c2"), 1].any()
            n += ref["image"].shape[0]
            batches.append(got)
        assert n == 4
        epochs.append(batches)
    for a, b in zip(*epochs):  # the next epoch draws other transforms
        assert not torch.equal(a["image"], b["image"]) and not torch.equal(a["label"], b["label"])
    # and with the identity settings the augmenting path gives the plain loader's geometry
    for ref, raw in zip(_loader(tree, strategy, False, augment=None), _loader(tree, strategy, True, augment={})):
        got = d.assemble_batch(raw, TARGET, "cuda")
        assert torch.equal(got["image"].cpu().view(torch.int32), ref["image"].view(torch.int32))
        assert torch.equal(got["label"].cpu(), ref["label"])


def _train(tree, raw, augment):
    from pcms_amd.utils.trainer import Trainer
    cfg = {"device": "cuda", "learning_rate": 1e-3, "batch_size": 2, "num_epochs": 2, "loss": "bce_dice",
           "precision": "bf16", "data_dir": tree, "validation": True, "target_size": TARGET,
           "device_resample": raw, "augment": augment, "augment_seed": 11}
    torch.manual_seed(0)
    tr = Trainer(cfg)
    assert tr.train_loader.dataset.device_resample == raw and tr.val_loader.dataset.augment is None
    first_val = tr.validate_epoch()  # before any step: the initial model on the validation loader
    losses = []
    train_epoch = tr.train_epoch

    def recorded():
        losses.append((tr.train_loader.dataset.epoch, train_epoch()))
        return losses[-1][1]

    tr.train_epoch = recorded
    torch.manual_seed(1)  # the shuffled order of the train loader
    tr.train()
    eng = tr.model.engine()
    torch.cuda.synchronize()
    return first_val, losses, eng.flat_p.clone(), eng.flat_bn.clone()


def test_trainer_two_epochs_bit_identical_on_both_loaders(tree):
    """bf16 build, 2 epochs of 2 batches of 2 (batch k + 1 assembled on the copy stream under
    step k): equal per-epoch losses and final weights / BN buffers on the two loaders; the
    epochs differ (other transforms); validation is the un-augmented one."""
    a = _train(tree, False, AUG)
    b = _train(tree, True, AUG)
    assert [e for e, _ in a[1]] == [0, 1] == [e for e, _ in b[1]]
    assert a[1] == b[1], (a[1], b[1])
    assert all(np.isfinite(v) for _, v in a[1])
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))
    plain = _train(tree, True, None)
    assert plain[0] == a[0] == b[0] and np.isfinite(a[0])  # the validation loss does not see `augment`
    assert plain[1] != b[1] and not torch.equal(plain[2], b[2])  # while training does
