"""Patch training through the loaders on the GPU: ``data.assemble_patch_batch`` (label on the grid,
pcms_foreground_pick, pcms_patch_resample_linear per modality, pcms_window_gather for the label
patches) must give the host loader's batch bit for bit; a ``Trainer`` with ``patches`` in its
config trains on those batches.  The tree is tests/test_patch_host.py's: five modalities of
different shapes and types, DWI missing (zero_fill)."""
import numpy as np
import pytest
import torch

from tests.test_patch_host import AUG, LABEL_SHAPE, PATCH, make_tree

pytestmark = pytest.mark.gpu


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp("patch_tree_gpu")))


def _loader(tree, raw, augment=None, **ps):
    patches = dict(dict(patch_size=PATCH, patches_per_case=3, foreground_prob=0.5, seed=4), **ps)
    return _data().get_dataloader(tree, batch_size=2, shuffle=False, device_resample=raw, augment=augment,
                                  augment_seed=9, patches=patches)


def _equal(got, ref, what):
    assert got["case_id"] == ref["case_id"], what
    for key in ("image", "label"):
        assert got[key].device.type == "cuda" and got[key].dtype == torch.float32 and got[key].shape == ref[key].shape
        a, b = got[key].cpu().view(torch.int32), ref[key].view(torch.int32)
        assert torch.equal(a, b), f"{what} {key}: {int((a != b).sum())} of {a.numel()} voxels differ"
    assert torch.equal(got["picks"].cpu(), ref["picks"]), (what, got["picks"].tolist(), ref["picks"].tolist())


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalise"])
@pytest.mark.parametrize("augment", [None, AUG], ids=["identity", "augment"])
def test_device_batches_equal_the_host_loader(tree, augment, normalise):
    d = _data()
    host, dev = _loader(tree, False, augment, normalise=normalise), _loader(tree, True, augment, normalise=normalise)
    seen = []
    for epoch in (0, 1):
        host.dataset.set_epoch(epoch)
        dev.dataset.set_epoch(epoch)
        ref, raw = next(iter(host)), next(iter(dev))
        got = d.assemble_batch(raw, None, "cuda")
        assert got["image"].shape == (6, 5) + PATCH and got["label"].shape == (6, 1) + PATCH
        assert got["case_id"] == ["p0"] * 3 + ["p1"] * 3
        _equal(got, ref, f"epoch {epoch}")
        again = d.device_batch(raw, "cuda")   # assembled twice: the same batch
        assert torch.equal(again["image"].view(torch.int32), got["image"].view(torch.int32))
        assert torch.equal(again["label"], got["label"]) and torch.equal(again["picks"], got["picks"])
        assert not got["image"][:, 1].any() and got["image"][:, 0].any()   # DWI is zero_fill
        seen.append(got)
    assert not torch.equal(seen[0]["picks"], seen[1]["picks"])
    assert not torch.equal(seen[0]["image"], seen[1]["image"])


@pytest.mark.parametrize("augment", [None, AUG], ids=["identity", "augment"])
def test_foreground_patches_hold_foreground(tree, augment):
    """foreground_prob = 1: the count in ``picks`` is the host form's T and no label patch is empty."""
    d = _data()
    dev = _loader(tree, True, augment, foreground_prob=1.0)
    got = d.assemble_batch(next(iter(dev)), None, "cuda")
    ds = dev.dataset
    for i in range(2):
        tf = d.draw_transform(augment if augment is not None else d.Augment(), 9, 0, i)
        lab = d.read_nifti(ds.case_list[i]["label_path"])
        grid = (d.resample_affine(lab, LABEL_SHAPE, *tf.affine(lab.shape, LABEL_SHAPE), nearest=True) > 0)
        origins, T = d.pick_origins(grid.astype(np.float32), PATCH, *d.draw_patches(ds.patches, 4, 0, i, LABEL_SHAPE))
        assert T > 0 and int(got["picks"][i, 9]) == T
        assert got["picks"][i, :9].cpu().tolist() == origins.reshape(-1).tolist()
    assert (got["label"].sum(dim=(1, 2, 3, 4)) > 0).all()


def test_a_grid_other_than_the_label_shape(tree):
    """``grid`` set: every volume, the label included, is resampled onto it."""
    d = _data()
    host, dev = _loader(tree, False, AUG, grid=(16, 56, 40)), _loader(tree, True, AUG, grid=(16, 56, 40))
    _equal(d.assemble_batch(next(iter(dev)), None, "cuda"), next(iter(host)), "grid (16, 56, 40)")


def test_trainer_steps_on_patches(tree):
    from pcms_amd.utils.trainer import Trainer
    cfg = {"device": "cuda", "learning_rate": 1e-3, "batch_size": 2, "num_epochs": 1, "loss": "bce_dice",
           "precision": "fp32", "data_dir": tree, "device_resample": True, "augment": AUG,
           "patches": dict(patch_size=PATCH, patches_per_case=3)}
    torch.manual_seed(0)
    tr = Trainer(cfg)
    shapes = []
    hook = tr.model.register_forward_pre_hook(lambda mod, args: shapes.append(tuple(args[0].shape)))
    losses = []
    for _ in range(2):
        for batch in tr.train_loader:
            losses.append(tr.step(batch))
    hook.remove()
    assert shapes == [(6, 5) + PATCH] * 2, shapes
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses), losses


def test_patches_none_is_todays_batch(tree):
    d = _data()
    kw = dict(batch_size=2, shuffle=False, target_size=(8, 16, 16))
    ref = next(iter(d.get_dataloader(tree, **kw)))
    raw = next(iter(d.get_dataloader(tree, device_resample=True, patches=None, **kw)))
    assert "patches" not in raw
    got = d.assemble_batch(raw, None, "cuda")
    assert set(got) == {"image", "label", "case_id"}
    assert torch.equal(got["image"].cpu().view(torch.int32), ref["image"].view(torch.int32))
    assert torch.equal(got["label"].cpu(), ref["label"])
