"""Mutually exclusive classes end to end on the GPU: the training step with
``n_classes=3, loss="softmax_dice_ce"`` on synthetic 16^3 data, the untouched ``n_classes=1`` path,
and ``predict_case`` of a three-class predictor against the host chain.  (Two samples per batch:
the bottleneck of a 16^3 input is one voxel, and a train-mode BatchNorm needs more than one value
per channel.)"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = (16, 16, 16)
FLIPS = ((2,), (0, 1))


def batch(seed, n_classes):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 5, *SHAPE, generator=g)
    if n_classes == 1:
        return x, (torch.rand(2, 1, *SHAPE, generator=g) < 0.1).float()
    y = torch.randint(0, n_classes, (2, 1) + SHAPE, generator=g).float()
    y[torch.rand(y.shape, generator=g) < 0.6] = 0.0  # mostly background
    return x, y


def model(n_classes):
    from pcms_amd.models.unet3d import UNet3D
    torch.manual_seed(0)
    return UNet3D(n_modalities=5, n_classes=n_classes, precision="fp32").cuda().train()


def config(**kw):
    return dict({"device": "cuda", "learning_rate": 1e-3, "batch_size": 2, "num_epochs": 1, "precision": "fp32"}, **kw)


def test_trainer_steps_on_three_classes():
    from pcms_amd.utils.losses import SoftmaxDiceCELoss
    from pcms_amd.utils.trainer import Trainer
    batches = [dict(zip(("image", "label"), batch(s, 3))) for s in (3, 4)]
    tr = Trainer(config(n_classes=3, loss="softmax_dice_ce", loss_args={"per_sample": True}), train_loader=batches,
                 val_loader=batches[:1])
    assert type(tr.criterion) is SoftmaxDiceCELoss and tr.criterion.per_sample
    assert tr.model.n_classes == 3 and tuple(tr.model.outc.weight.shape[:2]) == (3, tr.model.outc.weight.shape[1])
    p0 = tr.model.engine().flat_p.clone()
    losses = []
    for b in batches:
        losses.append(tr.step(b))
        g = tr.model.outc.weight.grad
        assert g is not None and torch.isfinite(g).all()
        assert all(g[c].abs().max().item() > 0 for c in range(3)), "a class row of the head has no gradient"
    assert all(math.isfinite(v) and v > 0 for v in losses), losses
    p1 = tr.model.engine().flat_p
    assert torch.isfinite(p1).all() and not torch.equal(p0, p1)
    # validation: the loss, and the mean foreground Dice of the argmax
    val = tr.validate_epoch()
    assert math.isfinite(val) and 0.0 <= tr.last_val_dice <= 1.0 and len(tr.last_val_class_dice) == 3
    from pcms_amd import classes
    with torch.no_grad():
        tr.model.eval()
        logits = tr.model(batches[0]["image"].cuda()).float().cpu()
    want = classes.class_overlap(logits.argmax(1).numpy(), batches[0]["label"][:, 0].numpy(), 3)
    dice, _ = classes.scores_of_counts(want)
    assert tr.last_val_class_dice == dice


def test_one_class_path_keeps_its_bits():
    """``n_classes=1`` with the default loss: the config key changes nothing -- the same losses and
    parameters, bit for bit, as a trainer whose config does not name it."""
    from pcms_amd.utils.losses import DiceLoss
    from pcms_amd.utils.trainer import Trainer
    batches = [dict(zip(("image", "label"), batch(s, 1))) for s in (3, 4)]
    runs = []
    for cfg in (config(), config(n_classes=1)):
        torch.manual_seed(0)
        tr = Trainer(cfg, train_loader=batches)
        assert type(tr.criterion) is DiceLoss and tr.model.n_classes == 1
        losses = [tr.step_async(b).cpu() for b in batches]
        runs.append((losses, tr.model.engine().flat_p.clone().cpu()))
    (l0, p0), (l1, p1) = runs
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(l0, l1))
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Three present modalities of different shapes, two missing; a class-map label with the values
    (0, 2, 5); a seeded three-class checkpoint."""
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    root = tmp_path_factory.mktemp("classes_case")
    rng = np.random.default_rng(5)
    vols = [rng.integers(0, 4000, size=(10, 14, 12)).astype(np.int16), None,
            (300.0 * rng.standard_normal((9, 15, 13))).astype(np.float32), None,
            rng.integers(0, 256, size=(11, 13, 12)).astype(np.uint8)]
    for mod, vol in zip(predict.MODALITIES, vols):
        os.makedirs(root / "case" / mod)
        if vol is not None:
            data.write_nifti(str(root / "case" / mod / "scan.nii"), vol, spacing=(0.6, 0.7, 3.0))
    label = str(root / "label.nii")
    data.write_nifti(label, rng.choice(np.array([0, 0, 2, 5, 7], dtype=np.uint8), size=(10, 14, 12)),
                     spacing=(0.6, 0.7, 3.0))
    ckpt = str(root / "model.pth")
    torch.save(model(3).state_dict(), ckpt)
    return {"dir": str(root / "case"), "native": (10, 14, 12), "label": label, "root": root,
            "predictor": predict.ModelPredictor(ckpt, device="cuda", precision="fp32", n_classes=3,
                                                class_values=(2, 5))}


@pytest.mark.parametrize("flips", [(), FLIPS])
def test_predict_case_equals_the_host_chain(case, flips):
    """Labels and probabilities byte-equal to host flip mean, then ``labels_on_grid``, on the
    device's own softmax output."""
    from pcms_amd import classes, predict
    pred = case["predictor"]
    x = predict.prepare_case_device(case["dir"], SHAPE, "zero_fill", True, "cuda")
    batch_ = torch.cat([x] + [torch.flip(x, dims=[2 + a for a in f]) for f in flips], dim=0)
    with torch.no_grad():
        probs = classes.softmax_planes_device(pred.model(batch_)).cpu().numpy()  # (C, k, D, H, W)
    mean = np.stack([predict.tta_mean(list(probs[c]), [()] + list(flips)) for c in range(3)])
    want, want_planes = classes.labels_on_grid(mean, case["native"])
    res = pred.predict_case(case["dir"], target_size=SHAPE, tta_flips=flips, return_probability=True)
    assert res.mask.dtype == np.uint8 and res.mask.shape == case["native"]
    assert np.array_equal(res.mask, want)
    assert np.array_equal(res.probability.view(np.int32), want_planes.view(np.int32))
    assert len(np.unique(want)) > 1, "the seeded network predicts one class everywhere"


def test_postprocess_scores_and_save(case):
    from pcms_amd import classes, data, predict
    pred = case["predictor"]
    plain = pred.predict_case(case["dir"], target_size=SHAPE)
    res = pred.predict_case(case["dir"], target_size=SHAPE, keep_largest=1, return_lesions=True)
    want = plain.mask.copy()
    for c in (1, 2):  # the host post-processing of labels == c; a removed voxel becomes 0
        own = (plain.mask == c).astype(np.uint8)
        want[(own != 0) & (predict.postprocess(own, keep_largest=1) == 0)] = 0
    assert np.array_equal(res.mask, want)
    assert all(r["class"] in (1, 2) for r in res.lesions)
    assert sorted(r["class"] for r in res.lesions) == [c for c in (1, 2) if (want == c).any()]
    scores = pred.score_case(plain, case["label"])
    label = classes.classes_of(data.read_nifti(case["label"]), (2, 5)).astype(np.uint8)
    dice, iou = classes.scores_of_counts(classes.class_overlap(plain.mask, label, 3))
    assert scores["class_dice"] == dice and scores["class_iou"] == iou
    assert scores["dice"] == sum(dice[1:]) / 2 and [r["class"] for r in scores["classes"]] == [1, 2]
    out = str(case["root"] / "labels.nii")
    pred.save_case(plain, out)
    assert np.array_equal(data.read_nifti(out), plain.mask)
    with pytest.raises(ValueError, match="sliding-window"):
        pred.predict_case(case["dir"], target_size=SHAPE, window=(16, 16, 16))


def test_evaluate_scores_every_class():
    """``evaluate(n_classes=3)``: per-class Dice / IoU of the arg-max against the class map, the
    surface metrics per foreground class through the host form of the same name."""
    from pcms_amd import classes, distance
    from pcms_amd.utils import metrics
    m = model(3).eval()
    x, y = batch(7, 3)
    r = metrics.evaluate(m, [{"image": x, "label": y}], n_classes=3, surface_metrics=True, lesion_metrics=True)
    with torch.no_grad():
        pred = m(x.cuda()).float().argmax(1).cpu().numpy().astype(np.uint8)
    assert len(r["cases"]) == 2 and len(np.unique(pred)) > 1
    for i, case_ in enumerate(r["cases"]):
        lab = y[i, 0].numpy().astype(np.uint8)
        dice, iou = classes.scores_of_counts(classes.class_overlap(pred[i], lab, 3))
        assert case_["class_dice"] == dice and case_["class_iou"] == iou
        assert case_["dice"] == sum(dice[1:]) / 2 and case_["iou"] == sum(iou[1:]) / 2
        want = [distance.surface_metrics((pred[i] == c).astype(np.uint8), (lab == c).astype(np.uint8)) for c in (1, 2)]
        assert case_["hd95"] == pytest.approx([w["hd95"] for w in want], rel=1e-6)
        assert case_["assd"] == pytest.approx([w["assd"] for w in want], rel=1e-6)
        assert case_["lesion_tp"] + case_["lesion_fn"] > 0
    assert r["mean_dice"] == sum(c["dice"] for c in r["cases"]) / 2 and len(r["mean_class_dice"]) == 3


@pytest.mark.parametrize("mode", ["plain", "augment", "patches"])
def test_device_loader_gives_the_host_loader_s_class_maps(tmp_path, mode):
    """``n_classes=3, class_values=(2, 5)``: the ``device_resample`` loader's assembled batch equals
    the host loader's, labels byte for byte -- plain, under an augmenting affine, and as patches."""
    from pcms_amd import data
    from tests.test_classes_host import make_dataset
    root = make_dataset(tmp_path)
    kw = dict(batch_size=2, shuffle=False, target_size=(8, 10, 8), n_classes=3, class_values=(2, 5))
    if mode == "augment":
        kw.update(augment={"flip_prob": (0.5, 0.5, 0.5), "rotate_deg": (10, 5, 5), "zoom": (0.9, 1.1),
                           "shift_frac": (0.05, 0.05, 0.05)}, augment_seed=3)
    if mode == "patches":
        kw.update(patches={"patch_size": (16, 16, 16), "patches_per_case": 2, "foreground_prob": 0.5, "grid": (16, 20, 18)})
    host = next(iter(data.get_dataloader(root, **kw)))
    dev = data.assemble_batch(next(iter(data.get_dataloader(root, device_resample=True, **kw))), None, "cuda")
    assert dev["label"].dtype == torch.float32 and dev["label"].shape == host["label"].shape
    assert torch.equal(dev["label"].cpu(), host["label"]) and torch.equal(dev["image"].cpu(), host["image"])
    assert set(np.unique(host["label"].numpy())) == {0.0, 1.0, 2.0}
