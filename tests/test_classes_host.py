"""The host forms of pcms_amd.classes (no GPU): the loss definition against torch and against the
existing region loss, the class table, the first-maximum rule, the per-class scores, and the
class-map labels of the host loader."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcms_amd  # noqa: F401
from pcms_amd import classes, data
from pcms_amd.utils import losses, metrics


def logits(C, seed=0, shape=(4, 5, 6), scale=3.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, C, *shape, generator=g, dtype=torch.float64) * scale
    y = torch.randint(0, C, (2,) + shape, generator=g)
    return x, y


@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("weighted", [False, True])
def test_ce_term_is_torch_cross_entropy(C, weighted):
    x, y = logits(C, seed=C)
    y[0, 0, 0, :3] = 255
    y[1, 2] = 255
    w = [0.2 + 0.7 * c for c in range(C)] if weighted else None
    got = classes.softmax_dice_ce_loss_host(x, y.float(), ce_weight=1.0, dice_weight=0.0, class_weights=w)
    want = F.cross_entropy(x, y, weight=None if w is None else torch.tensor(w, dtype=torch.float64), ignore_index=255)
    assert abs(got.item() - want.item()) <= 1e-12
    # (N, 1, ...) and uint8 targets are the same class map
    assert classes.softmax_dice_ce_loss_host(x, y[:, None].to(torch.uint8), 1.0, 0.0, class_weights=w).item() == got.item()


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("smooth", [1.0, 0.3])
def test_two_class_dice_is_the_region_loss(per_sample, smooth):
    """C = 2 without background, ce_weight = 0, nothing ignored: softmax_1 = sigmoid(x_1 - x_0), so
    this is ``region_voxel_loss_host`` at alpha = beta = 0.5 and smooth s / 2 -- the same Dice."""
    x, y = logits(2, seed=7)
    xr = x.clone().requires_grad_(True)
    got = classes.softmax_dice_ce_loss_host(xr, y[:, None].float(), ce_weight=0.0, dice_weight=1.0, smooth=smooth,
                                            per_sample=per_sample)
    dr = (x[:, 1:2] - x[:, 0:1]).clone().requires_grad_(True)
    want = losses.region_voxel_loss_host(dr, y[:, None].double(), alpha=0.5, beta=0.5, smooth=smooth / 2,
                                         per_sample=per_sample)
    assert abs(got.item() - want.item()) <= 1e-12
    got.backward()
    want.backward()
    assert (xr.grad[:, 1:2] - dr.grad).abs().max().item() <= 1e-12
    assert (xr.grad[:, 0:1] + dr.grad).abs().max().item() <= 1e-12


def test_ignored_voxels_and_empty_groups():
    x, y = logits(3, seed=1)
    y = y.float()
    base = classes.softmax_dice_ce_loss_host(x, y, per_sample=True)
    # an ignored voxel's logits do not matter and get no gradient
    y2, x2 = y.clone(), x.clone().requires_grad_(True)
    y2[0, 1, 2, 3] = 7.0
    y2[1, 0, 0, 0] = 1.5
    y2[1, 0, 0, 1] = -1.0
    loss = classes.softmax_dice_ce_loss_host(x2, y2, per_sample=True)
    loss.backward()
    assert loss.item() != base.item()
    for idx in ((0, slice(None), 1, 2, 3), (1, slice(None), 0, 0, 0), (1, slice(None), 0, 0, 1)):
        assert (x2.grad[idx] == 0).all()
    # nothing valid: CE = 0 and every Dice is smooth / smooth = 1, or 1 by rule at smooth = 0
    none = torch.full_like(y, 255.0)
    for smooth in (1.0, 0.0):
        assert classes.softmax_dice_ce_loss_host(x, none, smooth=smooth, include_background=True).item() == 0.0


def test_bad_arguments_raise():
    x, y = logits(3)
    y = y.float()
    for kw in (dict(smooth=-1.0), dict(ce_weight=float("nan")), dict(dice_weight=float("inf")), dict(smooth="1"),
               dict(ce_weight=True), dict(class_weights=(1.0, 1.0)), dict(class_weights=(1.0, -1.0, 1.0)),
               dict(class_weights=(1.0, float("nan"), 1.0))):
        with pytest.raises(ValueError):
            classes.softmax_dice_ce_loss_host(x, y, **kw)
    for kw in (dict(smooth=-1.0), dict(ce_weight=float("nan")), dict(class_weights=(1.0,)),
               dict(class_weights=(1.0, -2.0))):
        with pytest.raises(ValueError):
            losses.SoftmaxDiceCELoss(**kw)
    with pytest.raises(ValueError):
        classes.softmax_dice_ce_loss_host(x[:, :1], y)          # one logit plane
    with pytest.raises(ValueError):
        classes.softmax_dice_ce_loss_host(x, y[:, :2])          # not the logits' grid
    with pytest.raises(ValueError):
        classes.softmax_dice_ce_loss_host(torch.zeros(2, 9, 4, 4, 4), torch.zeros(2, 4, 4, 4))
    assert losses.LOSSES["softmax_dice_ce"] is losses.SoftmaxDiceCELoss
    crit = losses.create_criterion("softmax_dice_ce", {"class_weights": [1, 2, 3], "per_sample": True})
    assert crit.class_weights == (1.0, 2.0, 3.0) and crit.per_sample and not crit.include_background
    with pytest.raises(RuntimeError, match="ROCm device only"):
        crit(x.float(), y)


def test_classes_of_maps_unnamed_values_to_background():
    v = np.array([[0, 1, 2], [5, 7, 2], [-2, 5, 255]], dtype=np.int16)
    want = np.array([[0, 0, 1], [2, 0, 1], [0, 2, 0]], dtype=np.float32)
    got = classes.classes_of(v, (2, 5))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(classes.classes_of(v.astype(np.float64) + 1e-9, (2, 5)), want)  # the fp32 value decides
    assert np.array_equal(classes.classes_of(v, (2, 2.0 + 2.0 ** -30)), (v == 2).astype(np.float32))  # the first entry wins
    for bad in ((), tuple(range(1, 9)), (1.0, float("nan"))):
        with pytest.raises(ValueError):
            classes.classes_of(v, bad)
    assert classes.class_values_of(4) == (1.0, 2.0, 3.0) and classes.class_values_of(3, (2, 5)) == (2.0, 5.0)
    for n, values in ((3, (1,)), (3, (2, 2)), (3, (1, 0.1)), (1, None), (9, None), (True, None)):
        with pytest.raises(ValueError):
            classes.class_values_of(n, values)


def test_labels_on_grid_takes_the_first_maximum():
    rng = np.random.default_rng(3)
    p = rng.random((3, 4, 5, 6)).astype(np.float32)
    p[2] = p[1]                      # classes 1 and 2 equal on purpose
    p[0, :2] = 0.0                   # ... and above class 0 there
    labels, native = classes.labels_on_grid(p, (4, 5, 6))
    assert labels.dtype == np.uint8 and native.dtype == np.float32 and np.array_equal(native, p)
    assert (labels[:2] == 1).all() and not (labels == 2).any()
    # a finer native grid: the same first-maximum rule on the resampled planes, class 0 past the edge
    labels, native = classes.labels_on_grid(p, (8, 7, 6))
    assert native.shape == (3, 8, 7, 6) and np.array_equal(labels, np.argmax(native, axis=0))
    assert (native[:, -1] == 0).all() and (labels[-1] == 0).all() and not (labels == 2).any()
    with pytest.raises(ValueError):
        classes.labels_on_grid(p[0], (4, 5, 6))


def test_class_scores_agree_with_the_binary_scores():
    rng = np.random.default_rng(11)
    pred = rng.integers(0, 3, size=(6, 7, 8)).astype(np.uint8)
    ref = rng.integers(0, 3, size=(6, 7, 8)).astype(np.uint8)
    s = metrics.calculate_class_scores(pred, ref, 4)      # class 3 is in neither map
    assert len(s["dice"]) == len(s["iou"]) == 4
    for c in range(3):
        p, t = torch.from_numpy((pred == c).astype(np.float32)), torch.from_numpy((ref == c).astype(np.float32))
        assert abs(s["dice"][c] - metrics.calculate_dice_score(p, t)) <= 1e-6
        assert abs(s["iou"][c] - metrics.calculate_iou(p, t)) <= 1e-6
    assert s["dice"][3] == 1.0 and s["iou"][3] == 1.0      # an empty class scores 1.0
    assert s["mean_dice"] == sum(s["dice"][1:]) / 3 and s["mean_iou"] == sum(s["iou"][1:]) / 3
    counts = classes.class_overlap(pred, ref, 3)
    assert counts.dtype == np.int64 and counts[:, 0].sum() == pred.size and counts[:, 1].sum() == ref.size
    with pytest.raises(TypeError):
        metrics.calculate_class_scores(pred, torch.from_numpy(ref), 3)
    with pytest.raises(ValueError):
        classes.class_overlap(pred, ref[:2], 3)


def make_dataset(tmp_path):
    """Two cases of five (6, 9, 7) int16 modalities and a uint8 label with the values 0, 2, 5 and 9."""
    rng = np.random.default_rng(2)
    for cid in ("a", "b"):
        for m in data.DEFAULT_MODALITIES:
            p = tmp_path / "BPH-PCA" / "BPH" / m
            p.mkdir(parents=True, exist_ok=True)
            data.write_nifti(str(p / f"{cid}.nii"), rng.integers(0, 100, size=(6, 9, 7)).astype(np.int16))
        p = tmp_path / "BPH-PCA" / "ROI(BPH+PCA)" / "BPH"
        p.mkdir(parents=True, exist_ok=True)
        data.write_nifti(str(p / f"{cid}.nii"), rng.choice(np.array([0, 0, 2, 5, 9], dtype=np.uint8), size=(6, 9, 7)))
    return str(tmp_path)


@pytest.fixture()
def dataset_dir(tmp_path):
    return make_dataset(tmp_path)


@pytest.mark.parametrize("target", [(6, 9, 7), (8, 8, 8)])
def test_dataset_keeps_a_class_map(dataset_dir, target):
    from pcms_amd.resample import resample
    plain = data.ProstateDataset(dataset_dir, target_size=target)
    ds = data.ProstateDataset(dataset_dir, target_size=target, n_classes=3, class_values=(2, 5))
    lab = data.read_nifti(ds.case_list[0]["label_path"])
    got, binary = ds[0], plain[0]
    assert got["label"].shape == (1,) + target and got["label"].dtype == torch.float32
    assert np.array_equal(got["label"][0].numpy(), classes.classes_of(resample(lab, target, nearest=True), (2, 5)))
    assert set(np.unique(got["label"].numpy())) == {0.0, 1.0, 2.0}
    assert torch.equal(got["image"], binary["image"])
    # n_classes = 1 is today's label; the value 9 is foreground there and background in the class map
    assert torch.equal(binary["label"], data.ProstateDataset(dataset_dir, target_size=target, n_classes=1)[0]["label"])
    assert (binary["label"] >= (got["label"] > 0).float()).all() and binary["label"].sum() > (got["label"] > 0).sum()
    aug = data.ProstateDataset(dataset_dir, target_size=target, n_classes=3, class_values=(2, 5),
                               augment={"flip_prob": (1.0, 0.0, 0.0)})
    assert set(np.unique(aug[0]["label"].numpy())) <= {0.0, 1.0, 2.0} and aug[0]["label"].max() == 2.0
    raw = data.ProstateDataset(dataset_dir, target_size=target, n_classes=3, class_values=(2, 5), device_resample=True)
    loader = data.get_dataloader(dataset_dir, batch_size=2, shuffle=False, target_size=target, n_classes=3,
                                 class_values=(2, 5), device_resample=True)
    assert raw.class_values == (2.0, 5.0) and next(iter(loader))["class_values"] == (2.0, 5.0)
    with pytest.raises(ValueError, match="elastic"):
        data.ProstateDataset(dataset_dir, n_classes=3, augment={"elastic_grid": 4, "elastic_disp": (1.0, 1.0, 1.0)})
    with pytest.raises(ValueError):
        data.ProstateDataset(dataset_dir, class_values=(2, 5))
    with pytest.raises(ValueError):
        data.ProstateDataset(dataset_dir, n_classes=3, class_values=(2,))
