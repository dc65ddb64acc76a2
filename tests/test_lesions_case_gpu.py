"""The lesion analysis end to end on the GPU: component_table_device / overlap_pairs_device /
lesion_table_device / lesion_metrics_device equal their host forms exactly (integer tables on the
bytes, everything in fp64 computed on the host by the same functions), and predict_case /
score_case / evaluate carry them without changing what they returned before."""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_blocks import _net
from tests.test_lesions_host import CASE_SHAPE, case_masks, labels, mask, prob, same_table

pytestmark = pytest.mark.gpu

TARGET = (16, 16, 16)
SPACING = (3.0, 0.5, 0.75)
OLD_KEYS = {"dice", "iou", "hd", "hd95", "assd", "n_a", "n_b"}


def _mods():
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    return data, predict


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_metrics(got, exp):
    assert set(got) == set(exp)
    for k, v in exp.items():
        if isinstance(v, float) and math.isnan(v):
            assert math.isnan(got[k]), k
        else:
            assert got[k] == v and type(got[k]) is type(v), k


@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_component_table_device_equals_host(connectivity):
    _, predict = _mods()
    lab = labels(f"bernoulli{connectivity}", CASE_SHAPE, connectivity)
    for p in (None, prob(CASE_SHAPE)):
        exp = predict.component_table(lab, p)
        assert len(exp["label"]) >= 100
        same_table(predict.component_table_device(_dev(lab), None if p is None else _dev(p)), exp)
        # a table of 8 rows: the count comes back and the launches run once more at that size
        same_table(predict.component_table_device(_dev(lab), None if p is None else _dev(p), capacity=8), exp)
    same_table(predict.component_table_device(_dev(np.zeros(CASE_SHAPE, np.int32)), _dev(prob(CASE_SHAPE))),
               predict.component_table(np.zeros(CASE_SHAPE, np.int32), prob(CASE_SHAPE)))
    # labels from the labelling kernel itself
    m = mask(f"bernoulli{connectivity}", CASE_SHAPE)
    same_table(predict.component_table_device(predict.label_components_device(_dev(m), connectivity)),
               predict.component_table(lab))


def test_device_forms_reject_what_they_cannot_run():
    _, predict = _mods()
    lab = labels("bernoulli26", CASE_SHAPE, 26)
    pred, ref = case_masks()
    for call in (lambda: predict.component_table_device(torch.from_numpy(lab)),
                 lambda: predict.component_table_device(_dev(lab), torch.from_numpy(prob(CASE_SHAPE))),
                 lambda: predict.overlap_pairs_device(torch.from_numpy(lab), _dev(lab)),
                 lambda: predict.lesion_table_device(torch.from_numpy(pred)),
                 lambda: predict.lesion_metrics_device(_dev(pred), torch.from_numpy(ref)),
                 lambda: predict.lesion_metrics_device(pred, ref)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        predict.component_table_device(_dev(lab), capacity=0)
    with pytest.raises(ValueError):
        predict.component_table_device(_dev(lab.astype(np.int64)))
    with pytest.raises(ValueError):
        predict.component_table_device(_dev(lab), _dev(prob(CASE_SHAPE)[:-1]))
    bad = lab.copy()
    bad.reshape(-1)[int(np.flatnonzero(lab.reshape(-1) == 0)[3])] = lab.size + 7
    with pytest.raises(RuntimeError, match="not canonical"):
        predict.component_table_device(_dev(bad))


@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_overlap_pairs_device_equals_host(connectivity):
    _, predict = _mods()
    pred, ref = case_masks()
    la, lb = predict.label_components(pred, connectivity), predict.label_components(ref, connectivity)
    exp = predict.overlap_pairs(la, lb, connectivity)
    got = predict.overlap_pairs_device(_dev(la), _dev(lb), connectivity)
    assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp) and len(exp) >= 20
    none = predict.overlap_pairs_device(_dev(la), _dev(np.zeros_like(lb)), connectivity)
    assert none.shape == (0, 3) and none.dtype == np.int64


def test_lesion_table_and_metrics_device_equal_host():
    _, predict = _mods()
    pred, ref = case_masks()
    p = prob(CASE_SHAPE, nan=False)
    for connectivity in (6, 26):
        assert predict.lesion_table_device(_dev(pred), _dev(p), SPACING, connectivity) == \
            predict.lesion_table(pred, p, SPACING, connectivity)
        assert predict.lesion_table_device(_dev(ref), None, SPACING, connectivity) == \
            predict.lesion_table(ref, None, SPACING, connectivity)
        for min_iou in (0.1, 0.5):
            exp = predict.lesion_metrics(pred, ref, p, SPACING, connectivity, min_iou)
            _same_metrics(predict.lesion_metrics_device(_dev(pred), _dev(ref), _dev(p), SPACING, connectivity, min_iou),
                          exp)
    assert exp["tp"] < predict.lesion_metrics(pred, ref)["tp"]  # min_iou matters on these masks
    empty = np.zeros(CASE_SHAPE, np.uint8)
    _same_metrics(predict.lesion_metrics_device(_dev(empty), _dev(ref)), predict.lesion_metrics(empty, ref))
    _same_metrics(predict.lesion_metrics_device(_dev(pred), _dev(empty)), predict.lesion_metrics(pred, empty))
    assert predict.lesion_table_device(_dev(empty)) == []


# ---- predict_case / score_case on a synthetic case ------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The synthetic case of tests/test_predict_case_gpu.py: five modality folders of different
    shapes and dtypes (one missing), a label on a grid of its own, a seeded checkpoint."""
    data, predict = _mods()
    root = tmp_path_factory.mktemp("lesion_case")
    rng = np.random.default_rng(21)
    vols = [rng.integers(0, 4000, size=(12, 20, 18)).astype(np.int16),
            rng.integers(0, 900, size=(2, 10, 24, 17)).astype(np.uint16),
            (500.0 * rng.standard_normal((13, 19, 20))).astype(np.float32),
            None,
            rng.integers(0, 256, size=(11, 21, 16)).astype(np.uint8)]
    spacings = [(0.5, 0.6, 3.0), (1.5, 1.4, 3.5, 1.0), (0.7, 0.7, 2.5), None, (0.9, 0.8, 3.2)]
    for i, (mod, vol) in enumerate(zip(predict.MODALITIES, vols)):
        os.makedirs(root / "case" / mod)
        if vol is not None:
            data.write_nifti(str(root / "case" / mod / "scan.nii"), vol, spacing=spacings[i])
    label = str(root / "label.nii")
    label_vol = (rng.random((9, 22, 15)) > 0.93).astype(np.uint8)
    data.write_nifti(label, label_vol, spacing=(0.8, 0.75, 4.0))
    ckpt = str(root / "model.pth")
    torch.save(_net().state_dict(), ckpt)
    predictor = predict.ModelPredictor(ckpt, device="cuda", precision="fp32")
    # a threshold that leaves about a tenth of the voxels: several components
    probability = predictor.predict_case(str(root / "case"), target_size=TARGET, output_like=label,
                                         return_probability=True).probability
    return {"dir": str(root / "case"), "label": label, "label_vol": label_vol, "predictor": predictor,
            "threshold": float(np.quantile(probability, 0.9)), "spacing": (4.0, 0.75, 0.8)}


def _predict_case(case, **kw):
    return case["predictor"].predict_case(case["dir"], target_size=TARGET, output_like=case["label"],
                                          threshold=case["threshold"], **kw)


def test_predict_case_lesions(case):
    _, predict = _mods()
    plain = _predict_case(case, return_probability=True)
    assert plain.lesions is None and 0.05 < float(plain.mask.mean()) < 0.15
    assert tuple(float(v) for v in plain.geometry["pixdim"][1:4])[::-1] == pytest.approx(case["spacing"])
    spacing = tuple(float(v) for v in plain.geometry["pixdim"][1:4])[::-1]
    for kw in ({}, {"connectivity": 6}, {"min_voxels": 3, "fill_holes": True}):
        before = _predict_case(case, return_probability=True, **kw)
        res = _predict_case(case, return_probability=True, return_lesions=True, **kw)
        assert before.lesions is None
        assert res.mask.tobytes() == before.mask.tobytes() and res.mask.dtype == np.uint8
        assert res.probability.tobytes() == before.probability.tobytes()
        assert res.lesions == predict.lesion_table(res.mask, res.probability, spacing, kw.get("connectivity", 26))
        assert len(res.lesions) >= 2 and all(r["confidence"] > case["threshold"] for r in res.lesions)
    assert plain.mask.tobytes() == _predict_case(case, return_lesions=True).mask.tobytes()
    only = _predict_case(case, return_lesions=True)  # the probabilities are used, not returned
    assert only.probability is None and only.lesions == predict.lesion_table(plain.mask, plain.probability, spacing)
    # existing constructions stay valid
    assert predict.CasePrediction(plain.mask, None, plain.reference_path, plain.geometry).lesions is None


def test_score_case_lesions(case):
    _, predict = _mods()
    from pcms_amd.utils.metrics import calculate_dice_score, calculate_iou
    pred = case["predictor"]
    res = _predict_case(case, return_probability=True)
    spacing = tuple(float(v) for v in res.geometry["pixdim"][1:4])[::-1]
    old = pred.score_case(res, case["label"])
    m, lab = _dev(res.mask), _dev(case["label_vol"])
    expect = {"dice": calculate_dice_score(m, lab), "iou": calculate_iou(m, lab)}
    expect.update(predict.surface_metrics_device(m, lab, spacing))
    assert set(old) == OLD_KEYS and old == expect
    assert pred.score_case(res, case["label"], lesion_metrics=False) == old
    new = pred.score_case(res, case["label"], lesion_metrics=True)
    assert set(new) == OLD_KEYS | {"lesions"} and {k: new[k] for k in OLD_KEYS} == old
    exp = predict.lesion_metrics(res.mask, case["label_vol"], res.probability, spacing)
    _same_metrics(new["lesions"], exp)
    assert exp["n_ref"] >= 2 and exp["n_pred"] >= 2
    for connectivity, min_iou in ((6, 0.1), (26, 0.02)):
        got = pred.score_case(res, case["label"], lesion_metrics=True, min_iou=min_iou, connectivity=connectivity)
        _same_metrics(got["lesions"], predict.lesion_metrics(res.mask, case["label_vol"], res.probability, spacing,
                                                             connectivity, min_iou))
    bare = _predict_case(case)  # without probabilities: no confidence
    got = pred.score_case(bare, case["label"], lesion_metrics=True)["lesions"]
    _same_metrics(got, predict.lesion_metrics(bare.mask, case["label_vol"], None, spacing))


def test_evaluate_lesion_metrics():
    """evaluate over two batches of two cases: the default output is unchanged, the lesion entries
    are the sums of the per-case host scores.  The threshold is the 0.9 quantile of the network's
    own probabilities and the labels are sparse, so both sides have several components."""
    _, predict = _mods()
    from pcms_amd.utils.metrics import evaluate
    model = _net(7).eval()
    gen = torch.Generator().manual_seed(3)
    loader = [{"image": torch.rand(2, 5, 16, 16, 16, generator=gen),
               "label": (torch.rand(2, 1, 16, 16, 16, generator=gen) < 0.08).float(), "case_id": [f"a{b}", f"b{b}"]}
              for b in range(2)]
    with torch.no_grad():
        thr = float(torch.quantile(model.predict(loader[0]["image"].cuda()).reshape(-1).float(), 0.9))
    plain = evaluate(model, loader, threshold=thr)
    both = evaluate(model, loader, threshold=thr, lesion_metrics=True, min_iou=0.05, connectivity=6)
    assert set(plain) == {"cases", "mean_dice", "mean_iou"}
    assert set(both) == set(plain) | {"lesion_tp", "lesion_fp", "lesion_fn", "lesion_sensitivity", "lesion_precision",
                                      "lesion_f1", "mean_fp_per_case"}
    assert {k: both[k] for k in ("mean_dice", "mean_iou")} == {k: plain[k] for k in ("mean_dice", "mean_iou")}
    assert [{k: c[k] for k in ("case_id", "dice", "iou")} for c in both["cases"]] == plain["cases"]
    tp = fp = fn = 0
    i = 0
    for batch in loader:
        masks = model.inference(batch["image"].cuda(), threshold=thr).cpu().numpy()
        for k in range(masks.shape[0]):
            m = predict.lesion_metrics(masks[k, 0], batch["label"][k, 0].numpy() != 0, None, (1, 1, 1), 6, 0.05)
            c = both["cases"][i]
            assert (c["lesion_tp"], c["lesion_fp"], c["lesion_fn"]) == (m["tp"], m["fp"], m["fn"])
            assert m["n_pred"] >= 2 and m["n_ref"] >= 2
            tp, fp, fn = tp + m["tp"], fp + m["fp"], fn + m["fn"]
            i += 1
    assert (both["lesion_tp"], both["lesion_fp"], both["lesion_fn"]) == (tp, fp, fn)
    ratio = lambda a, b: a / b if b else float("nan")  # noqa: E731
    for key, v in (("lesion_sensitivity", ratio(tp, tp + fn)), ("lesion_precision", ratio(tp, tp + fp)),
                   ("lesion_f1", ratio(2 * tp, 2 * tp + fp + fn))):
        assert both[key] == v or (math.isnan(v) and math.isnan(both[key])), key
    assert both["mean_fp_per_case"] == fp / 4
