"""The surface-distance metrics through the Python surface, on the GPU: surface_metrics_device
against the host form (order statistics of bit-equal squared distances: hd, hd95 and the counts
exactly; assd from the device's sum of square roots, within the 1e-9 derived for n <= 2^20 terms),
the wrappers in utils.metrics, evaluate / ModelValidator with the flag on and off, and
ModelPredictor.score_case on a synthetic case with an anisotropic grid."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_blocks import _net

pytestmark = pytest.mark.gpu

SHAPE = (24, 40, 48)
SPACINGS = [(3.6, 0.3125, 0.3125), (2.2, 0.7, 0.9)]
GRID = (16, 16, 16)
ASSD_REL = 1e-9


def _mods():
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    from pcms_amd.utils import metrics
    return data, predict, metrics


def _ellipsoid(shape, centre, radii):
    d, h, w = np.indices(shape)
    return ((((d - centre[0]) / radii[0]) ** 2 + ((h - centre[1]) / radii[1]) ** 2
             + ((w - centre[2]) / radii[2]) ** 2) <= 1.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pair(kind):
    if kind == "ellipsoids":
        return _ellipsoid(SHAPE, (11, 18, 22), (7, 12, 15)), _ellipsoid(SHAPE, (13, 22, 27), (6, 13, 12)) * np.uint8(5)
    rng = np.random.default_rng(11)
    return tuple((rng.random(SHAPE) < p).astype(np.uint8) for p in (0.05, 0.3))


@functools.lru_cache(maxsize=None)
def _host(kind, spacing):
    return _mods()[1].surface_metrics(*_pair(kind), spacing)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _agree(got, exp, what):
    assert set(got) == set(exp) == {"hd", "hd95", "assd", "n_a", "n_b"}, what
    print(f"{what}: device {got} host {exp}")
    for key in ("hd", "hd95", "n_a", "n_b"):
        assert got[key] == exp[key], (what, key, got[key], exp[key])
    if math.isfinite(exp["assd"]):
        assert abs(got["assd"] - exp["assd"]) <= ASSD_REL * abs(exp["assd"]), (what, got["assd"], exp["assd"])
    else:
        assert got["assd"] == exp["assd"]


@pytest.mark.parametrize("kind", ["ellipsoids", "bernoulli"])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_device_metrics_equal_host(kind, spacing):
    _, predict, metrics = _mods()
    a, b = _pair(kind)
    exp = _host(kind, spacing)
    assert exp["n_a"] > 0 and exp["n_b"] > 0 and 0.0 < exp["assd"] < exp["hd95"] <= exp["hd"] < math.inf
    got = predict.surface_metrics_device(_cuda(a), _cuda(b), spacing)
    _agree(got, exp, f"{kind} {spacing}")
    assert all(type(got[k]) is float for k in ("hd", "hd95", "assd")) and type(got["n_a"]) is int
    # the wrappers: CUDA tensors on the device, numpy on the host, a channel dimension squeezed
    _agree(metrics.calculate_surface_metrics(_cuda(a)[None].float(), _cuda(b)[None].float(), spacing), exp, "wrapper")
    assert metrics.calculate_surface_metrics(a[None], b[None], spacing) == exp
    assert metrics.calculate_hd95(_cuda(a), _cuda(b), spacing) == exp["hd95"] == metrics.calculate_hd95(a, b, spacing)
    assert metrics.calculate_assd(a, b, spacing) == exp["assd"]
    assert abs(metrics.calculate_assd(_cuda(a), _cuda(b), spacing) - exp["assd"]) <= ASSD_REL * exp["assd"]


def test_device_surface_and_transform_equal_host():
    _, predict, _ = _mods()
    a, _ = _pair("ellipsoids")
    assert np.array_equal(predict.surface_device(_cuda(a)).cpu().numpy(), predict.surface(a))
    feat = predict.surface(a)
    for spacing in SPACINGS:
        sq = predict.distance_transform_device(_cuda(feat), spacing, squared=True)
        assert sq.dtype == torch.float64 and tuple(sq.shape) == SHAPE
        assert np.array_equal(sq.cpu().numpy().view(np.int64), predict.edt_sq(feat, spacing).view(np.int64))
        got = predict.distance_transform_device(_cuda(feat), spacing).cpu().numpy()
        exp = predict.distance_transform(feat, spacing)
        assert np.all(np.abs(got - exp) <= 2.0 ** -52 * exp)  # the device's square root: one ulp at most


def test_empty_rules_and_refusals():
    _, predict, metrics = _mods()
    a, _ = _pair("ellipsoids")
    z = np.zeros(SHAPE, np.uint8)
    both = predict.surface_metrics_device(_cuda(z), _cuda(z), SPACINGS[0])
    assert both == {"hd": 0.0, "hd95": 0.0, "assd": 0.0, "n_a": 0, "n_b": 0} == predict.surface_metrics(z, z)
    for x, y in ((a, z), (z, a)):
        one = predict.surface_metrics_device(_cuda(x), _cuda(y), SPACINGS[0])
        assert one == predict.surface_metrics(x, y, SPACINGS[0])
        assert one["hd"] == one["hd95"] == one["assd"] == math.inf and one["n_a"] + one["n_b"] > 0
    cpu = torch.from_numpy(a)
    for fn in (lambda: predict.surface_metrics_device(cpu, cpu, SPACINGS[0]), lambda: predict.surface_device(cpu),
               lambda: predict.distance_transform_device(cpu, SPACINGS[0]),
               lambda: metrics.calculate_surface_metrics(cpu, cpu), lambda: metrics.calculate_hd95(cpu[None], cpu[None])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    dev = _cuda(a)
    with pytest.raises(ValueError):
        predict.surface_metrics_device(dev, dev[:-1], SPACINGS[0])
    with pytest.raises(ValueError):
        predict.surface_metrics_device(dev, dev, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        predict.distance_transform_device(dev, (1.0, math.nan, 1.0))
    with pytest.raises(TypeError):
        metrics.calculate_surface_metrics(dev, a)


# ---- evaluate / ModelValidator -----------------------------------------------------------------
@pytest.fixture(scope="module")
def loader():
    """Two cases at 16^3 in one batch: the labels are blobs; the threshold that goes with them is
    the median of the network's own probabilities, so its masks are about half foreground."""
    model = _net(7)
    gen = torch.Generator().manual_seed(2)
    x = torch.rand(2, 5, *GRID, generator=gen)
    y = torch.from_numpy(np.stack([_ellipsoid(GRID, (8, 7, 8), (5, 4, 6)), _ellipsoid(GRID, (6, 9, 7), (4, 6, 3))]))
    with torch.no_grad():
        thr = float(model.predict(x.cuda()).median())
    return {"model": model, "batches": [{"image": x, "label": y[:, None].float(), "case_id": ["a", "b"]}],
            "threshold": thr}


def test_evaluate_with_surface_metrics(loader):
    _, predict, metrics = _mods()
    model, batches, thr = loader["model"], loader["batches"], loader["threshold"]
    spacing = (3.0, 0.5, 0.5)
    plain = metrics.evaluate(model, batches, threshold=thr)
    assert set(plain) == {"cases", "mean_dice", "mean_iou"}
    assert all(set(c) == {"case_id", "dice", "iou"} for c in plain["cases"])
    r = metrics.evaluate(model, batches, threshold=thr, surface_metrics=True, spacing=spacing)
    assert set(r) == {"cases", "mean_dice", "mean_iou", "mean_hd95", "mean_assd", "surface_cases"}
    assert all(set(c) == {"case_id", "dice", "iou", "hd95", "assd", "hd"} for c in r["cases"])
    assert [(c["case_id"], c["dice"], c["iou"]) for c in r["cases"]] == \
        [(c["case_id"], c["dice"], c["iou"]) for c in plain["cases"]]
    mask = model.inference(batches[0]["image"].cuda(), threshold=thr).cpu().numpy()
    assert 0.3 < float(mask.mean()) < 0.7
    for i, c in enumerate(r["cases"]):
        exp = predict.surface_metrics(mask[i, 0], batches[0]["label"][i, 0].numpy(), spacing)
        assert math.isfinite(exp["hd"]) and exp["hd"] > 0.0
        assert c["hd"] == exp["hd"] and c["hd95"] == exp["hd95"]
        assert abs(c["assd"] - exp["assd"]) <= ASSD_REL * exp["assd"]
    assert r["surface_cases"] == 2
    assert r["mean_hd95"] == (r["cases"][0]["hd95"] + r["cases"][1]["hd95"]) / 2
    assert r["mean_assd"] == (r["cases"][0]["assd"] + r["cases"][1]["assd"]) / 2
    # a case with an empty label is infinite and stays out of the means
    empty = [dict(batches[0], label=torch.cat([batches[0]["label"][:1], torch.zeros(1, 1, *GRID)]))]
    e = metrics.evaluate(model, empty, threshold=thr, surface_metrics=True, spacing=spacing)
    assert e["cases"][1]["hd95"] == math.inf and e["surface_cases"] == 1
    assert e["mean_hd95"] == r["cases"][0]["hd95"] and e["mean_assd"] == r["cases"][0]["assd"]


def test_validator_json_has_the_new_keys_only_when_asked(loader, tmp_path):
    _, _, metrics = _mods()
    base = {"timestamp", "avg_dice", "avg_iou", "case_count", "case_results"}
    for extra, keys in (({}, base), ({"surface_metrics": False}, base),
                        ({"surface_metrics": True, "spacing": [3.0, 0.5, 0.5]}, base | {"avg_hd95", "avg_assd"})):
        out = tmp_path / f"out{len(extra)}"
        v = metrics.ModelValidator({"device": "cuda", "save_dir": str(out), **extra}, model=loader["model"],
                                   test_loader=loader["batches"])
        v.validate()
        rep = json.loads((out / "validation_results.json").read_text())
        assert set(rep) == keys
        case_keys = {"case_id", "dice", "iou"} | ({"hd95", "assd", "hd"} if extra.get("surface_metrics") else set())
        assert all(set(c) == case_keys for c in rep["case_results"])
    # with the flag on, the averages are evaluate's at the validator's threshold of 0.5
    r = metrics.evaluate(loader["model"], loader["batches"], threshold=0.5, surface_metrics=True, spacing=(3.0, 0.5, 0.5))
    assert rep["case_count"] == 2
    if r["surface_cases"]:
        assert rep["avg_hd95"] == r["mean_hd95"] and rep["avg_assd"] == r["mean_assd"]


# ---- score_case ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Three present modalities on a (12, 20, 18) grid of 0.5 x 0.6 x 3.0 mm (x, y, z), a label on
    that grid, a label on another one, and a seeded checkpoint."""
    data, predict, _ = _mods()
    root = tmp_path_factory.mktemp("score_case")
    rng = np.random.default_rng(33)
    native = (12, 20, 18)
    for i, mod in enumerate(predict.MODALITIES):
        os.makedirs(root / "case" / mod)
        if i in (0, 2, 4):
            data.write_nifti(str(root / "case" / mod / "scan.nii"),
                             rng.integers(0, 3000, size=native).astype(np.int16), spacing=(0.5, 0.6, 3.0))
    label = _ellipsoid(native, (6, 9, 8), (4, 7, 6)) * np.uint8(2)  # binarised with != 0
    data.write_nifti(str(root / "label.nii"), label, spacing=(0.5, 0.6, 3.0))
    data.write_nifti(str(root / "other.nii"), label[:, :-1], spacing=(0.5, 0.6, 3.0))
    ckpt = str(root / "model.pth")
    torch.save(_net().state_dict(), ckpt)
    return {"dir": str(root / "case"), "label": str(root / "label.nii"), "other": str(root / "other.nii"),
            "label_array": label, "predictor": predict.ModelPredictor(ckpt, device="cuda", precision="fp32")}


def test_score_case(case):
    _, predict, _ = _mods()
    pred = case["predictor"]
    prob = pred.predict_case(case["dir"], target_size=GRID, return_probability=True).probability
    res = pred.predict_case(case["dir"], target_size=GRID, threshold=float(np.median(prob)))
    assert 0.3 < float(res.mask.mean()) < 0.7
    pixdim = res.geometry["pixdim"]
    assert tuple(round(float(v), 6) for v in pixdim[1:4]) == (0.5, 0.6, 3.0)
    spacing = (float(pixdim[3]), float(pixdim[2]), float(pixdim[1]))  # (z, y, x), the header's fp32 values
    lab = (case["label_array"] != 0).astype(np.uint8)
    exp = predict.surface_metrics(res.mask, lab, spacing)
    assert math.isfinite(exp["hd"]) and exp["hd"] > 0.0
    got = pred.score_case(res, case["label"])
    assert set(got) == {"dice", "iou", "hd", "hd95", "assd", "n_a", "n_b"}
    _agree({k: got[k] for k in exp}, exp, "score_case")
    inter = float((res.mask.astype(bool) & lab.astype(bool)).sum())
    total = float(res.mask.sum()) + float(lab.sum())
    assert got["dice"] == pytest.approx(2 * inter / (total + 1e-8), rel=1e-6)
    assert got["iou"] == pytest.approx(inter / (total - inter + 1e-8), rel=1e-6)
    # isotropic voxels would give other numbers: the spacing is what the header says
    assert predict.surface_metrics(res.mask, lab)["hd"] != exp["hd"]
    with pytest.raises(ValueError, match="grid"):
        pred.score_case(res, case["other"])
