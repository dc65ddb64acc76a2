"""The percentile intensity window through the public interface on the GPU: ``prepare_case_device``
equals ``predict.prepare_case`` bit for bit, ``predict_case`` (whole grid and ``window=``) follows
from that input, ``normalise=True`` still is the min-max form, and ``assemble_patch_batch`` with
``PatchSampling(normalise="percentile")`` equals the host loader's batch.  The case is the tiny
synthetic one of tests/test_predict_case_gpu.py, rebuilt here with a hot voxel in every modality."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_blocks import _net
from tests.test_patch_host import AUG, PATCH, make_tree

pytestmark = pytest.mark.gpu

TARGET = (16, 16, 16)


def _mods():
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    return data, predict


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Five modalities of different shapes around (12, 20, 18) and different dtypes, one 4-D, one
    missing, each with background zeros and one hot voxel; a seeded checkpoint."""
    data, predict = _mods()
    root = tmp_path_factory.mktemp("intensity_case")
    rng = np.random.default_rng(21)
    vols = [rng.integers(0, 4000, size=(12, 20, 18)).astype(np.int16),
            rng.integers(0, 900, size=(2, 10, 24, 17)).astype(np.uint16),   # 4-D: volume 0
            (500.0 * rng.standard_normal((13, 19, 20))).astype(np.float32),
            None,
            rng.integers(0, 200, size=(11, 21, 16)).astype(np.uint8)]
    for v in vols:
        if v is not None:
            v[rng.random(v.shape) < 0.4] = 0
            v.reshape(-1)[v.size // 3] = 30000 if v.dtype != np.uint8 else 255
    for mod, vol in zip(predict.MODALITIES, vols):
        os.makedirs(root / "case" / mod)
        if vol is not None:
            data.write_nifti(str(root / "case" / mod / "scan.nii"), vol, spacing=(0.5, 0.6, 3.0) + (1.0,) * (vol.ndim - 3))
    ckpt = str(root / "model.pth")
    torch.save(_net().state_dict(), ckpt)
    return {"dir": str(root / "case"), "vols": vols,
            "predictor": predict.ModelPredictor(ckpt, device="cuda", precision="fp32")}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _equal(got, exp):
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(_bits(got), _bits(exp)), f"{int((_bits(got) != _bits(exp)).sum())} of {got.size} differ"


def _forms():
    N = _mods()[1].Normalisation
    return ["percentile", N("percentile", above=0.0), {"method": "percentile", "lower": 2.0, "upper": 90.0}]


@pytest.mark.parametrize("handle_missing", ["zero_fill", "duplicate"])
@pytest.mark.parametrize("form", [0, 1, 2], ids=["name", "above0", "dict"])
def test_prepare_case_device_equals_host(case, handle_missing, form):
    _, predict = _mods()
    normalise = _forms()[form]
    exp = predict.prepare_case(case["dir"], TARGET, handle_missing, normalise)
    got = predict.prepare_case_device(case["dir"], TARGET, handle_missing, normalise, "cuda")
    assert got.shape == (1, 5) + TARGET and got.dtype == torch.float32 and got.is_cuda
    _equal(got[0].cpu().numpy(), exp)
    assert exp.min() >= 0.0 and exp.max() <= 1.0 and float(exp[0].max()) > 0.9
    minmax = predict.prepare_case(case["dir"], TARGET, handle_missing, True)
    # the hot voxel squeezes min-max's tissue, not the window's
    assert float(np.median(minmax[0][minmax[0] > 0])) < 0.1 < 0.25 < float(np.median(exp[0][exp[0] > 0]))


def test_normalise_true_is_still_the_minmax_form(case):
    _, predict = _mods()
    vols = [None if v is None else (v if v.ndim == 3 else v[0]) for v in case["vols"]]
    d = _mods()[0]
    exp = np.stack([np.zeros(TARGET, np.float32) if v is None else d.resample(predict.normalise(v), TARGET)
                    for v in vols])
    for normalise in (True, "minmax", predict.Normalisation()):
        got = predict.prepare_case_device(case["dir"], TARGET, "zero_fill", normalise, "cuda")
        _equal(got[0].cpu().numpy(), exp)
        _equal(predict.prepare_case(case["dir"], TARGET, "zero_fill", normalise), exp)
    with pytest.raises(ValueError):
        predict.prepare_case_device(case["dir"], TARGET, "zero_fill", "zscore", "cuda")


def test_predict_case_equals_the_host_pipeline(case):
    _, predict = _mods()
    pred = case["predictor"]
    norm = predict.Normalisation("percentile", above=0.0)
    x = torch.from_numpy(predict.prepare_case(case["dir"], TARGET, "zero_fill", norm))[None].cuda()
    native = case["vols"][0].shape
    prob = pred.model.predict(x)[0, 0].cpu().numpy()
    exp_mask, exp_prob = predict.mask_on_grid(prob, native)
    res = pred.predict_case(case["dir"], target_size=TARGET, normalise=norm, return_probability=True)
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)
    thr = float(np.median(exp_prob))   # about half the voxels on either side: no constant mask can pass
    exp_half = predict.mask_on_grid(prob, native, thr)[0]
    assert 0.4 < float(exp_half.mean()) < 0.6
    _equal(pred.predict_case(case["dir"], target_size=TARGET, normalise=norm, threshold=thr).mask, exp_half)
    other = pred.predict_case(case["dir"], target_size=TARGET, normalise=True, return_probability=True)
    assert not np.array_equal(other.probability, res.probability)


def test_predict_case_with_a_window_takes_the_setting(case):
    _, predict = _mods()
    pred = case["predictor"]
    norm = predict.Normalisation("percentile", above=0.0)
    grid, window = (16, 32, 32), (16, 16, 16)
    x = predict.prepare_case_device(case["dir"], grid, "zero_fill", norm, "cuda")
    _equal(x[0].cpu().numpy(), predict.prepare_case(case["dir"], grid, "zero_fill", norm))
    with torch.no_grad():
        prob = predict.sliding_window_device(pred.model.predict, x, window, 0.5, "gaussian", (), 4).cpu().numpy()
    exp_mask, exp_prob = predict.mask_on_grid(prob, case["vols"][0].shape)
    res = pred.predict_case(case["dir"], target_size=grid, normalise=norm, return_probability=True, window=window)
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)


# ---------------- the patch loader ----------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp("intensity_patch_tree")))


def _loader(tree, raw, augment, normalise):
    d = _mods()[0]
    ps = d.PatchSampling(patch_size=(16, 16, 16), patches_per_case=3, foreground_prob=0.5, seed=4, normalise=normalise)
    assert PATCH == (16, 16, 16)
    return d.get_dataloader(tree, batch_size=2, shuffle=False, device_resample=raw, augment=augment, augment_seed=9,
                            patches=ps)


@pytest.mark.parametrize("augment", [None, AUG], ids=["identity", "augment"])
@pytest.mark.parametrize("form", ["percentile", {"method": "percentile", "lower": 5.0, "upper": 80.0, "above": 0.0}],
                         ids=["name", "dict"])
def test_device_patch_batches_equal_the_host_loader(tree, augment, form):
    d, predict = _mods()
    host, dev = _loader(tree, False, augment, form), _loader(tree, True, augment, form)
    ref, raw = next(iter(host)), next(iter(dev))
    assert raw["normalise"] == predict.Normalisation.of(form)
    got = d.assemble_batch(raw, None, "cuda")
    assert got["image"].shape == (6, 5) + PATCH and got["case_id"] == ref["case_id"]
    for key in ("image", "label"):
        a, b = got[key].cpu().view(torch.int32), ref[key].view(torch.int32)
        assert torch.equal(a, b), f"{key}: {int((a != b).sum())} of {a.numel()} voxels differ"
    assert torch.equal(got["picks"].cpu(), ref["picks"])
    assert not got["image"][:, 1].any() and got["image"][:, 0].any()   # DWI is zero_fill
    minmax = next(iter(_loader(tree, False, augment, True)))
    assert not torch.equal(minmax["image"], ref["image"])              # the setting is not coerced to min-max
