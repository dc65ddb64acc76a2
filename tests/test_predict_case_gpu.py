"""ModelPredictor.predict_case end to end on the GPU, in three exact links: the device input
equals predict.prepare_case; the mask and probabilities equal predict.mask_on_grid (through
predict.tta_mean with flips) of the network's own output on that input; save_case writes those
voxels with the reference file's geometry."""
import os
import struct

import numpy as np
import pytest
import torch

from tests.test_gpu_blocks import _net

pytestmark = pytest.mark.gpu

TARGET = (16, 16, 16)
FLIPS = ((2,), (1, 2))


def _mods():
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    return data, predict


def _set_geometry(path, seed):
    """A non-trivial qform / sform written into the header of ``path``."""
    rng = np.random.default_rng(seed)
    with open(path, "r+b") as f:
        raw = bytearray(f.read(352))
        struct.pack_into("<f", raw, 76, -1.0)  # qfac
        raw[123] = 10
        struct.pack_into("<hh", raw, 252, 1, 1)
        struct.pack_into("<6f", raw, 256, *rng.uniform(-0.5, 0.5, 3), *rng.uniform(-150, 150, 3))
        struct.pack_into("<12f", raw, 280, *rng.uniform(-3, 3, 12))
        f.seek(0)
        f.write(raw)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Five modalities of different shapes around (12, 20, 18) and different dtypes, one 4-D, one
    missing; a label of yet another shape; a seeded checkpoint."""
    data, predict = _mods()
    root = tmp_path_factory.mktemp("predict_case")
    rng = np.random.default_rng(21)
    vols = [rng.integers(0, 4000, size=(12, 20, 18)).astype(np.int16),
            rng.integers(0, 900, size=(2, 10, 24, 17)).astype(np.uint16),   # 4-D: volume 0
            (500.0 * rng.standard_normal((13, 19, 20))).astype(np.float32),
            None,
            rng.integers(0, 256, size=(11, 21, 16)).astype(np.uint8)]
    spacings = [(0.5, 0.6, 3.0), (1.5, 1.4, 3.5, 1.0), (0.7, 0.7, 2.5), None, (0.9, 0.8, 3.2)]
    for i, (mod, vol) in enumerate(zip(predict.MODALITIES, vols)):
        os.makedirs(root / "case" / mod)
        if vol is not None:
            p = str(root / "case" / mod / "scan.nii")
            data.write_nifti(p, vol, spacing=spacings[i])
            _set_geometry(p, 30 + i)
    label = str(root / "label.nii")
    data.write_nifti(label, (rng.random((9, 22, 15)) > 0.7).astype(np.uint8), spacing=(0.8, 0.75, 4.0))
    _set_geometry(label, 40)
    ckpt = str(root / "model.pth")
    torch.save(_net().state_dict(), ckpt)
    return {"dir": str(root / "case"), "vols": vols, "label": label,
            "first": str(root / "case" / predict.MODALITIES[0] / "scan.nii"),
            "predictor": predict.ModelPredictor(ckpt, device="cuda", precision="fp32"), "root": root}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _equal(got, exp):
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(_bits(got), _bits(exp)), f"{int((_bits(got) != _bits(exp)).sum())} of {got.size} differ"


@pytest.mark.parametrize("handle_missing", ["zero_fill", "duplicate"])
@pytest.mark.parametrize("normalise", [True, False])
def test_prepare_case_device_equals_host(case, handle_missing, normalise):
    _, predict = _mods()
    exp = predict.prepare_case(case["dir"], TARGET, handle_missing, normalise)
    got = predict.prepare_case_device(case["dir"], TARGET, handle_missing, normalise, "cuda")
    assert got.shape == (1, 5) + TARGET and got.dtype == torch.float32 and got.is_cuda
    _equal(got[0].cpu().numpy(), exp)
    assert float(exp[3].max()) == (0.0 if handle_missing == "zero_fill" else float(exp[0].max()))
    with pytest.raises(FileNotFoundError):
        predict.prepare_case_device(case["dir"], TARGET, "skip", normalise, "cuda")
    with pytest.raises(ValueError):
        predict.prepare_case_device(case["dir"], None, handle_missing, normalise, "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict.prepare_case_device(case["dir"], TARGET, handle_missing, normalise, "cpu")


def _forward(case, x, flips=()):
    """The network's probabilities on x and on its flipped copies, one batch as predict_case runs
    it: (k, D, H, W) numpy."""
    batch = torch.cat([x] + [torch.flip(x, dims=[2 + a for a in f]) for f in flips], dim=0)
    return case["predictor"].model.predict(batch)[:, 0].cpu().numpy()


def test_predict_case_equals_host_forms(case):
    _, predict = _mods()
    pred = case["predictor"]
    x = predict.prepare_case_device(case["dir"], TARGET, "zero_fill", True, "cuda")
    native = case["vols"][0].shape
    exp_mask, exp_prob = predict.mask_on_grid(_forward(case, x)[0], native)
    res = pred.predict_case(case["dir"], target_size=TARGET, return_probability=True)
    assert res.reference_path == case["first"] and res.mask.dtype == np.uint8
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)
    assert pred.predict_case(case["dir"], target_size=TARGET).probability is None
    # the median of the probabilities as the threshold: about half the voxels on either side, so
    # a constant mask cannot pass
    thr = float(np.median(exp_prob))
    exp_half = predict.mask_on_grid(_forward(case, x)[0], native, thr)[0]
    assert 0.4 < float(exp_half.mean()) < 0.6
    _equal(pred.predict_case(case["dir"], target_size=TARGET, threshold=thr).mask, exp_half)


def test_predict_case_with_flips(case):
    _, predict = _mods()
    x = predict.prepare_case_device(case["dir"], TARGET, "zero_fill", True, "cuda")
    probs = _forward(case, x, FLIPS)
    mean = predict.tta_mean(list(probs), [()] + list(FLIPS))
    assert not np.array_equal(mean, probs[0])
    exp_mask, exp_prob = predict.mask_on_grid(mean, case["vols"][0].shape)
    res = case["predictor"].predict_case(case["dir"], target_size=TARGET, tta_flips=FLIPS, return_probability=True)
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)
    with pytest.raises(ValueError):
        case["predictor"].predict_case(case["dir"], target_size=TARGET, tta_flips=((3,),))


def test_output_like_selects_the_grid_and_save_case(case):
    data, predict = _mods()
    pred = case["predictor"]
    x = predict.prepare_case_device(case["dir"], TARGET, "zero_fill", True, "cuda")
    prob = _forward(case, x)[0]
    for ref, shape in ((None, (12, 20, 18)), (case["label"], (9, 22, 15))):
        res = pred.predict_case(case["dir"], target_size=TARGET, output_like=ref)
        ref = ref or case["first"]
        assert res.reference_path == ref and res.mask.shape == shape
        _equal(res.mask, predict.mask_on_grid(prob, shape)[0])
        assert res.geometry == data.read_nifti_geometry(ref)
        out = str(case["root"] / f"mask_{shape[0]}.nii")
        pred.save_case(res, out)
        assert np.array_equal(data.read_nifti(out), res.mask) and data.read_nifti(out).dtype == np.uint8
        assert data.read_nifti_geometry(out) == data.read_nifti_geometry(ref)
        assert open(out, "rb").read()[252:328] == open(ref, "rb").read()[252:328]
    res.mask = res.mask[:-1]
    with pytest.raises(ValueError):
        pred.save_case(res, str(case["root"] / "bad.nii"))


def test_normalise_false_feeds_the_loaders_tensor(case):
    """normalise=False: the network input is the tensor data.assemble_batch forms for the same
    files, and the mask follows from it."""
    data, predict = _mods()
    raws = [None if v is None else data.read_nifti_raw(os.path.join(case["dir"], m, "scan.nii"))
            for m, v in zip(predict.MODALITIES, case["vols"])]
    batch = data.assemble_batch({"raw_images": [raws], "raw_label": [data.read_nifti_raw(case["label"])],
                                 "case_id": ["c"], "target_size": TARGET}, device="cuda")
    x = predict.prepare_case_device(case["dir"], TARGET, "zero_fill", False, "cuda")
    assert torch.equal(x.view(torch.int32), batch["image"].view(torch.int32))
    res = case["predictor"].predict_case(case["dir"], target_size=TARGET, normalise=False, return_probability=True)
    exp_mask, exp_prob = predict.mask_on_grid(_forward(case, batch["image"])[0], case["vols"][0].shape)
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)
