"""ModelPredictor.predict_case(window=...) end to end on the GPU, in exact links: every batch the
network is given has window_batch * k entries and equals predict.gather_windows of
predict.prepare_case's volume (the tail padded with the last window); the mask and probabilities
equal predict.mask_on_grid of predict.blend_windows of the network's own recorded outputs; and
window=None still is the whole-volume path.  The recorded inputs and outputs are compared rather
than a second run of the network, whose plans may differ with the batch size."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_blocks import _net
from tests.test_predict_case_gpu import _bits, _equal, _forward, _mods, _set_geometry  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE = (24, 40, 48)
RESAMPLED = (20, 36, 40)
WINDOW = (16, 32, 32)
FLIPS = ((2,),)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Five modalities of one shape and different dtypes (target_size=None is legal), a seeded
    checkpoint at fp32."""
    data, predict = _mods()
    root = tmp_path_factory.mktemp("window_case")
    rng = np.random.default_rng(23)
    vols = [rng.integers(0, 4000, size=SHAPE).astype(np.int16),
            rng.integers(0, 900, size=SHAPE).astype(np.uint16),
            (500.0 * rng.standard_normal(SHAPE)).astype(np.float32),
            rng.integers(-200, 200, size=SHAPE).astype(np.int16),
            rng.integers(0, 256, size=SHAPE).astype(np.uint8)]
    for i, (mod, vol) in enumerate(zip(predict.MODALITIES, vols)):
        os.makedirs(root / "case" / mod)
        p = str(root / "case" / mod / "scan.nii")
        data.write_nifti(p, vol, spacing=(0.5, 0.6, 3.0))
        _set_geometry(p, 50 + i)
    ckpt = str(root / "model.pth")
    torch.save(_net().state_dict(), ckpt)
    return {"dir": str(root / "case"), "vols": vols,
            "predictor": predict.ModelPredictor(ckpt, device="cuda", precision="fp32")}


class _Recorder:
    """model.predict, keeping a host copy of every batch it is given and of every output."""

    def __init__(self, model):
        self.fn, self.inputs, self.outputs = model.predict, [], []

    def __call__(self, batch):
        self.inputs.append(batch.detach().cpu().numpy().copy())
        out = self.fn(batch)
        self.outputs.append(out.detach().float().cpu().numpy().copy())
        return out


def _windowed(case, monkeypatch, target, window_batch, **kw):
    """(result, recorder) of predict_case with the sliding window."""
    pred = case["predictor"]
    rec = _Recorder(pred.model)
    monkeypatch.setattr(pred.model, "predict", rec)
    res = pred.predict_case(case["dir"], target_size=target, tta_flips=FLIPS, return_probability=True, window=WINDOW,
                            overlap=0.5, window_batch=window_batch, **kw)
    monkeypatch.undo()
    return res, rec


def _expected_from_records(case, rec, target, window_batch):
    """The checks on the recorded batches, and mask_on_grid of the host blend of the recorded
    outputs."""
    _, predict = _mods()
    x = predict.prepare_case(case["dir"], target)
    grid = x.shape[1:]
    starts = predict.window_grid(grid, WINDOW, 0.5)
    K, k = len(starts), 1 + len(FLIPS)
    assert K == 8
    tiles = predict.gather_windows(x, starts, WINDOW, FLIPS)
    assert len(rec.inputs) == len(rec.outputs) == -(-K // window_batch)
    kept = []
    for b, (inp, out) in enumerate(zip(rec.inputs, rec.outputs)):
        first = b * window_batch
        real = min(window_batch, K - first)
        assert inp.shape == (window_batch * k, 5) + WINDOW and out.shape == (window_batch * k, 1) + WINDOW
        exp = np.concatenate([tiles[first * k:(first + real) * k]] + [tiles[(K - 1) * k:]] * (window_batch - real))
        _equal(inp, exp)
        kept.append(out[:real * k, 0])
    prob = predict.blend_windows(np.concatenate(kept), starts, WINDOW, predict.window_weights(WINDOW), grid, FLIPS)
    return predict.mask_on_grid(prob, SHAPE)


@pytest.mark.parametrize("target", [None, RESAMPLED], ids=["native", "resampled"])
def test_windowed_predict_case_equals_host_forms(case, monkeypatch, target):
    res, rec = _windowed(case, monkeypatch, target, 2)
    exp_mask, exp_prob = _expected_from_records(case, rec, target, 2)
    assert res.mask.shape == SHAPE and res.mask.dtype == np.uint8
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)
    assert float(np.ptp(exp_prob)) > 1e-3  # no constant volume can pass


def test_tail_batch_is_padded_and_dropped(case, monkeypatch):
    """window_batch = 3 over 8 windows: the last batch holds two windows and a repeat of the last
    one; its output is not blended."""
    res, rec = _windowed(case, monkeypatch, None, 3)
    exp_mask, exp_prob = _expected_from_records(case, rec, None, 3)
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)


def test_window_none_is_the_whole_volume_path(case, monkeypatch):
    _, predict = _mods()
    pred = case["predictor"]
    x = predict.prepare_case_device(case["dir"], None, "zero_fill", True, "cuda")
    exp_mask, exp_prob = predict.mask_on_grid(_forward(case, x)[0], SHAPE)
    rec = _Recorder(pred.model)
    monkeypatch.setattr(pred.model, "predict", rec)
    res = pred.predict_case(case["dir"], target_size=None, return_probability=True, window=None)
    monkeypatch.undo()
    assert [i.shape for i in rec.inputs] == [(1, 5) + SHAPE]
    _equal(res.probability, exp_prob)
    _equal(res.mask, exp_mask)


def test_window_with_postprocessing_and_lesions(case, monkeypatch):
    _, predict = _mods()
    plain, _ = _windowed(case, monkeypatch, None, 2)
    thr = float(np.quantile(plain.probability, 0.9))  # about a tenth of the voxels: several components
    res, _ = _windowed(case, monkeypatch, None, 2, threshold=thr, keep_largest=1, return_lesions=True)
    _equal(res.probability, plain.probability)
    raw = (plain.probability > np.float32(thr)).astype(np.uint8)
    _equal(res.mask, predict.postprocess(raw, keep_largest=1))
    assert 0 < int(res.mask.sum()) < int(raw.sum())
    spacing = tuple(float(v) for v in res.geometry["pixdim"][1:4])[::-1]
    assert res.lesions == predict.lesion_table(res.mask, res.probability, spacing) and len(res.lesions) == 1


def test_window_arguments_are_checked(case):
    pred = case["predictor"]
    for kw in (dict(window=(8, 32, 32)), dict(window=(16, 32)), dict(window=WINDOW, overlap=1.0),
               dict(window=WINDOW, overlap=-0.5), dict(window=WINDOW, blend="linear"),
               dict(window=WINDOW, window_batch=0)):
        with pytest.raises(ValueError):
            pred.predict_case(case["dir"], target_size=None, **kw)
