"""ModelPredictor.predict_case with mask post-processing, end to end on the GPU: the defaults
change nothing; with the options the mask equals predict.postprocess of the default call's mask;
the device forms equal the host forms on that mask and refuse CPU tensors."""
import numpy as np
import pytest
import torch

from tests.test_gpu_blocks import _net
from tests.test_predict_case_gpu import TARGET, _equal, _forward, _mods, case  # noqa: F401  (case: a fixture)

pytestmark = pytest.mark.gpu

# test_gpu_blocks._net's seed for the checkpoint here.  At the median threshold its mask has nine
# 26-connected components (2126, 9, 6, 5 voxels and specks); seed 4, the other test's, gives one.
WEIGHT_SEED = 8


@pytest.fixture(scope="module")
def half_mask(case):  # noqa: F811
    """(predictor, threshold, the default call's mask at the median probability: about half the
    voxels set)."""
    _, predict = _mods()
    ckpt = str(case["root"] / f"model_seed{WEIGHT_SEED}.pth")
    torch.save(_net(WEIGHT_SEED).state_dict(), ckpt)
    pred = predict.ModelPredictor(ckpt, device="cuda", precision="fp32")
    prob = pred.predict_case(case["dir"], target_size=TARGET, return_probability=True).probability
    thr = float(np.median(prob))
    mask = pred.predict_case(case["dir"], target_size=TARGET, threshold=thr).mask
    assert 0.4 < float(mask.mean()) < 0.6
    return pred, thr, mask


def test_defaults_change_nothing(case, half_mask):  # noqa: F811
    _, predict = _mods()
    pred, thr, mask = half_mask
    x = predict.prepare_case_device(case["dir"], TARGET, "zero_fill", True, "cuda")
    prob = pred.model.predict(x)[0, 0].cpu().numpy()
    _equal(mask, predict.mask_on_grid(prob, case["vols"][0].shape, thr)[0])  # what it returned before
    same = pred.predict_case(case["dir"], target_size=TARGET, threshold=thr, keep_largest=0, min_voxels=0,
                             fill_holes=False, connectivity=26)
    _equal(same.mask, mask)
    _equal(pred.predict_case(case["dir"], target_size=TARGET, threshold=thr, min_voxels=1, connectivity=6).mask, mask)
    with pytest.raises(TypeError):  # keyword-only
        pred.predict_case(case["dir"], TARGET, "zero_fill", True, thr, (), None, False, 1)
    with pytest.raises(ValueError):
        pred.predict_case(case["dir"], target_size=TARGET, keep_largest=9)
    with pytest.raises(ValueError):
        pred.predict_case(case["dir"], target_size=TARGET, connectivity=8)


def test_postprocessed_case_equals_host(case, half_mask):  # noqa: F811
    _, predict = _mods()
    pred, thr, mask = half_mask
    labels = predict.label_components(mask, 26)
    assert len(np.unique(labels[labels > 0])) >= 2, "the default mask needs at least two components"
    exp = predict.postprocess(mask, keep_largest=1, min_voxels=4, fill_holes=True)
    assert not np.array_equal(exp, mask)
    res = pred.predict_case(case["dir"], target_size=TARGET, threshold=thr, keep_largest=1, min_voxels=4,
                            fill_holes=True, return_probability=True)
    _equal(res.mask, exp)
    assert res.probability is not None and res.mask.flags["C_CONTIGUOUS"]
    for kw in ({"keep_largest": 2, "connectivity": 6}, {"min_voxels": 3, "connectivity": 18}, {"fill_holes": True}):
        _equal(pred.predict_case(case["dir"], target_size=TARGET, threshold=thr, **kw).mask,
               predict.postprocess(mask, **kw))


def test_device_forms(half_mask):
    _, predict = _mods()
    _, _, mask = half_mask
    dev = torch.from_numpy(mask).cuda()
    for connectivity in (6, 18, 26):
        for invert in (False, True):
            got = predict.label_components_device(dev, connectivity, invert)
            assert got.dtype == torch.int32 and got.is_cuda
            _equal(got.cpu().numpy(), predict.label_components((mask == 0) if invert else mask, connectivity))
        got = predict.postprocess_device(dev, keep_largest=2, min_voxels=2, fill_holes=True, connectivity=connectivity)
        assert got.dtype == torch.uint8 and got.is_cuda and got.data_ptr() != dev.data_ptr()
        _equal(got.cpu().numpy(), predict.postprocess(mask, 2, 2, True, connectivity))
    _equal(predict.postprocess_device(dev).cpu().numpy(), mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict.postprocess_device(torch.from_numpy(mask), keep_largest=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict.label_components_device(torch.from_numpy(mask))
    with pytest.raises(ValueError):
        predict.postprocess_device(dev.to(torch.int32), keep_largest=1)
    with pytest.raises(ValueError):
        predict.postprocess_device(dev, keep_largest=-1)
