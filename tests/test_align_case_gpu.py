"""Modality alignment on the device, end to end: ``prepare_case_device(align=...)``
against ``prepare_case``, ``predict_case`` on a case whose modalities have different shapes,
``register_rigid_device`` against ``register_rigid`` on the phantom, and the device loaders
(``assemble_batch`` / ``assemble_patch_batch``) against the host datasets -- all on the bits."""
import numpy as np
import pytest
import torch

from tests.test_align_host import (AUG, CORRECTIONS, MODS, PATCHES, REF_SHAPE, REF_WORLD, bits, coarse_case, make_tree,
                                   phantom, phantom_result, sform_geometry)
from tests.test_gpu_blocks import _net

pytestmark = pytest.mark.gpu


def _mods():
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    return data, predict


@pytest.mark.parametrize("normalise", [True, "percentile", False])
def test_prepare_case_device_world_equals_host(tmp_path, normalise):
    _, predict = _mods()
    root, _ = coarse_case(str(tmp_path / "case"))
    for target, to in ((None, "gaoqing-T2"), ((16, 32, 32), "gaoqing-T2"), ((16, 24, 40), None)):
        align = {"mode": "world", "to": to}
        exp = predict.prepare_case(root, target, normalise=normalise, align=align)
        got, report = predict.prepare_case_device(root, target, normalise=normalise, align=align, return_alignment=True)
        assert tuple(got.shape) == (1,) + exp.shape and got.dtype == torch.float32
        assert np.array_equal(bits(got[0].cpu().numpy()), bits(exp)), (normalise, target, to)
        assert exp[1].any() and set(report) == set(MODS)
    with pytest.raises(ValueError):
        predict.prepare_case_device(root, None, normalise=normalise)            # shapes differ: still an error


def test_predict_case_on_modalities_of_different_shapes(tmp_path):
    data, predict = _mods()
    root, _ = coarse_case(str(tmp_path / "case"))
    ckpt = str(tmp_path / "model.pth")
    torch.save(_net(5).state_dict(), ckpt)
    predictor = predict.ModelPredictor(ckpt, device="cuda", precision="fp32")
    kw = dict(window=(16, 32, 32), target_size=None, normalise=True)
    with pytest.raises(ValueError):
        predictor.predict_case(root, **kw)
    label = str(tmp_path / "label.nii")
    data.write_nifti(label, np.zeros(REF_SHAPE, np.uint8), geometry=sform_geometry(REF_WORLD))
    for extra, reference in ((dict(align={"to": "gaoqing-T2"}), "gaoqing-T2"),
                             (dict(align="world", output_like=label), None)):
        res = predictor.predict_case(root, return_probability=True, **kw, **extra)
        assert res.mask.shape == REF_SHAPE and res.mask.dtype == np.uint8 and res.probability.shape == REF_SHAPE
        assert np.isfinite(res.probability).all() and 0.0 <= res.probability.min() < res.probability.max() <= 1.0
        assert res.reference_path == (label if reference is None else f"{root}/{reference}/img.nii")
        assert set(res.alignment) == set(MODS) and res.alignment["ADC"]["params"] == (0.0,) * 6
    assert predictor.predict_case(root, target_size=(16, 32, 32)).alignment is None


def test_register_rigid_device_equals_host():
    data, predict = _mods()
    fixed, moving, gf, gm = phantom()
    raws = [data.RawVolume(torch.from_numpy(v.reshape(-1).view(np.uint8).copy()), 16, v.shape, 1.0, 0.0).to("cuda")
            for v in (fixed, moving)]
    got = predict.register_rigid_device(raws[0], raws[1], gf, gm)
    print("register_rigid_device:", got)
    assert got == phantom_result()
    with pytest.raises(RuntimeError):
        predict.register_rigid_device(raws[0].to("cpu"), raws[1], gf, gm)


def test_register_case_device_and_dataset(tmp_path):
    data, predict = _mods()
    tree = make_tree(str(tmp_path / "tree"), False, cases=1)
    ds = data.ProstateDataset(tree)
    settings = {"mode": "register", "levels": (((1, 2, 2), (1.0,)),)}          # a short search: this is plumbing
    files = ds.case_list[0]["modality_files"]
    got = predict.register_case_device(files, align=settings)
    assert set(got) == set(MODS) - {"ADC"}                                      # ADC, the first present, is fixed
    assert got == predict.register_case(files, align=settings)
    table = predict.register_dataset(ds, "cuda", align=settings)
    assert table == {"p0": {m: list(r["params"]) for m, r in got.items()}}
    import json
    assert json.loads(json.dumps(table)) == table


def _collated(data, tree, kw, device_resample):
    ds = data.ProstateDataset(tree, target_size=(16, 32, 32), device_resample=device_resample, align="world",
                              corrections=CORRECTIONS, **kw)
    samples = [ds[i] for i in range(len(ds))]
    if device_resample:
        return data.assemble_batch(data._CollateRaw((16, 32, 32), kw.get("patches"))(samples), device="cuda")
    if "patches" in kw:
        return data._collate_patches(samples)
    return {"image": torch.stack([s["image"] for s in samples]), "label": torch.stack([s["label"] for s in samples])}


@pytest.fixture(scope="module")
def coarse_tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp("align_coarse_gpu")), False)


@pytest.mark.parametrize("kind", ["plain", "augment", "patches", "patches_augment"])
def test_device_loaders_equal_the_host_datasets(coarse_tree, kind):
    data, _ = _mods()
    kw = {"plain": {}, "augment": dict(augment=AUG, augment_seed=3), "patches": dict(patches=PATCHES),
          "patches_augment": dict(patches=PATCHES, augment=AUG, augment_seed=3)}[kind]
    host, dev = _collated(data, coarse_tree, kw, False), _collated(data, coarse_tree, kw, True)
    for key in ("image", "label") + (("picks",) if "patches" in kw else ()):
        got, exp = dev[key].cpu(), host[key]
        assert got.shape == exp.shape and got.dtype == exp.dtype, (kind, key)
        assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (kind, key)
    assert host["image"].abs().sum() > 0 and host["label"].sum() > 0
    unaligned = data.ProstateDataset(coarse_tree, target_size=(16, 32, 32), **kw)[0]["image"]
    assert not torch.equal(unaligned, host["image"][:unaligned.shape[0]] if "patches" in kw else host["image"][0])
