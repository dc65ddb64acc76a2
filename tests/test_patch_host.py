"""Patch training, the host forms (no GPU): ``data.draw_patches`` / ``pick_origins`` /
``resample_patch`` / ``PatchSampling`` and the host loader with ``patches``.  ``resample_patch``
is defined as a slice of whole-grid ``resample_affine`` and is compared with it on the bits;
``pick_origins`` is compared with a brute-force ``np.flatnonzero``."""
import os

import numpy as np
import pytest
import torch

MODS = ["ADC", "DWI", "gaoqing-T2", "T2 fs", "T2 not fs"]   # the synthetic tree has no DWI file: zero_fill
LABEL_SHAPE = (12, 40, 48)
PATCH = (16, 16, 16)


def _data():
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    return data


def make_tree(root, cases=2):
    """``cases`` cases: the label at (12, 40, 48) with a blob at the volume centre, ADC (int16) at
    half that shape, gaoqing-T2 (float32) at the label's shape, T2 fs (uint8) at an odd shape, T2
    not fs (int16) at twice the label's, no DWI."""
    d = _data()
    rng = np.random.default_rng(11)
    lab_dir = os.path.join(root, "BPH-PCA", "ROI(BPH+PCA)", "BPH")
    os.makedirs(lab_dir)
    for m in MODS:
        os.makedirs(os.path.join(root, "BPH-PCA", "BPH", m))
    half = tuple(s // 2 for s in LABEL_SHAPE)
    for ci in range(cases):
        cid = f"p{ci}"
        d.write_nifti(os.path.join(root, "BPH-PCA", "BPH", "ADC", cid + ".nii"),
                      rng.integers(-200, 3000, size=half).astype(np.int16))
        d.write_nifti(os.path.join(root, "BPH-PCA", "BPH", "gaoqing-T2", cid + ".nii"),
                      (500.0 * rng.standard_normal(LABEL_SHAPE)).astype(np.float32))
        d.write_nifti(os.path.join(root, "BPH-PCA", "BPH", "T2 fs", cid + ".nii"),
                      rng.integers(0, 256, size=(10, 37, 50)).astype(np.uint8))
        d.write_nifti(os.path.join(root, "BPH-PCA", "BPH", "T2 not fs", cid + ".nii"),
                      rng.integers(-200, 3000, size=tuple(2 * s for s in LABEL_SHAPE)).astype(np.int16))
        lab = np.zeros(LABEL_SHAPE, np.uint8)
        lab[4:8, 16 + ci:24 + ci, 20:28] = 1 + ci
        d.write_nifti(os.path.join(lab_dir, cid + ".nii"), lab)
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp("patch_tree")))


AUG = dict(flip_prob=(0.5, 0.5, 0.5), rotate_deg=(10.0, 5.0, 5.0), zoom=(0.9, 1.1), shift_frac=(0.1, 0.1, 0.1),
           gain=(0.9, 1.1), bias=(-5.0, 5.0))


# ---------------- draws ----------------
def test_draw_patches_is_a_function_of_seed_epoch_and_case():
    d = _data()
    ps = d.PatchSampling(patch_size=PATCH, patches_per_case=5, foreground_prob=0.5, grid=LABEL_SHAPE)
    a = d.draw_patches(ps, 3, 1, 7)
    b = d.draw_patches(dict(patch_size=PATCH, patches_per_case=5, foreground_prob=0.5, grid=LABEL_SHAPE), 3, 1, 7)
    assert a[0].dtype == np.float64 and a[0].shape == (5,) and a[1].dtype == np.int32 and a[1].shape == (5, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for other in ((4, 1, 7), (3, 2, 7), (3, 1, 8)):
        c = d.draw_patches(ps, *other)
        assert not (np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])), other
    # the stream itself: five draws per patch, in order
    rng = np.random.default_rng([3, 1, 7, 1])
    for i in range(5):
        u = [rng.random() for _ in range(5)]
        assert a[0][i] == (u[1] if u[0] < 0.5 else -1.0)
        top = [max(g - w, 0) + 1 for g, w in zip(LABEL_SHAPE, PATCH)]
        assert a[1][i].tolist() == [int(np.floor(u[2 + k] * top[k])) for k in range(3)]
    # the grid smaller than the patch on D: that origin is always 0; the grid given aside
    assert (a[1][:, 0] == 0).all() and (a[1] >= 0).all()
    assert (a[1] <= np.array([0, 24, 32])).all()
    e = d.draw_patches(d.PatchSampling(patch_size=PATCH, patches_per_case=5), 3, 1, 7, grid=LABEL_SHAPE)
    assert np.array_equal(a[0], e[0]) and np.array_equal(a[1], e[1])
    with pytest.raises(ValueError):
        d.draw_patches(d.PatchSampling(patch_size=PATCH), 3, 1, 7)
    all_fg = d.draw_patches(dict(patch_size=PATCH, patches_per_case=8, foreground_prob=1.0, grid=LABEL_SHAPE), 0, 0, 0)
    none_fg = d.draw_patches(dict(patch_size=PATCH, patches_per_case=8, foreground_prob=0.0, grid=LABEL_SHAPE), 0, 0, 0)
    assert (all_fg[0] >= 0).all() and (all_fg[0] < 1).all() and (none_fg[0] == -1.0).all()
    assert np.array_equal(all_fg[1], none_fg[1])


def test_draw_transform_is_not_moved_by_the_patch_draws():
    d = _data()
    before = d.draw_transform(AUG, 5, 2, 3)
    d.draw_patches(dict(patch_size=PATCH, grid=LABEL_SHAPE), 5, 2, 3)
    after = d.draw_transform(AUG, 5, 2, 3)
    assert np.array_equal(before.L, after.L) and np.array_equal(before.shift_frac, after.shift_frac)
    assert before.gain == after.gain and before.bias == after.bias
    # pinned: the first draws of the stream [5, 2, 3] are the transform's, whatever draw_patches took
    rng = np.random.default_rng([5, 2, 3])
    flips = [rng.random() < 0.5 for _ in range(3)]
    angles = [m * (2.0 * rng.random() - 1.0) for m in AUG["rotate_deg"]]
    zoom = 0.9 + (1.1 - 0.9) * rng.random()
    assert np.array_equal(after.L, d.compose_transform(flips, angles, zoom))


# ---------------- pick ----------------
def _brute(label, patch, rank_u, fallback):
    G = label.shape
    fg = np.flatnonzero(label.reshape(-1) > 0)
    T = len(fg)
    out = []
    for u, fb in zip(rank_u, fallback):
        if u >= 0 and T > 0:
            r = min(T - 1, int(np.floor(np.float64(u) * np.float64(T))))
            flat = int(fg[r])
            v = (flat // (G[1] * G[2]), (flat // G[2]) % G[1], flat % G[2])
            out.append([min(max(v[a] - patch[a] // 2, 0), max(G[a] - patch[a], 0)) for a in range(3)])
        else:
            out.append([int(x) for x in fb])
    return np.array(out, np.int32), T


def _labels(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[2])
    n = int(np.prod(shape))
    one = np.zeros(n, np.float32)
    one[n // 3] = 1.0
    corners = np.zeros(shape, np.float32)
    for dd in (0, shape[0] - 1):
        for hh in (0, shape[1] - 1):
            for ww in (0, shape[2] - 1):
                corners[dd, hh, ww] = 2.0
    return {"none": np.zeros(shape, np.float32), "one": one.reshape(shape), "all": np.ones(shape, np.float32),
            "corners": corners, "sparse": (rng.random(shape) < 0.05).astype(np.float32),
            "signed": rng.integers(-2, 3, size=shape).astype(np.float32)}


@pytest.mark.parametrize("shape,patch", [((5, 7, 11), (4, 4, 4)), ((12, 40, 48), (16, 16, 16)),
                                         ((9, 33, 20), (16, 32, 16)), ((20, 20, 36), (16, 16, 32))])
def test_pick_origins_matches_brute_force(shape, patch):
    d = _data()
    last = np.nextafter(1.0, 0.0)
    for name, lab in _labels(shape).items():
        T = int((lab > 0).sum())
        ranks = [0.0, last, 0.5, -1.0, 0.25, -1.0]
        if T > 1:  # every rank of a small set, as (r + 0.5) / T
            ranks += [(r + 0.5) / T for r in range(min(T, 8))]
        rng = np.random.default_rng(T)
        fallback = np.stack([rng.integers(0, max(g - w, 0) + 1, size=len(ranks)) for g, w in zip(shape, patch)], 1)
        got, count = d.pick_origins(lab, patch, np.array(ranks), fallback.astype(np.int32))
        exp, T2 = _brute(lab, patch, ranks, fallback)
        assert count == T == T2, name
        assert got.dtype == np.int32 and np.array_equal(got, exp), (name, got.tolist(), exp.tolist())
        assert (got >= 0).all() and (got <= np.array([max(g - w, 0) for g, w in zip(shape, patch)])).all()
        if T > 0:  # a foreground patch contains its voxel: its label patch is not empty
            from pcms_amd.predict import gather_windows
            wins = gather_windows(lab[None], got, patch)
            for i, u in enumerate(ranks):
                if u >= 0:
                    assert (wins[i] > 0).any(), (name, i)


def test_pick_origins_hits_both_clamps_at_the_corners():
    d = _data()
    shape, patch = (12, 40, 48), (16, 16, 16)
    lab = _labels(shape)["corners"]
    T = 8
    got, count = d.pick_origins(lab, patch, [(r + 0.5) / T for r in range(T)], np.zeros((T, 3), np.int32))
    assert count == T
    # D is thinner than the patch: always 0; H and W: 0 at the low corner, G - w at the high one
    assert sorted(map(tuple, got.tolist())) == sorted((0, h, w) for h in (0, 24) for w in (0, 32) for _ in range(2))


def test_pick_origins_defines_the_untrusted_cases():
    d = _data()
    lab = _labels((12, 40, 48))["sparse"]
    last = np.nextafter(1.0, 0.0)
    a, _ = d.pick_origins(lab, PATCH, [float("nan"), 2.0, 1.0, -0.5], [[5, 99, -3]] * 4)
    b, _ = d.pick_origins(lab, PATCH, [last, last, last, -1.0], [[0, 24, 0]] * 4)
    assert np.array_equal(a, b)


# ---------------- resample_patch ----------------
def _transforms(d, n_in, grid):
    ident = d.volume_affine(np.eye(3), np.zeros(3), n_in, grid)
    L = d.compose_transform((True, False, True), (8.0, -5.0, 12.0), 1.15)
    bent = d.volume_affine(L, np.array([0.7, -2.2, 1.4]), n_in, grid)
    return {"identity": ident, "flip_rot_zoom": bent}


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalise"])
@pytest.mark.parametrize("which", ["identity", "flip_rot_zoom"])
def test_resample_patch_is_the_zero_padded_slice_of_the_whole_grid(which, normalise):
    d = _data()
    from pcms_amd.predict import normalise as norm
    src = (1000.0 * np.random.default_rng(3).standard_normal((11, 29, 23))).astype(np.float32)
    grid, patch = (12, 40, 40), (16, 16, 16)
    A, t = _transforms(d, src.shape, grid)[which]
    for gain, bias in ((1.0, 0.0), (1.25, -3.5)):
        whole = d.resample_affine(norm(src) if normalise else src, grid, A, t, gain=gain, bias=bias)
        assert np.count_nonzero(whole) > whole.size // 2
        pad = np.zeros(tuple(g + 2 * 20 for g in grid), np.float32)
        pad[20:20 + grid[0], 20:20 + grid[1], 20:20 + grid[2]] = whole
        # at 0, in the interior, at G - w, and sticking out below and above the grid
        for origin in ((0, 0, 0), (0, 7, 13), (0, 24, 24), (-4, 24, 24), (-3, -5, 30), (5, 33, -9), (-20, 0, 0)):
            got = d.resample_patch(src, grid, A, t, origin, patch, gain=gain, bias=bias, normalise=normalise)
            exp = pad[tuple(slice(20 + o, 20 + o + w) for o, w in zip(origin, patch))]
            assert got.dtype == np.float32 and got.shape == patch
            assert np.array_equal(got.view(np.int32), exp.view(np.int32)), (which, normalise, gain, origin)
        got = d.resample_patch(src, grid, A, t, (0, 7, 13), (16, 16, 18), gain=gain, bias=bias, normalise=normalise)
        assert np.array_equal(got.view(np.int32), pad[20:36, 27:43, 33:51].view(np.int32))


# ---------------- the loader ----------------
def _loader(tree, raw=False, **kw):
    d = _data()
    ps = dict(patch_size=PATCH, patches_per_case=3, foreground_prob=1.0, seed=4)
    ps.update(kw.pop("patches", {}))
    return d.get_dataloader(tree, batch_size=2, shuffle=False, modalities=MODS, device_resample=raw, patches=ps, **kw)


@pytest.mark.parametrize("augment", [None, AUG], ids=["plain", "augment"])
def test_host_loader_batches(tree, augment):
    d = _data()
    loader = _loader(tree, augment=augment, augment_seed=9)
    batches = list(loader)
    assert len(batches) == 1
    b = batches[0]
    assert b["image"].shape == (6, 5) + PATCH and b["image"].dtype == torch.float32
    assert b["label"].shape == (6, 1) + PATCH and b["label"].dtype == torch.float32
    assert b["case_id"] == ["p0"] * 3 + ["p1"] * 3
    assert b["picks"].shape == (2, 10) and b["picks"].dtype == torch.int32
    assert not b["image"][:, 1].any() and all(b["image"][:, c].any() for c in (0, 2, 3, 4))   # DWI: zero_fill
    assert set(np.unique(b["label"].numpy()).tolist()) <= {0.0, 1.0}
    # T > 0 through the host form itself, for every case, and every label patch holds foreground
    ds = loader.dataset
    for i in range(len(ds)):
        tf = d.draw_transform(augment if augment is not None else d.Augment(), 9, 0, i, len(MODS))
        lab = d.read_nifti(ds.case_list[i]["label_path"])
        grid = (d.resample_affine(lab, LABEL_SHAPE, *tf.affine(lab.shape, LABEL_SHAPE), nearest=True) > 0)
        origins, T = d.pick_origins(grid.astype(np.float32), PATCH, *d.draw_patches(ds.patches, 4, 0, i, LABEL_SHAPE))
        assert T > 0 and int(b["picks"][i, 9]) == T
        assert b["picks"][i, :9].tolist() == origins.reshape(-1).tolist()
    assert (b["label"].sum(dim=(1, 2, 3, 4)) > 0).all()
    # set_epoch moves the patch draws; the same epoch gives the same batch
    again = next(iter(loader))
    assert torch.equal(again["image"], b["image"]) and torch.equal(again["label"], b["label"])
    ds.set_epoch(1)
    moved = next(iter(loader))
    assert not torch.equal(moved["picks"], b["picks"])
    assert not torch.equal(moved["image"], b["image"])


def test_host_loader_patches_are_crops_of_the_whole_grid(tree):
    """Without augmentation the grid is the label's and the transform the plain resampler's: every
    patch is a crop of today's whole-case sample at target_size = the label shape."""
    d = _data()
    b = next(iter(_loader(tree, patches=dict(foreground_prob=0.5, normalise=False))))
    whole = d.ProstateDataset(tree, modalities=MODS, target_size=LABEL_SHAPE)
    from pcms_amd.predict import gather_windows
    for i in range(2):
        s = whole[i]
        origins = b["picks"][i, :9].view(3, 3).numpy()
        assert torch.equal(torch.from_numpy(gather_windows(s["image"].numpy(), origins, PATCH)), b["image"][3 * i:3 * i + 3])
        assert torch.equal(torch.from_numpy(gather_windows(s["label"].numpy(), origins, PATCH)), b["label"][3 * i:3 * i + 3])


def test_raw_loader_carries_the_draws_as_cpu_tensors(tree):
    d = _data()
    b = next(iter(_loader(tree, raw=True)))
    assert d.is_raw_batch(b) and b["patch_size"] == PATCH and b["normalise"] is False and len(b["patches"]) == 2
    for i, p in enumerate(b["patches"]):
        assert p["rank_u"].dtype == torch.float64 and p["rank_u"].shape == (3,) and p["rank_u"].device.type == "cpu"
        assert p["fallback"].dtype == torch.int32 and p["fallback"].shape == (3, 3)
        assert p["grid"] == LABEL_SHAPE and p["affine"][1] is None and len(p["affine"][0]) == 12
        r, f = d.draw_patches(dict(patch_size=PATCH, patches_per_case=3, foreground_prob=1.0), 4, 0, i, LABEL_SHAPE)
        assert np.array_equal(p["rank_u"].numpy(), r) and np.array_equal(p["fallback"].numpy(), f)
    with pytest.raises(RuntimeError, match="GPU"):
        d.assemble_batch(b, None, "cpu")


def test_patches_none_changes_nothing(tree):
    d = _data()
    a = d.get_dataloader(tree, batch_size=2, shuffle=False, modalities=MODS, target_size=(8, 16, 16))
    b = d.get_dataloader(tree, batch_size=2, shuffle=False, modalities=MODS, target_size=(8, 16, 16), patches=None)
    x, y = next(iter(a)), next(iter(b))
    assert set(x) == set(y) == {"image", "label", "case_id"}
    assert torch.equal(x["image"], y["image"]) and torch.equal(x["label"], y["label"])
    assert b.dataset.patches is None and b.collate_fn is a.collate_fn


def test_trainer_passes_the_key_through(tree):
    from pcms_amd.utils.trainer import Trainer
    ps = dict(patch_size=PATCH, patches_per_case=3)
    cfg = {"device": "cpu", "learning_rate": 1e-4, "batch_size": 2, "num_epochs": 1, "data_dir": tree,
           "validation": True, "augment": AUG, "patches": ps}
    tr = Trainer(dict(cfg))
    assert tr.train_loader.dataset.patches.patch_size == PATCH and tr.val_loader.dataset.patches.patches_per_case == 3
    assert tr.train_loader.dataset.augment is not None and tr.val_loader.dataset.augment is None
    assert next(iter(tr.val_loader))["image"].shape == (6, 5) + PATCH


@pytest.mark.parametrize("kw", [
    dict(patch_size=(16, 100, 128)), dict(patch_size=(8, 16, 16)), dict(patch_size=(0, 16, 16)),
    dict(patch_size=(16, 16)), dict(patch_size=(16.5, 16, 16)), dict(patch_size=(16, 16, 528)),
    dict(foreground_prob=-0.01), dict(foreground_prob=1.01), dict(foreground_prob=float("nan")),
    dict(patches_per_case=0), dict(patches_per_case=65), dict(patches_per_case=1.5),
    dict(grid=(0, 8, 8)), dict(grid=(8, 8)),
])
def test_patch_sampling_rejects(kw):
    d = _data()
    with pytest.raises(ValueError):
        d.PatchSampling(**kw)
    with pytest.raises(ValueError):
        d.PatchSampling.of(kw)


def test_elastic_with_patches_is_rejected(tree):
    d = _data()
    with pytest.raises(ValueError, match="elastic"):
        d.ProstateDataset(tree, modalities=MODS, augment=dict(elastic_grid=4, elastic_disp=1.0), patches=dict())
    with pytest.raises(ValueError, match="elastic"):
        d.get_dataloader(tree, modalities=MODS, augment=dict(elastic_grid=(4, 4, 4)), patches=d.PatchSampling())
    assert d.PatchSampling() == d.PatchSampling(patch_size=(16, 128, 128), patches_per_case=2, foreground_prob=0.5,
                                                 grid=None, normalise=False, seed=0)
