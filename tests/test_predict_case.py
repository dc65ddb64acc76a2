"""Host forms of case prediction (predict.normalise / prepare_case / tta_mean / mask_on_grid,
data.read_nifti_geometry and write_nifti's geometry keyword): the oracle of the device path,
pinned here by closed forms and by the functions they restate.  Comparisons are on bits."""
import hashlib
import os
import struct

import numpy as np
import pytest


def _mods():
    import pcms_amd  # noqa: F401
    from pcms_amd import data, predict
    return data, predict


def _same_bits(got, exp):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype == np.float32 and got.shape == exp.shape
    assert np.array_equal(got.view(np.int32), exp.view(np.int32))


def _sources():
    rng = np.random.default_rng(11)
    shape = (4, 5, 6)
    nan = (100.0 * rng.standard_normal(shape)).astype(np.float32)
    nan[1, 2, 3] = np.nan
    return {"uint8": rng.integers(3, 250, size=shape).astype(np.uint8),
            "int16": rng.integers(-3000, 3000, size=shape).astype(np.int16),
            "float32": (1000.0 * rng.standard_normal(shape)).astype(np.float32),
            "float64": 1000.0 * rng.standard_normal(shape) + 1e-7,
            "zeros": np.zeros(shape, np.int16), "nan": nan}


def _write_case(data, predict, root, vols):
    """vols: one array (or None: the folder stays empty) per modality."""
    for mod, vol in zip(predict.MODALITIES, vols):
        os.makedirs(os.path.join(root, mod), exist_ok=True)
        if vol is not None:
            data.write_nifti(os.path.join(root, mod, "img.nii"), vol)
    return str(root)


@pytest.mark.parametrize("name", ["uint8", "int16", "float32", "float64", "zeros", "nan"])
def test_normalise_is_load_multimodal_images_channel(tmp_path, name):
    data, predict = _mods()
    vol = _sources()[name]
    case = _write_case(data, predict, tmp_path / "case", [vol] * 5)
    with np.errstate(invalid="ignore"):
        img, _ = predict.load_multimodal_images(case)
        got = predict.normalise(vol)
    assert got.dtype == np.float32
    if name == "nan":
        assert np.isnan(got).all() and np.isnan(img[0]).all()
        return
    _same_bits(got, img[0])
    if name == "zeros":
        assert not got.any()
    else:
        assert got.min() == 0.0 and got.max() == 1.0


def test_prepare_case_closed_forms(tmp_path):
    data, predict = _mods()
    src = _sources()
    vols = [src["int16"], src["uint8"], src["float32"], src["float64"], src["int16"][::-1].copy()]
    case = _write_case(data, predict, tmp_path / "case", vols)
    # identity target: normalise alone
    got = predict.prepare_case(case, target_size=(4, 5, 6))
    assert got.shape == (5, 4, 5, 6) and got.dtype == np.float32
    for c, v in enumerate(vols):
        _same_bits(got[c], predict.normalise(data.read_nifti(os.path.join(case, predict.MODALITIES[c], "img.nii"))))
    _same_bits(predict.prepare_case(case, target_size=None), got)
    # normalise=False: the loader's channel
    target = (7, 3, 8)
    plain = predict.prepare_case(case, target_size=target, normalise=False)
    for c, v in enumerate(vols):
        _same_bits(plain[c], data.resample(v.astype(np.float32), target))
    # both: resample(normalise(.))
    both = predict.prepare_case(case, target_size=target)
    for c, v in enumerate(vols):
        _same_bits(both[c], data.resample(predict.normalise(v), target))


def test_prepare_case_mixed_shapes_and_missing(tmp_path):
    data, predict = _mods()
    rng = np.random.default_rng(12)
    four_d = rng.integers(0, 900, size=(2, 5, 7, 6)).astype(np.int16)  # volume 0 is used
    vols = [rng.integers(0, 900, size=(4, 5, 6)).astype(np.int16), four_d, None,
            rng.random((6, 4, 5)).astype(np.float32), rng.integers(0, 255, size=(3, 8, 4)).astype(np.uint8)]
    case = _write_case(data, predict, tmp_path / "case", vols)
    target = (5, 6, 4)
    exp = [None if v is None else data.resample(predict.normalise(v if v.ndim == 3 else v[0]), target) for v in vols]
    zf = predict.prepare_case(case, target_size=target, handle_missing="zero_fill")
    dup = predict.prepare_case(case, target_size=target, handle_missing="duplicate")
    for c in (0, 1, 3, 4):
        _same_bits(zf[c], exp[c])
        _same_bits(dup[c], exp[c])
    assert not zf[2].any()
    _same_bits(dup[2], exp[0])
    with pytest.raises(FileNotFoundError):
        predict.prepare_case(case, target_size=target, handle_missing="skip")
    with pytest.raises(ValueError):
        predict.prepare_case(case, target_size=None)
    with pytest.raises(ValueError):
        predict.prepare_case(case, target_size=target, handle_missing="mean")
    # the first modality missing: 'duplicate' still copies the first present one
    case2 = _write_case(data, predict, tmp_path / "case2", [None] + vols[:2] + vols[3:])
    dup2 = predict.prepare_case(case2, target_size=target, handle_missing="duplicate")
    _same_bits(dup2[0], dup2[1])
    _same_bits(dup2[1], exp[0])


def test_tta_mean():
    _, predict = _mods()
    rng = np.random.default_rng(13)
    p = rng.random((3, 4, 5)).astype(np.float32)
    _same_bits(predict.tta_mean([p], [()]), p)
    sym = p + np.flip(p, (0, 2))  # symmetric under the flip of axes 0 and 2
    _same_bits(predict.tta_mean([sym, sym], [(), (0, 2)]), sym)
    q, r = rng.random((3, 4, 5)).astype(np.float32), rng.random((3, 4, 5)).astype(np.float32)
    exp = ((p + q[:, :, ::-1]) + r[::-1, ::-1, :]) / np.float32(3)
    _same_bits(predict.tta_mean([p, q, r], [(), (2,), (0, 1)]), exp)
    with pytest.raises(ValueError):
        predict.tta_mean([p, q], [(2,), ()])


def test_mask_on_grid():
    data, predict = _mods()
    at = np.full((4, 5, 6), 0.3, np.float32)
    mask, prob = predict.mask_on_grid(at, (4, 5, 6), threshold=0.3)  # strict >: exactly at the threshold is 0
    assert mask.dtype == np.uint8 and not mask.any()
    _same_bits(prob, at)
    assert predict.mask_on_grid(at, (4, 5, 6), threshold=0.29)[0].all()
    p = np.random.default_rng(14).random((4, 5, 6)).astype(np.float32)
    mask, prob = predict.mask_on_grid(p, (8, 5, 9))
    _same_bits(prob, data.resample(p, (8, 5, 9)))
    assert np.array_equal(mask, (prob > np.float32(0.5)).astype(np.uint8))
    # the trailing-edge rule: native slice 7 samples 7 * 4 / 8 = 3.5 = n_tgt - 0.5, so it is background
    assert not prob[7].any() and not mask[7].any() and prob[6].all()


def _with_geometry(data, path, endian):
    """A file with a non-trivial qform / sform, in either byte order."""
    data.write_nifti(path, np.arange(24, dtype=np.int16).reshape(2, 3, 4), spacing=(0.5, 0.75, 3.0))
    raw = bytearray(open(path, "rb").read())
    struct.pack_into("<f", raw, 76, -1.0)  # qfac
    raw[123] = 10  # mm, s
    struct.pack_into("<hh", raw, 252, 1, 2)
    struct.pack_into("<6f", raw, 256, 0.1, -0.2, 0.3, -91.5, 126.25, -72.0)
    struct.pack_into("<12f", raw, 280, -0.49, 0.01, 0.2, 91.5, 0.02, 0.74, -0.1, -126.25, 0.03, 0.05, 2.9, -72.0)
    if endian == ">":  # re-encode every header field and the voxels big endian
        hdr = bytearray(352)
        struct.pack_into(">i", hdr, 0, 348)
        hdr[40:56] = struct.pack(">8h", *struct.unpack("<8h", raw[40:56]))
        hdr[70:74] = struct.pack(">hh", *struct.unpack("<hh", raw[70:74]))
        hdr[76:120] = struct.pack(">11f", *struct.unpack("<11f", raw[76:120]))
        hdr[123] = raw[123]
        hdr[252:256] = struct.pack(">hh", *struct.unpack("<hh", raw[252:256]))
        hdr[256:328] = struct.pack(">18f", *struct.unpack("<18f", raw[256:328]))
        hdr[344:348] = raw[344:348]
        raw = hdr + np.frombuffer(bytes(raw[352:]), "<i2").astype(">i2").tobytes()
    open(path, "wb").write(bytes(raw))
    return path


@pytest.mark.parametrize("endian", ["<", ">"])
def test_geometry_roundtrip(tmp_path, endian):
    data, _ = _mods()
    little = open(_with_geometry(data, str(tmp_path / "le.nii"), "<"), "rb").read()
    src = _with_geometry(data, str(tmp_path / "src.nii"), endian)
    assert np.array_equal(data.read_nifti(src), np.arange(24).reshape(2, 3, 4))
    geo = data.read_nifti_geometry(src)
    assert geo["pixdim"] == (-1.0, 0.5, 0.75, 3.0) and geo["xyzt_units"] == 10
    assert (geo["qform_code"], geo["sform_code"]) == (1, 2) and len(geo["srow_y"]) == 4
    out = str(tmp_path / "out.nii")
    data.write_nifti(out, np.ones((2, 3, 4), np.uint8), spacing=(9.0, 9.0, 9.0), geometry=geo)
    got = open(out, "rb").read()
    assert got[252:328] == little[252:328] and got[76:92] == little[76:92] and got[123] == little[123]
    assert data.read_nifti_geometry(out) == geo
    assert data.read_nifti_header(out)["spacing"] == (0.5, 0.75, 3.0)
    assert np.array_equal(data.read_nifti(out), np.ones((2, 3, 4), np.uint8))


def test_write_nifti_without_geometry_is_unchanged(tmp_path):
    """The bytes the writer produced before it had the geometry keyword (hashes taken on that
    commit): an int16 volume with a spacing, and a bool volume (stored as float32)."""
    data, _ = _mods()
    a = (np.arange(2 * 3 * 4).reshape(2, 3, 4) * 7 - 50).astype(np.int16)
    p = str(tmp_path / "a.nii")
    data.write_nifti(p, a, spacing=(0.5, 0.75, 3.0))
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == HASH_INT16
    p = str(tmp_path / "b.nii")
    data.write_nifti(p, a > 0)
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == HASH_BOOL
    p = str(tmp_path / "c.nii")
    data.write_nifti(p, a, spacing=(0.5, 0.75, 3.0), geometry=None)
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == HASH_INT16


HASH_INT16 = "84e3029b20b7a3853470fdcae996a47ad2a1e8df8570ad4e430ec080e62665d7"
HASH_BOOL = "d00f68c9ffe48cff78ba8df2d5753a759e834855377f577f27c2848b61ebaacc"
