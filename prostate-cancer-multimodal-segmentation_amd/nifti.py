"""NIfTI-1 files: header, voxels, undecoded bytes, geometry, and a minimal writer.

The reference reads NIfTI volumes with SimpleITK, which is absent here, so this module has its own
NIfTI-1 reader (``read_nifti``: .nii / .nii.gz, the header's scl_slope/scl_inter applied, array in
SimpleITK ``GetArrayFromImage`` order (z, y, x)).  ``read_nifti_raw`` -> ``RawVolume`` hands a file's
first volume over undecoded: what every kernel that reads a volume takes (``device_raw`` checks it,
``RawVolume.kernel_args`` spells it out).  ``read_nifti_geometry`` is where the grid lies in space
(``geometry.world_matrix``).
"""
from __future__ import annotations

import dataclasses
import gzip
import struct
from typing import Optional, Sequence, Tuple

import numpy as np
import torch


# NIfTI-1 datatype codes -> numpy dtypes
_NIFTI_DTYPES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8,
                 512: np.uint16, 768: np.uint32, 1024: np.int64, 1280: np.uint64}


def _open(path: str):
    return gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")


def read_nifti_header(path: str) -> dict:
    """Parse the 348-byte NIfTI-1 header (either byte order); ValueError if it is not one."""
    with _open(path) as f:
        raw = f.read(348)
    if len(raw) < 348:
        raise ValueError(f"{path}: truncated NIfTI header")
    for endian in ("<", ">"):
        if struct.unpack(endian + "i", raw[:4])[0] == 348:
            break
    else:
        raise ValueError(f"{path}: not a NIfTI-1 file (sizeof_hdr != 348)")
    dim = struct.unpack(endian + "8h", raw[40:56])
    datatype, bitpix = struct.unpack(endian + "hh", raw[70:74])
    pixdim = struct.unpack(endian + "8f", raw[76:108])
    vox_offset, scl_slope, scl_inter = struct.unpack(endian + "fff", raw[108:120])
    magic = raw[344:348]
    if magic not in (b"n+1\x00", b"ni1\x00"):
        raise ValueError(f"{path}: bad NIfTI magic {magic!r}")
    if datatype not in _NIFTI_DTYPES:
        raise ValueError(f"{path}: unsupported NIfTI datatype {datatype}")
    nd = dim[0]
    if not 1 <= nd <= 7:
        raise ValueError(f"{path}: bad dim[0] = {nd}")
    return {"endian": endian, "shape_xyz": tuple(int(d) for d in dim[1:1 + nd]), "datatype": datatype,
            "bitpix": bitpix, "spacing": tuple(float(p) for p in pixdim[1:1 + nd]),
            "vox_offset": int(vox_offset), "scl_slope": float(scl_slope), "scl_inter": float(scl_inter)}


def read_nifti(path: str) -> np.ndarray:
    """Voxel array in SimpleITK ``GetArrayFromImage`` order: (z, y, x), or (t, z, y, x).
    Intensity scaling (scl_slope != 0) is applied, as ITK's NIfTI reader does."""
    h = read_nifti_header(path)
    dt = np.dtype(_NIFTI_DTYPES[h["datatype"]]).newbyteorder(h["endian"])
    count = int(np.prod(h["shape_xyz"]))
    with _open(path) as f:
        f.read(max(h["vox_offset"], 352))
        buf = f.read(count * dt.itemsize)
    if len(buf) < count * dt.itemsize:
        raise ValueError(f"{path}: truncated voxel data")
    arr = np.frombuffer(buf, dtype=dt, count=count).reshape(h["shape_xyz"][::-1])
    if h["scl_slope"] not in (0.0, 1.0) or h["scl_inter"] != 0.0:
        slope = h["scl_slope"] if h["scl_slope"] != 0.0 else 1.0
        arr = arr.astype(np.float64) * slope + h["scl_inter"]
    return np.ascontiguousarray(arr)


@dataclasses.dataclass
class RawVolume:
    """The first 3-D volume of a NIfTI file as stored: its voxel bytes (1-D ``torch.uint8``,
    little endian), the NIfTI datatype code, the (D, H, W) shape and the header's scaling --
    what ``resample_device`` needs to form ``read_nifti``'s values on the GPU."""
    data: torch.Tensor
    code: int
    shape: Tuple[int, int, int]
    slope: float
    inter: float

    def pin_memory(self) -> "RawVolume":  # DataLoader(pin_memory=True) calls this on custom types
        return dataclasses.replace(self, data=self.data.pin_memory())

    def to(self, device, non_blocking: bool = False) -> "RawVolume":
        return dataclasses.replace(self, data=self.data.to(device, non_blocking=non_blocking))

    def numpy(self) -> np.ndarray:
        """The volume as ``read_nifti`` returns it (host bytes only)."""
        dt = np.dtype(_NIFTI_DTYPES[self.code]).newbyteorder("<")
        arr = np.frombuffer(self.data.numpy().tobytes(), dtype=dt).reshape(self.shape)
        if self.slope not in (0.0, 1.0) or self.inter != 0.0:
            arr = arr.astype(np.float64) * (self.slope if self.slope != 0.0 else 1.0) + self.inter
        return np.ascontiguousarray(arr)

    def kernel_args(self, flat: bool = False) -> tuple:
        """The argument group every C entry point takes for a volume: ``data, code, D, H, W, slope,
        inter``, or with ``flat`` ``data, code, n, slope, inter`` (pcms_volume_minmax / _window)."""
        dims = (int(np.prod(self.shape)),) if flat else tuple(self.shape)
        return (self.data, int(self.code), *dims, float(self.slope), float(self.inter))


def device_raw(raw, what: str) -> RawVolume:
    """``raw`` after the check every device form makes of a volume: RuntimeError unless it is a
    ``RawVolume`` whose bytes are on a GPU, ValueError unless they are the contiguous uint8 bytes
    of its shape and datatype -- a kernel reads that many."""
    if not isinstance(raw, RawVolume) or raw.data.device.type != "cuda":
        raise RuntimeError(f"{what} needs RawVolumes whose bytes are on a GPU (RawVolume.to(device)): pcms_amd has no "
                           "CPU fallback -- use the host form of the same name without _device")
    nbytes = int(np.prod(raw.shape)) * np.dtype(_NIFTI_DTYPES[raw.code]).itemsize
    if raw.data.dtype != torch.uint8 or not raw.data.is_contiguous() or raw.data.numel() != nbytes:
        raise ValueError(f"RawVolume.data must be the {nbytes} contiguous bytes of shape {raw.shape}, datatype "
                         f"{raw.code}; it holds {raw.data.numel()} of {raw.data.dtype}")
    return raw


def read_nifti_raw(path: str) -> RawVolume:
    """The first 3-D volume of ``path`` undecoded (a 4-D file contributes volume 0, as
    ``ProstateDataset._first_volume`` takes it); a big-endian file is byte-swapped here."""
    h = read_nifti_header(path)
    if len(h["shape_xyz"]) not in (3, 4):
        raise ValueError(f"unsupported image dimensions: {h['shape_xyz'][::-1]}")
    dt = np.dtype(_NIFTI_DTYPES[h["datatype"]]).newbyteorder(h["endian"])
    shape = tuple(int(v) for v in h["shape_xyz"][:3][::-1])
    nbytes = int(np.prod(shape)) * dt.itemsize
    with _open(path) as f:
        f.read(max(h["vox_offset"], 352))
        buf = f.read(nbytes)
    if len(buf) < nbytes:
        raise ValueError(f"{path}: truncated voxel data")
    arr = np.frombuffer(buf, dtype=dt)
    if h["endian"] == ">":
        arr = arr.astype(dt.newbyteorder("<"))
    data = torch.from_numpy(arr.view(np.uint8).copy())
    return RawVolume(data, int(h["datatype"]), shape, h["scl_slope"], h["scl_inter"])


# the header fields that place a volume in space: (name, byte offset, struct format)
_GEOMETRY_FIELDS = (("pixdim", 76, "4f"), ("xyzt_units", 123, "B"), ("qform_code", 252, "h"), ("sform_code", 254, "h"),
                    ("quatern_b", 256, "f"), ("quatern_c", 260, "f"), ("quatern_d", 264, "f"),
                    ("qoffset_x", 268, "f"), ("qoffset_y", 272, "f"), ("qoffset_z", 276, "f"),
                    ("srow_x", 280, "4f"), ("srow_y", 296, "4f"), ("srow_z", 312, "4f"))


def read_nifti_geometry(path: str) -> dict:
    """Where the file's voxel grid lies in space (either byte order): ``pixdim`` (pixdim[0..3],
    qfac first), ``xyzt_units``, ``qform_code`` / ``sform_code``, ``quatern_b/c/d``,
    ``qoffset_x/y/z`` and ``srow_x/y/z`` (four floats each) -- what SimpleITK's
    ``CopyInformation`` carries over as spacing, origin and direction, and what
    ``write_nifti(..., geometry=...)`` writes back."""
    endian = read_nifti_header(path)["endian"]
    with _open(path) as f:
        raw = f.read(348)
    geo = {}
    for name, off, fmt in _GEOMETRY_FIELDS:
        v = struct.unpack_from(endian + fmt, raw, off)
        geo[name] = v[0] if len(v) == 1 else tuple(v)
    return geo


def write_nifti(path: str, arr_zyx: np.ndarray, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                geometry: Optional[dict] = None) -> None:
    """Minimal NIfTI-1 writer (single file, little endian) for tests, synthetic data and
    predicted masks.  ``geometry`` (a ``read_nifti_geometry`` dict): its fields are written too
    and ``spacing`` is taken from its pixdim[1..3]; without it the header carries the spacing
    alone."""
    codes = {np.dtype(v): k for k, v in _NIFTI_DTYPES.items()}
    a = np.ascontiguousarray(arr_zyx)
    if a.dtype not in codes:
        a = a.astype(np.float32)
    a = a.astype(a.dtype.newbyteorder("<"))
    shape_xyz = a.shape[::-1]
    hdr = bytearray(352)
    struct.pack_into("<i", hdr, 0, 348)
    dims = [len(shape_xyz)] + list(shape_xyz) + [1] * (7 - len(shape_xyz))
    struct.pack_into("<8h", hdr, 40, *dims)
    struct.pack_into("<hh", hdr, 70, codes[a.dtype], a.dtype.itemsize * 8)
    pix =[1.0] + list(spacing) + [1.0] * (7 - len(spacing))
    struct.pack_into("<8f", hdr, 76, *pix[:8])
    struct.pack_into("<fff", hdr, 108, 352.0, 1.0, 0.0)
    if geometry is not None:  # pixdim[0..3] among them: the geometry's spacing replaces `spacing`
        for name, off, fmt in _GEOMETRY_FIELDS:
            v = geometry[name]
            struct.pack_into("<" + fmt, hdr, off, *(v if isinstance(v, (tuple, list)) else (v,)))
    hdr[344:348] = b"n+1\x00"
    data = bytes(hdr) + a.tobytes()
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)


def _shape_zyx(path: str) -> Tuple[int, int, int]:
    return tuple(int(v) for v in read_nifti_header(path)["shape_xyz"][:3][::-1])


def _first_volume(a: np.ndarray) -> np.ndarray:
    if a.ndim not in (3, 4):
        raise ValueError(f"unsupported image dimensions: {a.shape}")
    return a if a.ndim == 3 else a[0]
