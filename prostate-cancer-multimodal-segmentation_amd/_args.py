"""Argument checks and host-side kernel arguments shared by the kernel families.

The device forms take tensors that must already be on the GPU (there is no CPU fallback) and hand
some small arrays to the C entry points as host pointers; the host forms take (D, H, W) volumes and
integer triples.  What more than one family checks or builds alike lives here; a validator that
accepts something else (``window._three`` truncates, ``distance._spacing`` wants finite positive
numbers) stays with its family.
"""
from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np
import torch


def device_tensor(t, dtype: torch.dtype, ndim: int, what: str) -> torch.Tensor:
    """``t`` as a contiguous tensor, after the check every device form makes of an argument:
    RuntimeError unless it is a tensor on a GPU, ValueError unless it is a non-empty ``dtype`` tensor
    of ``ndim`` dimensions."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what} needs a {dtype} tensor on the GPU, not '{where}': pcms_amd has no CPU fallback -- "
                           "use the host form of the same name without _device")
    if t.dtype != dtype or t.dim() != ndim or t.numel() == 0:
        raise ValueError(f"{what} takes a non-empty {dtype} tensor of {ndim} dimensions, got {t.dtype} "
                         f"{tuple(t.shape)}")
    return t.contiguous()


# The arrays below are kernel *arguments* in host memory: the entry point reads them during the
# call (``ctypes.addressof``), so the caller keeps the returned object in a local until ``call``
# returns -- a temporary would be freed before the C side looks at it.
def host_affine12(twelve):
    """Row-major A[3][3], then t[3], as the twelve doubles an entry point reads during the call."""
    return (ctypes.c_double * 12)(*(float(v) for v in twelve))


def host_ints(values):
    """Flip masks (or any ints) as the ``int`` array an entry point reads during the call."""
    return (ctypes.c_int * len(values))(*values)


def host_floats(values):
    """Class weights or class values as the ``float`` array an entry point reads during the call."""
    return (ctypes.c_float * len(values))(*(float(v) for v in values))


def volume3(mask) -> np.ndarray:
    mask = np.asarray(mask)
    if mask.ndim != 3 or 0 in mask.shape:
        raise ValueError(f"a mask is a non-empty (D, H, W) volume, got shape {mask.shape}")
    return mask


def axes3(v, what: str) -> Tuple[int, int, int]:
    try:
        out = tuple(v)
    except TypeError:
        raise ValueError(f"{what} is three integers (d, h, w), got {v!r}") from None
    if len(out) != 3 or any(isinstance(a, bool) or int(a) != a for a in out):
        raise ValueError(f"{what} is three integers (d, h, w), got {v!r}")
    return tuple(int(a) for a in out)
