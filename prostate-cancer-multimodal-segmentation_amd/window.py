"""Sliding-window prediction (csrc/window.hip): host forms, then device forms.

``window_starts`` / ``window_grid`` / ``window_weights`` / ``gather_windows`` / ``blend_windows`` /
``sliding_window_predict`` are the host forms of cutting a volume into fixed-size overlapping
windows and blending the windows' probabilities with centre-weighted weights;
``gather_windows_device`` / ``blend_windows_device`` / ``sliding_window_device`` run them in HIP
kernels, bit for bit and independent of the batching; ``ModelPredictor.predict_case(...,
window=...)`` predicts a case at its native resolution through them.  ``tta_mean`` is the
test-time-augmentation mean a window's flipped copies are folded with (pcms_flip_mean's host form).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._args import device_tensor, host_ints
from ._lib import call


def tta_mean(probs: Sequence[np.ndarray], flips: Sequence[Tuple[int, ...]]) -> np.ndarray:
    """Test-time-augmentation mean, (D, H, W) float32: ``probs[j]`` is the probability volume
    of the input flipped along the axes ``flips[j]`` (out of 0, 1, 2; ``flips[0]`` must be
    ``()``), flipped back and summed in order in fp32, divided by ``float32(k)``."""
    flips = [tuple(int(a) for a in f) for f in flips]
    if len(probs) != len(flips) or not flips or flips[0] != ():
        raise ValueError("tta_mean needs one flip set per volume, the first of them ()")
    acc = np.asarray(probs[0], dtype=np.float32)
    for p, f in zip(probs[1:], flips[1:]):
        acc = acc + np.flip(np.asarray(p, dtype=np.float32), f)
    return acc / np.float32(len(flips))


def _flip_masks(flips) -> List[int]:
    """Flip sets (tuples of axes out of 0, 1, 2) as pcms_flip_mean's bit masks, () first."""
    masks = [0]
    for f in flips:
        f = tuple(int(a) for a in f)
        if not f or any(a not in (0, 1, 2) for a in f) or len(set(f)) != len(f):
            raise ValueError(f"a flip set holds distinct axes out of (0, 1, 2), got {f!r}")
        masks.append(sum(1 << a for a in f))
    return masks


# ---- sliding-window prediction --------------------------------------------------
# Fixed-size windows slide over a (D, H, W) grid; the row index of ``window_grid`` is *the* window
# index: entries, batches and the blend's order all follow it.  The host forms below define what
# csrc/window.hip computes, bit for bit: every product, sum and quotient rounds on its own in fp32.
MAX_WINDOW_AXIS = 512  # the blend kernel keeps three weight tables of this length in LDS; host forms agree


def window_starts(n: int, w: int, overlap: float) -> List[int]:
    """The window starts along one axis of ``n`` voxels for windows of ``w``: with
    ``step = max(1, int(w * (1.0 - overlap)))``, ``[0]`` when ``n <= w`` (the window sticks out
    past the volume), else ``ceil((n - w) / step) + 1`` starts ``min(i * step, n - w)``: the last
    window is flush with the end.  ValueError for ``w < 1``, ``n < 1`` or ``overlap`` outside
    ``[0, 1)``."""
    n, w, overlap = int(n), int(w), float(overlap)
    if w < 1 or n < 1 or not 0.0 <= overlap < 1.0:
        raise ValueError(f"window_starts needs n >= 1, w >= 1 and 0 <= overlap < 1, got {n}, {w}, {overlap}")
    step = max(1, int(w * (1.0 - overlap)))
    if n <= w:
        return [0]
    count = -(-(n - w) // step) + 1
    return [min(i * step, n - w) for i in range(count)]


def _three(v, what: str, cast=int) -> tuple:
    try:
        out = tuple(cast(a) for a in v)
    except TypeError:
        raise ValueError(f"{what} is three values (d, h, w), got {v!r}") from None
    if len(out) != 3:
        raise ValueError(f"{what} is three values (d, h, w), got {v!r}")
    return out


def window_grid(shape: Sequence[int], window: Sequence[int], overlap=0.5) -> np.ndarray:
    """All window starts on a (D, H, W) grid, int32 (K, 3): the Cartesian product of the three
    axes' ``window_starts``, d-major, then h, then w.  ``overlap`` is a scalar or one value per
    axis."""
    shape, window = _three(shape, "shape"), _three(window, "window")
    overlap = (float(overlap),) * 3 if np.ndim(overlap) == 0 else _three(overlap, "overlap", float)
    axes = [window_starts(n, w, o) for n, w, o in zip(shape, window, overlap)]
    return np.array([(a, b, c) for a in axes[0] for b in axes[1] for c in axes[2]], dtype=np.int32)


def window_weights(window: Sequence[int], blend: str = "gaussian",
                   sigma_scale: float = 0.125) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The per-axis blend weights of a window, three fp32 vectors (wd, wh, ww): 'gaussian' is
    ``exp(-0.5 * ((i - (w - 1) / 2) / (sigma_scale * w)) ** 2)`` in float64 cast to fp32,
    'constant' is ones.  The weight of window voxel (a, b, c) is
    ``fl32(fl32(wd[a] * wh[b]) * ww[c])``."""
    window = _three(window, "window")
    if any(w < 1 for w in window):
        raise ValueError(f"a window axis is at least 1, got {window}")
    if blend == "constant":
        return tuple(np.ones(w, dtype=np.float32) for w in window)
    if blend != "gaussian" or not float(sigma_scale) > 0.0:
        raise ValueError(f"blend is 'gaussian' (with sigma_scale > 0) or 'constant', got {blend!r}, {sigma_scale!r}")
    out = []
    for w in window:
        i = np.arange(w, dtype=np.float64)
        out.append(np.exp(-0.5 * ((i - (w - 1) / 2) / (float(sigma_scale) * w)) ** 2).astype(np.float32))
    return tuple(out)


def _window_args(starts, window, flips):
    """(starts as int64 (K, 3), window, pcms flip masks): what the four window forms check alike."""
    window = _three(window, "window")
    if any(not 1 <= w <= MAX_WINDOW_AXIS for w in window):
        raise ValueError(f"a window axis is in 1..{MAX_WINDOW_AXIS}, got {window}")
    starts = np.asarray(starts)
    if starts.ndim != 2 or starts.shape[1] != 3 or len(starts) == 0 or starts.dtype.kind not in "iu":
        raise ValueError(f"starts is a non-empty integer (K, 3) array, got {starts.dtype} {starts.shape}")
    return starts.astype(np.int64), window, _flip_masks(flips)


def _check_starts(starts: np.ndarray, shape) -> None:
    if (starts < 0).any() or (starts >= np.asarray(shape, np.int64)).any():
        raise ValueError(f"a window start lies outside the volume {tuple(shape)}")


def gather_windows(x: np.ndarray, starts, window: Sequence[int],
                   flips: Sequence[Tuple[int, ...]] = ()) -> np.ndarray:
    """The windows of a (C, D, H, W) volume as one network batch, float32
    (K * k, C, wd, wh, ww) with ``k = 1 + len(flips)``: entry ``i * k`` is window ``i`` (row ``i``
    of ``starts``), zero where it sticks out past the volume; entry ``i * k + j`` is that window
    flipped along ``flips[j - 1]`` -- the window is flipped, not the volume."""
    starts, window, masks = _window_args(starts, window, flips)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4 or 0 in x.shape:
        raise ValueError(f"gather_windows takes a non-empty (C, D, H, W) volume, got shape {x.shape}")
    _check_starts(starts, x.shape[1:])
    k = len(masks)
    out = np.zeros((len(starts) * k, x.shape[0]) + window, dtype=np.float32)
    for i, s in enumerate(starts.tolist()):
        n = [min(w, dim - a) for w, dim, a in zip(window, x.shape[1:], s)]
        win = out[i * k]
        win[:, :n[0], :n[1], :n[2]] = x[:, s[0]:s[0] + n[0], s[1]:s[1] + n[1], s[2]:s[2] + n[2]]
        for j, f in enumerate(flips, start=1):
            out[i * k + j] = np.flip(win, [1 + int(a) for a in f])
    return out


def _weight_vectors(weights, window) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    if len(weights) != 3:
        raise ValueError("weights are three vectors (wd, wh, ww)")
    weights = tuple(np.asarray(v) for v in weights)
    if any(v.dtype != np.float32 or v.shape != (w,) for v, w in zip(weights, window)):
        raise ValueError(f"weights are three float32 vectors of lengths {window}")
    return weights


def blend_windows(probs: np.ndarray, starts, window: Sequence[int], weights, shape: Sequence[int],
                  flips: Sequence[Tuple[int, ...]] = ()) -> np.ndarray:
    """The weighted blend of window probabilities on the (D, H, W) grid ``shape``, float32.
    ``probs`` is (K * k, wd, wh, ww) in ``gather_windows``' entry order.  In ascending window
    index ``m_i = tta_mean(probs[i*k:(i+1)*k], ((),) + flips)``, then over the part of the window
    inside the volume ``acc = acc + wgt * m_i`` (the product rounded, then the sum) and
    ``wsum = wsum + wgt``, with ``wgt = (wd[a] * wh[b]) * ww[c]`` from ``weights``; the result is
    ``acc / wsum``."""
    starts, window, masks = _window_args(starts, window, flips)
    shape = _three(shape, "shape")
    weights = _weight_vectors(weights, window)
    k = len(masks)
    probs = np.asarray(probs, dtype=np.float32)
    if probs.shape != (len(starts) * k,) + window:
        raise ValueError(f"probs is {(len(starts) * k,) + window}, got {probs.shape}")
    _check_starts(starts, shape)
    wgt = (weights[0][:, None, None] * weights[1][None, :, None]) * weights[2][None, None, :]
    acc = np.zeros(shape, dtype=np.float32)
    wsum = np.zeros(shape, dtype=np.float32)
    all_flips = [()] + [tuple(f) for f in flips]
    for i, s in enumerate(starts.tolist()):
        m = tta_mean(list(probs[i * k:(i + 1) * k]), all_flips)
        n = [min(w, dim - a) for w, dim, a in zip(window, shape, s)]
        box = (slice(s[0], s[0] + n[0]), slice(s[1], s[1] + n[1]), slice(s[2], s[2] + n[2]))
        part = (slice(0, n[0]), slice(0, n[1]), slice(0, n[2]))
        acc[box] = acc[box] + wgt[part] * m[part]
        wsum[box] = wsum[box] + wgt[part]
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / wsum


def _check_sliding(window, overlap, blend, window_batch) -> tuple:
    """The window as a tuple, after the checks every sliding-window driver makes first."""
    window = _three(window, "window")
    window_weights(window, blend)          # a bad window axis or blend
    window_grid(window, window, overlap)   # a bad overlap
    if any(w > MAX_WINDOW_AXIS for w in window):
        raise ValueError(f"a window axis is at most {MAX_WINDOW_AXIS}, got {window}")
    if not isinstance(window_batch, (int, np.integer)) or window_batch < 1:
        raise ValueError(f"window_batch is an integer >= 1, got {window_batch!r}")
    return window


def _batch_plan(K: int, window_batch: int) -> List[Tuple[int, int]]:
    """(first window, windows that count) per ``predict_fn`` call: every call carries
    ``window_batch`` windows, the last one padded with repeats of window K - 1."""
    return [(f, min(window_batch, K - f)) for f in range(0, K, window_batch)]


def sliding_window_predict(predict_fn, x: np.ndarray, window: Sequence[int], overlap=0.5, blend: str = "gaussian",
                           tta_flips: Sequence[Tuple[int, ...]] = (), window_batch: int = 4) -> np.ndarray:
    """Sliding-window prediction on the host, (D, H, W) float32 from a (C, D, H, W) volume:
    ``gather_windows`` over ``window_grid(x.shape[1:], window, overlap)``, ``predict_fn`` --
    ``(N, C, wd, wh, ww) -> (N, 1, wd, wh, ww)`` -- on batches of exactly ``window_batch * k``
    entries (``k = 1 + len(tta_flips)``; the last batch is padded with repeats of the final
    window, whose outputs are dropped), then ``blend_windows`` with ``window_weights(window,
    blend)``."""
    window = _check_sliding(window, overlap, blend, window_batch)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4:
        raise ValueError(f"sliding_window_predict takes a (C, D, H, W) volume, got shape {x.shape}")
    starts = window_grid(x.shape[1:], window, overlap)
    tiles = gather_windows(x, starts, window, tta_flips)
    K, k = len(starts), 1 + len(tta_flips)
    outs = []
    for first, real in _batch_plan(K, int(window_batch)):
        batch = tiles[first * k:(first + real) * k]
        if real < window_batch:
            batch = np.concatenate([batch] + [tiles[(K - 1) * k:]] * (window_batch - real))
        p = np.asarray(predict_fn(batch), dtype=np.float32)
        if p.shape != (window_batch * k, 1) + window:
            raise ValueError(f"predict_fn returned {p.shape}, not {(window_batch * k, 1) + window}")
        outs.append(p[:real * k, 0])
    return blend_windows(np.concatenate(outs), starts, window, window_weights(window, blend), x.shape[1:], tta_flips)


def _gather_enqueue(x: torch.Tensor, starts_dev: torch.Tensor, B: int, masks, window, out: torch.Tensor) -> None:
    """pcms_window_gather of the B windows at ``starts_dev`` (device int32, B rows) into ``out``."""
    host = host_ints(masks)
    call("pcms_window_gather", x, *x.shape, starts_dev, int(B), ctypes.addressof(host), len(masks), *window, out)


def gather_windows_device(x: torch.Tensor, starts, window: Sequence[int],
                          flips: Sequence[Tuple[int, ...]] = ()) -> torch.Tensor:
    """``gather_windows`` on the GPU, bit for bit (pcms_window_gather): a float32 CUDA volume
    (C, D, H, W) and the (K, 3) starts (a host array) in, the (K * k, C, wd, wh, ww) batch out,
    enqueued on the current stream.  A CPU tensor raises."""
    starts, window, masks = _window_args(starts, window, flips)
    x = device_tensor(x, torch.float32, 4, "gather_windows_device")
    _check_starts(starts, x.shape[1:])
    with torch.cuda.device(x.device):
        starts_dev = torch.from_numpy(starts.astype(np.int32)).to(x.device)
        out = torch.empty((len(starts) * len(masks), x.shape[0]) + window, dtype=torch.float32, device=x.device)
        _gather_enqueue(x, starts_dev, len(starts), masks, window, out)
    return out


def _blend_enqueue(probs: torch.Tensor, starts_dev: torch.Tensor, first: int, B: int, masks, wts: torch.Tensor,
                   window, acc: torch.Tensor, wsum: torch.Tensor) -> None:
    """pcms_window_blend of windows first .. first + B - 1 of the whole table ``starts_dev``."""
    host = host_ints(masks)
    call("pcms_window_blend", probs, starts_dev, int(first), int(B), ctypes.addressof(host), len(masks), wts, *window,
         acc, wsum, *acc.shape)


def _finish_enqueue(acc: torch.Tensor, wsum: torch.Tensor) -> torch.Tensor:
    prob = torch.empty_like(acc)
    call("pcms_window_finish", acc, wsum, prob, acc.numel())
    return prob


def blend_windows_device(probs: torch.Tensor, starts, window: Sequence[int], weights, shape: Sequence[int],
                         flips: Sequence[Tuple[int, ...]] = (), batch: Optional[int] = None) -> torch.Tensor:
    """``blend_windows`` on the GPU, bit for bit: pcms_window_blend over consecutive batches of
    ``batch`` windows (all K in one launch by default; the bits do not depend on it), then
    pcms_window_finish.  ``probs`` is a float32 CUDA tensor (K * k, wd, wh, ww); ``starts`` and
    ``weights`` are host arrays.  Returns the (D, H, W) float32 CUDA tensor.  A CPU tensor raises."""
    starts, window, masks = _window_args(starts, window, flips)
    shape = _three(shape, "shape")
    weights = _weight_vectors(weights, window)
    probs = device_tensor(probs, torch.float32, 4, "blend_windows_device")
    K, k = len(starts), len(masks)
    if tuple(probs.shape) != (K * k,) + window:
        raise ValueError(f"probs is {(K * k,) + window}, got {tuple(probs.shape)}")
    _check_starts(starts, shape)
    batch = K if batch is None else int(batch)
    if batch < 1:
        raise ValueError(f"batch is an integer >= 1, got {batch!r}")
    with torch.cuda.device(probs.device):
        starts_dev = torch.from_numpy(starts.astype(np.int32)).to(probs.device)
        wts = torch.from_numpy(np.concatenate(weights)).to(probs.device)
        acc = torch.zeros(shape, dtype=torch.float32, device=probs.device)
        wsum = torch.zeros(shape, dtype=torch.float32, device=probs.device)
        for first, real in _batch_plan(K, batch):
            _blend_enqueue(probs[first * k:(first + real) * k], starts_dev, first, real, masks, wts, window, acc, wsum)
        return _finish_enqueue(acc, wsum)


def sliding_window_device(predict_fn, x: torch.Tensor, window: Sequence[int], overlap=0.5, blend: str = "gaussian",
                          tta_flips: Sequence[Tuple[int, ...]] = (), window_batch: int = 4) -> torch.Tensor:
    """``sliding_window_predict`` on the GPU: ``x`` is the (1, C, D, H, W) float32 CUDA tensor of
    ``prepare_case_device``; per batch pcms_window_gather forms the ``window_batch * k`` entries
    (the last batch padded with repeats of the final window, so ``predict_fn`` sees one shape
    only), ``predict_fn`` maps them to (N, 1, wd, wh, ww) probabilities on the device, and
    pcms_window_blend accumulates the windows that count; pcms_window_finish divides.  Returns
    the (D, H, W) float32 probabilities on the device; everything is enqueued on the current
    stream.  A CPU tensor raises."""
    window = _check_sliding(window, overlap, blend, window_batch)
    masks = _flip_masks(tta_flips)
    x = device_tensor(x, torch.float32, 5, "sliding_window_device")
    if x.shape[0] != 1:
        raise ValueError(f"sliding_window_device takes one case, (1, C, D, H, W), got {tuple(x.shape)}")
    vol, shape = x[0], tuple(x.shape[2:])
    starts = window_grid(shape, window, overlap)
    K, k, wb = len(starts), len(masks), int(window_batch)
    plan = _batch_plan(K, wb)
    padded = np.concatenate([starts] + [starts[-1:]] * (len(plan) * wb - K))
    with torch.cuda.device(x.device):
        starts_dev = torch.from_numpy(padded).to(x.device)
        wts = torch.from_numpy(np.concatenate(window_weights(window, blend))).to(x.device)
        acc = torch.zeros(shape, dtype=torch.float32, device=x.device)
        wsum = torch.zeros(shape, dtype=torch.float32, device=x.device)
        batch = torch.empty((wb * k, vol.shape[0]) + window, dtype=torch.float32, device=x.device)
        for first, real in plan:
            _gather_enqueue(vol, starts_dev[first:first + wb], wb, masks, window, batch)
            probs = predict_fn(batch)
            if not isinstance(probs, torch.Tensor) or tuple(probs.shape) != (wb * k, 1) + window \
                    or probs.device != x.device:
                got = tuple(probs.shape) if isinstance(probs, torch.Tensor) else type(probs).__name__
                raise ValueError(f"predict_fn returned {got}, not a {(wb * k, 1) + window} tensor on {x.device}")
            probs = probs.float().contiguous()
            _blend_enqueue(probs, starts_dev, first, real, masks, wts, window, acc, wsum)
        return _finish_enqueue(acc, wsum)
