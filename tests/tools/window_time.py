"""Sliding-window prediction against whole-volume prediction at the native resolution, in one
process on one machine (test tooling, not a test): the synthetic case of
tests/tools/predict_time.py -- five int16 24x384x384 modalities -- through

  (a) ``predict_case(target_size=None)``: the whole native volume in one forward, the first call
      (which lays out the engine's plan and buffers for that shape) and the steady state apart;
  (b) ``predict_case(target_size=None, window=(16, 128, 128), overlap=0.5, window_batch=4)``: the
      same, first call and steady state, plus the sliding-window stage alone
      (``sliding_window_device`` on a prepared input) and the forwards alone (as many
      ``model.predict`` calls on a window batch as the stage makes).

Every leg is a wall-clock time around work that ends in a device synchronise, the median of
--runs after one warm-up.  The three kernels alone are timed with HIP events over 3 rotating
buffer sets after a warm-up, median of --reps windows of --iters launches, on the shapes of (b):
a batch of 4 windows out of the (5, 24, 384, 384) volume; each with the bytes it moves and the
fraction of the 6.3 TB/s the chip reaches on a copy.

Writes profiles/window_time.json (--out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests.tools.loader_time import cpu_model  # noqa: E402
from tests.tools.predict_time import RAW_SHAPE, make_case, median_ms  # noqa: E402

WINDOW = (16, 128, 128)
OVERLAP = 0.5
WINDOW_BATCH = 4
COPY_RATE = 6.3e12  # bytes / s


def first_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_us(fn, sets, reps, iters):
    for s in sets:
        fn(s)
    torch.cuda.synchronize()
    windows = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(sets[i % len(sets)])
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / iters * 1e3)
    return {"median_us": statistics.median(windows), "all_us": windows}


def kernel_times(L, predict, device, reps, iters):
    """HIP-event time of each kernel on the shapes of leg (b): the batch in the middle of the
    volume (windows 20..23: d = 0, h = 256, w = 0, 64, 128, 192; box 16 x 128 x 320)."""
    C, n, nwin = 5, int(np.prod(RAW_SHAPE)), int(np.prod(WINDOW))
    starts = predict.window_grid(RAW_SHAPE, WINDOW, OVERLAP)
    first, B = 20, WINDOW_BATCH
    lo, hi = starts[first:first + B].min(0), starts[first:first + B].max(0) + np.array(WINDOW)
    box = int(np.prod(np.minimum(hi, RAW_SHAPE) - lo))
    one, wflip = (ctypes.c_int * 1)(0), (ctypes.c_int * 2)(0, 4)
    wts = torch.from_numpy(np.concatenate(predict.window_weights(WINDOW))).to(device)
    sets = []
    for _ in range(3):
        sets.append({"x": torch.rand((C,) + RAW_SHAPE, device=device),
                     "starts": torch.from_numpy(starts).to(device),
                     "out": torch.empty((2 * B, C) + WINDOW, device=device),
                     "probs": torch.rand((2 * B,) + WINDOW, device=device),
                     "acc": torch.zeros(RAW_SHAPE, device=device), "wsum": torch.ones(RAW_SHAPE, device=device),
                     "prob": torch.empty(RAW_SHAPE, device=device)})

    def gather(k, fm):
        return lambda s: L.call("pcms_window_gather", s["x"], C, *RAW_SHAPE, s["starts"][first:first + B], B,
                                ctypes.addressof(fm), k, *WINDOW, s["out"])

    def blend(k, fm):
        return lambda s: L.call("pcms_window_blend", s["probs"], s["starts"], first, B, ctypes.addressof(fm), k, wts,
                                *WINDOW, s["acc"], s["wsum"], *RAW_SHAPE)

    # bytes: gather reads and writes every output element once (all four windows lie inside the
    # volume); blend reads k probabilities per (window, voxel) pair and reads and writes acc and
    # wsum once per voxel of the box; finish reads two volumes and writes one
    kernels = {
        "pcms_window_gather_k1": (gather(1, one), 2 * 4 * B * C * nwin),
        "pcms_window_gather_k2": (gather(2, wflip), 2 * 4 * 2 * B * C * nwin),
        "pcms_window_blend_k1": (blend(1, one), 4 * B * nwin + 4 * 4 * box),
        "pcms_window_blend_k2": (blend(2, wflip), 4 * 2 * B * nwin + 4 * 4 * box),
        "pcms_window_finish": (lambda s: L.call("pcms_window_finish", s["acc"], s["wsum"], s["prob"], n), 3 * 4 * n),
    }
    out = {"batch": {"first_window": first, "windows": B, "box_voxels": box}}
    for name, (fn, nbytes) in kernels.items():
        t = event_us(fn, sets, reps, iters)
        t["bytes"] = nbytes
        t["fraction_of_copy_rate"] = nbytes / (t["median_us"] * 1e-6) / COPY_RATE
        out[name] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window_time.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd import data, predict
    device = torch.device("cuda", 0)
    starts = predict.window_grid(RAW_SHAPE, WINDOW, OVERLAP)
    calls = -(-len(starts) // WINDOW_BATCH)
    out = {"device": torch.cuda.get_device_name(0), "host_cpu": cpu_model(), "raw_shape": list(RAW_SHAPE),
           "raw_dtype": "int16", "modalities": 5, "precision": a.precision, "window": list(WINDOW),
           "overlap": OVERLAP, "window_batch": WINDOW_BATCH, "windows": len(starts), "forward_calls": calls,
           "copy_rate_bytes_per_s": COPY_RATE,
           "method": f"legs: wall clock around work ending in a device synchronise, the first call apart, then the "
                     f"median of {a.runs} runs; kernels: HIP events, 3 rotating buffer sets, warm-up, median of "
                     f"{a.reps} windows of {a.iters} launches"}
    with tempfile.TemporaryDirectory() as root:
        make_case(root, data, predict)
        torch.manual_seed(0)
        ckpt = os.path.join(root, "model.pth")
        torch.save(pcms_amd.UNet3D(n_modalities=5, n_classes=1).state_dict(), ckpt)
        pred = predict.ModelPredictor(ckpt, device=str(device), precision=a.precision)
        pred.predict_case(root, target_size=(16, 16, 16))  # library load, file cache, the weight packs
        torch.cuda.synchronize()

        def whole():
            pred.predict_case(root, target_size=None)

        def windowed():
            pred.predict_case(root, target_size=None, window=WINDOW, overlap=OVERLAP, window_batch=WINDOW_BATCH)

        x = predict.prepare_case_device(root, None, "zero_fill", True, device)
        batch = torch.rand((WINDOW_BATCH, 5) + WINDOW, device=device)

        def stage():
            predict.sliding_window_device(pred.model.predict, x, WINDOW, OVERLAP, "gaussian", (), WINDOW_BATCH)

        def forwards():
            for _ in range(calls):
                pred.model.predict(batch)

        out["a_whole_volume_first_call_ms"] = first_ms(whole)
        out["a_whole_volume"] = median_ms(whole, a.runs)
        print(json.dumps(out), flush=True)
        out["b_sliding_window_first_call_ms"] = first_ms(windowed)
        out["b_sliding_window"] = median_ms(windowed, a.runs)
        out["b_sliding_window_stage"] = median_ms(stage, a.runs)
        out["b_forwards_alone"] = median_ms(forwards, a.runs)
        print(json.dumps(out), flush=True)
    out["kernels"] = kernel_times(L, predict, device, a.reps, a.iters)
    k = out["kernels"]
    per_case_us = calls * (k["pcms_window_gather_k1"]["median_us"] + k["pcms_window_blend_k1"]["median_us"]) + \
        k["pcms_window_finish"]["median_us"]
    out["window_kernels_per_case_ms"] = per_case_us / 1e3
    out["window_kernels_share_of_stage"] = per_case_us / 1e3 / out["b_sliding_window_stage"]["median_ms"]
    print(json.dumps(out["kernels"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
