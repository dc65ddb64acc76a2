"""Case prediction on the host and on the device, in one process on one machine (test tooling,
not a test): one synthetic case in a temporary directory -- five int16 24x384x384 modalities
written by data.write_nifti -- taken to the 128^3 training grid and its mask back to the native
grid through

  * the host forms ``predict.prepare_case`` + ``predict.mask_on_grid`` (numpy ``data.resample``
    both ways; the probabilities between them are a fixed random volume: the network is not
    part of this leg), and
  * ``ModelPredictor.predict_case`` without flips (upload of the files' bytes, the prediction
    kernels, the network's forward, one copy of the mask back), plus the same call's stages
    timed apart: ``prepare_case_device`` and the forward.

Every leg is a wall-clock time around work that ends in a device synchronise, the median of
--runs after a warm-up.  The four kernels alone are timed with HIP events over 3 rotating
buffer sets after a warm-up, median of --reps windows of --iters launches.

Writes profiles/predict_time.json (--out) with the host CPU model: the host figures depend on
it."""
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

RAW_SHAPE = (24, 384, 384)
TARGET = (128, 128, 128)


def make_case(root, data, predict):
    rng = np.random.default_rng(0)
    for m in predict.MODALITIES:
        os.makedirs(os.path.join(root, m))
        data.write_nifti(os.path.join(root, m, "scan.nii"), rng.integers(0, 4000, size=RAW_SHAPE).astype(np.int16),
                         spacing=(0.5, 0.5, 3.0))


def median_ms(fn, runs):
    fn()  # warm-up: library load, file cache, the engine's buffers and packs
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(times), "all_ms": times}


def kernel_times(L, device, reps, iters):
    """HIP-event time of each kernel on the case's shapes (bytes already on the device)."""
    rng = np.random.default_rng(1)
    n, nt = int(np.prod(RAW_SHAPE)), int(np.prod(TARGET))
    nwork = L.query("pcms_volume_minmax_work_floats", n)
    flips = (ctypes.c_int * 2)(0, 4)
    sets = []
    for _ in range(3):
        sets.append({"raw": torch.from_numpy(rng.integers(0, 4000, size=n).astype(np.int16).view(np.uint8).copy())
                     .to(device), "lohi": torch.empty(2, device=device), "work": torch.empty(nwork, device=device),
                     "x": torch.empty(TARGET, device=device), "probs": torch.rand((2,) + TARGET, device=device),
                     "prob": torch.empty(TARGET, device=device),
                     "mask": torch.empty(RAW_SHAPE, dtype=torch.uint8, device=device),
                     "native": torch.empty(RAW_SHAPE, device=device)})
    kernels = {
        "pcms_volume_minmax": lambda s: L.call("pcms_volume_minmax", s["raw"], 4, n, 1.0, 0.0, s["lohi"], s["work"]),
        "pcms_resample_linear_norm": lambda s: L.call("pcms_resample_linear_norm", s["raw"], 4, *RAW_SHAPE, 1.0, 0.0,
                                                      s["lohi"], s["x"], *TARGET),
        "pcms_flip_mean_k2": lambda s: L.call("pcms_flip_mean", s["probs"], 2, ctypes.addressof(flips), s["prob"],
                                              *TARGET),
        "pcms_prob_to_mask": lambda s: L.call("pcms_prob_to_mask", s["probs"], *TARGET, 0.5, s["mask"], None,
                                              *RAW_SHAPE),
        "pcms_prob_to_mask_with_prob": lambda s: L.call("pcms_prob_to_mask", s["probs"], *TARGET, 0.5, s["mask"],
                                                        s["native"], *RAW_SHAPE),
    }
    out = {}
    for name, fn in kernels.items():
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
        out[name] = {"median_us": statistics.median(windows), "all_us": windows}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "predict_time.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd import data, predict
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "host_cpu": cpu_model(), "host_threads_torch": torch.get_num_threads(),
           "raw_shape": list(RAW_SHAPE), "raw_dtype": "int16", "modalities": 5, "target_size": list(TARGET),
           "precision": a.precision,
           "method": f"legs: wall clock around work ending in a device synchronise, median of {a.runs} runs after one "
                     f"warm-up run; kernels: HIP events, 3 rotating buffer sets, warm-up, median of {a.reps} windows "
                     f"of {a.iters} launches"}
    with tempfile.TemporaryDirectory() as root:
        make_case(root, data, predict)
        torch.manual_seed(0)
        ckpt = os.path.join(root, "model.pth")
        torch.save(pcms_amd.UNet3D(n_modalities=5, n_classes=1).state_dict(), ckpt)
        pred = predict.ModelPredictor(ckpt, device=str(device), precision=a.precision)
        prob = np.random.default_rng(2).random(TARGET).astype(np.float32)

        def host():
            predict.prepare_case(root, TARGET)
            predict.mask_on_grid(prob, RAW_SHAPE)

        def host_prepare():
            predict.prepare_case(root, TARGET)

        def dev():
            pred.predict_case(root, target_size=TARGET)

        def dev_prepare():
            dev.x = predict.prepare_case_device(root, TARGET, "zero_fill", True, device)

        def dev_forward():
            pred.model.predict(dev.x)

        out["device_predict_case"] = median_ms(dev, a.runs)
        out["device_prepare_case_device"] = median_ms(dev_prepare, a.runs)
        out["device_forward"] = median_ms(dev_forward, a.runs)
        out["host_prepare_case_plus_mask_on_grid"] = median_ms(host, a.runs)
        out["host_prepare_case"] = median_ms(host_prepare, a.runs)
        print(json.dumps(out), flush=True)
    out["kernels"] = kernel_times(L, device, a.reps, a.iters)
    print(json.dumps(out["kernels"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
