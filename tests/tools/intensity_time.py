"""pcms_volume_window against pcms_volume_minmax on one buffer, in one process (test tooling, not
a test): a 24x512x512 int16 volume already on the device, two fills --

  * A: uniform random in 0..3999;
  * B: 90 % zeros, tissue in 50..900 (an MR volume: most lanes of a wave meet in one bin)

-- the select at (0.5, 99.5) over all voxels and over the voxels > 0, and the min-max kernel
(which reads the bytes once).  Stream-ordered times: HIP events around windows of --iters
launches over 3 rotating buffer sets after a warm-up, median of --reps windows; the two entry
points alternate window by window.  Every select's result is first compared with
``predict.intensity_window`` on the bits.

Writes profiles/intensity_time.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

RAW_SHAPE = (24, 512, 512)


def fills():
    rng = np.random.default_rng(0)
    n = int(np.prod(RAW_SHAPE))
    a = rng.integers(0, 4000, size=n).astype(np.int16)
    b = np.where(rng.random(n) < 0.9, 0, rng.integers(50, 901, size=n)).astype(np.int16)
    return {"A_uniform": a, "B_90pct_zeros": b}


def window_us(fn, sets, reps, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "intensity_time.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd import predict
    device = torch.device("cuda", 0)
    n = int(np.prod(RAW_SHAPE))
    out = {"device": torch.cuda.get_device_name(0), "raw_shape": list(RAW_SHAPE), "raw_dtype": "int16",
           "bytes": 2 * n, "window": [0.5, 99.5],
           "method": f"HIP events, 3 rotating buffer sets, warm-up, median of {a.reps} windows of {a.iters} launches, "
                     "the entry points alternating window by window; raw bytes already on the device",
           "fills": {}}
    nwork, nbytes = L.query("pcms_volume_minmax_work_floats", n), L.query("pcms_volume_window_work_bytes", n)
    for name, vol in fills().items():
        sets = [{"raw": torch.from_numpy(vol.view(np.uint8).copy()).to(device), "lohi": torch.empty(2, device=device),
                 "mm": torch.empty(nwork, device=device),
                 "work": torch.empty(nbytes, dtype=torch.uint8, device=device)} for _ in range(3)]
        kernels = {
            "pcms_volume_minmax": lambda s: L.call("pcms_volume_minmax", s["raw"], 4, n, 1.0, 0.0, s["lohi"], s["mm"]),
            "pcms_volume_window": lambda s: L.call("pcms_volume_window", s["raw"], 4, n, 1.0, 0.0, 5000, 995000, 0, 0.0,
                                                   s["lohi"], s["work"]),
            "pcms_volume_window_above0": lambda s: L.call("pcms_volume_window", s["raw"], 4, n, 1.0, 0.0, 5000, 995000,
                                                          1, 0.0, s["lohi"], s["work"]),
        }
        res = {}
        for key, above in (("pcms_volume_window", None), ("pcms_volume_window_above0", 0.0)):
            kernels[key](sets[0])
            got = sets[0]["lohi"].cpu().numpy()
            exp = predict.intensity_window(vol, 0.5, 99.5, above)
            assert np.array_equal(got.view(np.int32), exp.view(np.int32)), (name, key, got, exp)
            res[key + "_lohi"] = [float(v) for v in got]
        for fn in kernels.values():
            for s in sets:
                fn(s)
        torch.cuda.synchronize()
        windows = {k: [] for k in kernels}
        for _ in range(a.reps):
            for k, fn in kernels.items():
                windows[k].append(window_us(fn, sets, a.reps, a.iters))
        for k, w in windows.items():
            res[k] = {"median_us": statistics.median(w), "all_us": w}
        res["window_over_minmax"] = res["pcms_volume_window"]["median_us"] / res["pcms_volume_minmax"]["median_us"]
        out["fills"][name] = res
        print(name, json.dumps({k: v["median_us"] if isinstance(v, dict) else v for k, v in res.items()}), flush=True)
    f = out["fills"]
    out["B_over_A"] = {k: f["B_90pct_zeros"][k]["median_us"] / f["A_uniform"][k]["median_us"]
                       for k in ("pcms_volume_minmax", "pcms_volume_window", "pcms_volume_window_above0")}
    print("B / A", json.dumps(out["B_over_A"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
