"""Surface-distance metrics on the device and on the host, in one process on one machine (test
tooling, not a test).  The pair is 24x384x384 at spacing (3.6, 0.3125, 0.3125): an ellipsoid
(radii 9, 110, 140) and the same ellipsoid shifted by (1, 9, -12) and dilated (radii 10, 118, 150).

  * ``--steps edt``: pcms_mask_surface, pcms_edt_sq (of the first mask's surface) and
    pcms_surface_distance_stats, each timed with HIP events over 3 rotating buffer sets after a
    warm-up, median of --reps windows of --iters calls (a call is its whole chain of launches);
  * ``--steps metrics``: the whole ``predict.surface_metrics_device`` call, wall clock around a call
    that ends in its device-to-host copy, and its pieces on the device as the differences show them;
  * ``--steps host``: the numpy host form ``predict.surface_metrics`` and, where scipy imports,
    MedPy's recipe on scipy.ndimage (binary_erosion, distance_transform_edt twice, np.percentile).

Every device result is compared with the host form before it is timed.  Each step merges its
figures into profiles/surface_metrics_time.json (--out), so that a caller can give every step a
time limit of its own.  The figures are reported, not asserted."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests.tools.loader_time import cpu_model  # noqa: E402
from tests.tools.postprocess_time import host_ms  # noqa: E402

SHAPE = (24, 384, 384)
SPACING = (3.6, 0.3125, 0.3125)


def make_pair():
    d, h, w = np.indices(SHAPE, dtype=np.float32)
    c = [(s - 1) / 2 for s in SHAPE]
    a = ((d - c[0]) / 9) ** 2 + ((h - c[1]) / 110) ** 2 + ((w - c[2]) / 140) ** 2 <= 1
    b = ((d - c[0] - 1) / 10) ** 2 + ((h - c[1] - 9) / 118) ** 2 + ((w - c[2] + 12) / 150) ** 2 <= 1
    return a.astype(np.uint8), b.astype(np.uint8)


def windows_us(fn, sets, reps, iters):
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


def step_edt(L, predict, a, b, device, reps, iters):
    import ctypes
    sp = (ctypes.c_double * 3)(*SPACING)
    nwork = L.query("pcms_edt_work_bytes", *SHAPE)
    surf_b = predict.surface(b)
    sets = [{"a": torch.from_numpy(a).to(device), "b": torch.from_numpy(b).to(device),
             "feat": torch.from_numpy(surf_b).to(device), "surf": torch.empty(SHAPE, dtype=torch.uint8, device=device),
             "sq": torch.empty(SHAPE, dtype=torch.float64, device=device),
             "sd": torch.empty(SHAPE, dtype=torch.float64, device=device),
             "stats": torch.empty(3, dtype=torch.float64, device=device),
             "work": torch.empty(nwork, dtype=torch.uint8, device=device)} for _ in range(3)]
    calls = {
        "pcms_mask_surface": lambda s: L.call("pcms_mask_surface", s["b"], s["surf"], *SHAPE),
        "pcms_edt_sq": lambda s: L.call("pcms_edt_sq", s["feat"], ctypes.addressof(sp), s["sq"], s["work"], *SHAPE),
        "pcms_surface_distance_stats": lambda s: L.call("pcms_surface_distance_stats", s["a"], s["sq"], s["sd"],
                                                        s["stats"], s["work"], *SHAPE),
    }
    for fn in calls.values():  # in this order: the statistics read the transform
        for s in sets:
            fn(s)
    torch.cuda.synchronize()
    host_sq = predict.edt_sq(surf_b, SPACING)
    surf_a = predict.surface(a) != 0
    for s in sets:  # the results are the host form's before anything is timed
        assert np.array_equal(s["surf"].cpu().numpy(), surf_b)
        assert np.array_equal(s["sq"].cpu().numpy().view(np.int64), host_sq.view(np.int64))
        assert np.array_equal(s["sd"].cpu().numpy().view(np.int64), np.where(surf_a, host_sq, -1.0).view(np.int64))
        assert int(s["stats"].cpu().numpy().view(np.int64)[0]) == int(surf_a.sum())
    out = {}
    for name, fn in calls.items():
        out[name] = windows_us(fn, sets, reps, iters)
        print(name, out[name]["median_us"], flush=True)
    return {"device_calls": out, "surface_voxels": {"a": int(surf_a.sum()), "b": int(surf_b.sum())}}


def step_metrics(predict, a, b, device, runs):
    da, db = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
    got = predict.surface_metrics_device(da, db, SPACING)
    exp = predict.surface_metrics(a, b, SPACING)
    assert all(got[k] == exp[k] for k in ("hd", "hd95", "n_a", "n_b")), (got, exp)
    assert abs(got["assd"] - exp["assd"]) <= 1e-9 * exp["assd"], (got, exp)
    times = []
    for _ in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        predict.surface_metrics_device(da, db, SPACING)
        times.append((time.perf_counter() - t0) * 1e3)
    times = times[1:]  # the first run warms the allocator
    # the PyTorch plumbing on its own: select, concatenate, sort
    sd = torch.where(torch.from_numpy(predict.surface(a) != 0).to(device),
                     torch.rand(SHAPE, dtype=torch.float64, device=device), -1.0)
    plumbing = windows_us(lambda s: torch.sort(torch.cat([s[s >= 0], s[s >= 0]])), [sd, sd.clone(), sd.clone()], 5, 20)
    print("surface_metrics_device", statistics.median(times), "select+cat+sort", plumbing["median_us"], flush=True)
    return {"surface_metrics_device": {"median_ms": statistics.median(times), "all_ms": times, "result": got},
            "select_cat_sort": plumbing}


def scipy_chain(a, b):
    from scipy import ndimage as ndi
    st = ndi.generate_binary_structure(3, 1)
    sa, sb = (m.astype(bool) ^ ndi.binary_erosion(m.astype(bool), st) for m in (a, b))
    da = ndi.distance_transform_edt(~sb, sampling=SPACING)[sa]
    db = ndi.distance_transform_edt(~sa, sampling=SPACING)[sb]
    return {"hd": float(max(da.max(), db.max())), "hd95": float(np.percentile(np.hstack([da, db]), 95)),
            "assd": float((da.mean() + db.mean()) / 2)}


def step_host(predict, a, b, host_runs):
    out = {"host_numpy": host_ms(lambda: predict.surface_metrics(a, b, SPACING), 1)}
    exp = predict.surface_metrics(a, b, SPACING)
    try:
        got = scipy_chain(a, b)
    except ImportError:
        return out
    assert all(abs(got[k] - exp[k]) <= 1e-12 * exp[k] for k in got), (got, exp)
    out["host_scipy"] = host_ms(lambda: scipy_chain(a, b), host_runs)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_metrics_time.json"))
    ap.add_argument("--steps", default="edt,metrics,host")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd import predict
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    ma, mb = make_pair()
    out.update({"host_cpu": cpu_model(), "shape": list(SHAPE), "spacing": list(SPACING),
                "masks": "ellipsoid (radii 9, 110, 140); the same shifted by (1, 9, -12), radii 10, 118, 150",
                "foreground_voxels": [int(ma.sum()), int(mb.sum())],
                "method": f"device calls: HIP events, 3 rotating buffer sets, warm-up, median of {a.reps} windows of "
                          f"{a.iters} calls; surface_metrics_device: wall clock, median of {a.runs} runs after a "
                          f"warm-up run; host: wall clock (numpy one run, scipy median of {a.host_runs})"})
    steps = a.steps.split(",")
    if "edt" in steps or "metrics" in steps:
        device = torch.device("cuda", 0)
        out["device"] = torch.cuda.get_device_name(0)
    if "edt" in steps:
        out.update(step_edt(L, predict, ma, mb, device, a.reps, a.iters))
    if "metrics" in steps:
        out.update(step_metrics(predict, ma, mb, device, a.runs))
    if "host" in steps:
        out.update(step_host(predict, ma, mb, a.host_runs))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
