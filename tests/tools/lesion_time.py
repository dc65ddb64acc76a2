"""The component table and the lesion metrics on the device and on the host, in one process on
one machine (test tooling, not a test).  The mask is postprocess_time.py's: 24x384x384, an
ellipsoid plus 0.2 % speckle (seed 0), a few thousand components of which one is large; the
metrics score it against a copy shifted by (1, 6, 9) voxels.

  * pcms_component_table with and without prob on the mask's labels (26-connectivity), and with
    prob on the ellipsoid alone (one component: every atomic lands in one row) and on the speckle
    alone (thousands of tiny components), each timed with HIP events over 3 rotating buffer sets
    after a warm-up, median of --reps windows of --iters calls (a call is its whole chain of
    launches); pcms_components_label beside it, the yardstick;
  * ``predict.component_table_device`` / ``lesion_table_device`` / ``lesion_metrics_device``: wall
    clock around a call that ends in its device-to-host copies;
  * the numpy host forms ``predict.component_table`` and ``predict.lesion_metrics``.

Every device result is compared with the host form before it is timed.  Writes
profiles/lesion_time.json (--out).  The figures are reported, not asserted."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests.tools.loader_time import cpu_model  # noqa: E402
from tests.tools.postprocess_time import host_ms, make_mask  # noqa: E402
from tests.tools.predict_time import RAW_SHAPE, median_ms  # noqa: E402

CAPACITY = 8192
SHIFT = (1, 6, 9)


def make_prob(mask):
    """fp32 in [0, 1): higher inside the mask, the maximum of a component rarely repeated."""
    rng = np.random.default_rng(1)
    return (0.5 * rng.random(RAW_SHAPE, dtype=np.float32) + 0.5 * (mask != 0)).astype(np.float32)


def table_bytes(table, header):
    return torch.cat([table.view(torch.uint8), header.view(torch.uint8)]).cpu().numpy()


def device_times(L, predict, cases, device, reps, iters):
    """cases: name -> (labels, prob or None, host table)."""
    from pcms_amd import lesions
    nwork = L.query("pcms_component_table_work_bytes", *RAW_SHAPE)
    out = {}
    for name, (lab, prob, host) in cases.items():
        nbytes = L.query("pcms_component_table_bytes", CAPACITY, int(prob is not None))
        sets = [{"labels": torch.from_numpy(lab).to(device), "prob": None if prob is None else
                 torch.from_numpy(prob).to(device), "table": torch.empty(nbytes // 8, dtype=torch.int64, device=device),
                 "header": torch.empty(2, dtype=torch.int32, device=device),
                 "work": torch.empty(nwork // 4, dtype=torch.int32, device=device)} for _ in range(3)]

        def fn(s):
            L.call("pcms_component_table", s["labels"], s["prob"], s["table"], CAPACITY, s["header"], s["work"],
                   *RAW_SHAPE)

        for s in sets:
            fn(s)
        torch.cuda.synchronize()
        raws = [table_bytes(s["table"], s["header"]) for s in sets]
        assert all(np.array_equal(r, raws[0]) for r in raws), name
        status, K = (int(v) for v in raws[0][-8:].view(np.int32))
        assert status == 0 and K == len(host["label"]) <= CAPACITY, name
        got = lesions._table_columns(raws[0][:-8], CAPACITY, K, prob is not None)
        assert all(np.array_equal(got[k].view(np.uint8), host[k].view(np.uint8)) for k in host), name
        windows = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(sets[i % len(sets)])
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / iters * 1e3)
        out[name] = {"components": K, "median_us": statistics.median(windows), "all_us": windows}
        print(name, K, out[name]["median_us"], flush=True)
    return out


def label_time(L, mask, device, reps, iters):
    nwork = L.query("pcms_components_work_ints", *RAW_SHAPE)
    sets = [{"mask": torch.from_numpy(mask).to(device), "labels": torch.empty(RAW_SHAPE, dtype=torch.int32, device=device),
             "work": torch.empty(nwork, dtype=torch.int32, device=device)} for _ in range(3)]

    def fn(s):
        L.call("pcms_components_label", s["mask"], 0, 26, s["labels"], s["work"], *RAW_SHAPE)

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


def same_metrics(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (isinstance(b[k], float) and b[k] != b[k] and a[k] != a[k])
                                    for k in b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lesion_time.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd import predict
    device = torch.device("cuda", 0)
    mask = make_mask()
    prob = make_prob(mask)
    d, h, w = np.indices(RAW_SHAPE, dtype=np.float32)
    c = [(s - 1) / 2 for s in RAW_SHAPE]
    ellipsoid = (((d - c[0]) / 9) ** 2 + ((h - c[1]) / 110) ** 2 + ((w - c[2]) / 140) ** 2 <= 1).astype(np.uint8)
    speckle = (mask & ~ellipsoid).astype(np.uint8)
    other = np.ascontiguousarray(np.roll(mask, SHIFT, axis=(0, 1, 2)))
    lab = predict.label_components(mask, 26)
    out = {"device": torch.cuda.get_device_name(0), "host_cpu": cpu_model(), "mask_shape": list(RAW_SHAPE),
           "mask": "ellipsoid (radii 9, 110, 140) | Bernoulli(0.002), np.random.default_rng(0); the reference of the "
                   f"metrics is np.roll of it by {SHIFT}",
           "prob": "0.5 * uniform(rng 1) + 0.5 inside the mask, fp32",
           "foreground_voxels": int(mask.sum()), "table_capacity": CAPACITY,
           "method": f"device calls: HIP events, 3 rotating buffer sets, warm-up, median of {a.reps} windows of "
                     f"{a.iters} calls; *_device wrappers: wall clock, median of {a.runs} runs after a warm-up run; "
                     f"host: wall clock, median of {a.host_runs} runs"}
    cases = {"table_c26": (lab, None, predict.component_table(lab)),
             "table_c26_prob": (lab, prob, predict.component_table(lab, prob))}
    for name, m in (("table_ellipsoid_prob", ellipsoid), ("table_speckle_prob", speckle)):
        lm = predict.label_components(m, 26)
        cases[name] = (lm, prob, predict.component_table(lm, prob))
    out["device_calls"] = device_times(L, predict, cases, device, a.reps, a.iters)
    out["device_calls"]["label_c26"] = label_time(L, mask, device, a.reps, a.iters)
    print("label_c26", out["device_calls"]["label_c26"]["median_us"], flush=True)

    dm, do, dp, dl = (torch.from_numpy(x).to(device) for x in (mask, other, prob, lab))
    sp = (3.0, 0.5, 0.5)
    host_metrics = predict.lesion_metrics(mask, other, prob, sp)
    assert same_metrics(predict.lesion_metrics_device(dm, do, dp, sp), host_metrics)
    assert predict.lesion_table_device(dm, dp, sp) == predict.lesion_table(mask, prob, sp)
    out["metrics"] = {k: host_metrics[k] for k in ("tp", "fp", "fn", "n_pred", "n_ref", "sensitivity", "precision")}
    out["component_table_device"] = median_ms(lambda: predict.component_table_device(dl, dp, CAPACITY), a.runs)
    out["component_table_device_default_capacity"] = median_ms(lambda: predict.component_table_device(dl, dp), a.runs)
    out["lesion_table_device"] = median_ms(lambda: predict.lesion_table_device(dm, dp, sp), a.runs)
    out["lesion_metrics_device"] = median_ms(lambda: predict.lesion_metrics_device(dm, do, dp, sp), a.runs)
    print(json.dumps({k: out[k]["median_ms"] for k in out if k.endswith("_device") or k.endswith("_default_capacity")}), flush=True)
    out["host_component_table"] = host_ms(lambda: predict.component_table(lab, prob), a.host_runs)
    out["host_bincount"] = host_ms(lambda: np.bincount(lab.reshape(-1)), a.host_runs)
    out["host_lesion_table"] = host_ms(lambda: predict.lesion_table(mask, prob, sp), a.host_runs)
    out["host_lesion_metrics"] = host_ms(lambda: predict.lesion_metrics(mask, other, prob, sp), a.host_runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v["median_ms"] for k, v in out.items() if k.startswith("host_") and k != "host_cpu"}),
          flush=True)


if __name__ == "__main__":
    main()
