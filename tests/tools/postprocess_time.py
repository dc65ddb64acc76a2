"""Mask post-processing on the device and on the host, in one process on one machine (test
tooling, not a test).  The mask is 24x384x384: an ellipsoid plus 0.2 % speckle (seed 0), a few
thousand components of which one is large.

  * pcms_components_label and pcms_mask_postprocess at several settings, each timed with HIP
    events over 3 rotating buffer sets after a warm-up, median of --reps windows of --iters calls
    (a call is its whole chain of launches: the kernels are internal to the library, so the
    stages are read from the differences between settings);
  * ``ModelPredictor.predict_case`` on predict_time.py's synthetic case with and without
    post-processing (wall clock around a call that ends in the device-to-host copy);
  * the numpy host form ``predict.postprocess`` and, where scipy imports, scipy.ndimage's chain
    label + bincount + keep-largest + binary_fill_holes.

Every device result is compared with the host form before it is timed.  Writes
profiles/postprocess_time.json (--out).  The figures are reported, not asserted."""
import argparse
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
from tests.tools.predict_time import RAW_SHAPE, TARGET, make_case, median_ms  # noqa: E402


def make_mask():
    rng = np.random.default_rng(0)
    d, h, w = np.indices(RAW_SHAPE, dtype=np.float32)
    c = [(s - 1) / 2 for s in RAW_SHAPE]
    ellipsoid = ((d - c[0]) / 9) ** 2 + ((h - c[1]) / 110) ** 2 + ((w - c[2]) / 140) ** 2 <= 1
    return (ellipsoid | (rng.random(RAW_SHAPE) < 0.002)).astype(np.uint8)


def host_ms(fn, runs):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(times), "all_ms": times}


def scipy_chain(mask, connectivity):
    from scipy import ndimage as ndi
    lab, count = ndi.label(mask, ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))
    sizes = np.bincount(lab.reshape(-1))
    sizes[0] = 0
    return ndi.binary_fill_holes(lab == int(np.argmax(sizes))).astype(np.uint8), count


def device_times(L, predict, mask, device, reps, iters):
    nwork = L.query("pcms_components_work_ints", *RAW_SHAPE)
    sets = [{"mask": torch.from_numpy(mask).to(device), "out": torch.empty(RAW_SHAPE, dtype=torch.uint8, device=device),
             "labels": torch.empty(RAW_SHAPE, dtype=torch.int32, device=device),
             "work": torch.empty(nwork, dtype=torch.int32, device=device)} for _ in range(3)]

    def label(connectivity, invert=0):
        return lambda s: L.call("pcms_components_label", s["mask"], invert, connectivity, s["labels"], s["work"],
                                *RAW_SHAPE)

    def post(keep, min_voxels, fill, connectivity):
        return lambda s: L.call("pcms_mask_postprocess", s["mask"], s["out"], s["work"], keep, min_voxels, int(fill),
                                connectivity, *RAW_SHAPE)

    calls = {"label_c6": (label(6), None), "label_c26": (label(26), None), "label_c6_invert": (label(6, 1), None),
             "post_identity": (post(0, 0, False, 26), (0, 0, False, 26)),
             "post_min4_c26": (post(0, 4, False, 26), (0, 4, False, 26)),
             "post_keep1_c6": (post(1, 0, False, 6), (1, 0, False, 6)),
             "post_keep1_c26": (post(1, 0, False, 26), (1, 0, False, 26)),
             "post_keep8_c26": (post(8, 0, False, 26), (8, 0, False, 26)),
             "post_fill_only": (post(0, 0, True, 26), (0, 0, True, 26)),
             "post_keep1_fill_c6": (post(1, 0, True, 6), (1, 0, True, 6)),
             "post_keep1_fill_c26": (post(1, 0, True, 26), (1, 0, True, 26)),
             "post_keep1_min4_fill_c26": (post(1, 4, True, 26), (1, 4, True, 26))}
    out = {}
    for name, (fn, host_args) in calls.items():
        for s in sets:
            fn(s)
        torch.cuda.synchronize()
        assert all(int(s["work"][0]) == 0 for s in sets), name
        if host_args is not None:  # the result is the host form's before it is timed
            assert np.array_equal(sets[0]["out"].cpu().numpy(), predict.postprocess(mask, *host_args)), name
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
        print(name, out[name]["median_us"], flush=True)
    assert np.array_equal(sets[0]["labels"].cpu().numpy(), predict.label_components(mask == 0, 6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "postprocess_time.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd import predict, data
    device = torch.device("cuda", 0)
    mask = make_mask()
    lab = predict.label_components(mask, 26)
    sizes = np.unique(lab[lab > 0], return_counts=True)[1]
    out = {"device": torch.cuda.get_device_name(0), "host_cpu": cpu_model(), "mask_shape": list(RAW_SHAPE),
           "mask": "ellipsoid (radii 9, 110, 140) | Bernoulli(0.002), np.random.default_rng(0)",
           "foreground_voxels": int(mask.sum()), "components_c26": int(len(sizes)), "largest_c26": int(sizes.max()),
           "method": f"device calls: HIP events, 3 rotating buffer sets, warm-up, median of {a.reps} windows of "
                     f"{a.iters} calls; predict_case: wall clock, median of {a.runs} runs after a warm-up run; host: "
                     f"wall clock, median of {a.host_runs} runs"}
    out["device_calls"] = device_times(L, predict, mask, device, a.reps, a.iters)
    with tempfile.TemporaryDirectory() as root:
        make_case(root, data, predict)
        torch.manual_seed(0)
        ckpt = os.path.join(root, "model.pth")
        torch.save(pcms_amd.UNet3D(n_modalities=5, n_classes=1).state_dict(), ckpt)
        pred = predict.ModelPredictor(ckpt, device=str(device), precision=a.precision)
        prob = pred.predict_case(root, target_size=TARGET, return_probability=True).probability
        thr = float(np.median(prob))
        plain = pred.predict_case(root, target_size=TARGET, threshold=thr).mask
        posted = pred.predict_case(root, target_size=TARGET, threshold=thr, keep_largest=1, min_voxels=4,
                                   fill_holes=True).mask
        assert np.array_equal(posted, predict.postprocess(plain, 1, 4, True))
        plab = predict.label_components(plain, 26)
        out["predict_case_mask"] = {"threshold": "median probability", "foreground_voxels": int(plain.sum()),
                                    "components_c26": int(len(np.unique(plab[plab > 0]))),
                                    "foreground_after": int(posted.sum())}
        out["predict_case_plain"] = median_ms(lambda: pred.predict_case(root, target_size=TARGET, threshold=thr), a.runs)
        out["predict_case_keep1_min4_fill"] = median_ms(
            lambda: pred.predict_case(root, target_size=TARGET, threshold=thr, keep_largest=1, min_voxels=4,
                                      fill_holes=True), a.runs)
    print(json.dumps({k: v for k, v in out.items() if k.startswith("predict_case")}), flush=True)
    for connectivity in (6, 26):
        out[f"host_numpy_keep1_fill_c{connectivity}"] = host_ms(
            lambda: predict.postprocess(mask, 1, 0, True, connectivity), a.host_runs)
        try:
            got, count = scipy_chain(mask, connectivity)
        except ImportError:
            continue
        assert np.array_equal(got, predict.postprocess(mask, 1, 0, True, connectivity))
        out[f"host_scipy_keep1_fill_c{connectivity}"] = host_ms(lambda: scipy_chain(mask, connectivity), a.host_runs)
        out[f"components_c{connectivity}"] = int(count)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k.startswith("host")}), flush=True)


if __name__ == "__main__":
    main()
