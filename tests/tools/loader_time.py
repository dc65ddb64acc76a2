"""Loader throughput with and without device-side resampling, in one process on one machine
(test tooling, not a test): a synthetic dataset in a temporary directory -- 8 cases of five
int16 24x384x384 modalities plus a label, written by data.write_nifti -- read to 128x128x64
batches through

  * the default loader (numpy ``data.resample`` on the host), and
  * the ``device_resample`` loader plus ``data.assemble_batch`` (pinned upload of the files'
    bytes, one resample launch per volume),

each timed by the wall clock over whole passes (cases / s, the batch resident on the GPU at the
end of both).  The resample kernels alone are timed with HIP events over 3 rotating buffer sets
after a warm-up: the launches of one case (five linear, one label), min of --reps x --iters.

Writes profiles/loader_device_resample.json (--out) with the host CPU model: the host figures
depend on it."""
import argparse
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

RAW_SHAPE = (24, 384, 384)
TARGET = (128, 128, 64)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def make_tree(root, data, cases):
    rng = np.random.default_rng(0)
    lab_dir = os.path.join(root, "BPH-PCA", "ROI(BPH+PCA)", "BPH")
    os.makedirs(lab_dir)
    for m in data.DEFAULT_MODALITIES:
        os.makedirs(os.path.join(root, "BPH-PCA", "BPH", m))
    for c in range(cases):
        for m in data.DEFAULT_MODALITIES:
            vol = rng.integers(0, 4000, size=RAW_SHAPE).astype(np.int16)
            data.write_nifti(os.path.join(root, "BPH-PCA", "BPH", m, f"case{c:02d}.nii"), vol)
        lab = np.zeros(RAW_SHAPE, np.uint8)
        lab[8:16, 100:280, 120:260] = 1
        data.write_nifti(os.path.join(lab_dir, f"case{c:02d}.nii"), lab)


def one_pass(loader, data, device):
    n = 0
    t0 = time.perf_counter()
    for batch in loader:
        batch = data.device_batch(batch, device)
        x = batch["image"].to(device, non_blocking=True)
        y = batch["label"].to(device, non_blocking=True)
        n += x.shape[0]
    torch.cuda.synchronize()
    del x, y
    return n / (time.perf_counter() - t0)


def kernel_time(data, device, reps, iters):
    """HIP-event time of one case's resample launches (bytes already on the device)."""
    rng = np.random.default_rng(1)
    sets = []
    for _ in range(3):
        vols = [data.RawVolume(torch.from_numpy(rng.integers(0, 4000, size=RAW_SHAPE).astype(np.int16)
                                                .reshape(-1).view(np.uint8).copy()).to(device), 4, RAW_SHAPE, 1.0, 0.0)
                for _ in range(5)]
        lab = data.RawVolume(torch.from_numpy((rng.random(RAW_SHAPE) > 0.7).astype(np.uint8).reshape(-1))
                             .to(device), 2, RAW_SHAPE, 1.0, 0.0)
        sets.append((vols, lab, torch.empty((5,) + TARGET, device=device), torch.empty((1,) + TARGET, device=device)))

    def case(s):
        for c, v in enumerate(s[0]):
            data.resample_device(v, TARGET, out=s[2][c])
        data.resample_device(s[1], TARGET, nearest=True, out=s[3][0])

    def linear(s):
        data.resample_device(s[0][0], TARGET, out=s[2][0])

    def label(s):
        data.resample_device(s[1], TARGET, nearest=True, out=s[3][0])

    def timed(fn):
        best = []
        for _ in range(reps):
            for s in sets:
                fn(s)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(sets[i % len(sets)])
            e1.record()
            e1.synchronize()
            best.append(e0.elapsed_time(e1) / iters * 1e3)
        return best

    t_case, t_lin, t_lab = timed(case), timed(linear), timed(label)
    return {"per_case_us": min(t_case), "per_case_us_all": t_case, "linear_launch_us": min(t_lin),
            "label_launch_us": min(t_lab), "launches_per_case": 6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loader_device_resample.json"))
    ap.add_argument("--cases", type=int, default=8)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "host_cpu": cpu_model(), "host_threads_torch": torch.get_num_threads(),
           "cases": a.cases, "batch_size": a.batch, "raw_shape": list(RAW_SHAPE), "raw_dtype": "int16",
           "target_size": list(TARGET), "num_workers": 0,
           "method": f"wall clock over whole passes of the dataset (best of {a.passes} after one warm-up pass), the "
                     "batch on the GPU at the end of both paths; kernels: HIP events, 3 rotating buffer sets, "
                     f"warm-up, min of {a.reps} x {a.iters}"}
    with tempfile.TemporaryDirectory() as root:
        make_tree(root, data, a.cases)
        loaders = {k: data.get_dataloader(root, batch_size=a.batch, shuffle=False, target_size=TARGET,
                                          device_resample=(k == "device_resample")) for k in ("default", "device_resample")}
        rates = {k: [] for k in loaders}
        one_pass(loaders["device_resample"], data, device)  # warm-up: library load, pinned pool, file cache
        for _ in range(a.passes):  # alternating, so both see the same machine state
            for k, ld in loaders.items():
                rates[k].append(one_pass(ld, data, device))
                print(json.dumps({k: rates[k][-1]}), flush=True)
        # what the device path's host side still spends per case: reading the files
        ds = loaders["device_resample"].dataset
        t0 = time.perf_counter()
        for i in range(len(ds)):
            ds[i]
        out["device_resample_host_read_ms_per_case"] = (time.perf_counter() - t0) / len(ds) * 1e3
    out["default_cases_per_s"] = max(rates["default"])
    out["device_resample_cases_per_s"] = max(rates["device_resample"])
    out["cases_per_s_all"] = rates
    out["speedup"] = out["device_resample_cases_per_s"] / out["default_cases_per_s"]
    out["resample_kernels"] = kernel_time(data, device, a.reps, a.iters)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
