"""Patch training's batch assembly against whole-grid assembly, in one process on one machine
(test tooling, not a test): the synthetic case of tests/tools/predict_time.py -- five int16
24x384x384 modalities -- plus a uint8 label with a lesion of a fraction of a percent of the grid.

  (a) ``assemble_batch`` of a patch-training batch (``patches``: P = 2 and P = 4 patches of
      (16, 128, 128), foreground_prob 1, no augmentation geometry beyond the identity draw, with
      and without ``normalise``): label on the grid, pick, [minmax,] patch resample per modality,
      label gather;
  (b) the existing ``assemble_batch`` of the same case onto the whole (24, 384, 384) grid, through
      the plain entry points and through the augmenting ones (``augment={}``, the identity draw).

Both legs start from a raw batch whose bytes are already on the device (the upload is the same in
both) and are timed with HIP events around the whole assembly, the median of --reps windows of
--iters assemblies after a warm-up.  The kernels of (a) alone are timed the same way over 3
rotating buffer sets, each with the bytes it moves and the fraction of the 6.3 TB/s the chip
reaches on a copy.

Writes profiles/patch_time.json (--out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests.tools.loader_time import cpu_model  # noqa: E402
from tests.tools.predict_time import RAW_SHAPE  # noqa: E402
from tests.tools.window_time import COPY_RATE, event_us  # noqa: E402

PATCH = (16, 128, 128)
LESION = (slice(9, 15), slice(150, 190), slice(200, 236))   # 8640 voxels, 0.24 % of the grid


def make_tree(root, data):
    rng = np.random.default_rng(0)
    lab_dir = os.path.join(root, "BPH-PCA", "ROI(BPH+PCA)", "BPH")
    os.makedirs(lab_dir)
    for m in data.DEFAULT_MODALITIES:
        os.makedirs(os.path.join(root, "BPH-PCA", "BPH", m))
        data.write_nifti(os.path.join(root, "BPH-PCA", "BPH", m, "case.nii"),
                         rng.integers(0, 4000, size=RAW_SHAPE).astype(np.int16), spacing=(0.5, 0.5, 3.0))
    lab = np.zeros(RAW_SHAPE, np.uint8)
    lab[LESION] = 1
    data.write_nifti(os.path.join(lab_dir, "case.nii"), lab, spacing=(0.5, 0.5, 3.0))


def on_device(batch, device):
    """The raw batch with every volume's bytes (and the patch draws) on the device."""
    batch = dict(batch)
    batch["raw_images"] = [[r.to(device) for r in case] for case in batch["raw_images"]]
    batch["raw_label"] = [r.to(device) for r in batch["raw_label"]]
    if "patches" in batch:
        batch["patches"] = [dict(p, rank_u=p["rank_u"].to(device), fallback=p["fallback"].to(device))
                            for p in batch["patches"]]
    return batch


def assembly_us(data, batch, device, reps, iters):
    t = event_us(lambda _: data.assemble_batch(batch, None, device), [None], reps, iters)
    return {"median_ms": t["median_us"] / 1e3, "all_ms": [v / 1e3 for v in t["all_us"]]}


def kernel_times(L, data, device, P, reps, iters):
    """HIP-event time of each launch of leg (a) at P patches, on the case's shapes."""
    rng = np.random.default_rng(1)
    n, nwin = int(np.prod(RAW_SHAPE)), int(np.prod(PATCH))
    lab = np.zeros(RAW_SHAPE, np.float32)
    lab[LESION] = 1.0
    ident = (ctypes.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    one = (ctypes.c_int * 1)(0)
    A = ctypes.addressof(ident)
    nwork, nmm = L.query("pcms_foreground_pick_work_ints", n), L.query("pcms_volume_minmax_work_floats", n)
    sets = []
    for k in range(3):
        origins = np.stack([rng.integers(0, g - w + 1, size=P) for g, w in zip(RAW_SHAPE, PATCH)], 1).astype(np.int32)
        sets.append({"raw": torch.from_numpy(rng.integers(0, 4000, size=n).astype(np.int16).view(np.uint8).copy())
                     .to(device), "label_raw": torch.from_numpy((lab > 0).astype(np.uint8).reshape(-1).copy()).to(device),
                     "label": torch.from_numpy(lab).to(device), "rank": torch.rand(P, dtype=torch.float64, device=device),
                     "fallback": torch.from_numpy(origins).to(device),
                     "picks": torch.from_numpy(np.concatenate([origins.reshape(-1), [0]]).astype(np.int32)).to(device),
                     "work": torch.empty(nwork, dtype=torch.int32, device=device),
                     "lohi": torch.tensor([0.0, 3999.0], device=device), "mm": torch.empty(nmm, device=device),
                     "grid_out": torch.empty(RAW_SHAPE, device=device),
                     "image": torch.empty((P, 5) + PATCH, device=device),
                     "labels": torch.empty((P, 1) + PATCH, device=device)})

    def patch(lohi):
        return lambda s: L.call("pcms_patch_resample_linear", s["raw"], 4, *RAW_SHAPE, 1.0, 0.0, A,
                                s["lohi"] if lohi else None, 1.0, 0.0, *RAW_SHAPE, s["picks"], P, s["image"][0, 2],
                                5 * nwin, *PATCH)

    # bytes: the label launch reads one byte and writes one float per grid voxel; the pick reads
    # the grid label once (plus one chunk per patch); minmax reads the volume; a patch launch
    # writes P patches and reads at most as many source voxels (the identity here: exactly, as
    # int16); the gather reads and writes P patches
    kernels = {
        "pcms_resample_affine_label_grid": (lambda s: L.call("pcms_resample_affine_label", s["label_raw"], 2, *RAW_SHAPE,
                                                              1.0, 0.0, A, s["grid_out"], *RAW_SHAPE), 5 * n),
        "pcms_foreground_pick": (lambda s: L.call("pcms_foreground_pick", s["label"], n, *RAW_SHAPE, *PATCH, s["rank"],
                                                   s["fallback"], P, s["picks"], s["work"]),
                                 4 * n + 4 * P * L.query("pcms_foreground_pick_chunk")),
        "pcms_volume_minmax": (lambda s: L.call("pcms_volume_minmax", s["raw"], 4, n, 1.0, 0.0, s["lohi"], s["mm"]),
                               2 * n),
        "pcms_patch_resample_linear": (patch(False), (4 + 2) * P * nwin),
        "pcms_patch_resample_linear_lohi": (patch(True), (4 + 2) * P * nwin),
        "pcms_window_gather_label": (lambda s: L.call("pcms_window_gather", s["label"], 1, *RAW_SHAPE, s["fallback"], P,
                                                      ctypes.addressof(one), 1, *PATCH, s["labels"]), 2 * 4 * P * nwin),
    }
    out = {}
    for name, (fn, nbytes) in kernels.items():
        t = event_us(fn, sets, reps, iters)
        t["bytes"] = nbytes
        t["fraction_of_copy_rate"] = nbytes / (t["median_us"] * 1e-6) / COPY_RATE
        out[name] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "patch_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd import data
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "host_cpu": cpu_model(), "raw_shape": list(RAW_SHAPE),
           "raw_dtype": "int16", "modalities": 5, "patch": list(PATCH), "lesion_voxels": 6 * 40 * 36,
           "copy_rate_bytes_per_s": COPY_RATE,
           "method": f"assemblies and kernels: HIP events, warm-up, median of {a.reps} windows of {a.iters}; kernels "
                     "over 3 rotating buffer sets; raw bytes already on the device in both legs"}
    with tempfile.TemporaryDirectory() as root:
        make_tree(root, data)
        for P in (2, 4):
            for norm in (False, True):
                ps = dict(patch_size=PATCH, patches_per_case=P, foreground_prob=1.0, normalise=norm)
                batch = on_device(next(iter(data.get_dataloader(root, batch_size=1, shuffle=False, device_resample=True,
                                                                patches=ps))), device)
                got = data.assemble_batch(batch, None, device)
                assert int(got["picks"][0, 3 * P]) == out["lesion_voxels"] and (got["label"].sum(dim=(1, 2, 3, 4)) > 0).all()
                out[f"a_patches_P{P}" + ("_normalise" if norm else "")] = assembly_us(data, batch, device, a.reps, a.iters)
        whole = on_device(next(iter(data.get_dataloader(root, batch_size=1, shuffle=False, device_resample=True,
                                                        target_size=RAW_SHAPE))), device)
        out["b_whole_grid"] = assembly_us(data, whole, device, a.reps, a.iters)
        # the same through the augmenting entry points (the identity draw): the launches leg (a) replaces
        whole = on_device(next(iter(data.get_dataloader(root, batch_size=1, shuffle=False, device_resample=True,
                                                        target_size=RAW_SHAPE, augment={}))), device)
        out["b_whole_grid_affine"] = assembly_us(data, whole, device, a.reps, a.iters)
        print(json.dumps(out), flush=True)
    for P in (2, 4):
        out[f"kernels_P{P}"] = kernel_times(L, data, device, P, a.reps, a.iters * 2)
        print(json.dumps(out[f"kernels_P{P}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
