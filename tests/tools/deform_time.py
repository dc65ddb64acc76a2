"""GPU time of the deforming resample launches against the affine ones, in one process (test
tooling, not a test; the method of augment_time.py, whose case, transform and step measurement it
takes): the six launches of a case -- five int16 24x384x384 modalities (linear) and a uint8 label
(nearest) to 128x128x64, the bytes and the control grid already on the device -- timed with HIP
events over 3 rotating buffer sets after a warm-up, affine and deform legs alternating rep by
rep, min of --reps x --iters each.  The field is an (8, 8, 8) control grid (the largest allowed:
12 KB in LDS, six rounds of the copy per workgroup) with control displacements uniform in
[-4, 4] output voxels.

The yardstick is the affine launch in the same process; the case's share of a training step
(bf16 build, batch 2 of 5x128x128x64, HIP events around ``Trainer.step_async``) is measured in
the same run, so that the cost is known -- the copy-stream prefetch hides it, nothing is gated.

Writes profiles/deform_time.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests.tools.augment_time import FLIPS, RAW_SHAPE, ROTATE_DEG, SHIFT, TARGET, ZOOM, step_time  # noqa: E402

GRID, DISP = (8, 8, 8), 4.0


def kernel_times(data, device, reps, iters):
    rng = np.random.default_rng(1)
    sets = []
    for _ in range(3):
        vols = [data.RawVolume(torch.from_numpy(rng.integers(0, 4000, size=RAW_SHAPE).astype(np.int16)
                                                .reshape(-1).view(np.uint8).copy()).to(device), 4, RAW_SHAPE, 1.0, 0.0)
                for _ in range(5)]
        lab = data.RawVolume(torch.from_numpy((rng.random(RAW_SHAPE) > 0.7).astype(np.uint8).reshape(-1))
                             .to(device), 2, RAW_SHAPE, 1.0, 0.0)
        field = torch.from_numpy(DISP * (2.0 * rng.random(GRID + (3,)) - 1.0)).to(device)
        sets.append((vols, lab, torch.empty((5,) + TARGET, device=device), torch.empty((1,) + TARGET, device=device),
                     field))
    A, t = data.volume_affine(data.compose_transform(FLIPS, ROTATE_DEG, ZOOM), SHIFT, RAW_SHAPE, TARGET)
    a12 = tuple(float(v) for v in A.reshape(-1)) + tuple(float(v) for v in t)
    gains, biases = (0.9, 0.95, 1.05, 1.1, 1.02), (-20.0, 10.0, 5.0, -5.0, 15.0)

    def case(s, field):
        for c, v in enumerate(s[0]):
            data.resample_device(v, TARGET, out=s[2][c], affine=a12, gain=gains[c], bias=biases[c], field=field)
        data.resample_device(s[1], TARGET, nearest=True, out=s[3][0], affine=a12, field=field)

    def linear(s, field):
        data.resample_device(s[0][0], TARGET, out=s[2][0], affine=a12, gain=gains[0], bias=biases[0], field=field)

    def label(s, field):
        data.resample_device(s[1], TARGET, nearest=True, out=s[3][0], affine=a12, field=field)

    legs = {"affine_case": lambda s: case(s, None), "deform_case": lambda s: case(s, s[4]),
            "affine_linear": lambda s: linear(s, None), "deform_linear": lambda s: linear(s, s[4]),
            "affine_label": lambda s: label(s, None), "deform_label": lambda s: label(s, s[4])}
    times = {k: [] for k in legs}
    for _ in range(reps):  # the legs alternate, so all see the same machine state
        for k, fn in legs.items():
            for s in sets:
                fn(s)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(sets[i % len(sets)])
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters * 1e3)
    s = sets[0]
    case(s, s[4])
    torch.cuda.synchronize()
    deformed = s[2][0].clone()
    inside = float((deformed != 0).float().mean())  # int16 draws in [0, 4000): a zero is (almost surely) outside
    case(s, None)
    torch.cuda.synchronize()
    changed = float((deformed != s[2][0]).float().mean())
    return times, inside, changed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deform_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    device = torch.device("cuda", 0)
    times, inside, changed = kernel_times(data, device, a.reps, a.iters)
    steps = step_time(device, a.warmup, a.steps)
    times2, _, _ = kernel_times(data, device, a.reps, a.iters)  # again after the steps: clocks and caches as in training
    best = {k: min(times[k] + times2[k]) for k in times}
    step_us = statistics.median(steps)
    out = {"device": torch.cuda.get_device_name(0), "raw_shape": list(RAW_SHAPE), "raw_dtype": "int16 (label uint8)",
           "target_size": list(TARGET), "launches_per_case": 6,
           "transform": {"rotate_deg": ROTATE_DEG, "zoom": ZOOM, "flips": FLIPS, "shift_voxels": SHIFT,
                         "gain_bias": "per modality, not identity"},
           "field": {"elastic_grid": list(GRID), "max_control_displacement_voxels": DISP, "inside_share": inside,
                     "share_of_voxels_changed_by_the_field": changed},
           "method": "HIP events, 3 rotating buffer sets, warm-up, affine and deform legs alternating rep by rep, "
                     f"min of 2 x {a.reps} x {a.iters} (before and after the timed steps); launches issued back to "
                     "back from Python, so launch gaps are in the figures; step: median of "
                     f"{a.steps} event-timed Trainer.step_async after {a.warmup} warm-up steps, bf16, batch 2",
           "affine_per_case_us": best["affine_case"], "deform_per_case_us": best["deform_case"],
           "deform_over_affine_case": best["deform_case"] / best["affine_case"],
           "affine_linear_launch_us": best["affine_linear"], "deform_linear_launch_us": best["deform_linear"],
           "affine_label_launch_us": best["affine_label"], "deform_label_launch_us": best["deform_label"],
           "all_us": {k: times[k] + times2[k] for k in times},
           "step_us_batch2": step_us, "step_us_per_case": step_us / 2, "step_us_all": steps,
           "deform_case_over_step_case": best["deform_case"] / (step_us / 2)}
    out["hidden_by_prefetch"] = bool(best["deform_case"] < step_us / 2)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
