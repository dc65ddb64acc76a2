"""GPU time of the augmenting resample launches against the plain ones, in one process (test
tooling, not a test; the method of loader_time.py): the six launches of a case -- five int16
24x384x384 modalities (linear) and a uint8 label (nearest) to 128x128x64, the bytes already on
the device -- timed with HIP events over 3 rotating buffer sets after a warm-up, plain and
affine legs alternating rep by rep, min of --reps x --iters each.  The affine leg uses a
general transform (three rotations, zoom, a flip, a shift, gain and bias per modality), so the
gather is not axis-aligned and the intensity step runs.

The yardstick is the plain launch in the same process; the one sanity condition is that the
augmented case stays below the per-case time of a training step measured in the same run
(bf16 build, batch 2 of 5x128x128x64, HIP events around ``Trainer.step_async``), so the
copy-stream prefetch still hides it.

Writes profiles/augment_time.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

RAW_SHAPE = (24, 384, 384)
TARGET = (128, 128, 64)
ROTATE_DEG, ZOOM, FLIPS, SHIFT = (10.0, 5.0, -5.0), 1.1, (False, False, True), (3.0, -4.0, 1.5)


def kernel_times(data, device, reps, iters):
    rng = np.random.default_rng(1)
    sets = []
    for _ in range(3):
        vols = [data.RawVolume(torch.from_numpy(rng.integers(0, 4000, size=RAW_SHAPE).astype(np.int16)
                                                .reshape(-1).view(np.uint8).copy()).to(device), 4, RAW_SHAPE, 1.0, 0.0)
                for _ in range(5)]
        lab = data.RawVolume(torch.from_numpy((rng.random(RAW_SHAPE) > 0.7).astype(np.uint8).reshape(-1))
                             .to(device), 2, RAW_SHAPE, 1.0, 0.0)
        sets.append((vols, lab, torch.empty((5,) + TARGET, device=device), torch.empty((1,) + TARGET, device=device)))
    A, t = data.volume_affine(data.compose_transform(FLIPS, ROTATE_DEG, ZOOM), SHIFT, RAW_SHAPE, TARGET)
    a12 = tuple(float(v) for v in A.reshape(-1)) + tuple(float(v) for v in t)
    gains, biases = (0.9, 0.95, 1.05, 1.1, 1.02), (-20.0, 10.0, 5.0, -5.0, 15.0)

    def plain_case(s):
        for c, v in enumerate(s[0]):
            data.resample_device(v, TARGET, out=s[2][c])
        data.resample_device(s[1], TARGET, nearest=True, out=s[3][0])

    def affine_case(s):
        for c, v in enumerate(s[0]):
            data.resample_device(v, TARGET, out=s[2][c], affine=a12, gain=gains[c], bias=biases[c])
        data.resample_device(s[1], TARGET, nearest=True, out=s[3][0], affine=a12)

    legs = {"plain_case": plain_case, "affine_case": affine_case,
            "plain_linear": lambda s: data.resample_device(s[0][0], TARGET, out=s[2][0]),
            "affine_linear": lambda s: data.resample_device(s[0][0], TARGET, out=s[2][0], affine=a12, gain=gains[0],
                                                            bias=biases[0]),
            "plain_label": lambda s: data.resample_device(s[1], TARGET, nearest=True, out=s[3][0]),
            "affine_label": lambda s: data.resample_device(s[1], TARGET, nearest=True, out=s[3][0], affine=a12)}
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
    affine_case(s)
    torch.cuda.synchronize()
    inside = float((s[2][0] != 0).float().mean())  # int16 draws in [0, 4000): a zero is (almost surely) outside
    return times, inside


def step_time(device, warmup, steps):
    """Median HIP-event time of one training step (bf16 build, batch 2 of 5x128x128x64 resident on the GPU)."""
    from pcms_amd.synthetic import make_batch
    from pcms_amd.utils.trainer import Trainer
    torch.manual_seed(0)
    tr = Trainer({"device": str(device), "learning_rate": 1e-4, "batch_size": 2, "num_epochs": 1, "loss": "bce_dice",
                  "precision": "bf16"})
    batches = []
    for i in range(2):
        b = make_batch(2, TARGET, seed=100 + i)
        batches.append({"image": b["image"].to(device), "label": b["label"].to(device), "case_id": b["case_id"]})
    for i in range(warmup):
        tr.step_async(batches[i % 2])
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    for i in range(steps):
        tr.step_async(batches[i % 2])
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import data
    device = torch.device("cuda", 0)
    times, inside = kernel_times(data, device, a.reps, a.iters)
    steps = step_time(device, a.warmup, a.steps)
    times2, _ = kernel_times(data, device, a.reps, a.iters)  # again after the steps: clocks and caches as in training
    best = {k: min(times[k] + times2[k]) for k in times}
    step_us = statistics.median(steps)
    out = {"device": torch.cuda.get_device_name(0), "raw_shape": list(RAW_SHAPE), "raw_dtype": "int16 (label uint8)",
           "target_size": list(TARGET), "launches_per_case": 6,
           "transform": {"rotate_deg": ROTATE_DEG, "zoom": ZOOM, "flips": FLIPS, "shift_voxels": SHIFT,
                         "gain_bias": "per modality, not identity", "inside_share": inside},
           "method": "HIP events, 3 rotating buffer sets, warm-up, plain and affine legs alternating rep by rep, "
                     f"min of 2 x {a.reps} x {a.iters} (before and after the timed steps); launches issued back to "
                     "back from Python, so launch gaps are in the figures; step: median of "
                     f"{a.steps} event-timed Trainer.step_async after {a.warmup} warm-up steps, bf16, batch 2",
           "plain_per_case_us": best["plain_case"], "affine_per_case_us": best["affine_case"],
           "affine_over_plain_case": best["affine_case"] / best["plain_case"],
           "plain_linear_launch_us": best["plain_linear"], "affine_linear_launch_us": best["affine_linear"],
           "plain_label_launch_us": best["plain_label"], "affine_label_launch_us": best["affine_label"],
           "all_us": {k: times[k] + times2[k] for k in times},
           "step_us_batch2": step_us, "step_us_per_case": step_us / 2, "step_us_all": steps,
           "affine_case_over_step_case": best["affine_case"] / (step_us / 2)}
    out["hidden_by_prefetch"] = bool(best["affine_case"] < step_us / 2)
    if not out["hidden_by_prefetch"]:
        out["why_not_hidden"] = "the six augmenting launches of a case take longer than the case's share of a step"
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
