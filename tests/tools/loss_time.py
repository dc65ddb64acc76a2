"""Forward + backward time of the losses at the flagship logits shape (test tooling, not a test):
logits (2, 1, 64, 128, 128) fp32, targets Bernoulli(0.1), one process, one GPU.

Timed forms, interleaved in every window so that clock and neighbour drift hits all alike:
  * ``bce_dice``            BCEDiceLoss, the existing path (pcms_loss_fwd / _bwd);
  * ``tversky``             TverskyLoss(): region term only, no power, no voxel term;
  * ``tversky_per_sample``  the same with per_sample=True (groups = N * C);
  * ``focal_tversky_focal`` FocalTverskyFocalLoss(per_sample=True): both terms, both powers.

Two legs:
  * ``kernels``: the C entry points on preallocated buffers (two launches forward, one backward),
    HIP events around --iters forward + backward pairs over 3 rotating input sets;
  * ``module``: the ``nn.Module`` call + ``backward()`` through autograd (allocations and the
    Python side included), the same way.
Each figure is the median of --reps windows after a warm-up window of every form; the ratio of each
new form to ``bce_dice`` is taken per window and its median recorded.

Writes profiles/loss_time.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests.tools.loader_time import cpu_model  # noqa: E402

SHAPE = (2, 1, 64, 128, 128)


def window(fn, sets, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def measure(forms, sets, reps, iters):
    for fn in forms.values():  # warm-up: code objects, the allocator's blocks
        window(fn, sets, iters)
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            us[k].append(window(fn, sets, iters))
    out = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "all_us": v} for k, v in us.items()}
    for k in forms:
        if k != "bce_dice":
            out[k]["ratio_to_bce_dice"] = statistics.median(a / b for a, b in zip(us[k], us["bce_dice"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loss_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    from pcms_amd.utils import losses
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    M = 1
    for s in SHAPE:
        M *= s
    sets = []
    for _ in range(3):
        x = (torch.randn(SHAPE, generator=g) * 3).to(dev)
        t = (torch.rand(SHAPE, generator=g) < 0.1).float().to(dev)
        sets.append({"x": x, "t": t, "dx": torch.empty_like(x), "xg": x.clone().requires_grad_(True)})
    one = torch.ones((), device=dev)

    def region_form(groups, alpha, beta, gamma, smooth, fg, use_fa, fa, wr, wv):
        nvox = M // groups
        rows = L.query("pcms_region_loss_rows", nvox, groups)
        part = torch.empty(groups * rows * 4, device=dev)
        sums = torch.empty(groups * 4, dtype=torch.float64, device=dev)
        coef, loss = torch.empty(groups * 2, device=dev), torch.empty((), device=dev)

        def fn(s):
            L.call("pcms_region_loss_fwd", s["x"], s["t"], nvox, groups, alpha, beta, gamma, smooth, fg, use_fa, fa, wr, wv,
                   part, sums, coef, loss)
            L.call("pcms_region_loss_bwd", s["x"], s["t"], nvox, groups, fg, use_fa, fa, wv, coef, one, s["dx"])
        return fn

    rows = L.query("pcms_loss_rows", M)
    part = torch.empty(rows * 4, device=dev)
    sums, loss = torch.empty(4, dtype=torch.float64, device=dev), torch.empty((), device=dev)

    def bce_dice(s):
        L.call("pcms_loss_fwd", s["x"], s["t"], M, 1.0, 0.5, 0.5, part, sums, loss)
        L.call("pcms_loss_bwd", s["x"], s["t"], M, sums, 1.0, 0.5, 0.5, one, s["dx"])

    groups = SHAPE[0] * SHAPE[1]
    kernels = {"bce_dice": bce_dice,
               "tversky": region_form(1, 0.3, 0.7, 1.0, 1.0, 0.0, 0, 0.0, 1.0, 0.0),
               "tversky_per_sample": region_form(groups, 0.3, 0.7, 1.0, 1.0, 0.0, 0, 0.0, 1.0, 0.0),
               "focal_tversky_focal": region_form(groups, 0.3, 0.7, 0.75, 1.0, 2.0, 1, 0.25, 0.5, 0.5)}

    def module_form(crit):
        def fn(s):
            s["xg"].grad = None
            crit(s["xg"], s["t"]).backward()
        return fn

    modules = {"bce_dice": module_form(losses.BCEDiceLoss()), "tversky": module_form(losses.TverskyLoss()),
               "tversky_per_sample": module_form(losses.TverskyLoss(per_sample=True)),
               "focal_tversky_focal": module_form(losses.FocalTverskyFocalLoss(per_sample=True))}
    out = {"device": torch.cuda.get_device_name(0), "host_cpu": cpu_model(), "logits_shape": list(SHAPE),
           "bytes_moved_per_pair": 5 * 4 * M,  # x and t read twice, dx written once: the same for every form
           "method": f"HIP events around {a.iters} forward + backward pairs over 3 rotating input sets (72 MB in all: "
                     f"inside the Infinity Cache, as the logits are in the step); forms interleaved; one warm-up "
                     f"window each; median of {a.reps} windows; ratio_to_bce_dice: the median of the per-window ratios"}
    out["kernels"] = measure(kernels, sets, a.reps, a.iters)
    print(json.dumps({k: v["median_us"] for k, v in out["kernels"].items()}), flush=True)
    out["module"] = measure(modules, sets, a.reps, a.iters)
    print(json.dumps({k: v["median_us"] for k, v in out["module"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
