"""Time of ``SoftmaxDiceCELoss`` forward + backward against the same loss composed from torch ops
on the same device, and against the bytes it has to move.

    python tests/bench_classes.py [--shape 2 3 128 128 64] [--iters 200] [--out profiles/classes_time.json]

The two forms alternate in blocks of ``--iters`` calls, five blocks each, timed by device events;
the figure is the median block.  Bytes: the C logit planes and the label are read by the forward
and again by the backward, the C gradient planes are written once."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_loss(x, t, ce_weight=0.5, dice_weight=0.5, smooth=1.0):
    """The definition with torch ops (no ignored voxels in the timed input): F.cross_entropy plus
    the Dice of softmax and one-hot sums over the batch, foreground classes."""
    y = t[:, 0].long()
    p = torch.softmax(x, dim=1)
    onehot = F.one_hot(y, x.shape[1]).permute(0, 4, 1, 2, 3).to(p.dtype)
    dims = (0, 2, 3, 4)
    dice = (2.0 * (p * onehot).sum(dims) + smooth) / (p.sum(dims) + onehot.sum(dims) + smooth)
    return ce_weight * F.cross_entropy(x, y) + dice_weight * (1.0 - dice[1:]).mean()


def block(fn, x, t, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        x.grad = None
        fn(x, t).backward()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # microseconds per forward + backward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[2, 3, 128, 128, 64])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd.utils.losses import SoftmaxDiceCELoss
    assert torch.cuda.is_available(), "bench_classes needs a ROCm GPU"
    N, C = a.shape[:2]
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(*a.shape, generator=g) * 3).cuda().requires_grad_(True)
    t = torch.randint(0, C, (N, 1) + tuple(a.shape[2:]), generator=g).float().cuda()
    ours = SoftmaxDiceCELoss()
    l0, l1 = ours(x, t).item(), torch_loss(x, t).item()
    assert abs(l0 - l1) <= 1e-5 * max(1.0, abs(l1)), (l0, l1)
    for fn in (ours, torch_loss):  # warm-up: code objects, the allocator's blocks
        block(fn, x, t, 20)
    times = {"hip": [], "torch": []}
    for _ in range(5):
        times["hip"].append(block(ours, x, t, a.iters))
        times["torch"].append(block(torch_loss, x, t, a.iters))
    voxels = t.numel()
    moved = (2 * (C + 1) + C) * 4 * voxels
    hip, ref = statistics.median(times["hip"]), statistics.median(times["torch"])
    result = {"shape": a.shape, "iters": a.iters, "loss_hip": l0, "loss_torch": l1,
              "hip_us": hip, "torch_us": ref, "hip_us_blocks": times["hip"], "torch_us_blocks": times["torch"],
              "speedup": ref / hip, "bytes_moved": moved, "hip_TBps": moved / (hip * 1e-6) / 1e12,
              "note": "forward + backward per call, device events around blocks of calls (autograd and launch "
                      "overhead included); bytes: C logit planes and the fp32 label read twice, C planes written once"}
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
