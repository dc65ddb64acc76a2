"""Benchmark: train volumes/s of the 5-channel 3D U-Net (128x128x64, batch 2 per GPU,
BCEDiceLoss, Adam) on MI355X — SURVEY.md §8(d), BASELINE.json config 2 (N=1) / config 3
(N=8, launched by torch.distributed.run, one process per GPU, RCCL all-reduce).

One "step" = Trainer.step on a synthetic batch held in pinned host memory: the H2D copy
(issued one batch ahead on the trainer's copy stream, SURVEY §8d's unit of work) + forward +
loss + backward + (all-reduce) + Adam.  The K timed steps run back to back between a barrier +
device synchronize on both sides; per-step times are HIP events recorded on the compute
stream at every step boundary, max over ranks, and ``value`` uses their MEDIAN (the wall time
of the K steps is reported beside it).  Prints ONE JSON line (rank 0).

A plain run sets up, warms up, times the K steps and prints the line (``roofline``,
``cpu_baseline``, ``fp32_parity_build_value`` and ``clock`` are null).  ``--dump-outputs DIR``
also writes what the last timed step left (the loss it returned, the parameters, gradients and
BatchNorm buffers it updated) as ``DIR/<name>.npy``.  ``--full`` adds the other legs: the
shader clock over the timed steps and the roofline of the stem conv
(forward + weight-gradient kernels, HBM-bound: ``frac`` on BASELINE.md's 578.9 MB at N=2,
``frac_fused`` on the 847.3 MB the product's kernels move with the stem's BatchNorm-backward
apply fused into the weight gradient), their launch
durations measured with HIP events on the launch stream inside the timed steps, the fp32
parity build's rate, and the CPU oracle timed on the host cores
(rank 0, N=1 only: 1 warm-up + 3 timed steps at the config batch, median).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E (MI355X_MICROARCH.md)
MFMA_BF16_PEAK = 2.5e15    # dense bf16 FLOP/s
FLOP_PER_VOL = 5.72e12     # conv fwd+dgrad+wgrad per 5x128x128x64 volume


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2, help="volumes per GPU")
    ap.add_argument("--size", type=str, default="128,128,64")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--zero-fill", action="store_true", help="config 4: 1-2 modalities zeroed")
    ap.add_argument("--ckpt-decoder", action="store_true", help="config 5: decoder activation checkpointing")
    ap.add_argument("--fp32-steps", type=int, default=5, help="timed steps of the fp32 parity build (0: skip)")
    ap.add_argument("--full", action="store_true",
                    help="also measure the stem roofline (HIP events inside the timed steps) and the shader "
                         "clock, the fp32 parity build (--fp32-steps) and the CPU oracle baseline "
                         "(unless --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (loss, parameters, gradients, "
                         "BatchNorm buffers) as DIR/<name>.npy (float32; a fixed seeded sample of a large array)")
    ap.add_argument("--plumbing", action="store_true",
                    help="launcher check only (CPU, gloo): every rank joins the group, rank 0 prints the "
                         "world size it saw; no GPU work, no measurement")
    return ap.parse_args()


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(a) -> int:
    """``--gpus N`` (N > 1) run as a plain ``python bench.py``: relaunch this script as N
    ranks (one process per GPU, LOCAL_RANK = GPU index) through torch.distributed.run on
    127.0.0.1, wait for them and return their exit status.  Called before this process
    touches the GPU (the children initialise HIP; the parent never does)."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this host driver
    return subprocess.call(cmd, env=env)


def plumbing(a, world, rank):
    """The launcher path without a GPU: each rank joins a gloo group and contributes 1 to
    an all-reduce; rank 0 prints the rank count it saw."""
    dist.init_process_group("gloo")
    seen = torch.ones(1)
    dist.all_reduce(seen)
    if rank == 0:
        print(json.dumps({"plumbing": True, "n_gpus": world, "ranks_seen": int(seen.item()),
                          "requested": a.gpus, "backend": dist.get_backend()}), flush=True)
    dist.destroy_process_group()


def stem_roofline(tr, N, spatial, reps, in_step=None):
    """Roofline of the stem conv (5->64, k3) forward + weight-gradient kernels.  ``in_step``:
    their average launch durations (s) measured with HIP events on the launch stream inside
    the timed training steps (the engine's ``kernel_timer``) -- what is reported.  Without
    them (a shape or build the stem kernels do not run), separate back-to-back launches on
    rotating buffer sets are timed instead."""
    from pcms_amd import _lib as L
    eng = tr.model.engine()
    code = eng.code
    D, H, W = spatial
    nvox = N * D * H * W
    cs = eng.convs[0]
    T = eng.tdtype
    sets = []
    for i in range(0 if in_step and len(in_step) == 2 else 3):
        xin = torch.rand(nvox * eng.cp, device="cuda").to(T)
        y = torch.empty(nvox * 64, dtype=T, device="cuda")
        dy = torch.randn(nvox * 64, device="cuda").to(T)
        sets.append((xin, y, dy))
    rows = L.query("pcms_conv3_mblocks", N, D, H, W)
    stats = torch.empty(rows * (64 * 2 + 1), device="cuda")
    dw = torch.zeros(64 * 5 * 27, device="cuda")
    dwt = torch.empty(max(L.query("pcms_conv3_wgrad_ws_floats", code, N, D, H, W, eng.cp, 0, 64, 512),
                          L.query("pcms_stem_wgrad_ws_floats", N, D, H, W, 5)), device="cuda")

    eng._ensure_packs()

    sup = L.query("pcms_stem_supported", N, D, H, W) if eng.stem_fast else 0

    def fwd(s):
        if sup & 1:
            L.call("pcms_stem_fwd", s[0], eng.stem_pack, cs.mod.bias, s[1], stats, N, D, H, W, eng.stem_dense)
        else:
            L.call("pcms_conv3_fwd", code, s[0], eng.cp, None, 0, cs.fwd, cs.mod.bias, s[1], None, 64, None,
                   stats, 0, N, D, H, W, 64, 1)

    bn = eng.enc[0].b0
    coef = torch.zeros(3 * 64, device="cuda")

    def wgrad(s):
        if sup & 2:  # the product path: the stem's BN0 backward apply fused in (y = s[1])
            L.call("pcms_stem_wgrad_bn", s[0], s[2], s[1], bn.scale, bn.shift, bn.mean, bn.invstd, coef, dw, dwt, 5,
                   N, D, H, W)
        else:
            L.call("pcms_conv3_wgrad", code, s[0], eng.cp, None, 0, s[2], dw, dwt, N, D, H, W, 64, 5, 512, 0)

    res = dict(in_step) if in_step else {}
    for name, fn in (("fwd", fwd), ("wgrad", wgrad)):
        if name in res:
            continue
        for i in range(reps):  # warm-up: one untimed batch of launches
            fn(sets[i % 3])
        torch.cuda.synchronize()
        trials = []
        for _ in range(3):  # median of 3 averages of `reps` back-to-back launches
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for i in range(reps):
                fn(sets[i % 3])
            ev1.record()
            ev1.synchronize()
            trials.append(ev0.elapsed_time(ev1) / reps * 1e-3)  # s per launch
        res[name] = statistics.median(trials)
    es = 2 if code == 1 else 4
    # algorithmic bytes: X (5 ch) + W + Y  /  X + dY + dW; with the stem's
    # BatchNorm + ReLU backward apply fused into its weight gradient (pcms_stem_wgrad_bn) the
    # backward reads dA (the ReLU output's gradient) and Y (pre-BN) instead of dY
    xb = nvox * 5 * es
    yb = nvox * 64 * es
    fused = bool(sup & 2)
    fwd_bytes = xb + 64 * 5 * 27 * es + yb
    wg_bytes = xb + (2 if fused else 1) * yb + 64 * 5 * 27 * 4
    t = res["fwd"] + res["wgrad"]
    # the headline follows BASELINE.md / SURVEY §8(d): the conv alone, X + W + Y / X + dY + dW
    # = 578.9 MB at N=2, achieved = 578.9e6 / t / 8e12
    s8d_bytes = fwd_bytes + xb + yb + 64 * 5 * 27 * 4
    achieved = s8d_bytes / t
    # the bytes the product's fused kernels must move over the same t (the stem's BN-backward
    # apply fused into its weight gradient reads dA and the pre-BN Y: 847.3 MB at N=2)
    fused_bytes = fwd_bytes + wg_bytes
    # HBM bytes per fwd+wgrad pair from the PMC counters (FETCH_SIZE / WRITE_SIZE in separate
    # rocprofv3 passes, gfx950 FETCH correction: tests/kexp/pmc_stem_traffic.sh), committed
    # for the shape they were measured on; null for any other shape
    traffic = None
    fk = "stem_fwd_direct_kernel<DENSE>" if eng.stem_dense else "stem_fwd_direct_kernel"
    kernel = (f"stem conv3d 5->64 fwd + wgrad with the BN0 backward apply fused in ({fk} + "
              "stem_wgrad_stream_kernel<BN>)" if fused else
              f"stem conv3d 5->64 fwd + wgrad ({fk} + stem_wgrad_stream_kernel)")
    tf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r6_stem_traffic.json")
    if os.path.exists(tf):
        with open(tf) as f:
            rec = json.load(f)
        if rec.get("shape") == [N, D, H, W] and code == 1 and rec.get("kernel") == kernel:
            traffic = rec["traffic_bytes_per_pair"]
    return {"bound": "hbm", "achieved": round(achieved / 1e9, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK, 4), "traffic": traffic,
            "kernel": kernel,
            "algorithmic_bytes": s8d_bytes,
            "frac_fused": round(fused_bytes / t / HBM_PEAK, 4), "achieved_fused": round(fused_bytes / t / 1e9, 1),
            "algorithmic_bytes_fused": fused_bytes,
            "t_fwd_us": round(res["fwd"] * 1e6, 1),
            "t_wgrad_us": round(res["wgrad"] * 1e6, 1),
            "timing": "HIP events around each launch inside the timed steps" if in_step else
                      f"{reps} back-to-back launches, median of 3"}


class ClockProbe:
    """Shader clock over a stretch of device work (pcms_clock_probe): a stamp is one tiny
    launch of single-wave workgroups that record (s_memtime, s_memrealtime, CU location);
    between two stamps a CU's average clock is d(memtime) / d(memrealtime) x 100 MHz.  The
    cycle counters of different CUs carry different offsets, so only stamps written by the
    same CU are paired (1024 workgroups per stamp: every CU appears in both).  Stamps are
    enqueued on the current stream, outside the per-step events."""

    def __init__(self, nblocks: int = 1024):
        self.nblocks = nblocks

    def stamp(self):
        from pcms_amd import _lib as L
        buf = torch.zeros(3 * self.nblocks, dtype=torch.int64, device="cuda")
        # the raw entry point (tools may wrap _lib.call to time every library call)
        rc = L.load().pcms_clock_probe(buf.data_ptr(), self.nblocks, L.stream())
        if rc != 0:
            raise L.HipError(f"pcms_clock_probe failed with status {rc}")
        return buf

    @staticmethod
    def mhz(a, b):
        """Per-XCD clock (MHz) between stamps a and b: the median over that XCD's CUs seen in
        both stamps (first stamp of a CU in a, last in b)."""
        first, last = {}, {}
        for t, r, loc in a.view(-1, 3).cpu().tolist():
            if loc not in first or r < first[loc][1]:
                first[loc] = (t, r)
        for t, r, loc in b.view(-1, 3).cpu().tolist():
            if loc not in last or r > last[loc][1]:
                last[loc] = (t, r)
        per = {}
        for loc, (ta, ra) in first.items():
            if loc in last and last[loc][1] > ra:
                tb, rb = last[loc]
                per.setdefault(int(loc) & 0xff, []).append((tb - ta) / (rb - ra) * 100.0)
        return {x: round(statistics.median(v), 1) for x, v in sorted(per.items())}

    @staticmethod
    def summary(per):
        vals = list(per.values())
        if not vals:
            return None
        return {"sclk_mhz": round(statistics.median(vals), 1), "sclk_mhz_min": min(vals), "sclk_mhz_max": max(vals),
                "per_xcd": per}


def stem_clock(tr, N, spatial, reps=30):
    """The shader clock over `reps` back-to-back launches of each stem kernel (the product's
    calls, on the training buffers, after the timed steps): the figure the stem roofline can
    be normalised with.  Returns {"fwd": {...}, "wgrad": {...}} or None."""
    from pcms_amd import _lib as L
    eng = tr.model.engine()
    if not (eng.stem_sup & 3) == 3 or eng.bufs is None:
        return None
    b = eng.bufs
    D, H, W = spatial
    cs = eng.convs[0]
    bn = eng.enc[0].b0
    dw = torch.zeros(64 * 5 * 27, device="cuda")
    calls = {
        "fwd": lambda: L.call("pcms_stem_fwd", b["xin"], eng.stem_pack, cs.mod.bias, b["e0_y1"], b["stats"], N, D, H,
                              W, eng.stem_dense),
        "wgrad": lambda: L.call("pcms_stem_wgrad_bn", b["xin"], b["gA0"], b["e0_y1"], bn.scale, bn.shift, bn.mean,
                                bn.invstd, b["coef"], dw, b["dwt"], 5, N, D, H, W),
    }
    probe = ClockProbe()
    out = {}
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a = probe.stamp()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        z = probe.stamp()
        torch.cuda.synchronize()
        s = ClockProbe.summary(ClockProbe.mhz(a, z)) or {}
        s.pop("per_xcd", None)
        s["us_per_launch"] = round(e0.elapsed_time(e1) / reps * 1e3, 1)
        out[name] = s
    return out


def cpu_baseline(n, spatial):
    """The CPU oracle (a restatement of utils/trainer.py:179-195 on torch CPU fp32) timed on
    this host at the config batch: 1 warm-up + 3 timed BCEDice train steps, median."""
    from oracle import unet3d_cpu as ref
    from pcms_amd.synthetic import make_batch, step_seed
    # every core this process may run on (torch.set_num_threads(len(affinity))),
    # capped only by a cgroup CPU quota if one is set (threads beyond it would only time-slice)
    affinity = max(1, len(os.sched_getaffinity(0)))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()[:2]
            if q != "max":
                quota = max(1, math.ceil(int(q) / int(period)))
    except (OSError, ValueError):
        pass
    cores = min(affinity, quota) if quota else affinity
    torch.set_num_threads(cores)
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    torch.manual_seed(0)
    sd = ref.init_params(5, 1)
    step = ref.RefStep(sd, lr=1e-4, loss="bce_dice")
    times = []
    for i in range(4):
        b = make_batch(n, spatial, seed=step_seed(0, i))
        t0 = time.perf_counter()
        step.step(b["image"], b["label"])
        times.append(time.perf_counter() - t0)
    med = statistics.median(times[1:])
    return {"value": round(n / med, 4), "unit": "volumes/s", "cores": cores, "kind": "port", "cpu_model": model,
            "threads": torch.get_num_threads(), "affinity_cpus": affinity, "cgroup_cpu_quota": quota,
            "sample": f"1 warm-up + 3 timed train steps (fwd+BCEDice+bwd+Adam), batch {n} x "
                      f"5x{'x'.join(map(str, spatial))}, torch CPU fp32, median {med:.1f} s/step"}


def _pinned_batches(n, spatial, rank, count, zero_fill):
    from pcms_amd.synthetic import make_batch, step_seed
    out = []
    for i in range(count):
        b = make_batch(n, spatial, seed=step_seed(rank, i), zero_fill=zero_fill)
        out.append({"image": b["image"].pin_memory(), "label": b["label"].pin_memory(), "case_id": b["case_id"]})
    return out


def timed_steps(tr, host_batches, warmup, steps, world, clock=True):
    """K steps back to back, bracketed by a barrier + device synchronize on both sides (the
    host enqueues ahead of the GPU, as a training loop without per-step host syncs does).
    Per-step times come from HIP events recorded on the compute stream at every step
    boundary; returns (per-step seconds, max over ranks), the wall time of the K steps, and
    the last loss, and the shader clock over the K steps (ClockProbe.summary, this rank;
    None without ``clock``)."""
    def loader():
        while True:
            yield from host_batches
    it = tr._prefetched(loader())
    for _ in range(warmup):
        tr.step_async(next(it))
    torch.cuda.synchronize()
    timer = tr.model.engine().kernel_timer
    if timer is not None:
        timer.clear()  # only the timed steps' launches count
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    probe = ClockProbe() if clock else None
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # shader clock over the K steps: a stamp on each side, outside the step events
    ck0 = probe.stamp() if probe else None
    evs[0].record()
    last = None
    for i in range(steps):
        last = tr.step_async(next(it))
        evs[i + 1].record()
    ck1 = probe.stamp() if probe else None
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    ts = [evs[i].elapsed_time(evs[i + 1]) * 1e-3 for i in range(steps)]
    tt = torch.tensor(ts + [wall], device="cuda", dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    tt = tt.cpu().tolist()
    return tt[:-1], tt[-1], last, ClockProbe.summary(ClockProbe.mhz(ck0, ck1)) if probe else None


DUMP_MAX_ELEMS = 4 << 20   # per array: 16 MB as float32, four arrays stay well under 64 MB


def dump_outputs(dirname, tr, loss):
    """What the last timed step computed, as ``dirname/<name>.npy`` (float32): the loss
    Trainer.step_async returned and the state it left behind -- the flat parameters after
    Adam, the flat gradient of that step and the BatchNorm running buffers.  An array above
    DUMP_MAX_ELEMS is sampled at indices drawn once from a generator seeded by its length,
    so two builds run with the same arguments write the same elements."""
    import numpy as np
    eng = tr.model.engine()
    os.makedirs(dirname, exist_ok=True)
    torch.cuda.synchronize()
    arrays = (("loss", loss.reshape(1)), ("params", eng.flat_p), ("grads", eng.flat_g),
              ("bn_buffers", eng.flat_bn))
    for name, t in arrays:
        t = t.detach().reshape(-1).float().cpu()
        if t.numel() > DUMP_MAX_ELEMS:
            g = torch.Generator().manual_seed(t.numel())
            t = t[torch.randint(t.numel(), (DUMP_MAX_ELEMS,), generator=g).sort().values]
        np.save(os.path.join(dirname, name + ".npy"), t.numpy())


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}", file=sys.stderr, flush=True)
        sys.exit(2)
    if a.plumbing:
        return plumbing(a, world, rank)
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        if dist.get_world_size() != a.gpus:
            print(f"bench.py: RCCL group has {dist.get_world_size()} ranks, --gpus {a.gpus}", file=sys.stderr)
            sys.exit(2)
    import pcms_amd  # noqa: F401
    from pcms_amd.utils.trainer import Trainer

    spatial = tuple(int(v) for v in a.size.split(","))
    torch.manual_seed(0)
    cfg = {"device": f"cuda:{local}", "learning_rate": 1e-4, "batch_size": a.batch, "num_epochs": 1,
           "loss": "bce_dice", "precision": a.precision, "checkpoint_decoder": a.ckpt_decoder}
    tr = Trainer(cfg)
    host = _pinned_batches(a.batch, spatial, rank, 2, a.zero_fill)
    if a.full:
        tr.model.engine().kernel_timer = {}
    dp_info = None
    if world > 1:
        sync = tr._grad_sync()[1]
        sync.exposed_events = []
    ts, wall, last, clock = timed_steps(tr, host, a.warmup, a.steps, world, clock=a.full)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, tr, last)
    timer = tr.model.engine().kernel_timer or {}
    tr.model.engine().kernel_timer = None
    if world > 1:
        # the all-reduce time the backward did not hide: HIP events on the compute stream
        # around GradSync.finish()'s waits, the timed steps only (the last `steps` pairs)
        if tr._grad_sync()[1] is not sync:  # re-flattened during the warm-up: no record
            sync.exposed_events = []
        evs = sync.exposed_events[-a.steps:]
        sync.exposed_events = None
        exp = [e0.elapsed_time(e1) for e0, e1 in evs]
        et = torch.tensor([statistics.mean(exp) if exp else 0.0, max(exp) if exp else 0.0],
                          device="cuda", dtype=torch.float64)
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        dp_info = {"allreduce_ms_exposed": round(float(et[0]), 3), "allreduce_ms_exposed_max": round(float(et[1]), 3),
                   "buckets_mb": [round((hi - lo) * 4 / 2**20, 1) for lo, hi in sync.launched],
                   "bucket_order": "backward order (decoder first, stem last); each launched async as the backward "
                                   "finishes its modules, the rest waited for before Adam",
                   "grad_mb": round(tr.model.engine().flat_g.numel() * 4 / 2**20, 1)}
    in_step = {}
    for key, name in (("fwd", "stem_fwd"), ("wgrad", "stem_wgrad")):
        evs = timer.get(name, [])
        if evs:
            in_step[key] = statistics.mean(e0.elapsed_time(e1) for e0, e1 in evs) * 1e-3
    loss = float(last) if last is not None else float("nan")
    med = statistics.median(ts)
    vols_step = world * a.batch
    value = vols_step / med
    roof = stem_roofline(tr, a.batch, spatial, a.kernel_reps, in_step if len(in_step) == 2 else None) \
        if a.full and rank == 0 else None
    if roof is not None and rank == 0:
        roof["clock_standalone"] = stem_clock(tr, a.batch, spatial)
    # the fp32 parity build (the one that meets the 1e-3 logit bar) on the same batches
    fp32 = None
    if a.full and a.fp32_steps > 0 and a.precision != "fp32":
        del tr
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        tr32 = Trainer(dict(cfg, precision="fp32"))
        ts32, _, _, _ = timed_steps(tr32, host, 2, a.fp32_steps, world)
        fp32 = round(vols_step / statistics.median(ts32), 3)
        del tr32
    cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline(a.batch, spatial)
    if rank == 0:
        vox = spatial[0] * spatial[1] * spatial[2]
        flops = FLOP_PER_VOL * vox / (128 * 128 * 64) * vols_step
        size = "x".join(map(str, spatial))
        out = {
            "metric": f"train volumes/sec (5ch {size})", "value": round(value, 3), "unit": "volumes/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(med * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.precision,
            "data": "synthetic (U[0,1) images, ellipsoid labels; random-init weights, seed 0), pinned host "
                    "batches copied H2D inside each step (prefetched one step ahead)",
            "config": {"workload": f"UNet3D 5->1, {a.batch} x 5x{size} per GPU, "
                                   f"BCEDiceLoss, Adam(1e-4, wd 1e-5){', zero_fill' if a.zero_fill else ''}"
                                   f"{', decoder checkpointing' if a.ckpt_decoder else ''}",
                       "global_batch": vols_step, "parallelism": f"dp{world}"},
            "roofline": roof, "cpu_baseline": cpu,
            "mfma_util_step": round(flops / med / MFMA_BF16_PEAK, 4), "final_loss": round(loss, 5),
            "step_ms": {"median": round(med * 1e3, 3), "mean": round(statistics.mean(ts) * 1e3, 3),
                        "min": round(min(ts) * 1e3, 3), "max": round(max(ts) * 1e3, 3),
                        "wall_per_step": round(wall / a.steps * 1e3, 3),
                        "timing": "HIP events on the compute stream at every step boundary, K steps "
                                  "back to back between a barrier + synchronize on both sides"},
            "fp32_parity_build_value": fp32,
            # the shader clock the XCDs held over the K timed steps (pcms_clock_probe stamps
            # on both sides of them; rank 0): normalises the line against other boxes
            "clock": clock,
        }
        if dp_info is not None:
            out["dp"] = dp_info
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
