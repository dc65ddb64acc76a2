"""pcms_joint_histogram and a whole register_case_device, timed in one process (test tooling, not
a test).  A synthetic case of sums of Gaussians defined in world millimetres over a
zero background: three T2 series at 24x384x384 (3 x 0.5 x 0.5 mm, int16) and a diffusion pair at
20x128x128 (3.6 x 1.5 x 1.5 mm, int16, a smaller field of view, another contrast, a true motion
of (1.5, -2.0, 1.0) mm and 3 degrees about z).

  * one histogram evaluation, fixed 24x384x384 against moving 20x128x128 at 32 bins, stride
    (1, 1, 1) and (1, 2, 2): stream-ordered times, HIP events around windows of --iters calls over
    3 rotating buffer sets after a warm-up, median of --reps windows, the two strides alternating
    window by window; beside each the bytes the evaluation has to fetch (the fixed rows the
    lattice touches -- a stride along W still fetches the whole row -- plus the moving volume
    once) and that count over the measured HBM copy rate (6.29 TB/s);
  * register_case_device of the written case: host wall time around the call, files to result,
    ending in the last table read back, median of --case-reps runs after one warm-up run.

The first table is compared with predict.joint_histogram on the counts.  Writes
profiles/align_time.json (--out)."""
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

FIX_SHAPE, FIX_SPACING = (24, 384, 384), (3.0, 0.5, 0.5)
MOV_SHAPE, MOV_SPACING = (20, 128, 128), (3.6, 1.5, 1.5)
TRUE_MOTION = (1.5, -2.0, 1.0, 3.0, 0.0, 0.0)
COPY_RATE = 6.29e12  # bytes / s, the measured float4 copy


def geometry(spacing_zyx, origin_xyz):
    sx, sy, sz = spacing_zyx[::-1]
    return {"pixdim": (1.0, sx, sy, sz), "xyzt_units": 2, "qform_code": 0, "sform_code": 1, "quatern_b": 0.0,
            "quatern_c": 0.0, "quatern_d": 0.0, "qoffset_x": 0.0, "qoffset_y": 0.0, "qoffset_z": 0.0,
            "srow_x": (sx, 0.0, 0.0, origin_xyz[0]), "srow_y": (0.0, sy, 0.0, origin_xyz[1]),
            "srow_z": (0.0, 0.0, sz, origin_xyz[2])}


def make_case(root, data):
    """The five files of the case and their geometries; the volumes as int16 in 0..3000."""
    gf, gm = geometry(FIX_SPACING, (-96.0, -96.0, -36.0)), geometry(MOV_SPACING, (-94.0, -97.0, -34.0))
    rng = np.random.default_rng(5)
    centres = rng.uniform((-60, -60, -25), (60, 60, 25), size=(9, 3))
    sigmas, amps = rng.uniform(8.0, 25.0, size=9), rng.uniform(0.4, 1.0, size=9)

    def value(xyz):
        v = np.zeros(xyz.shape[:-1])
        for a, c, s in zip(amps, centres, sigmas):
            v += a * np.exp(-((xyz - c) ** 2).sum(axis=-1) / (2.0 * s * s))
        return np.clip(v, 0.0, 1.0)

    def points(geo, shape):
        w = data.world_matrix(geo)
        z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
        return np.stack([x, y, z, np.ones_like(x)], axis=-1) @ w.T

    body = value(points(gf, FIX_SHAPE)[..., :3])
    body[body < 0.15] = 0.0                                   # air: most of an MR volume is one value
    T = data.rigid_world(TRUE_MOTION, data.world_centre(gf, FIX_SHAPE))
    seen = value((points(gm, MOV_SHAPE) @ np.linalg.inv(T).T)[..., :3])
    seen[seen < 0.15] = 0.0
    vols = {"gaoqing-T2": (3000.0 * body, gf), "T2 fs": (3000.0 * np.sqrt(body), gf), "T2 not fs": (2500.0 * body ** 2, gf),
            "DWI": (3000.0 * np.where(seen > 0, (1.0 - seen) ** 2 + 0.05, 0.0), gm), "ADC": (2800.0 * seen, gm)}
    for m, (v, g) in vols.items():
        os.makedirs(os.path.join(root, m))
        data.write_nifti(os.path.join(root, m, "img.nii"), v.astype(np.int16), geometry=g)
    return {m: v.astype(np.int16) for m, (v, g) in vols.items()}, gf, gm


def window_us(fn, sets, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "align_time.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--case-reps", type=int, default=3)
    a = ap.parse_args()
    import pcms_amd  # noqa: F401
    from pcms_amd import align, data, intensity, predict
    device = torch.device("cuda", 0)
    root = tempfile.mkdtemp(prefix="align_time_")
    vols, gf, gm = make_case(root, data)
    fix, mov = vols["gaoqing-T2"], vols["DWI"]
    A, t = data.align_affine(gf, gm)
    bins = 32
    out = {"device": torch.cuda.get_device_name(0), "fixed": list(FIX_SHAPE), "moving": list(MOV_SHAPE), "dtype": "int16",
           "bins": bins, "copy_rate_bytes_per_s": COPY_RATE,
           "method": f"HIP events, 3 rotating buffer sets, warm-up, median of {a.reps} windows of {a.iters} calls, the "
                     "strides alternating window by window; raw bytes and windows already on the device",
           "evaluation": {}}

    def raw(v):
        return data.RawVolume(torch.from_numpy(v.reshape(-1).view(np.uint8).copy()), 4, v.shape, 1.0, 0.0).to(device)

    sets = []
    for _ in range(3):
        s = {"fix": raw(fix), "mov": raw(mov), "work": align._joint_work(bins, device)}
        s["fl"], s["ml"] = intensity._window_device(s["fix"], None), intensity._window_device(s["mov"], None)
        sets.append(s)
    strides = {"stride_1_1_1": (1, 1, 1), "stride_1_2_2": (1, 2, 2)}
    calls = {k: (lambda s, st=st: align._joint_enqueue(s["fix"], s["mov"], A, t, s["fl"], s["ml"], bins, st, s["work"]))
             for k, st in strides.items()}
    for k, st in strides.items():
        got = calls[k](sets[0]).cpu().numpy().astype(np.int64)
        exp = predict.joint_histogram(fix, mov, A, t, intensity._host_lohi(fix, None), intensity._host_lohi(mov, None), bins, st)
        assert np.array_equal(got, exp), (k, int(got.sum()), int(exp.sum()))
        lattice = int(np.prod([-(-n // s) for n, s in zip(FIX_SHAPE, st)]))
        fetched = FIX_SHAPE[0] // st[0] * -(-FIX_SHAPE[1] // st[1]) * FIX_SHAPE[2] * 2 + int(np.prod(MOV_SHAPE)) * 2
        out["evaluation"][k] = {"lattice_voxels": lattice, "overlap_voxels": int(got.sum()), "bytes": fetched,
                                "roofline_us": fetched / COPY_RATE * 1e6,
                                "nmi": predict.normalised_mutual_information(got)}
    for fn in calls.values():
        for s in sets:
            fn(s)
    torch.cuda.synchronize()
    windows = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            windows[k].append(window_us(fn, sets, a.iters))
    for k, w in windows.items():
        e = out["evaluation"][k]
        e.update(median_us=statistics.median(w), all_us=w)
        e["bytes_per_s"] = e["bytes"] / (e["median_us"] * 1e-6)
        print(k, json.dumps({x: e[x] for x in ("median_us", "roofline_us", "bytes", "overlap_voxels")}), flush=True)

    walls, result = [], None
    for i in range(a.case_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = predict.register_case_device(root, normalise=True, align={"mode": "register", "to": "gaoqing-T2"})
        torch.cuda.synchronize()
        if i:
            walls.append(time.perf_counter() - t0)
    out["register_case_device"] = {
        "wall_s_median": statistics.median(walls), "wall_s_all": walls, "true_motion": list(TRUE_MOTION),
        "fixed_modality": "gaoqing-T2",
        "results": {m: {"params": list(r["params"]), "before": r["before"], "after": r["after"],
                        "evaluations": r["evaluations"]} for m, r in result.items()}}
    print("register_case_device", json.dumps(out["register_case_device"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
