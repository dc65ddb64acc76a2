"""pcms_stem_dgrad launch times beside what the reference executes for the same gradient --
aten's conv3d backward-input on the same dy and w, bf16 channels_last_3d -- in one process,
alternating (HIP events, 3 rotating buffer sets, warm-up, repeated; test tooling, not a test).

Writes both times, the bytes computed from the shapes (dy read once + dx written once) and
their share of the 6.29 TB/s measured copy peak to profiles/stem_dgrad_time.json (--out)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

PEAK = 6.29e12  # measured copy peak, bytes / s
SHAPES = [(2, 128, 128, 64), (1, 256, 256, 96)]
CIN = 5


def _time(fn, sets, iters):
    for s in sets:
        fn(s)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def measure(N, D, H, W, reps, iters):
    import pcms_amd  # noqa: F401
    from pcms_amd import _lib as L
    T = torch.bfloat16
    nvox = N * D * H * W
    w = torch.randn(64, CIN, 3, 3, 3, device="cuda") * 0.2
    pack = torch.empty(L.query("pcms_stem_dgrad_pack_elems", L.BF16), dtype=T, device="cuda")
    L.call("pcms_stem_dgrad_pack", L.BF16, w, pack, CIN)
    # one storage per set, seen as NDHWC by the kernel and as channels_last_3d NCDHW by aten
    sets = []
    for _ in range(3):
        dy = torch.randn(N, D, H, W, 64, device="cuda").to(T)
        sets.append((dy, dy.permute(0, 4, 1, 2, 3), torch.empty(N, CIN, D, H, W, device="cuda")))
    wa = w.to(T).contiguous(memory_format=torch.channels_last_3d)
    xa = torch.empty(N, CIN, D, H, W, dtype=T, device="cuda").contiguous(memory_format=torch.channels_last_3d)

    def ours(s):
        L.call("pcms_stem_dgrad", L.BF16, s[0], pack, s[2], N, D, H, W, CIN)

    def aten(s):
        return torch.ops.aten.convolution_backward(s[1], xa, wa, None, [1, 1, 1], [1, 1, 1], [1, 1, 1], False,
                                                   [0, 0, 0], 1, [True, False, False])[0]

    nbytes = nvox * 64 * 2 + nvox * CIN * 4
    rec = {"shape": [N, D, H, W], "cin_w": CIN, "dtype": "bf16", "bytes": nbytes,
           "floor_us_at_6.29TBps": nbytes / PEAK * 1e6}
    aten_err = None
    try:
        got = aten(sets[0]).float()
        ours(sets[0])
        torch.cuda.synchronize()
        scale = float(got.abs().max())
        rec["max_abs_diff_vs_aten_over_max"] = float((sets[0][2] - got).abs().max()) / max(scale, 1e-30)
        del got
    except Exception as e:  # the library behind aten may not run this shape on this machine
        aten_err = f"{type(e).__name__}: {e}"[:300]
    t_ours, t_aten = [], []
    for _ in range(reps):  # alternating, so both see the same clocks
        t_ours.append(_time(ours, sets, iters))
        if aten_err is None:
            t_aten.append(_time(aten, sets, iters))
    rec["pcms_stem_dgrad_us"] = min(t_ours)
    rec["pcms_stem_dgrad_us_all"] = t_ours
    rec["share_of_peak"] = nbytes / (min(t_ours) * 1e-6) / PEAK
    if aten_err is None:
        rec["aten_conv3d_backward_input_us"] = min(t_aten)
        rec["aten_conv3d_backward_input_us_all"] = t_aten
        rec["aten_share_of_peak"] = nbytes / (min(t_aten) * 1e-6) / PEAK
        rec["speedup_vs_aten"] = min(t_aten) / min(t_ours)
    else:
        rec["aten_conv3d_backward_input_us"] = "not measured"
        rec["aten_error"] = aten_err
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stem_dgrad_time.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK, "method": "HIP events, 3 rotating "
           f"buffer sets, warm-up, min of {a.reps} x {a.iters} launches, kernel and aten alternating in one process",
           "runs": []}
    for shp in SHAPES:
        rec = measure(*shp, a.reps, a.iters)
        print(json.dumps(rec), flush=True)
        out["runs"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
