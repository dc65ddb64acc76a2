"""bench.py's plain run: the result line and ``--dump-outputs``.

One short run at a small size: ``--steps`` sets the number of timed steps, the line carries
``ms_per_step``, the legs behind ``--full`` are off (null), and the dump holds the last timed
step's loss, parameters, gradients and BatchNorm buffers as finite float32 arrays of at most
64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size", "32,32,16", "--dump-outputs", str(out)], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "volumes/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(2 / (rec["ms_per_step"] * 1e-3), rel=1e-3)
    for leg in ("roofline", "cpu_baseline", "fp32_parity_build_value", "clock"):
        assert rec[leg] is None, leg
    files = sorted(os.listdir(out))
    assert files == ["bn_buffers.npy", "grads.npy", "loss.npy", "params.npy"]
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype == np.float32 and a.ndim == 1 and a.size > 0, name
        assert np.isfinite(a).all(), name
    assert arrays["loss"].shape == (1,)
    assert float(arrays["loss"][0]) == pytest.approx(rec["final_loss"], abs=1e-5)
    assert arrays["params"].shape == arrays["grads"].shape
    assert np.abs(arrays["grads"]).max() > 0
