"""Scratch / LDS / register resources of the sliding-window kernels (CPU: device assembly only;
the method of tests/test_lesions_resources.py).

The LDS figures are the design (csrc/window.hip):
* window_blend_kernel: the three per-axis weight tables at the longest window axis the entry point
  accepts, 3 x 512 floats = 6144 bytes, staged once per workgroup;
* window_gather_kernel (vector and scalar stores), window_finish_kernel: none.
No kernel may use scratch.  These are streaming kernels whose only latency hiding is occupancy:
64 VGPRs keep eight waves per SIMD."""
import os
import shutil

import pytest

from tests.test_distance_resources import _meta
from tests.test_kernel_resources import CSRC, HIPCC

# kernel-name fragment -> LDS bytes per workgroup
LDS = {
    "window_gather_kernelILb1EE": 0, "window_gather_kernelILb0EE": 0,
    "window_blend_kernel": 3 * 512 * 4, "window_finish_kernel": 0,
}
VGPR_BUDGET = 64


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_window_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "window.hip"), str(tmp_path))
    assert len(meta) == len(LDS), sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
