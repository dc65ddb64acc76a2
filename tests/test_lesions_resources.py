"""Scratch / LDS / register resources of the component-table kernels (CPU: device assembly only;
the method of tests/test_distance_resources.py).

The LDS figures are the design (csrc/lesions.hip):
* lt_count_kernel, lt_scatter_kernel: the four waves' root counts = 16 bytes;
* lt_scan_kernel: the four waves' sums of a 256-entry tile = 16 bytes;
* lt_init_kernel, lt_decode_kernel: none;
* lt_accum_kernel (with and without prob): none -- the reduction is across the lanes of a wave
  (register shuffles), there is no workgroup stage.
No kernel may use scratch.  64 VGPRs keep eight waves per SIMD: the accumulation is a chain of
dependent gathers (label -> root -> rank) and atomics, hidden by occupancy alone."""
import os
import shutil

import pytest

from tests.test_distance_resources import _meta
from tests.test_kernel_resources import CSRC, HIPCC

# kernel-name fragment -> LDS bytes per workgroup
LDS = {
    "lt_init_kernel": 0, "lt_count_kernel": 16, "lt_scan_kernel": 16, "lt_scatter_kernel": 16,
    "lt_accum_kernelILb0EE": 0, "lt_accum_kernelILb1EE": 0, "lt_decode_kernel": 0,
}
VGPR_BUDGET = 64


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_lesion_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "lesions.hip"), str(tmp_path))
    assert len(meta) == len(LDS), sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
