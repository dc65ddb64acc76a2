"""Scratch / LDS / register resources of the joint-histogram kernels (CPU: device assembly only;
the method of tests/test_intensity_resources.py).

The LDS figures are the design (csrc/align.hip):
* joint_hist_kernel (ten moving source types; the fixed type is a run-time switch): the workgroup's
  64 x 64 table of 32-bit counts = 16384 bytes, whatever the bin count of the call;
* joint_zero_kernel and joint_sum_kernel: none.
No kernel may use scratch.  The histogram kernel hides the latency of its gather by occupancy
alone: at most 128 VGPRs keep four waves per SIMD, which are four 256-thread workgroups per CU, and
their four 16 KiB tables fit the CU's 160 KiB, so LDS does not bind before the registers do."""
import os
import shutil

import pytest

from tests.test_distance_resources import _meta
from tests.test_kernel_resources import CSRC, HIPCC

# the Itanium codes of the ten NIfTI element types: u8 i16 i32 f32 f64 i8 u16 u32 i64 u64
TYPES = "hsifdatjlm"
# kernel-name fragment -> LDS bytes per workgroup
LDS = {"joint_zero_kernel": 0, "joint_sum_kernel": 0}
LDS.update({f"joint_hist_kernelI{t}E": 16384 for t in TYPES})
VGPR_BUDGET = 128


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_align_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "align.hip"), str(tmp_path))
    assert len(meta) == len(LDS) == 12, sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
    # four waves per SIMD are four 256-thread workgroups per CU: their tables fit its LDS
    assert 4 * max(LDS.values()) <= 160 << 10
