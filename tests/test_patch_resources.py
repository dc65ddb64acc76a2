"""Scratch / LDS / register resources of the patch-training kernels (CPU: device assembly only;
the method of tests/test_window_resources.py).

The LDS figures are the design (csrc/patch.hip):
* foreground_count_kernel (vector and scalar loads), foreground_scan_kernel, foreground_pick_kernel:
  the four waves' counts or totals, 4 ints = 16 bytes;
* patch_resample_kernel (ten source types, with and without the normalised corner): none.
No kernel may use scratch.  These are streaming kernels whose only latency hiding is occupancy:
64 VGPRs keep eight waves per SIMD."""
import os
import shutil

import pytest

from tests.test_distance_resources import _meta
from tests.test_kernel_resources import CSRC, HIPCC

# the Itanium codes of the ten NIfTI element types: u8 i16 i32 f32 f64 i8 u16 u32 i64 u64
TYPES = "hsifdatjlm"
# kernel-name fragment -> LDS bytes per workgroup
LDS = {"foreground_count_kernelILb1EE": 16, "foreground_count_kernelILb0EE": 16, "foreground_scan_kernel": 16,
       "foreground_pick_kernel": 16}
LDS.update({f"patch_resample_kernelI{t}Lb{norm}EE": 0 for t in TYPES for norm in (0, 1)})
VGPR_BUDGET = 64


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_patch_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "patch.hip"), str(tmp_path))
    assert len(meta) == len(LDS) == 24, sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
