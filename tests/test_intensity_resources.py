"""Scratch / LDS / register resources of the intensity-window kernels (CPU: device assembly only;
the method of tests/test_window_resources.py).

The LDS figures are the design (csrc/intensity.hip):
* window_hist_kernel (ten source types): the workgroup's two 256-bin rows of 32-bit counts, one per
  rank = 2048 bytes;
* window_scan_kernel: the four waves' totals of the two rows, 8 words = 32 bytes;
* window_init_kernel, resample_linear_window_kernel and patch_resample_window_kernel (ten source
  types each): none.
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
LDS = {"window_init_kernel": 0, "window_scan_kernel": 32}
LDS.update({f"window_hist_kernelI{t}E": 2048 for t in TYPES})
LDS.update({f"resample_linear_window_kernelI{t}E": 0 for t in TYPES})
LDS.update({f"patch_resample_window_kernelI{t}E": 0 for t in TYPES})
VGPR_BUDGET = 64


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_intensity_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "intensity.hip"), str(tmp_path))
    assert len(meta) == len(LDS) == 32, sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
