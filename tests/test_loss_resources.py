"""Scratch / LDS / register resources of the region + voxel loss kernels (CPU: device assembly
only; the method of tests/test_intensity_resources.py).

csrc/losses.hip has 8 kernels:
* region_partial_kernel<VOX, POW>, three forms (region sums only; + BCE voxel term; + focal
  power): the four waves' four sums, 4 x 4 floats = 64 bytes;
* region_finalize_kernel<GR1>, two forms (gamma == 1: no power; any gamma): the 256 threads' two
  fp64 running sums (region terms, voxel sums), 2 x 256 x 8 = 4096 bytes;
* region_bwd_kernel<VOX, POW>, three forms: none.
No kernel may use scratch.  These are streaming kernels whose only latency hiding is occupancy:
64 VGPRs keep eight waves per SIMD."""
import os
import shutil

import pytest

from tests.test_distance_resources import _meta
from tests.test_kernel_resources import CSRC, HIPCC

FORMS = ("ILb0ELb0EE", "ILb1ELb0EE", "ILb1ELb1EE")  # <VOX, POW>
# kernel-name fragment -> LDS bytes per workgroup
LDS = {f"region_partial_kernel{f}": 64 for f in FORMS}
LDS.update({"region_finalize_kernelILb1EE": 4096, "region_finalize_kernelILb0EE": 4096})
LDS.update({f"region_bwd_kernel{f}": 0 for f in FORMS})
VGPR_BUDGET = 64


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_loss_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "losses.hip"), str(tmp_path))
    assert len(meta) == len(LDS) == 8, sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
