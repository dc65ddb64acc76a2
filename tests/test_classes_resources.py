"""Scratch / LDS / register resources of the kernels of csrc/classes.hip (CPU: device assembly
only; the method of tests/test_loss_resources.py).

The 44 kernels:
* softmax_partial_kernel<C>, C = 2..8: the four waves' 3C + 2 sums, (3C + 2) x 4 floats;
* softmax_finalize_kernel: the 256 threads' fp64 region sums, 256 x 8 = 2048 bytes;
* softmax_bwd_kernel<C> and softmax_planes_kernel<C>, C = 2..8: none;
* probs_to_labels_kernel: none; class_overlap_kernel: 3 x 8 counters of 4 bytes = 96 bytes;
* resample_classes_kernel<T> and resample_affine_classes_kernel<T>, the ten NIfTI element types: none.
No kernel may use scratch.  They are streaming kernels whose only latency hiding is occupancy: a
thread of the C-plane kernels holds four voxels of C logits, so the budget is 128 VGPRs -- four
waves per SIMD -- at C = 8."""
import os
import shutil

import pytest

from tests.test_distance_resources import _meta
from tests.test_kernel_resources import CSRC, HIPCC

CLASSES = range(2, 9)
TYPES = "ahstijlmfd"  # int8, uint8, int16, uint16, int32, uint32, int64, uint64, float, double
# kernel-name fragment -> LDS bytes per workgroup
LDS = {f"softmax_partial_kernelILi{c}EE": 16 * (3 * c + 2) for c in CLASSES}
LDS["softmax_finalize_kernel"] = 2048
LDS.update({f"softmax_bwd_kernelILi{c}EE": 0 for c in CLASSES})
LDS.update({f"softmax_planes_kernelILi{c}EE": 0 for c in CLASSES})
LDS.update({"probs_to_labels_kernel": 0, "class_overlap_kernel": 96})
LDS.update({f"resample_classes_kernelI{t}E": 0 for t in TYPES})
LDS.update({f"resample_affine_classes_kernelI{t}E": 0 for t in TYPES})
VGPR_BUDGET = 128


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_class_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "classes.hip"), str(tmp_path))
    assert len(meta) == len(LDS) == 44, sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
