"""Register / scratch resources of the input-gradient kernels (CPU: device assembly only; the
method of tests/test_kernel_resources.py).

Budgets, from the waves per SIMD each kernel plans for (512 VGPRs per SIMD lane, accumulation
registers included):
* stem_dgrad_mfma_kernel: one 256-thread workgroup per CU (its 118 KB of LDS allow no second
  one), i.e. one wave per SIMD: 512.  It keeps the next box's halo (21 x 4 registers) in flight
  beside the MFMAs, and the compiler may hold weight fragments across the unrolled taps.
* stem_dgrad_plain_kernel (the fp32 parity build): two 256-thread workgroups per CU by LDS
  (2 x 54 KB), two waves per SIMD: 256.
* bn_relu_bwd_eval_kernel / head_bn_bwd_eval_kernel: HBM streams that want at least four waves
  per SIMD in flight: 128.
No kernel may use scratch: a spill would add memory traffic to passes bound by it."""
import os
import shutil

import pytest

from tests.test_kernel_resources import CSRC, HIPCC, _meta

KERNELS = {
    "stem_dgrad.hip": {"stem_dgrad_mfma_kernel": 512, "stem_dgrad_plain_kernel": 256, "stem_dgrad_pack_kernel": 128},
    "ops_bn.hip": {"bn_relu_bwd_eval_kernel": 128},
    "ops_head.hip": {"head_bn_bwd_eval_kernel": 128},
}


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
@pytest.mark.parametrize("src", sorted(KERNELS))
def test_input_grad_kernels_fit_their_budget(src, tmp_path):
    meta = _meta(os.path.join(CSRC, src), str(tmp_path))
    for key, budget in KERNELS[src].items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert hits, f"{key} not found in {src}"
        for name, (priv, vgpr) in hits:
            assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
            assert vgpr <= budget, f"{name}: {vgpr} VGPRs (budget {budget}: its waves per SIMD)"
