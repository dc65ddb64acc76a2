"""Register / scratch resources of the hand-pipelined kernels (CPU: device assembly only).

The big-box convs (32x32x16 and 16x16x32), the stem kernels and the bf16 general conv count their vector-memory
operations by hand (LDS-DMA from inline asm + counted ``s_waitcnt vmcnt``); a register spill
inside such a loop adds scratch loads whose compiler-inserted waits drain the pipeline.  The
kernels must therefore fit their VGPR budget with no scratch (private segment 0).  The
ConvTranspose LDS kernel relies on two 512-thread workgroups per CU: <= 128 VGPRs."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prostate-cancer-multimodal-segmentation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

KERNELS = {
    "conv3_big.hip": ["conv3_fwd_big_kernel"],
    "conv3_b16.hip": ["conv3_fwd_b16_kernelILb0ELi8ELi4E", "conv3_fwd_b16_kernelILb1ELi8ELi4E",
                      "conv3_fwd_b16_kernelILb0ELi4ELi4E", "conv3_fwd_b16_kernelILb1ELi4ELi4E",
                      "conv3_fwd_b16_kernelILb0ELi4ELi8E", "conv3_fwd_b16_kernelILb1ELi4ELi8E"],
    "conv3_fwd.hip": ["conv3_fwd_kernelItLi2ELi2ELi3ELi4E", "conv3_fwd_kernelItLi2ELin1ELin1ELin1E"],
    "conv3_wgrad.hip": ["conv3_wgrad_kernelI4x6_t", "wgrad_reduce_fused_kernel"],
    "stem.hip": ["stem_fwd_direct_kernelILi2ELi3E", "stem_fwd_direct_kernelILi3ELi2E", "stem_wgrad_stream_kernel"],
    "convt.hip": ["convt_lds_kernel", "convt_fwd_stream_kernel"],
    # streaming fusions: a spill there would add scratch traffic to an HBM-bound pass
    "ops_pool.hip": ["maxpool_bwd_bn_kernel", "bn_relu_pool_kernel"],
    "ops_head.hip": ["head_bwd_kernel", "head_bn_apply_kernel"],
}
# (the 4-deep 16x16x32 conv runs one 256-thread workgroup per CU: one wave per SIMD)
VGPR_BUDGET = {"convt_lds_kernel": 128, "conv3_fwd_b16_kernelILb0ELi4ELi4E": 512, "conv3_fwd_b16_kernelILb1ELi4ELi4E": 512,
               "conv3_fwd_b16_kernelILb0ELi4ELi8E": 512, "conv3_fwd_b16_kernelILb1ELi4ELi8E": 512}
# scratch allowed where a kernel's only spills sit outside its vmcnt-counted pipeline (checked
# in the device assembly when the budget was set): the 128-channel 16x16x32 conv keeps 256
# accumulators live and reloads one value in its prologue / final BN reduction
SCRATCH_BUDGET = {"conv3_fwd_b16_kernelILb0ELi4ELi8E": 8, "conv3_fwd_b16_kernelILb1ELi4ELi8E": 24,
                  # the fp32 build's weight gradient: spills in its flush only (partial-row
                  # addresses after the box loop; round 5 held 460 B, some inside the staging)
                  "conv3_wgrad_kernelI4x6_t": 160}


def _meta(src, tmp):
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO}/include", "-Wno-unused-function",
                    "-Wno-inline-asm", "--cuda-device-only", "-S", "-o", out, src], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)", s):
        blk = s[m.start():m.start() + 2000]
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        vgpr = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        meta[m.group(1)] = (int(priv.group(1)), int(vgpr.group(1)))
    return meta


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
@pytest.mark.parametrize("src", sorted(KERNELS))
def test_pipelined_kernels_do_not_spill(src, tmp_path):
    meta = _meta(os.path.join(CSRC, src), str(tmp_path))
    for key in KERNELS[src]:
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert hits, f"{key} not found in {src}"
        for name, (priv, vgpr) in hits:
            assert priv <= SCRATCH_BUDGET.get(key, 0), f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
            budget = VGPR_BUDGET.get(key, 256)
            assert vgpr <= budget, f"{name}: {vgpr} VGPRs (budget {budget}: its waves per SIMD)"
