"""Scratch / LDS / register resources of the distance-transform kernels (CPU: device assembly
only; the method of tests/test_kernel_resources.py).

The LDS figures are the design (csrc/distance.hip):
* edt_line_kernel<T, 32768>: the slab of lines of one workgroup where it fits 32 KiB -- H = 384
  rows of 32 16-bit integers are 24 KiB -- plus the 256 bytes of the workgroup-wide OR ("any
  feature in the slab"): four 256-thread workgroups share a CU's 160 KiB;
* edt_line_kernel<T, 65536>: longer lines, plus the same 256 bytes: two workgroups per CU (the
  floor the design keeps at H = 384 is two);
* edt_w_kernel: four waves x 32 words of 64 feature bits = 1 KiB;
* the statistics kernels: four waves' (count, max, sum) = 96 bytes; surface_kernel: none.
No kernel may use scratch: the H and D walks are LDS-latency loops that a spill would stall.  64
VGPRs keep eight waves per SIMD possible wherever LDS allows them."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_kernel_resources import CSRC, HIPCC, REPO

# kernel-name fragment -> LDS bytes per workgroup
LDS = {
    "surface_kernel": 0,
    "edt_w_kernelIh": 1024, "edt_w_kernelIt": 1024,
    "edt_line_kernelIhLi32768E": 33024, "edt_line_kernelItLi32768E": 33024, "edt_line_kernelIdLi32768E": 33024,
    "edt_line_kernelIhLi65536E": 65792, "edt_line_kernelItLi65536E": 65792, "edt_line_kernelIdLi65536E": 65792,
    "sd_partial_kernel": 96, "sd_finish_kernel": 96,
}
VGPR_BUDGET = 64


def _meta(src, tmp):
    """name -> (scratch bytes, LDS bytes, VGPRs) from the code object metadata."""
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO}/include", "-Wno-unused-function",
                    "--cuda-device-only", "-S", "-o", out, src], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = open(out).read()
    meta = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", s.split("amdhsa.kernels:")[1])[1:]:
        field = lambda key: re.search(rf"\.{key}:\s+(\S+)", blk).group(1)  # noqa: E731
        meta[field("name")] = (int(field("private_segment_fixed_size")), int(field("group_segment_fixed_size")),
                               int(field("vgpr_count")))
    return meta


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")
def test_distance_kernels_use_no_scratch_and_the_designed_lds(tmp_path):
    meta = _meta(os.path.join(CSRC, "distance.hip"), str(tmp_path))
    assert len(meta) == len(LDS), sorted(meta)
    for key, lds in LDS.items():
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 1, f"{key}: {[n for n, _ in hits]}"
        name, (priv, group, vgpr) = hits[0]
        assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
        assert group == lds, f"{name}: {group} B of LDS, designed for {lds}"
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs (budget {VGPR_BUDGET})"
    # two workgroups of the largest kernel fit a CU's 160 KiB
    assert 2 * max(LDS.values()) <= 160 << 10
