"""Register / scratch resources of the deforming resample kernels (CPU: device assembly only),
by the method of tests/test_augment.py::test_affine_kernels_fit_their_budget: gather kernels that
hide their loads with occupancy -- at least four waves per SIMD, so at most 128 VGPRs, and no
scratch.  Moving the shared device pieces into resample_common.h must leave resample.hip with
exactly its ten instances of each affine kernel."""
import os
import shutil

import pytest

from tests.test_kernel_resources import CSRC, HIPCC, _meta

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("bash") is None, reason="hipcc not available")


def test_deform_kernels_fit_their_budget(tmp_path):
    meta = _meta(os.path.join(CSRC, "deform.hip"), str(tmp_path))
    for key in ("resample_deform_linear_kernel", "resample_deform_label_kernel"):
        hits = [(n, v) for n, v in meta.items() if key in n]
        assert len(hits) == 10, f"{key}: one instance per NIfTI datatype expected, found {len(hits)}"
        for name, (priv, vgpr) in hits:
            assert priv == 0, f"{name}: {priv} B of scratch (spills) at {vgpr} VGPRs"
            assert vgpr <= 128, f"{name}: {vgpr} VGPRs (budget 128)"
    assert not [n for n in meta if "resample_affine_" in n]  # the affine kernels stay in resample.hip


def test_resample_hip_keeps_its_affine_kernels(tmp_path):
    meta = _meta(os.path.join(CSRC, "resample.hip"), str(tmp_path))
    for key in ("resample_affine_linear_kernel", "resample_affine_label_kernel"):
        assert len([n for n in meta if key in n]) == 10, key
    assert not [n for n in meta if "deform" in n]
