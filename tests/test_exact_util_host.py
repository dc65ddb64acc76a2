"""CPU tests of tests/exact_util.py: the guard rejects a case whose sums could round, the bit
comparator flags the single-term errors the 1e-2 bar of tests/test_gpu_ops.py lets through
(that recorded pass is why the exact tests exist), and the two-part values of the split-bf16
cases split as claimed."""
import pytest
import torch
import torch.nn.functional as F

from tests.exact_util import (B2, GRAIN2, assert_bits_equal, assert_exact_case, bits_mismatch, gen, operands,
                              signs, small_ints, split3, ternary)
from tests.test_gpu_ops import close

N, C, S = 2, 64, (8, 8, 16)
BOX = (8, 8, 16)


def _case(fill):
    g = gen("host", fill)
    x, w = operands(fill, (N, C, *S), (C, C, 3, 3, 3), 27 * C, g)
    b = small_ints(C, g)
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    bound = F.conv3d(x.abs().double(), w.abs().double(), b.abs().double(), padding=1).max().item()
    assert_exact_case(ref, bound, torch.bfloat16, nvox=N * S[0] * S[1] * S[2])
    return x, w, b, ref


def test_guard_rejects_overflowing_case():
    """cin = 256 at density 1.0: max|y| ~ 300, odd values above 256 (the interior sums of 6912
    +-1 terms are even, the odd bias makes them odd) that bf16 cannot hold."""
    g = gen("overflow")
    x = signs((1, 256, 8, 8, 8), g)
    w = signs((64, 256, 3, 3, 3), g)
    ref = F.conv3d(x.double(), w.double(), torch.ones(64, dtype=torch.float64), padding=1)
    assert ref.abs().max().item() > 256
    with pytest.raises(AssertionError, match="not representable"):
        assert_exact_case(ref, 27 * 256, torch.bfloat16)
    assert_exact_case(ref, 27 * 256, torch.float32)  # the same sums are exact in fp32
    with pytest.raises(AssertionError, match="partial sums"):
        assert_exact_case(ref, 27 * 256, torch.float32, grain=2.0 ** -12)
    with pytest.raises(AssertionError, match="channel sums"):
        assert_exact_case(ref, 27 * 256, torch.float32, nvox=2 ** 17)


def _passes_close(got, ref, tol):
    try:
        close(got, ref, tol)
    except AssertionError:
        return False
    return True


def test_comparator_flags_single_term_errors_the_gaussian_bar_passes():
    passed_by_close = {}
    # (1) one packed weight element lost: (co 5, ci 3, tap 26), dense weights (fill B)
    x, w, b, ref = _case("B")
    w2 = w.clone()
    assert w2[5, 3, 2, 2, 2] != 0
    w2[5, 3, 2, 2, 2] = 0
    got = F.conv3d(x.double(), w2.double(), b.double(), padding=1)
    msg = bits_mismatch(got.permute(0, 2, 3, 4, 1), ref.permute(0, 2, 3, 4, 1), "lost weight", BOX)
    assert msg is not None and "c=5" in msg and ("diff +1" in msg or "diff -1" in msg), msg
    with pytest.raises(AssertionError, match="lost weight"):
        assert_bits_equal(got, ref, "lost weight")
    passed_by_close["lost weight element"] = _passes_close(got, ref, 1e-2)
    # (2) one stale halo term at the far corner voxel of each box, all cout (fill A)
    x, w, b, ref = _case("A")
    got = ref.clone()
    got[:, :, BOX[0] - 1::BOX[0], BOX[1] - 1::BOX[1], BOX[2] - 1::BOX[2]] += 1.0
    msg = bits_mismatch(got.permute(0, 2, 3, 4, 1), ref.permute(0, 2, 3, 4, 1), "stale halo", BOX)
    assert msg is not None and f"{N * C} of" in msg and "+ (7, 7, 15)" in msg and "diff +1" in msg, msg
    passed_by_close["stale halo term"] = _passes_close(got, ref, 1e-2)
    # (3) one voxel's row replaced by its neighbour's in the BatchNorm channel sums
    yv = ref.permute(0, 2, 3, 4, 1).reshape(-1, C)
    sums = yv.sum(0)
    bad = sums - yv[777] + yv[778]
    assert bits_mismatch(bad, sums, "BN channel sums") is not None
    nvox = yv.shape[0]
    passed_by_close["BN row counted twice"] = _passes_close(bad / nvox, sums / nvox, 1e-3)
    # the recorded fact: the present bars pass single-term errors the exact comparator rejects
    assert passed_by_close["lost weight element"] and passed_by_close["stale halo term"], passed_by_close
    assert any(passed_by_close.values())


def test_comparator_accepts_equal_values_and_rejects_nan():
    ref = torch.tensor([0.0, -3.0, 256.0], dtype=torch.float64)
    assert_bits_equal(torch.tensor([-0.0, -3.0, 256.0]).bfloat16(), ref, "zeros")
    assert bits_mismatch(torch.tensor([float("nan"), -3.0, 256.0]), ref, "nan") is not None


def test_two_part_values_split_as_claimed():
    """v = a + b 2^-12, a in {0, +-1}, |b| <= 8: h = a and m = b 2^-12 exactly, l = 0 (a = 0: the
    single part h = v), under the emulation of split3x8; so with an integer other operand the
    kept products hh, mh / hm are multiples of 2^-12 and no product is dropped."""
    a = torch.tensor([-1.0, 0.0, 1.0]).view(3, 1).expand(3, 2 * B2 + 1)
    b = torch.arange(-B2, B2 + 1).float().view(1, -1).expand(3, 2 * B2 + 1)
    v = a + b * GRAIN2
    assert torch.equal(v.double(), a.double() + b.double() * GRAIN2)  # exact in fp32
    h, m, lo = split3(v)
    nz = a != 0
    assert torch.equal(h[nz], a[nz]) and torch.equal(m[nz], (b * GRAIN2)[nz])
    assert torch.equal(h[~nz], v[~nz]) and torch.equal(m[~nz], torch.zeros_like(m[~nz]))
    assert torch.equal(lo, torch.zeros_like(lo))
    assert torch.equal(h + m, v)
    # integers have one part only: they exercise the hh product alone
    hi, mi, li = split3(ternary((1000,), gen("ints"), 0.5))
    assert not mi.any() and not li.any()
