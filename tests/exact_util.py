"""Integer-valued fills, the exactness guard and the bit comparator of the exact op tests
(tests/test_conv_exact.py, tests/test_exact_util_host.py).

The Gaussian op tests hold a bf16 output to 1e-2 of max|y|: about four times the output
rounding itself, so an error the size of one product term passes.  Here the operands are small
integers (or, for the split-bf16 fp32 kernels, integers plus a multiple of 2^-12), chosen so that
every product, every partial sum in any order and the stored result are exactly representable.
A correct kernel then returns the reference's very values, whatever its summation order, split-K
plan or tile walk, and the difference of a wrong one reads as a count of missing or extra terms.
"""
from __future__ import annotations

import torch

TERMS = 864          # non-zero product terms per output a fill aims at (sigma ~ 29, 6 sigma < 256)
GRAIN2 = 2.0 ** -12  # the grain of the two-part values (h = a, m = b 2^-12, l = 0)
B2 = 8               # |b| <= 8: |m| <= 2^-9, at most a tie that rounds h back to a


def gen(*key) -> torch.Generator:
    """A seeded generator per case: key is any tuple of ints / strings."""
    seed = 0
    for k in key:
        for ch in (str(k) + "|"):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def signs(shape, g):
    """Every element +1 or -1."""
    return (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1).float()


def ternary(shape, g, density):
    """Elements in {-1, 0, +1}, non-zero with probability ``density``."""
    s = signs(shape, g)
    if density >= 1.0:
        return s
    return s * (torch.rand(tuple(shape), generator=g) < density).float()


def density_for(k, terms=TERMS):
    """The density of the sparse operand of a sum over ``k`` products: about ``terms`` of them
    are non-zero (1 / cin above 32 input channels of a 3x3x3 conv)."""
    return min(1.0, terms / float(k))


def operands(fill, xshape, wshape, k, g, terms=TERMS):
    """(activations, weights) of a fill, fp32 holding integers.  ``k``: products per output.
    A: dense +-1 activations, sparse weights -- a wrong or unzeroed halo voxel, a misplaced read
    always changes a sum.  B: sparse activations, dense +-1 weights -- the loss of any single
    packed weight element is visible."""
    if fill == "A":
        return signs(xshape, g), ternary(wshape, g, density_for(k, terms))
    assert fill == "B", fill
    return ternary(xshape, g, density_for(k, terms)), signs(wshape, g)


def activations(fill, shape, k, g, terms=TERMS):
    """The activations of ``fill`` alone (also dy of a dgrad / wgrad: filled the same way)."""
    return signs(shape, g) if fill == "A" else ternary(shape, g, density_for(k, terms))


def weights(fill, shape, k, g, terms=TERMS):
    """The weights of ``fill`` alone (k: the most products per output of any direction they serve)."""
    return ternary(shape, g, density_for(k, terms)) if fill == "A" else signs(shape, g)


def small_ints(n, g, lim=4):
    """A bias of small integers in [-lim, lim]."""
    return torch.randint(-lim, lim + 1, (n,), generator=g).float()


def two_part(a, g):
    """v = a + b 2^-12, |b| <= 8, for integer a in {0, +-1}: two bf16 parts h = a, m = b 2^-12
    and l = 0 (a = 0: the single part h = b 2^-12).  Exact in fp32."""
    b = torch.randint(-B2, B2 + 1, tuple(a.shape), generator=g).float()
    return a + b * GRAIN2


def split3(v):
    """torch emulation of the kernels' split3x8: h = rne(v), m = rne(v - h), l = rne(v - h - m),
    each a bf16 value (returned as fp32)."""
    v = v.float()
    h = v.to(torch.bfloat16).float()
    r = v - h
    m = r.to(torch.bfloat16).float()
    lo = (r - m).to(torch.bfloat16).float()
    return h, m, lo


def assert_exact_case(ref, bound, out_dtype, grain=1.0, nvox=None):
    """The guard that makes "exact" a theorem: asserted on the CPU before anything is launched.

    * ``ref`` (fp64) survives the round trip through the output type bit for bit (bf16 with
      integer values: |y| <= 256);
    * ``bound / grain < 2^24``: ``bound`` is conv(|x|, |w|) + |b|, the largest magnitude any
      partial sum can reach in any order, ``grain`` the power of two every term is a multiple
      of -- so every fp32 partial sum is an integer multiple of the grain below 2^24 grains;
    * ``nvox * max|ref| < 2^24`` (``nvox`` given: outputs with BatchNorm partial rows), so any
      row's channel sum is exact too.
    """
    assert ref.dtype == torch.float64
    assert torch.equal(ref.to(out_dtype).double(), ref), \
        f"reference is not representable in {out_dtype}: max|y| = {ref.abs().max().item()}"
    bound = float(bound)
    assert bound / grain < 2 ** 24, f"partial sums may leave the exact range: bound {bound} / grain {grain}"
    assert torch.equal(torch.round(ref / grain) * grain, ref), "reference is not a multiple of the grain"
    if nvox is not None:
        m = ref.abs().max().item()
        assert nvox * m / grain < 2 ** 24, f"channel sums may leave the exact range: {nvox} x {m}"


def _fmt_index(idx, names, box):
    s = "(" + ", ".join(f"{n}={i}" for n, i in zip(names, idx)) + ")"
    if box is not None and len(idx) == 5:
        _, d, h, w, _ = idx
        s += (f" box ({d // box[0]}, {h // box[1]}, {w // box[2]})"
              f" + ({d % box[0]}, {h % box[1]}, {w % box[2]})")
    return s


def bits_mismatch(got, ref, what, box=None, first=6):
    """None when ``got`` holds exactly the values of ``ref``; else the failure message: the
    number of wrong elements, the first few indices -- (n, d, h, w, c) of an NDHWC tensor, with
    the box index and box-relative coordinates when ``box`` = (bd, bh, bw) is given -- got and
    expected there, and their difference (with the integer fills: the number of missing or
    extra terms; with the two-part values a multiple of 2^-12).  The comparison is of values:
    +0 and -0 are the same value (the sign of a zero sum
    depends on the summation order, which the guard leaves free); NaN never matches."""
    g = got.detach().cpu().double()
    r = ref.detach().cpu().double()
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    bad = ~(g == r)
    nbad = int(bad.sum().item())
    if nbad == 0:
        return None
    names = ("n", "d", "h", "w", "c") if g.dim() == 5 else tuple(f"i{k}" for k in range(g.dim()))
    lines = [f"{what}: {nbad} of {g.numel()} elements differ from the exact reference"]
    for idx in bad.nonzero()[:first].tolist():
        gv, rv = g[tuple(idx)].item(), r[tuple(idx)].item()
        lines.append(f"  {_fmt_index(idx, names, box)}: got {gv!r} expected {rv!r} diff {gv - rv:+g}")
    return "\n".join(lines)


def assert_bits_equal(got, ref, what, box=None):
    msg = bits_mismatch(got, ref, what, box)
    assert msg is None, msg
