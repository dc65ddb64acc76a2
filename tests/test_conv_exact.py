"""Exact op tests of the MFMA kernels: the 3x3x3 conv (32x32x16 and 16x16x32 forms, split-K,
dgrad packs, fused input BatchNorm + ReLU), its weight gradient, ConvTranspose and the stem, fed
integer-valued operands (tests/exact_util.py) and held to the very values of the fp64 reference.

Every case is built on the CPU and passes ``assert_exact_case`` before anything is launched:
under its conditions any correct kernel is exact, whatever its summation order, so a mismatch
is a kernel or pack bug, never noise, and the comparator's index dump says where.  Every case
runs with both fills (A: dense +-1 activations, sparse weights; B: sparse activations, dense
+-1 weights); the fp32 build's split-bf16 kernels (codes 0 = bf16x6, 2 = bf16x3) get one operand
at a time with two bf16 parts (a + b 2^-12), so the cross products hm / mh are exercised too.
The launches and switches are those of tests/test_gpu_ops.py.

BatchNorm partial rows: the counts add up to nvox, the channel sums merged over the rows equal
the reference's integer channel sums, the variance stays at the 1e-3 bar of test_gpu_ops.py (M2
about a row mean is not exact).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.exact_util import (GRAIN2, TERMS, activations, assert_bits_equal, assert_exact_case, gen, operands,
                              small_ints, ternary, two_part, weights)
from tests.test_gpu_ops import DEV, _lib, _pack16, bn_moments, close, ndhwc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FILLS = ("A", "B")
DT = {0: torch.float32, 1: BF, 2: torch.float32}
# (code, two-part operand): bf16 with integers; the fp32 codes with each operand two-part in turn
BF16_ONLY = [(1, None)]
X6 = [(0, "x"), (0, "w")]
X6_X3 = X6 + [(2, "x"), (2, "w")]


def _d(t):
    return None if t is None else t.double()


def to_ndhwc(ref):
    return ref.permute(0, 2, 3, 4, 1)


@functools.lru_cache(maxsize=None)
def conv_case(tag, fill, N, cin, cout, S, bias=True, dgrad=False, two=None, code=1, stats=True, terms=TERMS):
    """One guarded 3x3x3 case (shared, never modified): x (N, cin, *S), w (cout, cin, 3, 3, 3), b,
    the fp64 forward reference and, with ``dgrad``, dy (N, cout, *S) and the fp64 input gradient."""
    g = gen(tag, fill, N, cin, cout, S, two)
    kw = 27 * (max(cin, cout) if dgrad else cin)
    x = activations(fill, (N, cin, *S), 27 * cin, g, terms)
    w = weights(fill, (cout, cin, 3, 3, 3), kw, g, terms)
    b = small_ints(cout, g) if bias else None
    grain = 1.0 if two is None else GRAIN2
    if two == "x":
        x = two_part(x, g)
    elif two == "w":
        w = two_part(w, g)
    dt = DT[code]
    c = {"x": x, "w": w, "b": b}
    c["ref"] = F.conv3d(x.double(), w.double(), _d(b), padding=1)
    bound = F.conv3d(x.abs().double(), w.abs().double(), _d(b.abs()) if bias else None, padding=1).max().item()
    nvox = N * S[0] * S[1] * S[2]
    assert_exact_case(c["ref"], bound, dt, grain, nvox if stats and two is None else None)
    if dgrad:
        dy = activations(fill, (N, cout, *S), 27 * cout, g, terms)
        if two == "x":
            dy = two_part(dy, g)
        c["dy"] = dy
        c["dref"] = F.conv_transpose3d(dy.double(), w.double(), padding=1)
        bound = F.conv_transpose3d(dy.abs().double(), w.abs().double(), padding=1).max().item()
        assert_exact_case(c["dref"], bound, dt, grain)
    return c


def assert_two_box_merge_exact(ref, bias, nb):
    """The guard of a slot's second box, asserted before the launch.  Both big-box kernels keep a
    running mean per (wave, channel) between boxes (nb voxels per wave and box, a power of two)
    and shift the next box by it.  After one box the mean K = b + s / nb has log2(nb) fraction
    bits; the second box's shifted values y - K, their partial sums, the box mean K + s1 / nb
    (2 log2(nb) fraction bits) and the merged mean rmean + delta / 2 (one more) are all exact in
    fp32 when, per channel, with dev = |y - b| and T' = the mean of the 128 largest dev (a bound
    on |mean - b| over any nb >= 128 voxels):

      nb^2 (max dev + T') <= 2^24   and   2 nb^2 (T' + |b|) <= 2^24

    The row sum is then the sum of the waves' mean x count, each an integer.  (From the third
    box on nb / nnew is 1/3, 1/4, ...: not exact, see check_bn.)"""
    cout = ref.shape[1]
    dev = (ref.transpose(0, 1).reshape(cout, -1) - bias.double().view(cout, 1)).abs()
    k = min(128, dev.shape[1])
    t = dev.topk(k, dim=1).values.mean(1)
    assert (nb * nb * (dev.max(1).values + t)).max().item() <= 2 ** 24, "a second box's shifted sums could round"
    assert (2 * nb * nb * (t + bias.double().abs())).max().item() <= 2 ** 24, "a merged mean could round"


def check_bn(stats, rows, cout, nvox, ref, what, walk=None, bias=None):
    """Counts sum to nvox; the channel sums over the rows are the reference's integer sums,
    with no tolerance; the variance at the Gaussian tests' bar.

    ``walk`` = (sum depth, voxels per wave and box, voxels per box) for the big-box kernels,
    whose slots may walk several boxes: the boxes each row merged are its count / voxels per
    box.  Rows of one or two boxes are exact (assert_two_box_merge_exact) and every such row's
    sums must be integers; when no slot walked a third box the merged sums must equal the
    reference's, as everywhere else.

    The one exception: a slot that walks three boxes or more.  Both kernels merge the next box
    into the running mean by ``rme[0] = rmean + delta * (nb / nnew)`` (conv3_big.hip,
    conv3_b16.hip: the Chan merge that keeps the variance accurate when |mean| >> std).  From
    the third box on nb / nnew = 1/3, 1/4, ... is not a power of two, the running mean K is no
    longer a short binary fraction, and the next box's shifted values e = acc + (bias - K) round:
    the row sum is deliberately not the integer.  The merged sums are then held to the bound that
    follows from that line (u = 2^-24):

      |sum - exact| <= u [ depth (sum_v |y_v - b| + nvox max_v |y_v - b|)     the shifted sums
                           + rows nb W B (4 (B + 1) + W) max|y| ]             the merges

    depth: roundings a term of a wave's shifted box sum passes through (the lane's chain, the
    cross-lane adds, the shift itself); |K - b| <= max |y - b| since K is a mean of outputs; per
    merge at most 8 roundings of quantities within max|y| (mean units, k nb voxels at box k:
    4 nb B (B + 1) per wave), W products and W - 1 adds within W B nb max|y| for the row sum over
    the W = voxels per box / nb waves; B: the most boxes a row merged."""
    st = stats.detach().cpu().double()
    part = st[: rows * cout * 2].view(rows, cout, 2)
    cnt = st[rows * cout * 2: rows * cout * 2 + rows]
    assert cnt.sum().item() == nvox, (cnt.sum().item(), nvox)
    yref = ref.transpose(0, 1).reshape(cout, -1)
    got = part[:, :, 0].sum(0)
    B = 1
    if walk is not None:
        depth, nb, box_vox = walk
        boxes = cnt / box_vox
        assert torch.equal(boxes, boxes.round()) and boxes.min().item() >= 1, boxes.tolist()
        B, W = int(boxes.max().item()), box_vox // nb
        short = part[boxes <= 2, :, 0]
        assert torch.equal(short, short.round()), f"{what}: a row of at most two boxes holds a non-integer sum"
    if B <= 2:
        assert_bits_equal(got, yref.sum(1), f"{what}: BN channel sums over {rows} rows")
    else:
        dev = (yref - bias.double().view(cout, 1)).abs()
        bound = 2.0 ** -24 * (depth * (dev.sum(1) + nvox * dev.max(1).values)
                              + rows * nb * W * B * (4 * (B + 1) + W) * yref.abs().max())
        err = (got - yref.sum(1)).abs()
        assert (err <= bound).all(), (f"{what}: BN channel sums of rows of up to {B} boxes: max err "
                                      f"{err.max().item():.3e}, max err / bound {(err / bound).max().item():.3e}")
    _, var = bn_moments(stats, rows, cout, nvox)
    close(var, yref.var(1, unbiased=False), 1e-3, f"{what}: stats var")


# (sum depth, voxels per wave and box) of the two big-box kernels' BatchNorm epilogues:
# conv3_big.hip: a lane adds 16 values of each of its 8 M-tiles in one chain, one cross-lane add,
# the shift, 8x8x16 boxes on 4 waves; conv3_b16.hip: 8 M-tiles per lane, 4 DPP stages, the shift,
# one d-plane of 8x16 per wave
WALK_BIG = (16 * 8 + 2, 256)
WALK_B16 = (8 + 4 + 1, 128)


def dev_x(x, dt, cin_store=None):
    """(N, C, *S) CPU fp32 -> NDHWC device tensor of dt, zero-padded to cin_store channels."""
    if cin_store is not None and cin_store != x.shape[1]:
        xs = torch.zeros(x.shape[0], cin_store, *x.shape[2:])
        xs[:, : x.shape[1]] = x
        x = xs
    return ndhwc(x.to(dt)).to(DEV)


def join(y0, y1, split):
    got = y0.cpu()
    return torch.cat([got, y1.cpu()], -1) if split else got


# ------------------------------------------------------------------ pcms_conv3_fwd

FWD_BF16 = [(2, 8, 64, (16, 16, 16), 1),        # stem-padded (5 real channels of 8)
            (1, 64, 64, (9, 10, 11), 1),        # partial boxes
            (2, 256, 128, (4, 4, 4), 4),        # split-K through pcms_split_epilogue
            (1, 64, 64, (1, 1, 1), 2)]          # one voxel
FWD_F32 = [(1, 64, 64, (9, 10, 11), 1), (2, 256, 128, (4, 4, 4), 4)]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("code,two,N,cin,cout,S,split",
                         [ct + c for ct in BF16_ONLY for c in FWD_BF16] + [ct + c for ct in X6_X3 for c in FWD_F32])
def test_conv3_fwd_exact(fill, code, two, N, cin, cout, S, split):
    L = _lib()
    dt = DT[code]
    cin_real = 5 if cin == 8 else cin
    c = conv_case("fwd", fill, N, cin_real, cout, S, two=two, code=code)
    xd = dev_x(c["x"], dt, cin)
    wpack = torch.empty(L.query("pcms_conv3_pack_elems", code, cout, cin_real), dtype=dt, device=DEV)
    L.call("pcms_conv3_pack", code, c["w"].to(DEV), wpack, cout, cin_real, 0)
    bd = c["b"].to(DEV)
    y = torch.full((N, *S, cout), float("nan"), dtype=dt, device=DEV)
    nvox = N * S[0] * S[1] * S[2]
    rows = L.query("pcms_conv3_fwd_rows", code, N, *S, cin, 0, cout)
    stats = torch.zeros(max(rows, L.query("pcms_split_epilogue_rows", nvox)) * (cout * 2 + 1), device=DEV)
    if split == 1:
        L.call("pcms_conv3_fwd", code, xd, cin, None, 0, wpack, bd, y, None, cout, None, stats, 0, N, *S, cout, 1)
    else:
        ns = L.query("pcms_conv3_splits", code, cin, split)
        assert ns > 1
        acc = torch.full((ns * nvox * cout,), float("nan"), device=DEV)
        L.call("pcms_conv3_fwd", code, xd, cin, None, 0, wpack, bd, y, None, cout, acc, None, 0, N, *S, cout, split)
        L.call("pcms_split_epilogue", code, acc, ns, bd, y, None, cout, stats, cout, nvox, 0)
        rows = L.query("pcms_split_epilogue_rows", nvox)
    torch.cuda.synchronize()
    assert_bits_equal(y, to_ndhwc(c["ref"]), f"conv3 fwd code {code} fill {fill} two-part {two}")
    if two is None:
        check_bn(stats, rows, cout, nvox, c["ref"], "conv3 fwd")


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("code,two", BF16_ONLY + X6_X3)
def test_conv3_dual_source_and_dgrad_split_output_exact(fill, code, two):
    """conv over cat([skip, up]) from two pointers, and the dgrad whose output splits back."""
    L = _lib()
    dt = DT[code]
    N, S, cs, cout = 2, (8, 6, 10), 64, 64
    c = conv_case("dual", fill, N, 2 * cs, cout, S, bias=False, dgrad=True, two=two, code=code, stats=False)
    x, w = c["x"], c["w"]
    wp = torch.empty(L.query("pcms_conv3_pack_elems", code, cout, 2 * cs), dtype=dt, device=DEV)
    L.call("pcms_conv3_pack", code, w.to(DEV), wp, cout, 2 * cs, 0)
    y = torch.full((N, *S, cout), float("nan"), dtype=dt, device=DEV)
    L.call("pcms_conv3_fwd", code, dev_x(x[:, :cs], dt), cs, dev_x(x[:, cs:], dt), cs, wp, None, y, None, cout,
           None, None, 0, N, *S, cout, 1)
    wd = torch.empty(L.query("pcms_conv3_pack_elems", code, 2 * cs, cout), dtype=dt, device=DEV)
    L.call("pcms_conv3_pack", code, w.to(DEV), wd, cout, 2 * cs, 1)
    gs = torch.full((N, *S, cs), float("nan"), dtype=dt, device=DEV)
    gu = torch.full((N, *S, cs), float("nan"), dtype=dt, device=DEV)
    L.call("pcms_conv3_fwd", code, dev_x(c["dy"], dt), cout, None, 0, wd, None, gs, gu, cs, None, None, 0,
           N, *S, 2 * cs, 1)
    torch.cuda.synchronize()
    assert_bits_equal(y, to_ndhwc(c["ref"]), f"dual-source fwd code {code} fill {fill} two-part {two}")
    assert_bits_equal(join(gs, gu, True), to_ndhwc(c["dref"]), f"dgrad split output code {code} fill {fill} {two}")


@pytest.mark.parametrize("fill", FILLS)
def test_conv3_small_box_two_mtiles_per_wave_exact(fill):
    """8x8x4 boxes on four waves of 2 M-tiles and on two waves of 4, unsplit and split-K."""
    L = _lib()
    N, S, cin, cout = 2, (8, 8, 4), 128, 128
    c = conv_case("mtw2", fill, N, cin, cout, S)
    wp = torch.empty(L.query("pcms_conv3_pack_elems", 1, cout, cin), dtype=BF, device=DEV)
    L.call("pcms_conv3_pack", 1, c["w"].to(DEV), wp, cout, cin, 0)
    xd, bd = dev_x(c["x"], BF), c["b"].to(DEV)
    nvox = N * S[0] * S[1] * S[2]
    rows = L.query("pcms_conv3_fwd_rows", 1, N, *S, cin, 0, cout)
    outs = []
    old = L.query("pcms_conv3_small_box_mtw2", -1)
    try:
        for on in (1, 0):
            L.query("pcms_conv3_small_box_mtw2", on)
            y = torch.full((N, *S, cout), float("nan"), dtype=BF, device=DEV)
            st = torch.zeros(rows * (cout * 2 + 1), device=DEV)
            L.call("pcms_conv3_fwd", 1, xd, cin, None, 0, wp, bd, y, None, cout, None, st, 0, N, *S, cout, 1)
            ns = L.query("pcms_conv3_splits", 1, cin, 3)
            acc = torch.full((ns * nvox * cout,), float("nan"), device=DEV)
            ys = torch.full_like(y, float("nan"))
            L.call("pcms_conv3_fwd", 1, xd, cin, None, 0, wp, bd, ys, None, cout, acc, None, 0, N, *S, cout, 3)
            L.call("pcms_split_epilogue", 1, acc, ns, bd, ys, None, cout, None, cout, nvox, 0)
            outs.append((on, y, st, ys))
    finally:
        L.query("pcms_conv3_small_box_mtw2", old)
    torch.cuda.synchronize()
    for on, y, st, ys in outs:
        assert_bits_equal(y, to_ndhwc(c["ref"]), f"small-box fwd mtw2={on} fill {fill}", box=(8, 8, 4))
        assert_bits_equal(ys, to_ndhwc(c["ref"]), f"small-box split-K fwd mtw2={on} fill {fill}", box=(8, 8, 4))
        check_bn(st, rows, cout, nvox, c["ref"], f"small-box mtw2={on}")


def _two_sources(c, c0, c1, dt=BF):
    x = c["x"]
    return dev_x(x[:, :c0], dt), (dev_x(x[:, c0:], dt) if c1 else None)


@pytest.mark.parametrize("fill", FILLS)
def test_conv3_fwd_big_box_exact(fill):
    """The persistent 32x32x16 big-box forward, dual source, 5 slots over 6 boxes (2 + 1 x 4):
    the first slot merges a second box into its running moments (nbdone > 0, K = the running
    mean), and no slot walks a third, so the channel sums are exact."""
    L = _lib()
    N, c0, c1, cout, cy0, S, wgs = 1, 64, 64, 64, 64, (16, 24, 16), 5
    c = conv_case("big", fill, N, c0 + c1, cout, S)
    assert_two_box_merge_exact(c["ref"], c["b"], WALK_BIG[1])
    old = L.query("pcms_conv3_big_min_boxes", 1)
    old_w = L.query("pcms_conv3_big_max_wgs", wgs)
    try:
        cin = c0 + c1
        wp = torch.empty(-(-cin // 32) * 27 * cout * 32, dtype=BF, device=DEV)
        L.call("pcms_conv3_pack", 1, c["w"].to(DEV), wp, cout, cin, 0)
        y0 = torch.full((N, *S, cy0), float("nan"), dtype=BF, device=DEV)
        nvox = N * S[0] * S[1] * S[2]
        rows = L.query("pcms_conv3_fwd_rows", 1, N, *S, c0, c1, cout)
        nbox = N * (S[0] // 8) * (S[1] // 8) * (S[2] // 16)
        assert rows == min(nbox, wgs // (cout // 64))  # big-box path taken
        stats = torch.zeros(rows * (cout * 2 + 1), device=DEV)
        xa, xb = _two_sources(c, c0, c1)
        L.call("pcms_conv3_fwd", 1, xa, c0, xb, c1, wp, c["b"].to(DEV), y0, None, cy0, None, stats, 0, N, *S, cout, 1)
        torch.cuda.synchronize()
    finally:
        L.query("pcms_conv3_big_min_boxes", old)
        L.query("pcms_conv3_big_max_wgs", old_w)
    assert_bits_equal(y0, to_ndhwc(c["ref"]), f"big-box fwd fill {fill}", box=(8, 8, 16))
    assert -(-nbox // rows) == 2
    check_bn(stats, rows, cout, nvox, c["ref"], "big-box fwd", walk=WALK_BIG + (1024,), bias=c["b"])


# ------------------------------------------------------------------ pcms_conv3_fwd16

FWD16_8DEEP = [(1, 64, 0, 64, 64, (8, 8, 16), 0),
               (2, 32, 32, 128, 64, (16, 8, 32), 0),
               (1, 16, 48, 64, 64, (8, 16, 16), 0),
               (2, 64, 0, 64, 64, (16, 16, 32), 3),
               (1, 64, 0, 256, 128, (8, 16, 16), 3)]
FWD16_4DEEP = [(1, 64, 0, 64, 64, (12, 8, 16), 0),
               (2, 16, 16, 64, 64, (20, 8, 16), 3)]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nt8,N,c0,c1,cout,cy0,S,wgs",
                         [(nt8,) + c for nt8 in (1, 0) for c in FWD16_8DEEP] + [(None,) + c for c in FWD16_4DEEP])
def test_conv3_fwd16_exact(fill, nt8, N, c0, c1, cout, cy0, S, wgs):
    """The 16x16x32 big-box kernel with the pack16 weights (tap pairs, the zero 28th tap): 8-deep
    boxes at both nt8 values (nt8 1: 128-channel outputs run on 4-deep boxes), 4-deep boxes
    (D % 8 != 0; nt8 left as it is).  With wgs 3 the slots of (16, 16, 32) walk 6 / 5 / 5 boxes,
    those of (20, 8, 16) 4 / 3 / 3, and the one slot of (8, 16, 16) -> 256 channels walks its 2
    8-deep boxes (nt8 0: exact sums) or its 4 4-deep boxes (nt8 1)."""
    L = _lib()
    cin = c0 + c1
    c = conv_case("fwd16", fill, N, cin, cout, S)
    assert_two_box_merge_exact(c["ref"], c["b"], WALK_B16[1])
    old = L.query("pcms_conv3_big_min_boxes", 1)
    old_w = L.query("pcms_conv3_big_max_wgs", wgs)
    old_nt = L.query("pcms_conv3_b16_nt8", -1 if nt8 is None else nt8)
    try:
        assert L.query("pcms_conv3_big16_ok", N, *S, c0, c1, cout) == 1
        w16, _ = _pack16(L, c["w"], cout, cin, dgrad=False)
        nvox = N * S[0] * S[1] * S[2]
        rows = L.query("pcms_conv3_fwd16_rows", N, *S, c0, c1, cout)
        # the box depth the kernel runs (b16_config: 128-channel blocks take 4-deep boxes)
        bd = 4 if S[0] % 8 or (L.query("pcms_conv3_b16_nt8", -1) and cout % 128 == 0) else 8
        y0 = torch.full((N, *S, cy0), float("nan"), dtype=BF, device=DEV)
        y1 = torch.full((N, *S, max(cout - cy0, 8)), float("nan"), dtype=BF, device=DEV)
        stats = torch.full((rows * (cout * 2 + 1),), float("nan"), device=DEV)
        xa, xb = _two_sources(c, c0, c1)
        L.call("pcms_conv3_fwd16", xa, c0, xb, c1, None, None, w16, c["b"].to(DEV), y0,
               y1 if cout > cy0 else None, cy0, stats, 0, N, *S, cout)
        torch.cuda.synchronize()
    finally:
        L.query("pcms_conv3_big_min_boxes", old)
        L.query("pcms_conv3_big_max_wgs", old_w)
        L.query("pcms_conv3_b16_nt8", old_nt)
    assert_bits_equal(join(y0, y1, cout > cy0), to_ndhwc(c["ref"]), f"fwd16 nt8={nt8} fill {fill}", box=(bd, 8, 16))
    check_bn(stats, rows, cout, nvox, c["ref"], f"fwd16 nt8={nt8}", walk=WALK_B16 + (bd * 128,), bias=c["b"])


@functools.lru_cache(maxsize=None)
def dgrad16_case(fill, N, cout, cin, S):
    g = gen("dgrad16", fill, N, cout, cin, S)
    dy, w = operands(fill, (N, cout, *S), (cout, cin, 3, 3, 3), 27 * cout, g)
    ref = F.conv_transpose3d(dy.double(), w.double(), padding=1)
    bound = F.conv_transpose3d(dy.abs().double(), w.abs().double(), padding=1).max().item()
    assert_exact_case(ref, bound, BF)
    return dy, w, ref


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nt8", [1, 0])
@pytest.mark.parametrize("N,cout,cin,S,wgs", [(1, 64, 128, (16, 16, 16), 3), (1, 64, 256, (8, 8, 16), 0)])
def test_conv3_dgrad16_exact(fill, nt8, N, cout, cin, S, wgs):
    """The dgrad pack16 form (rows Cin, k Cout, taps mirrored) with the split output."""
    L = _lib()
    dy, w, ref = dgrad16_case(fill, N, cout, cin, S)
    old = L.query("pcms_conv3_big_min_boxes", 1)
    old_w = L.query("pcms_conv3_big_max_wgs", wgs)
    old_nt = L.query("pcms_conv3_b16_nt8", nt8)
    try:
        _, d16 = _pack16(L, w, cout, cin, fwd=False)
        cy0 = cin // 2
        y0 = torch.full((N, *S, cy0), float("nan"), dtype=BF, device=DEV)
        y1 = torch.full((N, *S, cin - cy0), float("nan"), dtype=BF, device=DEV)
        L.call("pcms_conv3_fwd16", dev_x(dy, BF), cout, None, 0, None, None, d16, None, y0, y1, cy0, None, 0,
               N, *S, cin)
        torch.cuda.synchronize()
    finally:
        L.query("pcms_conv3_big_min_boxes", old)
        L.query("pcms_conv3_big_max_wgs", old_w)
        L.query("pcms_conv3_b16_nt8", old_nt)
    assert_bits_equal(join(y0, y1, True), to_ndhwc(ref), f"dgrad16 nt8={nt8} fill {fill}", box=(8, 8, 16))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("N,C,S", [(1, 64, (8, 16, 16)), (1, 64, (12, 8, 16))])
def test_conv3_fwd16_input_bn_relu_exact(fill, N, C, S):
    """The input BatchNorm + ReLU in the staging of pcms_conv3_fwd16 (8-deep and 4-deep boxes):
    isc in {1, 2}, ish in {-1, 0, 1}, so a = relu(sc y + sh) is a small integer, against the
    integer reference conv(a) -- not against the unfused kernel.  The halo stays zero
    (relu(0 sc + 1) would be 1)."""
    L = _lib()
    y1, w, sc, sh, b, ref = bnin_case(fill, N, C, S)
    nvox = N * S[0] * S[1] * S[2]
    old = L.query("pcms_conv3_big_min_boxes", 1)
    old_w = L.query("pcms_conv3_big_max_wgs", 0)
    try:
        assert L.query("pcms_conv3_big16_ok", N, *S, C, 0, C) == 1
        w16, _ = _pack16(L, w, C, C, dgrad=False)
        rows = L.query("pcms_conv3_fwd16_rows", N, *S, C, 0, C)
        y = torch.full((N, *S, C), float("nan"), dtype=BF, device=DEV)
        st = torch.full((rows * (2 * C + 1),), float("nan"), device=DEV)
        L.call("pcms_conv3_fwd16", dev_x(y1, BF), C, None, 0, sc.to(DEV), sh.to(DEV), w16, b.to(DEV), y, None, C,
               st, 0, N, *S, C)
        torch.cuda.synchronize()
    finally:
        L.query("pcms_conv3_big_min_boxes", old)
        L.query("pcms_conv3_big_max_wgs", old_w)
    assert_bits_equal(y, to_ndhwc(ref), f"fwd16 + input BN/ReLU fill {fill}", box=(4 if S[0] % 8 else 8, 8, 16))
    check_bn(st, rows, C, nvox, ref, "fwd16 + input BN/ReLU")


@functools.lru_cache(maxsize=None)
def bnin_case(fill, N, C, S):
    g = gen("bnin16", fill, N, C, S)
    # a is non-negative with E[a^2] up to ~3: a fifth of the usual terms keeps |y| <= 256
    y1, w = operands(fill, (N, C, *S), (C, C, 3, 3, 3), 27 * C, g, terms=160)
    sc = torch.randint(1, 3, (C,), generator=g).float()
    sh = torch.randint(-1, 2, (C,), generator=g).float()
    b = small_ints(C, g)
    a = torch.relu(y1 * sc.view(1, C, 1, 1, 1) + sh.view(1, C, 1, 1, 1))
    ref = F.conv3d(a.double(), w.double(), b.double(), padding=1)
    bound = F.conv3d(a.double(), w.abs().double(), b.abs().double(), padding=1).max().item()
    nvox = N * S[0] * S[1] * S[2]
    assert_exact_case(ref, bound, BF, nvox=nvox)
    return y1, w, sc, sh, b, ref


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("N,c0,c1,cout,S", [(2, 64, 0, 128, (8, 16, 8)), (2, 128, 128, 128, (4, 16, 8))])
def test_conv3_fwd16_split_exact(fill, N, c0, c1, cout, S):
    """The split-K form of the 16x16x32 kernel summed by pcms_split_epilogue: forward with BN
    partial rows, and the dgrad direction with the split output."""
    L = _lib()
    cin = c0 + c1
    c = conv_case("split16", fill, N, cin, cout, S, dgrad=True)
    sp = L.query("pcms_conv3_fwd16_split_ok", N, *S, c0, c1, cout)
    assert sp >= 2
    w16, d16 = _pack16(L, c["w"], cout, cin)
    nvox = N * S[0] * S[1] * S[2]
    acc = torch.full((sp * nvox * cout,), float("nan"), device=DEV)
    xa, xb = _two_sources(c, c0, c1)
    L.call("pcms_conv3_fwd16_split", xa, c0, xb, c1, w16, acc, N, *S, cout, sp)
    y = torch.full((N, *S, cout), float("nan"), dtype=BF, device=DEV)
    rows = L.query("pcms_split_epilogue_rows", nvox)
    stats = torch.full((rows * (cout * 2 + 1),), float("nan"), device=DEV)
    L.call("pcms_split_epilogue", 1, acc, sp, c["b"].to(DEV), y, None, cout, stats, cout, nvox, 0)
    spd = L.query("pcms_conv3_fwd16_split_ok", N, *S, cout, 0, cin)
    assert spd >= 2
    accd = torch.full((spd * nvox * cin,), float("nan"), device=DEV)
    L.call("pcms_conv3_fwd16_split", dev_x(c["dy"], BF), cout, None, 0, d16, accd, N, *S, cin, spd)
    cy0 = cin // 2 if cin >= 128 else cin
    o0 = torch.full((N, *S, cy0), float("nan"), dtype=BF, device=DEV)
    o1 = torch.full((N, *S, max(cin - cy0, 8)), float("nan"), dtype=BF, device=DEV)
    L.call("pcms_split_epilogue", 1, accd, spd, None, o0, o1 if cin > cy0 else None, cy0, None, cin, nvox, 0)
    torch.cuda.synchronize()
    assert_bits_equal(y, to_ndhwc(c["ref"]), f"fwd16 split fill {fill}", box=(4, 16, 8))
    check_bn(stats, rows, cout, nvox, c["ref"], "fwd16 split")
    assert_bits_equal(join(o0, o1, cin > cy0), to_ndhwc(c["dref"]), f"dgrad16 split fill {fill}", box=(4, 16, 8))


# ------------------------------------------------------------------ ConvTranspose

@functools.lru_cache(maxsize=None)
def convt_case(fill, Sin, Sout, cin, cout, two, code):
    """x (N, cin, *Sin), w (cin, cout, 2, 2, 2), b; the padded forward, and gout with the input,
    weight and bias gradients, all fp64 (autograd on integers: exact)."""
    N = 2
    g = gen("convt", fill, Sin, Sout, cin, cout, two)
    kw = max(cin, 8 * cout)  # products per output: forward cin, dgrad 8 taps x cout
    x = activations(fill, (N, cin, *Sin), cin, g)
    w = weights(fill, (cin, cout, 2, 2, 2), kw, g)
    gout = activations(fill, (N, cout, *Sout), 8 * cout, g)
    b = small_ints(cout, g)
    grain = 1.0 if two is None else GRAIN2
    if two == "x":
        x, gout = two_part(x, g), two_part(gout, g)
    elif two == "w":
        w = two_part(w, g)

    def fwd(xx, ww, bb):
        u = F.conv_transpose3d(xx, ww, bb, stride=2)
        dz, dyy, dxx = (Sout[i] - u.shape[2 + i] for i in range(3))
        return F.pad(u, [dxx // 2, dxx - dxx // 2, dyy // 2, dyy - dyy // 2, dz // 2, dz - dz // 2])

    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    up = fwd(xr, wr, br)
    up.backward(gout.double())
    dt = DT[code]
    assert_exact_case(up.detach(), fwd(x.abs().double(), w.abs().double(), b.abs().double()).max().item(), dt, grain)
    xa = x.abs().double().requires_grad_(True)
    fwd(xa, w.abs().double(), None).backward(gout.abs().double())
    assert_exact_case(xr.grad, xa.grad.max().item(), dt, grain)
    nout = N * Sout[0] * Sout[1] * Sout[2]
    if two is None:  # the gradients' terms are +-1 products: at most one per output voxel
        assert_exact_case(wr.grad, nout, torch.float32)
        assert_exact_case(br.grad, nout, torch.float32)
    return {"x": x, "w": w, "b": b, "gout": gout, "up": up.detach(), "dx": xr.grad, "dw": wr.grad, "db": br.grad}


CONVT = [((4, 4, 2), (8, 8, 4), 128, 64), ((2, 2, 3), (5, 4, 7), 128, 64), ((8, 8, 4), (16, 16, 8), 1024, 512)]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("code,two,Sin,Sout,cin,cout",
                         [ct + c for ct in BF16_ONLY for c in CONVT] + [ct + CONVT[0] for ct in X6])
def test_convt_exact(fill, code, two, Sin, Sout, cin, cout):
    """pcms_convt_fwd / _fwd_ws / _dgrad / _dgrad_ws (padded edges, the K-split forms of the
    small grids) and, for bf16, pcms_convt_wgrad / _wgrad_bias (fp32 sums of integers)."""
    L = _lib()
    N, dt = 2, DT[code]
    c = convt_case(fill, Sin, Sout, cin, cout, two, code)
    fp = torch.empty(L.query("pcms_convt_pack_elems", code, cin, cout), dtype=dt, device=DEV)
    dp = torch.empty(L.query("pcms_convt_pack_elems", code, cin, cout), dtype=dt, device=DEV)
    wdev = c["w"].to(DEV)
    L.call("pcms_convt_pack", code, wdev, fp, cin, cout, 0)
    L.call("pcms_convt_pack", code, wdev, dp, cin, cout, 1)
    xd, god, bd = dev_x(c["x"], dt), dev_x(c["gout"], dt), c["b"].to(DEV)
    out = torch.full((N, *Sout, cout), float("nan"), dtype=dt, device=DEV)
    L.call("pcms_convt_fwd", code, xd, fp, bd, out, N, *Sin, cin, cout, *Sout)
    nfs = L.query("pcms_convt_fwd_ws_floats", N, *Sin, cin, cout)
    outs = torch.full_like(out, float("nan"))
    fws = torch.full((max(nfs, 1),), float("nan"), device=DEV)
    L.call("pcms_convt_fwd_ws", code, xd, fp, bd, outs, fws, N, *Sin, cin, cout, *Sout)
    dx = torch.full((N, *Sin, cin), float("nan"), dtype=dt, device=DEV)
    L.call("pcms_convt_dgrad", code, god, dp, dx, N, *Sin, cin, cout, *Sout)
    nws = L.query("pcms_convt_dgrad_ws_floats", N, *Sin, cin, cout)
    dxs = torch.full_like(dx, float("nan"))
    dws = torch.full((max(nws, 1),), float("nan"), device=DEV)
    L.call("pcms_convt_dgrad_ws", code, god, dp, dxs, dws, N, *Sin, cin, cout, *Sout)
    if two is None:
        dw = torch.zeros(cin, cout, 2, 2, 2, device=DEV)
        ws = torch.empty(L.query("pcms_convt_wgrad_ws_floats", N, *Sin, cin, cout, 64), device=DEV)
        L.call("pcms_convt_wgrad", code, xd, god, dw, ws, N, *Sin, cin, cout, *Sout, 64)
        dw2, db2 = torch.zeros_like(dw), torch.zeros(cout, device=DEV)
        bws2 = torch.empty(max(1, L.query("pcms_convt_wgrad_bias_ws_floats", code, N, *Sin, cin, cout, 64)),
                           device=DEV)
        L.call("pcms_convt_wgrad_bias", code, xd, god, dw2, db2, ws, bws2, N, *Sin, cin, cout, *Sout, 64)
    torch.cuda.synchronize()
    tag = f"code {code} fill {fill} two-part {two}"
    assert_bits_equal(out, to_ndhwc(c["up"]), f"convT fwd (+pad) {tag}")
    assert_bits_equal(outs, to_ndhwc(c["up"]), f"convT fwd (+pad, K-split) {tag}")
    assert_bits_equal(dx, to_ndhwc(c["dx"]), f"convT dgrad {tag}")
    assert_bits_equal(dxs, to_ndhwc(c["dx"]), f"convT dgrad (K-split) {tag}")
    if two is None:
        assert_bits_equal(dw, c["dw"], f"convT wgrad {tag}")
        assert_bits_equal(dw2, c["dw"], f"convT wgrad (fused with bias) {tag}")
        assert_bits_equal(db2, c["db"], f"convT bias grad (fused) {tag}")


# ------------------------------------------------------------------ stem (bf16)

@functools.lru_cache(maxsize=None)
def stem_case(fill, N, S, cin):
    g = gen("stem", fill, N, S, cin)
    x, w = operands(fill, (N, cin, *S), (64, cin, 3, 3, 3), 27 * cin, g)
    b = small_ints(64, g)
    dy = activations(fill, (N, 64, *S), 27 * 64, g)
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    nvox = N * S[0] * S[1] * S[2]
    assert_exact_case(ref, 27 * cin + 4, BF, nvox=nvox)
    dw = torch.nn.grad.conv3d_weight(x.double(), (64, cin, 3, 3, 3), dy.double(), padding=1)
    assert_exact_case(dw, nvox, torch.float32)
    return {"x": x, "w": w, "b": b, "dy": dy, "ref": ref, "dw": dw}


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("cin", [5, 3])
@pytest.mark.parametrize("N,S", [(2, (16, 16, 16)), (3, (4, 4, 16)), (1, (12, 16, 32))])
def test_stem_fwd_wgrad_exact(fill, cin, N, S):
    """pcms_stem_fwd in both forms (K-dense and 14 tap pairs): the reference's values, hence each
    other's (no tie allowance: integers have no ties), exact BN channel sums; pcms_stem_wgrad in
    both column forms."""
    L = _lib()
    assert L.query("pcms_stem_supported", N, *S) == 3
    c = stem_case(fill, N, S, cin)
    xd = dev_x(c["x"], BF, 8)
    wp = torch.empty(L.query("pcms_stem_pack_elems"), dtype=BF, device=DEV)
    L.call("pcms_stem_pack", c["w"].to(DEV), wp, cin)
    nvox = N * S[0] * S[1] * S[2]
    rows = L.query("pcms_stem_fwd_rows", N, *S)
    outs = []
    for dense in (16, 0):
        y = torch.full((N, *S, 64), float("nan"), dtype=BF, device=DEV)
        stats = torch.zeros(rows * (64 * 2 + 1), device=DEV)
        L.call("pcms_stem_fwd", xd, wp, c["b"].to(DEV), y, stats, N, *S, dense)
        outs.append((dense, y, stats))
    guard = 4096
    dws = []
    dyd = dev_x(c["dy"], BF)
    ws = torch.empty(L.query("pcms_stem_wgrad_ws_floats", N, *S, cin), device=DEV)
    old = L.query("pcms_stem_wgrad_dense", -1)
    try:
        for dense in (1, 0):
            L.query("pcms_stem_wgrad_dense", dense)
            dw = torch.zeros(64 * cin * 27 + guard, device=DEV)
            L.call("pcms_stem_wgrad", xd, dyd, dw, ws, cin, N, *S)
            torch.cuda.synchronize()
            dws.append((dense, dw))
    finally:
        L.query("pcms_stem_wgrad_dense", old)
    for dense, y, stats in outs:
        assert_bits_equal(y, to_ndhwc(c["ref"]), f"stem fwd dense={dense} cin={cin} fill {fill}")
        check_bn(stats, rows, 64, nvox, c["ref"], f"stem fwd dense={dense}")
    assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
    for dense, dw in dws:
        assert dw[64 * cin * 27:].abs().max().item() == 0.0, "stem wgrad wrote past the weight gradient"
        assert_bits_equal(dw[:64 * cin * 27].view(64, cin, 3, 3, 3), c["dw"],
                          f"stem wgrad dense={dense} cin={cin} fill {fill}")


@functools.lru_cache(maxsize=None)
def stem_dgrad_case(fill, cin_w, N, S):
    g = gen("stem dgrad", fill, N, S, cin_w)
    dy, w = operands(fill, (N, 64, *S), (64, cin_w, 3, 3, 3), 27 * 64, g)
    exp = torch.nn.grad.conv3d_input((N, cin_w, *S), w.double(), dy.double(), padding=1)
    bound = torch.nn.grad.conv3d_input((N, cin_w, *S), w.abs().double(), dy.abs().double(), padding=1).max().item()
    assert_exact_case(exp, bound, torch.float32)
    return dy, w, exp


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("cin_w", [5, 3])
@pytest.mark.parametrize("N,S", [(1, (1, 1, 1)), (3, (4, 4, 16))])
def test_stem_dgrad_exact(fill, cin_w, N, S):
    """pcms_stem_dgrad, bf16 operands and fp32 dx (NCDHW): one voxel, and a batch of boxes."""
    L = _lib()
    dy, w, exp = stem_dgrad_case(fill, cin_w, N, S)
    pack = torch.empty(L.query("pcms_stem_dgrad_pack_elems", 1), dtype=BF, device=DEV)
    L.call("pcms_stem_dgrad_pack", 1, w.reshape(64, cin_w, 27).contiguous().to(DEV), pack, cin_w)
    dx = torch.full((exp.numel(),), float("nan"), device=DEV)
    L.call("pcms_stem_dgrad", 1, dev_x(dy, BF), pack, dx, N, *S, cin_w)
    torch.cuda.synchronize()
    assert_bits_equal(dx.view(N, cin_w, *S), exp, f"stem dgrad cin_w={cin_w} fill {fill} (index: n, ci, d, h, w)")


# ------------------------------------------------------------------ pcms_conv3_wgrad

@functools.lru_cache(maxsize=None)
def wgrad_case(fill, N, c0, c1, cout, S, two=None):
    """x (N, cin, *S) (5 real channels when cin is 8), dy (N, cout, *S) filled the same way, the
    integer prior contents of dw, and the fp64 weight gradient."""
    g = gen("wgrad", fill, N, c0, c1, cout, S, two)
    cin = c0 + c1
    cin_real = 5 if cin == 8 else cin
    nvox = N * S[0] * S[1] * S[2]
    grain = 1.0 if two is None else GRAIN2
    # two-part: nvox products of up to (1 + 2^-9) each in grains of 2^-12 must stay below 2^24
    dens = {"A": 1.0, "B": 0.5}[fill]
    dens_int = min(dens, 2.0 ** 23 * grain / nvox) if two else dens
    x = ternary((N, cin_real, *S), g, dens_int if two == "dy" else dens)
    dy = ternary((N, cout, *S), g, dens_int if two == "x" else dens)
    if two == "x":
        x = two_part(x, g)
    elif two == "dy":
        dy = two_part(dy, g)
    init = small_ints(cout * cin_real * 27, g)
    dw = torch.nn.grad.conv3d_weight(x.double(), (cout, cin_real, 3, 3, 3), dy.double(), padding=1)
    if two is None:
        bound = nvox + 4
    else:
        bound = torch.nn.grad.conv3d_weight(x.abs().double(), (cout, cin_real, 3, 3, 3), dy.abs().double(),
                                            padding=1).max().item() + 4
    assert_exact_case(dw, bound, torch.float32, grain)
    assert_exact_case(dw + init.double().view_as(dw), bound, torch.float32, grain)
    return {"x": x, "dy": dy, "init": init, "dw": dw, "cin_real": cin_real}


def run_wgrad(L, code, c, N, c0, c1, cout, S, store, what):
    dt = DT[code]
    cin_real = c["cin_real"]
    guard = 4096
    n = cout * cin_real * 27
    dw_full = torch.zeros(n + guard, device=DEV)
    dw_full[:n] = c["init"].to(DEV)
    ws = torch.empty(L.query("pcms_conv3_wgrad_ws_floats", code, N, *S, c0, c1, cout, 256), device=DEV)
    x = c["x"]
    dyd = dev_x(c["dy"], dt)
    if c1:
        L.call("pcms_conv3_wgrad", code, dev_x(x[:, :c0], dt), c0, dev_x(x[:, c0:], dt), c1, dyd, dw_full, ws,
               N, *S, cout, cin_real, 256, store)
    else:
        L.call("pcms_conv3_wgrad", code, dev_x(x, dt, c0), c0, None, 0, dyd, dw_full, ws, N, *S, cout, cin_real,
               256, store)
    torch.cuda.synchronize()
    assert dw_full[n:].abs().max().item() == 0.0, "wgrad wrote past the weight gradient"
    exp = c["dw"] if store else c["dw"] + c["init"].double().view_as(c["dw"])
    assert_bits_equal(dw_full[:n].view(cout, cin_real, 3, 3, 3), exp, what + " (index: co, ci, kd, kh, kw)")


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("store", [1, 0])
@pytest.mark.parametrize("tg", [64, 0])
@pytest.mark.parametrize("k16", [1, 0])
@pytest.mark.parametrize("N,c0,c1,cout,S", [(1, 64, 0, 64, (9, 10, 11)), (2, 64, 64, 64, (8, 8, 8)),
                                            (2, 128, 0, 128, (16, 16, 8)), (2, 64, 0, 64, (8, 8, 4))])
def test_conv3_wgrad_exact(fill, store, tg, k16, N, c0, c1, cout, S):
    """The bf16 weight gradient, stored (the buffer's old contents must not leak) or accumulated
    onto integer contents; both MFMA forms, tap groups on and off; guard words past the end."""
    L = _lib()
    c = wgrad_case(fill, N, c0, c1, cout, S)
    old_tg = L.query("pcms_conv3_wgrad_tg_maxbox", tg)
    old_k = L.query("pcms_conv3_wgrad_k16", k16)
    try:
        run_wgrad(L, 1, c, N, c0, c1, cout, S, store, f"wgrad k16={k16} tg={tg} store={store} fill {fill}")
    finally:
        L.query("pcms_conv3_wgrad_tg_maxbox", old_tg)
        L.query("pcms_conv3_wgrad_k16", old_k)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("two", ["x", "dy"])
@pytest.mark.parametrize("x6dma", [1, 0])
@pytest.mark.parametrize("N,c0,c1,cout,S", [(2, 8, 0, 64, (16, 16, 16)), (2, 64, 64, 64, (8, 8, 8))])
def test_conv3_wgrad_x6_exact(fill, two, x6dma, N, c0, c1, cout, S):
    """fp32 build (bf16x6) weight gradient, the box stream and the register staging: x two-part
    with integer dy, then the reverse (the products hm / mh of the voxel-K split tiles)."""
    L = _lib()
    c = wgrad_case(fill, N, c0, c1, cout, S, two)
    old = L.query("pcms_conv3_wgrad_x6_dma", x6dma)
    try:
        for store in (1, 0):
            run_wgrad(L, 0, c, N, c0, c1, cout, S, store, f"x6 wgrad dma={x6dma} two-part {two} store={store} {fill}")
    finally:
        L.query("pcms_conv3_wgrad_x6_dma", old)
