"""The streaming kernels of csrc/ops_bn.hip (BatchNorm + ReLU forward / backward), ops_pool.hip
(the pool fusions), ops_head.hip (the 1x1x1 head), ops_update.hip (the loss, Adam, the gradient
clip) and ops_layout.hip (pack / unpack / add) in the regimes the
product runs them in: several trips per thread under a capped grid (unrolled main loop + tail,
``VoxQR`` steps across sample boundaries) and both finalize paths of the partial-row reductions
(split at 512 rows; ``colsum2_kernel``'s 4-rows-in-flight loop from 769 rows).

A. the finalize paths over synthetic partial rows (no switch);
B. every kernel at a small shape with ``pcms_stream_grid_cap`` at 1 and 3;
C. the product's own caps, reached by shape (no switch);
D. the whole training step with the switch at 3, against the goldens.

References are explicit fp64 formulas on the same already-rounded inputs and the same fp32
coefficient vectors (scale, shift, mean, invstd, coef) the kernel receives -- not autograd through
``batch_norm`` -- so the ReLU mask is decided identically (``fma(y, sc, sh)`` is correctly rounded:
its sign is the exact sign, and ``y * sc`` is exact in fp64) and no element is excluded.

Tolerances: per-element outputs and all of B use the bar of the existing op test of the same
entry point (tests/test_gpu_ops.py, test_input_grad_ops.py, test_step_variants.py).  A's outputs
are fp64 sums rounded once to fp32: ``close(..., 1e-6)``.  Reduced outputs of C use the a-priori
bound of recursive fp32 summation, ``|err| <= 2 (trips + 64) 2^-24 sum|t_i|`` per output, with
``sum|t_i|`` from the reference's own terms in fp64, ``trips`` the accumulations per thread taken
from the library's row query, 64 for the in-block combine and 2 for the rounding of each product.
Adam asserts on the step: ``|dp - dp_ref| <= 2^-23 max|p| + 1e-4 max|dp_ref|``.  Every C case and
every Adam case prints its err / bound ratio as a ``MARGIN`` line (``pytest -s``); the ratios
measured on the MI355X are in profiles/stream_regime_margins.json.
"""
import contextlib
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_parity as parity
from tests.test_gpu_ops import DEV, DTS, _lib, close, head_case, ncdhw, ndhwc

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
TPB = 256          # threads per block of every kernel here
CAPS = [1, 3]      # section B's values of the switch
SMALL_ROWS = 512   # rows <= this: the one-launch finalize (kSmallRows)
COLSUM2_MAIN = 768  # rows > this: colsum2_kernel's main loop runs (64 row groups x 4 lanes x 3 + 1)


@contextlib.contextmanager
def grid_cap(v):
    """pcms_stream_grid_cap set to v for the body (v <= 0: left as it is), then restored."""
    L = _lib()
    old = L.query("pcms_stream_grid_cap", v)
    try:
        yield L
    finally:
        L.query("pcms_stream_grid_cap", old)


def cdiv(a, b):
    return -(-a // b)


def f32(x):
    return float(np.float32(x))


def margin(test, err, bound, **extra):
    rec = {"test": test, "err": float(err), "bound": float(bound), "err_over_bound": float(err) / float(bound)}
    rec.update(extra)
    print("\nMARGIN " + json.dumps(rec))
    return rec["err_over_bound"]


def sum_bound(test, got, ref, abs_sum, trips):
    """got (fp32, device or cpu) vs ref (fp64) per output under the recursive-summation bound."""
    bound = 2.0 * (trips + 64) * U24 * abs_sum.double()
    err = (got.double().cpu().reshape(-1) - ref.double().reshape(-1)).abs()
    bound = bound.reshape(-1)
    # (a channel whose ReLU passes nothing has no terms: its sum is exactly 0)
    assert (err[bound == 0] == 0).all() and (bound > 0).any(), test
    i = int(torch.where(bound > 0, err / bound, torch.zeros_like(err)).argmax())
    r = margin(test, err[i], bound[i], trips=int(trips))
    assert r <= 1.0, f"{test}: err {err[i]:.3e} > bound {bound[i]:.3e} (output {i})"


# (the switch's own set / query / restore behaviour: tests/test_capi.py, no GPU needed)
# ---------------------------------------------------------------------------------------------
# A. finalize paths over synthetic partial rows
# ---------------------------------------------------------------------------------------------
ROWS_A = [1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 768, 769, 1025, 2500]


def test_rows_cover_every_finalize_path():
    one = [r for r in ROWS_A if r <= SMALL_ROWS]
    assert any(r <= 256 for r in one) and any(r > 256 for r in one)    # one and two 256-row trips
    assert any(SMALL_ROWS < r <= COLSUM2_MAIN for r in ROWS_A)           # two-stage, colsum2's tail only
    assert any(r > COLSUM2_MAIN for r in ROWS_A)                         # two-stage, its main loop
    assert any(r > 4 * 256 + COLSUM2_MAIN for r in ROWS_A)               # main loop twice + tail


@pytest.mark.parametrize("ratio", [0.3, 50.0])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("rows", ROWS_A)
def test_bn_finalize_paths(rows, C, ratio):
    L = _lib()
    g = torch.Generator().manual_seed(rows * 3 + C)
    cnt = torch.tensor([0.0, 1.0, 7.0, 64.0])[torch.randint(0, 4, (rows,), generator=g)]
    cnt[0] = 64.0
    std = torch.rand(C, generator=g) + 0.5
    mu = ratio * std * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    n = cnt[:, None]
    rmean = mu + std * torch.randn(rows, C, generator=g) / n.clamp_min(1).sqrt()
    s = (rmean * n).float()                                                      # n = 0: zero
    m2 = (std ** 2 * (n - 1).clamp_min(0) * (0.5 + torch.rand(rows, C, generator=g))).float()  # n <= 1: zero
    part = torch.cat([torch.stack([s, m2], -1).flatten(), cnt]).contiguous()
    count = float(cnt.sum())
    # fp64 Chan merge of the same fp32 rows (tests.test_gpu_ops.bn_moments)
    sd, md, nd = s.double(), m2.double(), cnt.double()[:, None]
    mean = sd.sum(0) / count
    nz = cnt > 0
    var = (md.sum(0) + (nd[nz] * (sd[nz] / nd[nz] - mean) ** 2).sum(0)) / count
    inv = 1.0 / torch.sqrt(var + 1e-5)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    mom = f32(0.1)
    exp = {"scale": gamma.double() * inv, "shift": beta.double() - mean * gamma.double() * inv, "mean": mean,
           "invstd": inv, "running_mean": (1 - mom) * rm.double() + mom * mean,
           "running_var": (1 - mom) * rv.double() + mom * var * count / (count - 1)}
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    nbt = torch.full((), 5, dtype=torch.int64, device=DEV)
    out = {k: torch.full((C,), float("nan"), device=DEV) for k in ("scale", "shift", "mean", "invstd")}
    ws = torch.empty(L.query("pcms_bn_ws_doubles", C), dtype=torch.float64, device=DEV)
    L.call("pcms_bn_finalize", part.to(DEV), rows, C, count, gamma.to(DEV), beta.to(DEV), rmd, rvd, nbt, 0.1, 1e-5,
           out["scale"], out["shift"], out["mean"], out["invstd"], ws)
    torch.cuda.synchronize()
    out.update(running_mean=rmd, running_var=rvd)
    assert int(nbt) == 6
    for k, e in exp.items():
        close(out[k], e, 1e-6, f"bn_finalize rows={rows} {k}")


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("rows", ROWS_A)
def test_bn_bwd_finish_paths(rows, C):
    L = _lib()
    g = torch.Generator().manual_seed(rows * 5 + C)
    part = torch.randn(rows, C, 2, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1
    invstd = torch.rand(C, generator=g) + 0.2
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)  # the kernels add into them
    nvox = 3 * rows + 5
    s1, s2 = part[:, :, 0].double().sum(0), part[:, :, 1].double().sum(0)
    k1 = gamma.double() * invstd.double()
    coef_ref = torch.stack([k1, -k1 * s2 / nvox, -k1 * s1 / nvox], 1)
    dg, db = dg0.to(DEV), db0.to(DEV)
    coef = torch.full((3 * C,), float("nan"), device=DEV)
    ws = torch.empty(L.query("pcms_bn_ws_doubles", C), dtype=torch.float64, device=DEV)
    L.call("pcms_bn_relu_bwd_finish", 0, None, None, None, None, None, invstd.to(DEV), gamma.to(DEV), part.to(DEV),
           rows, coef, dg, db, None, C, nvox, ws)
    torch.cuda.synchronize()
    close(db, db0.double() + s1, 1e-6, f"bwd finish rows={rows} dbeta")
    close(dg, dg0.double() + s2, 1e-6, f"bwd finish rows={rows} dgamma")
    for j, what in enumerate(("k1", "k2", "k3")):
        close(coef.view(C, 3)[:, j], coef_ref[:, j], 1e-6, f"bwd finish rows={rows} {what}")


# ---------------------------------------------------------------------------------------------
# fp64 references of the BatchNorm + ReLU family, channels last: y, da (nvox, C) fp64
# ---------------------------------------------------------------------------------------------
def bn_coeffs(y, gamma, beta):
    """The fp32 coefficient vectors of a train-mode BatchNorm over y (nvox, C) fp64."""
    m = y.mean(0)
    inv = 1.0 / torch.sqrt(y.var(0, unbiased=False) + 1e-5)
    sc = (gamma.double() * inv).float()
    sh = (beta.double() - m * gamma.double() * inv).float()
    return sc, sh, m.float(), inv.float()


def bn_bwd_ref(y, da, sc, sh, mean, invstd, gamma):
    """mask, (sum g, sum g xhat) with their absolute sums, coef and dy = k1 g + k2 xhat + k3."""
    nvox = y.shape[0]
    mask = y * sc.double() + sh.double() > 0
    gq = da * mask
    xhat = (y - mean.double()) * invstd.double()
    t2 = gq * xhat
    s1, s2 = gq.sum(0), t2.sum(0)
    k1 = gamma.double() * invstd.double()
    k2, k3 = -k1 * s2 / nvox, -k1 * s1 / nvox
    dy = k1 * gq + k2 * xhat + k3
    return {"mask": mask, "s1": s1, "s2": s2, "abs1": gq.abs().sum(0), "abs2": t2.abs().sum(0),
            "coef": torch.stack([k1, k2, k3], 1), "dy": dy}


def vec_lanes(code, C):
    """(VEC, VL): channels per 16-byte vector and voxel lanes per block of the BN kernels."""
    vec = 8 if code else 4
    return vec, TPB // (C // vec)


# ---------------------------------------------------------------------------------------------
# B. capped grids at small shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dt,code,tol", DTS)
@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024])
def test_bn_relu_family_capped(C, dt, code, tol, cap):
    N, S = 2, (3, 5, 7)
    nvox = N * S[0] * S[1] * S[2]
    g = torch.Generator().manual_seed(11 + C)
    y = (torch.randn(nvox, C, generator=g) * 3 + 1).to(dt)
    da = torch.randn(nvox, C, generator=g).to(dt)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1  # the mask is on the product, not on y
    beta = torch.randn(C, generator=g)
    sc, sh, mean, invstd = bn_coeffs(y.double(), gamma, beta)
    ref = bn_bwd_ref(y.double(), da.double(), sc, sh, mean, invstd, gamma)
    with grid_cap(cap) as L:
        rows = L.query("pcms_bn_bwd_rows", code, C, nvox)
        vec, VL = vec_lanes(code, C)
        assert rows == min(cap, cdiv(nvox, VL * 4))  # (C = 64 bf16: 128 voxels per block, two blocks)
        assert nvox % (VL * 4) != 0
        assert nvox > 2 * rows * VL, "the reduce kernel's two-rows-in-flight loop does not run"
        yd, dad = y.to(DEV), da.to(DEV)
        co = [t.to(DEV) for t in (sc, sh, mean, invstd)]
        a = torch.full_like(yd, float("nan"))
        L.call("pcms_bn_relu", code, yd, a, co[0], co[1], C, nvox)
        part = torch.empty(rows * C * 2, device=DEV)
        coef = torch.empty(3 * C, device=DEV)
        dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dy = torch.full_like(yd, float("nan"))
        ws = torch.empty(L.query("pcms_bn_ws_doubles", C), dtype=torch.float64, device=DEV)
        L.call("pcms_bn_relu_bwd", code, dad, yd, *co, gamma.to(DEV), part, coef, dgam, dbet, dy, C, nvox, ws)
        dye = torch.full_like(yd, float("nan"))
        L.call("pcms_bn_relu_bwd_eval", code, dad, yd, co[0], co[1], dye, C, nvox)
        torch.cuda.synchronize()
    z = y.double() * sc.double() + sh.double()
    close(a, torch.relu(z), tol, "bn+relu fwd")
    close(dy, ref["dy"], 5 * tol, "bn+relu bwd")
    close(dgam, ref["s2"], 1e-3 if code else 1e-5, "dgamma")
    close(dbet, ref["s1"], 1e-3 if code else 1e-5, "dbeta")
    close(dye, da.double() * ref["mask"] * sc.double(), tol, "eval bn+relu bwd")


def pool_chain(L, dt, code, C, N, S, seed=6):
    """The Down3D boundary chain on the device and its fp64 reference.  Returns what the callers
    assert on: device outputs, reference values, the row counts."""
    D, H, W = S
    nvox = N * D * H * W
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(N, C, *S, generator=g) * 1.5).to(dt)
    y[:, :, :2, :2, :2] = -3.0  # ReLU ties at zero inside a pooling cell
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    P = tuple(s // 2 for s in S)
    dp = torch.randn(N, C, *P, generator=g).to(dt)
    skip = torch.randn(N, C, *S, generator=g).to(dt)
    yl = ndhwc(y).reshape(nvox, C).double()
    sc, sh, mean, invstd = bn_coeffs(yl, gamma, beta)
    co = [t.to(DEV) for t in (sc, sh, mean, invstd)]
    gd = gamma.to(DEV)
    yd, dpd = ndhwc(y).to(DEV), ndhwc(dp).to(DEV)
    o = {}
    # forward: unfused and fused
    a0, p0 = torch.empty_like(yd), torch.empty(N, *P, C, dtype=dt, device=DEV)
    L.call("pcms_bn_relu", code, yd, a0, co[0], co[1], C, nvox)
    L.call("pcms_maxpool_fwd", code, a0, p0, N, *S, C)
    a1, p1 = torch.full_like(a0, float("nan")), torch.full_like(p0, float("nan"))
    L.call("pcms_bn_relu_pool", code, yd, a1, p1, co[0], co[1], N, *S, C)
    # backward: unfused, fused with the stored da, fused consumer form
    r0 = L.query("pcms_bn_bwd_rows", code, C, nvox)
    r1 = L.query("pcms_maxpool_bwd_bn_rows", code, N, *S, C)
    part = torch.empty(max(r0, r1) * C * 2, device=DEV)
    coef = torch.empty(3 * C, device=DEV)
    bnws = torch.empty(L.query("pcms_bn_ws_doubles", C), dtype=torch.float64, device=DEV)
    da0 = ndhwc(skip).to(DEV)
    L.call("pcms_maxpool_bwd", code, a0, dpd, da0, N, *S, C)
    dg0, db0, dy0 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.full_like(yd, float("nan"))
    L.call("pcms_bn_relu_bwd", code, da0, yd, *co, gd, part, coef, dg0, db0, dy0, C, nvox, bnws)
    da1 = ndhwc(skip).to(DEV)
    part.fill_(float("nan"))
    L.call("pcms_maxpool_bwd_bn", code, yd, *co, dpd, da1, part, N, *S, C)
    part1 = part[: r1 * C * 2].clone()
    dg1, db1, dy1 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.full_like(yd, float("nan"))
    L.call("pcms_bn_relu_bwd_finish", code, da1, yd, *co, gd, part, r1, coef, dg1, db1, dy1, C, nvox, bnws)
    da2 = ndhwc(skip).to(DEV)
    part.fill_(float("nan"))
    L.call("pcms_maxpool_bwd_bn_sums", code, yd, *co, dpd, da2, part, N, *S, C)
    part2 = part[: r1 * C * 2].clone()
    dg2, db2, dy2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.full_like(yd, float("nan"))
    L.call("pcms_bn_relu_bwd_finish", code, da2, yd, *co, gd, part, r1, coef, dg2, db2, None, C, nvox, bnws)
    L.call("pcms_maxpool_bn_apply", code, yd, *co, coef, dpd, da2, dy2, N, *S, C)
    torch.cuda.synchronize()
    # the fused forms against the unfused ones, as tests.test_gpu_ops does
    assert torch.equal(da2, ndhwc(skip).to(DEV)), "pcms_maxpool_bwd_bn_sums wrote da"
    assert torch.equal(part1, part2), "partial rows differ"
    assert torch.equal(dg1, dg2) and torch.equal(db1, db2)
    assert torch.equal(dy1.view(torch.uint8), dy2.view(torch.uint8))
    assert torch.equal(a0, a1) and torch.equal(p0, p1)
    assert torch.equal(da0, da1)
    # fp64 reference from the kernels' stated semantics: a = round_T(relu(fma(y, sc, sh))) as
    # stored; the argmax is the first maximum of the stored values in scan order
    o["a_ref"] = torch.relu(yl * sc.double() + sh.double())
    a_st = ncdhw(a1.cpu()).double()
    p_st, idx = F.max_pool3d(a_st, 2, return_indices=True)
    pooled = torch.zeros(N, C, D * H * W, dtype=torch.float64)
    pooled.scatter_add_(2, idx.view(N, C, -1), dp.double().view(N, C, -1))
    da_ref = (skip.double() + pooled.view(N, C, D, H, W)).to(dt).double()  # stored (and summed) rounded to T
    ref = bn_bwd_ref(yl, ndhwc(da_ref).reshape(nvox, C), sc, sh, mean, invstd, gamma)
    o.update(a=a1.view(nvox, C), p=p1, p_ref=ndhwc(p_st), da=da1.view(nvox, C), da_ref=ndhwc(da_ref).reshape(nvox, C),
             dy=dy1.view(nvox, C), dy_unfused=dy0.view(nvox, C), dg=dg1, db=db1, dg_unfused=dg0, db_unfused=db0,
             ref=ref, rows_bn=r0, rows_pool=r1, nvox=nvox)
    return o


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dt,code,tol", DTS)
@pytest.mark.parametrize("S", [(7, 5, 9), (8, 6, 10)])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_pool_chain_capped(C, S, dt, code, tol, cap):
    N = 2
    with grid_cap(cap) as L:
        o = pool_chain(L, dt, code, C, N, S)
        vec, VL = vec_lanes(code, C)
        cells = N * cdiv(S[0], 2) * cdiv(S[1], 2) * cdiv(S[2], 2)
        assert o["rows_pool"] == cap and o["rows_bn"] == cap
        assert cells * (C // vec) > o["rows_pool"] * TPB, "a thread of the cell kernels makes one trip only"
        # (the plain pool kernels have one thread per pooled cell and vector: C = 64 bf16 has 384)
        assert N * (S[0] // 2) * (S[1] // 2) * (S[2] // 2) * (C // vec) > min(CAPS) * TPB
        assert o["nvox"] > 2 * o["rows_bn"] * VL
    ref = o["ref"]
    close(o["a"], o["a_ref"], tol, "bn+relu (pool) fwd")
    assert torch.equal(o["p"].cpu().double(), o["p_ref"]), "pooled output is not the max of the stored a"
    close(o["da"], o["da_ref"], tol, "da = skip + dp at the argmax")
    close(o["dg"], o["dg_unfused"], 1e-5, "dgamma fused vs unfused")
    close(o["db"], o["db_unfused"], 1e-5, "dbeta fused vs unfused")
    close(o["dy"], o["dy_unfused"], 1e-5 if not code else 1e-2, "dy fused vs unfused")
    # vs fp64: the fp32 bars of the existing chain test; bf16 sums the same T-rounded da in fp32
    # (pcms_bn_relu_bwd's bf16 bar for dgamma / dbeta) and rounds dy to bf16 once
    close(o["dy"], ref["dy"], 1e-4 if not code else 1e-2, "dy vs fp64")
    close(o["dg"], ref["s2"], 1e-4 if not code else 1e-3, "dgamma vs fp64")
    close(o["db"], ref["s1"], 1e-4 if not code else 1e-3, "dbeta vs fp64")


HEAD_N, HEAD_S = 3, (5, 6, 7)


def head_preconditions(L, cap, N, V):
    rows = L.query("pcms_head_bn_bwd_rows", V, N)
    assert rows == cap
    assert L.query("pcms_head_bwd_ws_floats", V, N, 1) == (rows + 1) * 65
    stride = rows * TPB // 8  # voxels per trip of the whole grid
    assert N * V > 4 * stride, "the 4-voxels-in-flight loops do not run"
    assert V % stride != 0, "trips end on the sample boundaries"
    return rows


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dt,code,tol", DTS)
@pytest.mark.parametrize("ncls", [1, 2, 3, 4])
def test_head_capped(ncls, dt, code, tol, cap):
    with grid_cap(cap) as L:
        head_preconditions(L, cap, HEAD_N, HEAD_S[0] * HEAD_S[1] * HEAD_S[2])
        head_case(L, dt, code, tol, ncls, HEAD_N, HEAD_S)


def head_bn_case(L, dt, code, tol, ncls, N, S, shift):
    """pcms_head_bn_fwd / _bwd / _bwd_eval against the unfused sequence and explicit fp64."""
    C = 64
    V = S[0] * S[1] * S[2]
    nvox = N * V
    g = torch.Generator().manual_seed(4 + ncls)
    y = (torch.randn(N, V, C, generator=g) * 2 + shift).to(dt)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    w = torch.randn(ncls, C, generator=g) * 0.1
    b = torch.randn(ncls, generator=g)
    dl = torch.randn(N, ncls, V, generator=g)
    yl = y.reshape(nvox, C).double()
    sc, sh, mean, invstd = bn_coeffs(yl, gamma, beta)
    co = [t.to(DEV) for t in (sc, sh, mean, invstd)]
    yd, W2, bd, dld, gd = y.to(DEV), w.to(DEV), b.to(DEV), dl.to(DEV), gamma.to(DEV)
    # unfused
    a = torch.empty_like(yd)
    L.call("pcms_bn_relu", code, yd, a, co[0], co[1], C, nvox)
    lg0 = torch.empty(N, ncls, V, device=DEV)
    L.call("pcms_head_fwd", code, a, W2, bd, lg0, V, N, ncls, 0, 0.5)
    ws = torch.empty(L.query("pcms_head_bwd_ws_floats", V, N, ncls), device=DEV)
    da = torch.empty_like(yd)
    dw0, db0 = torch.zeros(ncls, 64, device=DEV), torch.zeros(ncls, device=DEV)
    L.call("pcms_head_bwd", code, a, dld, W2, da, dw0, db0, ws, V, N, ncls)
    rows = max(L.query("pcms_bn_bwd_rows", code, C, nvox), L.query("pcms_head_bn_bwd_rows", V, N))
    part = torch.empty(rows * C * 2, device=DEV)
    coef = torch.empty(3 * C, device=DEV)
    bnws = torch.empty(L.query("pcms_bn_ws_doubles", C), dtype=torch.float64, device=DEV)
    dg0, dbt0 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dy0 = torch.empty_like(yd)
    L.call("pcms_bn_relu_bwd", code, da, yd, *co, gd, part, coef, dg0, dbt0, dy0, C, nvox, bnws)
    # fused
    lg1 = torch.full_like(lg0, float("nan"))
    L.call("pcms_head_bn_fwd", code, yd, co[0], co[1], W2, bd, lg1, V, N, ncls, 0, 0.5)
    dw1, db1 = torch.zeros_like(dw0), torch.zeros_like(db0)
    dg1, dbt1 = torch.zeros_like(dg0), torch.zeros_like(dbt0)
    dy1 = torch.full_like(yd, float("nan"))
    L.call("pcms_head_bn_bwd", code, yd, *co, gd, dld, W2, dw1, db1, ws, part, coef, dg1, dbt1, dy1, V, N, ncls, bnws)
    dye = torch.full_like(yd, float("nan"))
    L.call("pcms_head_bn_bwd_eval", code, yd, co[0], co[1], dld, W2, dye, V, N, ncls)
    torch.cuda.synchronize()
    assert torch.equal(lg0, lg1)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    close(dg1, dg0, 1e-5, "dgamma fused vs unfused")
    close(dbt1, dbt0, 1e-5, "dbeta fused vs unfused")
    close(dy1, dy0, 1e-5 if not code else 1e-2, "dy fused vs unfused")
    # explicit fp64: the head input is a2 = round_T(relu(fma(y, sc, sh))) as pcms_bn_relu stores
    # it; the head's gradient is rounded to T before it feeds the BatchNorm-backward sums
    close(a, torch.relu(yl * sc.double() + sh.double()).view(N, V, C), tol, "stored head input")
    a2 = a.cpu().double()
    dl64 = dl.double()
    lg_ref = torch.einsum("nvc,kc->nkv", a2, w.double()) + b.double().view(1, ncls, 1)
    da_lin = torch.einsum("nkv,kc->nvc", dl64, w.double())
    ref = bn_bwd_ref(yl, da_lin.to(dt).double().reshape(nvox, C), sc, sh, mean, invstd, gamma)
    close(lg1, lg_ref, 1e-5 if not code else 2e-2, "fused logits vs fp64")
    close(dy1.view(nvox, C), ref["dy"], 1e-4 if not code else 3e-2, "fused dy vs fp64")
    close(dg1, ref["s2"], 1e-4 if not code else 3e-2, "fused dgamma vs fp64")
    close(dbt1, ref["s1"], 1e-4 if not code else 3e-2, "fused dbeta vs fp64")
    close(dw1, torch.einsum("nkv,nvc->kc", dl64, a2), 1e-5 if not code else 2e-2, "fused head wgrad vs fp64")
    close(db1, dl64.sum((0, 2)), 1e-5, "fused head bias grad vs fp64")
    close(dye.view(nvox, C), da_lin.reshape(nvox, C) * ref["mask"] * sc.double(), tol, "eval head + bn bwd")


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dt,code,tol,shift", [d + (0.3,) for d in DTS] + [DTS[0] + (100.0,)])
@pytest.mark.parametrize("ncls", [1, 2, 3, 4])
def test_head_bn_capped(ncls, dt, code, tol, shift, cap):
    with grid_cap(cap) as L:
        head_preconditions(L, cap, HEAD_N, HEAD_S[0] * HEAD_S[1] * HEAD_S[2])
        head_bn_case(L, dt, code, tol, ncls, HEAD_N, HEAD_S, shift)


def loss_ref(x, t, smooth, wb, wd, gout):
    """fp64: the four sums with their absolute sums, the loss and dL/dx."""
    x, t = x.double().reshape(-1), t.double().reshape(-1)
    M = x.numel()
    p = torch.sigmoid(x)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    terms = torch.stack([p * t, p, t, bce])
    sums = terms.sum(1)
    I, P, T, B = sums.tolist()
    den, num = P + T + smooth, 2 * I + smooth
    loss = wb * B / M + wd * (1 - num / den)
    dx = gout * (wb * (p - t) / M + wd * (-(2 * t * den - num) / den ** 2) * p * (1 - p))
    return sums, terms.abs().sum(1), loss, dx


def loss_inputs(M, seed, background=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, generator=g) * 3
    idx = torch.randperm(M, generator=g)[:400]
    x[idx] = torch.tensor([30.0, -30.0, 90.0, -90.0]).repeat(100)  # saturated sigmoid / softplus
    t = torch.zeros(M) if background else (torch.rand(M, generator=g) < 0.3).float()
    return x, t


def run_loss(L, x, t, wb, wd, gout):
    M = x.numel()
    rows = L.query("pcms_loss_rows", M)
    part = torch.full((rows * 4,), float("nan"), device=DEV)
    sums = torch.empty(4, dtype=torch.float64, device=DEV)
    loss = torch.empty((), device=DEV)
    xd, td = x.to(DEV), t.to(DEV)
    L.call("pcms_loss_fwd", xd, td, M, 1.0, wb, wd, part, sums, loss)
    dx = torch.full_like(xd, float("nan"))
    L.call("pcms_loss_bwd", xd, td, M, sums, 1.0, wb, wd, None if gout is None else torch.tensor(gout, device=DEV), dx)
    torch.cuda.synchronize()
    return rows, sums.cpu(), loss.item(), dx.cpu()


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("gout", [None, 0.7])
@pytest.mark.parametrize("wb,wd,background", [(0.0, 1.0, False), (0.5, 0.5, False), (1.0, 0.0, False),
                                              (0.5, 0.5, True)])
def test_loss_capped(wb, wd, background, gout, cap):
    M = 2 * 23 * 24 * 25
    x, t = loss_inputs(M, 2, background)
    with grid_cap(cap) as L:
        rows, sums, loss, dx = run_loss(L, x, t, wb, wd, gout)
        assert rows == cap
        assert M > 2 * 8 * rows * TPB and M % (rows * TPB) != 0, "not two 8-way trips plus a tail per thread"
    rs, _, rl, rdx = loss_ref(x, t, 1.0, wb, wd, 1.0 if gout is None else f32(gout))
    assert abs(loss - rl) < 1e-6, (loss, rl)
    close(sums, rs, 1e-6, "loss sums")
    close(dx, rdx, 1e-5, "loss grad")


ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_coef(step, wd):
    return (ADAM["lr"] / (1 - ADAM["b1"] ** step), ADAM["b1"], ADAM["b2"], ADAM["eps"], wd,
            math.sqrt(1 - ADAM["b2"] ** step))


def adam_ref(p, g, m, v, coef, s):
    """One step in fp64 from the fp32 state, with the fp32 coefficients the kernel receives;
    returns (p, g written back, m, v)."""
    step_size, b1, b2, eps, wd, bc2 = (f32(c) for c in coef)
    one_b1, one_b2 = f32(1.0 - b1), f32(1.0 - b2)
    gw = g if s == 1.0 else g * torch.tensor(s, dtype=torch.float32)  # fp32 product, written back
    gi = gw.double()
    if wd != 0.0:
        gi = gi + wd * p.double()
    m1 = m.double() + one_b1 * (gi - m.double())
    v1 = v.double() * b2 + one_b2 * gi * gi
    p1 = p.double() - step_size * (m1 / (torch.sqrt(v1) / bc2 + eps))
    return p1, gw, m1, v1


def adam_check(test, before, after, ref, sel=None):
    """|dp - dp_ref| <= 2^-23 max|p| + 1e-4 max|dp_ref|; m, v at 1e-6; returns err / bound."""
    (p0, _, _, _), (p1, g1, m1, v1), (pr, gr, mr, vr) = before, after, ref
    if sel is not None:
        p0, p1, g1, m1, v1, pr, gr, mr, vr = (t[sel] for t in (p0, p1, g1, m1, v1, pr, gr, mr, vr))
    dp, dpr = p1.double() - p0.double(), pr - p0.double()
    bound = 2.0 ** -23 * p0.abs().max().item() + 1e-4 * dpr.abs().max().item()
    err = (dp - dpr).abs().max().item()
    r = margin(test, err, bound)
    assert r <= 1.0, f"{test}: step err {err:.3e} > {bound:.3e}"
    close(m1, mr, 1e-6, test + " m")
    close(v1, vr, 1e-6, test + " v")
    assert torch.equal(g1.view(torch.int32), gr.view(torch.int32)), test + ": g written back"
    return r


def run_adam(L, test, n, gscale, gmul, wd, seed=4):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gm = None if gmul is None else torch.tensor([gmul], device=DEV)
    s = f32(gscale) if gmul is None else f32(f32(gscale) * f32(gmul))
    worst = 0.0
    for step in range(1, 4):
        gr = torch.randn(n, generator=g).to(DEV)
        before = tuple(t.cpu().clone() for t in (p, gr, m, v))
        coef = adam_coef(step, wd)
        L.call("pcms_adam", p, gr, m, v, n, *coef, gscale, gm)
        torch.cuda.synchronize()
        worst = max(worst, adam_check(f"{test}_step{step}", before, tuple(t.cpu() for t in (p, gr, m, v)),
                                      adam_ref(*before, coef, s)))
    return worst


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("gmul", [None, 0.25])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_adam_capped(gscale, gmul, wd, cap):
    n = 10007
    with grid_cap(cap) as L:
        assert n > cap * TPB  # (pcms_adam has no row query: its grid is min(16384, the switch))
        run_adam(L, f"adam_n{n}_cap{cap}_gs{gscale}_gm{gmul}_wd{wd}", n, gscale, gmul, wd)


def ranges_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1,
            torch.rand(n, generator=g) * 0.01]


def run_adam_ranges(L, test, n, rng, seed=8):
    """pcms_adam_ranges (gscale 0.5, gmul 0.25, wd 1e-5) and pcms_fill_ranges over ``rng``."""
    state = ranges_state(n, seed)
    dev = [t.to(DEV) for t in state]
    rt = torch.tensor(rng, dtype=torch.int64, device=DEV)
    mx = max(e - b for b, e in rng)
    inside = torch.zeros(n, dtype=torch.bool)
    for b, e in rng:
        inside[b:e] = True
    coef = adam_coef(2, 1e-5)
    L.call("pcms_adam_ranges", *dev, rt, len(rng), mx, *coef, 0.5, torch.tensor([0.25], device=DEV))
    torch.cuda.synchronize()
    after = [t.cpu() for t in dev]
    for a, b in zip(after, state):
        assert torch.equal(a[~inside].view(torch.int32), b[~inside].view(torch.int32)), "wrote outside the ranges"
    r = adam_check(test, state, after, adam_ref(*state, coef, 0.125), sel=inside)
    fill = state[0].clone().to(DEV)
    L.call("pcms_fill_ranges", fill, rt, len(rng), mx, 0.02)
    torch.cuda.synchronize()
    exp = torch.where(inside, torch.tensor(0.02), state[0])
    assert torch.equal(fill.cpu().view(torch.int32), exp.view(torch.int32))
    return r, mx


@pytest.mark.parametrize("cap", CAPS)
def test_adam_ranges_and_fill_capped(cap):
    # five ranges of very different length, an empty one, unaligned begins
    rng = [(3, 5003), (5010, 5010), (5011, 5012), (5101, 5878), (6001, 6130)]
    with grid_cap(cap) as L:
        _, mx = run_adam_ranges(L, f"adam_ranges_cap{cap}", 6200, rng)
        assert mx > cap * TPB


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("apply", [0, 1])
@pytest.mark.parametrize("max_norm", [0.0, 1e-3, 1e6])
@pytest.mark.parametrize("n", [3, 4, 4098, 10007])
def test_grad_clip_capped(n, max_norm, apply, cap):
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(n))
    gscale = 0.5
    norm = float(g0.double().norm()) * gscale
    mul_ref = gscale * (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)
    with grid_cap(cap) as L:
        if n >= 4098:
            assert n // 4 > cap * TPB  # (rows = min(1024, the switch): several 16-byte trips per thread)
        gd = g0.to(DEV)
        ws = torch.full((L.query("pcms_grad_clip_ws_doubles"),), float("nan"), dtype=torch.float64, device=DEV)
        mul = torch.full((1,), float("nan"), device=DEV)
        L.call("pcms_grad_clip", gd, n, gscale, max_norm, apply, ws, None, mul)
        torch.cuda.synchronize()
    assert abs(mul.item() - mul_ref) <= 1e-6 * mul_ref, (mul.item(), mul_ref)
    if max_norm == 0.0 or max_norm == 1e6:
        assert mul.item() == gscale  # no clipping: the coefficient is exactly 1
    if apply:
        torch.testing.assert_close(gd.cpu(), (g0.double() * mul_ref).float(), rtol=2e-6, atol=1e-12)
        assert torch.equal(gd.cpu(), g0 * mul.cpu())  # one fp32 product per element
    else:
        assert torch.equal(gd.cpu().view(torch.int32), g0.view(torch.int32))


def test_grad_clip_misaligned_gradient():
    L = _lib()
    buf = torch.zeros(64, device=DEV)
    ws = torch.zeros(L.query("pcms_grad_clip_ws_doubles"), dtype=torch.float64, device=DEV)
    mul = torch.zeros(1, device=DEV)
    rc = L.load().pcms_grad_clip(buf.data_ptr() + 4, 16, 1.0, 1.0, 1, ws.data_ptr(), None, mul.data_ptr(), L.stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert buf.abs().max().item() == 0.0 and mul.item() == 0.0


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dt,code", [(torch.float32, 0), (torch.bfloat16, 1)])
def test_pack_unpack_add_capped(dt, code, cap):
    N = 3
    with grid_cap(cap) as L:
        for S in [(11, 12, 13), (11, 13, 9)]:  # V % 4 == 0: 4 voxels per thread; odd V: the scalar route
            V = S[0] * S[1] * S[2]
            assert (N * V // 4 if V % 4 == 0 else N * V) > cap * TPB
            x = torch.rand(N, 5, V, generator=torch.Generator().manual_seed(V))
            out = torch.full((N, V, 8), float("nan"), dtype=dt, device=DEV)
            L.call("pcms_pack_input", code, x.to(DEV), out, N, 5, V, 8)
            torch.cuda.synchronize()
            exp = torch.zeros(N, V, 8)
            exp[..., :5] = x.transpose(1, 2)
            assert torch.equal(out.cpu(), exp.to(dt)), f"pack input V={V}"
            # NDHWC (8 stored channels) -> NCDHW fp32, the first 3
            back = torch.full((N, 3, V), float("nan"), device=DEV)
            L.call("pcms_unpack_output", code, out, back, N, 3, 8, V)
            torch.cuda.synchronize()
            assert torch.equal(back.cpu(), exp.to(dt).float()[..., :3].transpose(1, 2)), f"unpack output V={V}"
        n = 8 * 1237
        assert n // (8 if code else 4) > cap * TPB
        g = torch.Generator().manual_seed(3)
        a, b = torch.randn(n, generator=g).to(dt), torch.randn(n, generator=g).to(dt)
        dst = a.to(DEV)
        L.call("pcms_add", code, dst, b.to(DEV), n)
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), (a.float() + b.float()).to(dt)), "add"


# ---------------------------------------------------------------------------------------------
# C. the product's own caps, reached by shape (no switch)
# ---------------------------------------------------------------------------------------------
def no_switch(L):
    assert L.query("pcms_stream_grid_cap", -1) >= 2 ** 30


def test_loss_at_its_row_cap():
    L = _lib()
    no_switch(L)
    M = 2 * 1024 * 2048 + 3 * 2048 + 5
    x, t = loss_inputs(M, 12)
    rows, sums, loss, dx = run_loss(L, x, t, 0.5, 0.5, 0.7)
    assert rows == 1024 and cdiv(M, 8 * TPB) > rows, "rows not capped"
    trips = cdiv(M, rows * TPB)
    assert trips > 16  # two 8-way trips and a tail
    rs, ra, rl, rdx = loss_ref(x, t, 1.0, 0.5, 0.5, f32(0.7))
    sum_bound("loss_sums_M4200453", sums, rs, ra, trips)
    assert abs(loss - rl) < 1e-6, (loss, rl)
    close(dx, rdx, 1e-5, "loss grad")


def test_adam_at_its_grid_cap():
    L = _lib()
    no_switch(L)
    n = 2 * 16384 * 256 + 1234
    assert cdiv(n, TPB) > 2 * 16384  # (pcms_adam's grid is capped at 16384 blocks: three trips)
    run_adam(L, f"adam_n{n}", n, 0.5, 0.25, 1e-5)


def test_adam_ranges_at_its_grid_cap():
    L = _lib()
    no_switch(L)
    rng = [(1, 18), (18, 18), (21, 600022), (600023, 600024), (600101, 601000)]
    _, mx = run_adam_ranges(L, "adam_ranges_600001", 601003, rng)
    assert mx == 600001 and cdiv(mx, TPB) > 2048  # (grid.x capped at 2048 blocks)


def test_grad_clip_at_its_row_cap():
    L = _lib()
    no_switch(L)
    n = 2 * 1024 * 256 * 4 + 3
    rows = L.query("pcms_grad_clip_ws_doubles")
    assert cdiv(n // 4 + 1, TPB) > rows, "rows not capped"
    trips = cdiv(n // 4, rows * TPB)
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    gd = g0.to(DEV)
    ws = torch.empty(rows, dtype=torch.float64, device=DEV)
    norm, mul = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
    L.call("pcms_grad_clip", gd, n, 1.0, 1.0, 1, ws, norm, mul)
    torch.cuda.synchronize()
    ref = float(g0.double().norm())
    # the bound on the sum of squares, through the square root (half the relative error)
    sum_bound("grad_clip_norm_n2097155", norm, torch.tensor([ref]), torch.tensor([ref / 2]), trips)
    coef = 1.0 / (ref + 1e-6)
    assert abs(mul.item() - coef) <= 1e-6 * coef
    torch.testing.assert_close(gd.cpu(), (g0.double() * coef).float(), rtol=2e-6, atol=1e-12)


@pytest.mark.parametrize("ncls", [1, 2])
def test_head_bwd_at_its_row_cap(ncls):
    L = _lib()
    no_switch(L)
    dt, code, tol = DTS[1]
    N, S = 2, (40, 50, 50)
    V = S[0] * S[1] * S[2]
    rows = L.query("pcms_head_bn_bwd_rows", V, N)
    U = 4 if ncls == 1 else 2
    assert rows == 2048 and cdiv(N * V * 8, TPB) > rows, "rows not capped"
    assert N * V > (U - 1) * rows * TPB // 8, "the unrolled loop does not run"
    trips = cdiv(N * V, rows * TPB // 8)
    g = torch.Generator().manual_seed(9)
    a = torch.relu(torch.randn(N, V, 64, generator=g)).to(dt)
    w = torch.randn(ncls, 64, generator=g) * 0.1
    dl = torch.randn(N, ncls, V, generator=g)
    ad, dld, wd_ = a.to(DEV), dl.to(DEV), w.to(DEV)
    da = torch.full_like(ad, float("nan"))
    dw, db = torch.zeros(ncls, 64, device=DEV), torch.zeros(ncls, device=DEV)
    ws = torch.empty(L.query("pcms_head_bwd_ws_floats", V, N, ncls), device=DEV)
    L.call("pcms_head_bwd", code, ad, dld, wd_, da, dw, db, ws, V, N, ncls)
    torch.cuda.synchronize()
    a64, dl64 = a.double(), dl.double()
    close(da, torch.einsum("nkv,kc->nvc", dl64, w.double()), tol, "head dgrad")
    sum_bound(f"head_bwd_dw_ncls{ncls}", dw, torch.einsum("nkv,nvc->kc", dl64, a64),
              torch.einsum("nkv,nvc->kc", dl64.abs(), a64), trips)
    sum_bound(f"head_bwd_db_ncls{ncls}", db, dl64.sum((0, 2)), dl64.abs().sum((0, 2)), trips)


@pytest.mark.parametrize("dt,code,tol,S", [DTS[1] + ((16, 24, 24),), DTS[0] + ((16, 16, 17),)])
def test_bn_relu_bwd_at_its_row_cap(dt, code, tol, S):
    L = _lib()
    no_switch(L)
    C, N = 1024, 2
    nvox = N * S[0] * S[1] * S[2]
    vec, VL = vec_lanes(code, C)
    rows = L.query("pcms_bn_bwd_rows", code, C, nvox)
    assert cdiv(nvox, VL * 4) > SMALL_ROWS, "not the VL * 16 regime"
    assert rows == L.query("pcms_bn_bwd_rows_cap", -1) == 512 and cdiv(nvox, VL * 16) > rows, "rows not capped"
    trips = cdiv(nvox, rows * VL)
    assert trips > 16
    g = torch.Generator().manual_seed(13)
    y = (torch.randn(nvox, C, generator=g) * 3 + 1).to(dt)
    da = torch.randn(nvox, C, generator=g).to(dt)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1
    beta = torch.randn(C, generator=g)
    sc, sh, mean, invstd = bn_coeffs(y.double(), gamma, beta)
    co = [t.to(DEV) for t in (sc, sh, mean, invstd)]
    yd, dad = y.to(DEV), da.to(DEV)
    part = torch.empty(rows * C * 2, device=DEV)
    coef = torch.empty(3 * C, device=DEV)
    dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dy = torch.full_like(yd, float("nan"))
    ws = torch.empty(L.query("pcms_bn_ws_doubles", C), dtype=torch.float64, device=DEV)
    L.call("pcms_bn_relu_bwd", code, dad, yd, *co, gamma.to(DEV), part, coef, dgam, dbet, dy, C, nvox, ws)
    torch.cuda.synchronize()
    ref = bn_bwd_ref(y.double(), da.double(), sc, sh, mean, invstd, gamma)
    name = f"bn_relu_bwd_C1024_{'bf16' if code else 'fp32'}"
    sum_bound(name + "_dgamma", dgam, ref["s2"], ref["abs2"], trips)
    sum_bound(name + "_dbeta", dbet, ref["s1"], ref["abs1"], trips)
    close(dy, ref["dy"], 5 * tol, "bn+relu bwd")


def test_maxpool_bwd_bn_at_its_row_cap():
    L = _lib()
    no_switch(L)
    dt, code, tol = DTS[1]
    C, N, S = 64, 2, (42, 40, 40)
    o = pool_chain(L, dt, code, C, N, S)
    vec, _ = vec_lanes(code, C)
    cells = N * cdiv(S[0], 2) * cdiv(S[1], 2) * cdiv(S[2], 2)
    rows = o["rows_pool"]
    assert rows == L.query("pcms_bn_bwd_rows_cap", -1) == 512 and cells * (C // vec) > rows * TPB, "rows not capped"
    trips = 8 * cdiv(cells * (C // vec), rows * TPB)  # a thread adds the 8 children of each of its cells
    ref = o["ref"]
    assert torch.equal(o["p"].cpu().double(), o["p_ref"])
    close(o["da"], o["da_ref"], tol, "da = skip + dp at the argmax")
    sum_bound("maxpool_bwd_bn_dgamma", o["dg"], ref["s2"], ref["abs2"], trips)
    sum_bound("maxpool_bwd_bn_dbeta", o["db"], ref["s1"], ref["abs1"], trips)
    close(o["dy"], ref["dy"], 1e-2, "dy vs fp64")


# ---------------------------------------------------------------------------------------------
# D. the whole step under the switch: the engine sizes every workspace from the queries, and
# every streaming kernel runs its multi-trip form inside the real sequence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd_bcedice", "c16_ncls2_dice"])
def test_fp32_parity_full_step_capped(name):
    with grid_cap(3) as L:
        assert 3 in L.switches()
        parity.fp32_parity_full_step(name, False)


def test_bf16_parity_step_capped():
    with grid_cap(3) as L:
        assert 3 in L.switches()
        parity.bf16_parity_step("odd_bcedice", False)
