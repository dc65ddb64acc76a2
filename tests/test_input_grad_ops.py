"""Kernel-level numerics of the input-gradient entry points: pcms_stem_dgrad (the stem conv's
input gradient), pcms_bn_relu_bwd_eval and pcms_head_bn_bwd_eval (the eval-mode BatchNorm +
ReLU backward and its fusion with the head), each against fp64 PyTorch on the CPU with the
same, already-rounded inputs (the conventions of tests/test_gpu_ops.py)."""
import functools

import pytest
import torch

from tests.test_gpu_ops import DEV, DTS, _lib, close, ncdhw, ndhwc, q

pytestmark = pytest.mark.gpu

# (N, (D, H, W)): one voxel; odd sizes, partial boxes; a W tail; batch seams (no gradient may
# cross samples); the hot stem shape; many boxes per workgroup of the persistent grid
STEM_SHAPES = [(1, (1, 1, 1)), (1, (9, 10, 11)), (1, (6, 20, 33)), (3, (4, 4, 16)), (2, (16, 16, 16)),
               (2, (32, 64, 64))]
# bf16: bf16-exact products, fp32 sums, fp32 result (the stem weight-gradient test's bar for the
# same arithmetic); fp32: DTS
STEM_TOL = {1: 1e-4, 0: 2e-5}
GUARD = 4096


@functools.lru_cache(maxsize=None)
def _stem_case(N, S, dt):
    """(dy device NDHWC, w fp32 [64][5][27] rounded to dt, expected dx fp64 (N, 5, D, H, W)) --
    one fp64 reference per shape and type; the cin_w = 3 case is its first three channels with
    the weight's first three input channels (dx[ci] reads W[:, ci] only)."""
    g = torch.Generator().manual_seed(1000 + 7 * N + S[0] * 31 + S[1] * 5 + S[2])
    dy = torch.randn(N, 64, *S, generator=g)
    w = torch.randn(64, 5, 3, 3, 3, generator=g)  # asymmetric: a mirrored or transposed tap layout cannot pass
    dy64, dyd = q(dy, dt)
    w64 = w.to(dt).double()
    exp = torch.nn.grad.conv3d_input((N, 5, *S), w64, dy64, padding=1)
    return ndhwc(dyd), w.to(dt).float(), exp


@pytest.mark.parametrize("N,S", STEM_SHAPES)
@pytest.mark.parametrize("dt,code,_tol", DTS)
@pytest.mark.parametrize("cin_w", [5, 3])
def test_stem_dgrad(cin_w, dt, code, _tol, N, S):
    L = _lib()
    dyd, w, exp = _stem_case(N, S, dt)
    exp = exp[:, :cin_w]
    wd = w[:, :cin_w].contiguous().to(DEV)
    pack = torch.empty(L.query("pcms_stem_dgrad_pack_elems", code), dtype=dt, device=DEV)
    L.call("pcms_stem_dgrad_pack", code, wd, pack, cin_w)
    n = exp.numel()
    runs = []
    for _ in range(2):
        buf = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV)
        buf[:GUARD] = 12345.678
        buf[GUARD + n:] = -8765.4321
        guard = torch.cat([buf[:GUARD], buf[GUARD + n:]]).clone().view(torch.int32)
        dx = buf[GUARD:GUARD + n]
        L.call("pcms_stem_dgrad", code, dyd, pack, dx, N, *S, cin_w)
        torch.cuda.synchronize()
        assert not torch.isnan(dx).any(), "an element of dx was not written"
        assert torch.equal(torch.cat([buf[:GUARD], buf[GUARD + n:]]).view(torch.int32), guard), "guard overwritten"
        runs.append(dx.clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
    close(runs[0].view(N, cin_w, *S), exp, STEM_TOL[code], f"stem dgrad {N}x{S} cin_w={cin_w}")


def test_stem_dgrad_bad_arguments():
    L = _lib()
    lib = L.load()
    one = torch.zeros(64, device=DEV)
    for args in [(1, one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 1, 1, 1, 9),   # cin_w > 8
                 (1, one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 0, 1, 1, 5),   # empty volume
                 (1, None, one.data_ptr(), one.data_ptr(), 1, 1, 1, 1, 5),            # NULL dy
                 (3, one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 1, 1, 1, 5),   # no such dtype
                 (1, one.data_ptr(), one.data_ptr(), one.data_ptr(), 2, 256, 256, 128, 5)]:  # dy of 2 GiB
        assert lib.pcms_stem_dgrad(*args, L.stream()) < 0, args


def _bn_case(dt, C, N, S, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(N, C, *S, generator=g) * 3 + 1).to(dt)
    sc = torch.rand(C, generator=g) + 0.5
    sc[::3] *= -1  # negative gamma: the mask is on the product, not on y
    sh = torch.randn(C, generator=g)
    return y, sc, sh, g


def _mask_and_check(L, code, y, yd, sc, sh, C, nvox):
    """The ReLU mask of pcms_bn_relu's own output (NCDHW bool, so no element is excluded) and the
    fp64 mask of the same expression: they may differ only where y sc + sh rounds across zero."""
    a = torch.empty_like(yd)
    L.call("pcms_bn_relu", code, yd, a, sc.to(DEV), sh.to(DEV), C, nvox)
    mask = ncdhw(a.cpu()) > 0
    m64 = (y.double() * sc.double().view(1, C, 1, 1, 1) + sh.double().view(1, C, 1, 1, 1)) > 0
    assert (mask != m64).float().mean().item() < 1e-3
    return mask, m64


@pytest.mark.parametrize("dt,code,tol", DTS)
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("N,S", [(2, (3, 5, 7)), (1, (16, 16, 16))])
def test_bn_relu_bwd_eval(dt, code, tol, C, N, S):
    L = _lib()
    nvox = N * S[0] * S[1] * S[2]
    y, sc, sh, g = _bn_case(dt, C, N, S, 21)
    da = torch.randn(N, C, *S, generator=g).to(dt)
    yd = ndhwc(y).to(DEV)
    mask, m64 = _mask_and_check(L, code, y, yd, sc, sh, C, nvox)
    # fp64 autograd of relu(y sc + sh), its mask replaced by the kernel forward's own
    yr = y.double().requires_grad_(True)
    torch.relu(yr * sc.double().view(1, C, 1, 1, 1) + sh.double().view(1, C, 1, 1, 1)).backward(da.double())
    exp = torch.where(mask, da.double() * sc.double().view(1, C, 1, 1, 1), torch.zeros((), dtype=torch.float64))
    agree = mask == m64
    assert torch.equal(exp[agree], yr.grad[agree])
    dy = torch.full_like(yd, float("nan"))
    L.call("pcms_bn_relu_bwd_eval", code, ndhwc(da).to(DEV), yd, sc.to(DEV), sh.to(DEV), dy, C, nvox)
    torch.cuda.synchronize()
    assert not torch.isnan(dy.float()).any()
    close(ncdhw(dy.cpu()), exp, tol, "eval bn+relu bwd")


@pytest.mark.parametrize("dt,code,tol", DTS)
@pytest.mark.parametrize("ncls", [1, 3])
@pytest.mark.parametrize("N,S", [(2, (3, 5, 7)), (1, (16, 16, 16))])
def test_head_bn_bwd_eval(dt, code, tol, ncls, N, S):
    L = _lib()
    C = 64
    V = S[0] * S[1] * S[2]
    y, sc, sh, g = _bn_case(dt, C, N, S, 22)
    w = torch.randn(ncls, C, generator=g)
    dl = torch.randn(N, ncls, *S, generator=g)
    yd = ndhwc(y).to(DEV)
    mask, m64 = _mask_and_check(L, code, y, yd, sc, sh, C, N * V)
    # fp64 autograd of conv1x1(relu(y sc + sh)), the mask replaced as above
    da = torch.einsum("nkdhw,kc->ncdhw", dl.double(), w.double())
    exp = torch.where(mask, da * sc.double().view(1, C, 1, 1, 1), torch.zeros((), dtype=torch.float64))
    yr = y.double().requires_grad_(True)
    a = torch.relu(yr * sc.double().view(1, C, 1, 1, 1) + sh.double().view(1, C, 1, 1, 1))
    torch.nn.functional.conv3d(a, w.double().view(ncls, C, 1, 1, 1)).backward(dl.double())
    agree = mask == m64
    torch.testing.assert_close(exp[agree], yr.grad[agree], rtol=1e-12, atol=1e-12)
    dy = torch.full_like(yd, float("nan"))
    L.call("pcms_head_bn_bwd_eval", code, yd, sc.to(DEV), sh.to(DEV), dl.to(DEV), w.to(DEV), dy, V, N, ncls)
    torch.cuda.synchronize()
    assert not torch.isnan(dy.float()).any()
    close(ncdhw(dy.cpu()), exp, tol, "eval head + bn bwd")
