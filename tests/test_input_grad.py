"""The gradient of the network input through ``UNet3D`` (training and eval mode), end to end
against the CPU oracle (oracle/unet3d_cpu.py, a differentiable function of ``x``).

Setup: ``UNet3D(5, 1)`` from seed 0 (eval cases: running statistics perturbed as
tests/test_gpu_blocks._net does), ``x = rand(2, 5, *S)`` a leaf that requires grad.  Training
target: BCEDice on a ``rand < 0.4`` label; eval target: ``sigmoid(logits).sum()`` (saliency).

Bars
* fp32 build: relative L2 of ``x.grad`` to the oracle's fp64 ``x.grad`` <= max(10 x rl_ref,
  5e-2), rl_ref the oracle's own fp32-vs-fp64 distance (computed here) and 5e-2 the project's
  floor for small shapes (GRAD_RL2 of tests/test_gpu_parity.py: one ReLU or arg-max flip
  reroutes a gradient element).
* bf16 build: relative L2 to the fp32 oracle <= 2 x the oracle's own bf16-autocast distance.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import unet3d_cpu as ref
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

S_HOT, S_ODD = (32, 32, 16), (20, 18, 24)  # S_ODD: no hot stem shape, pads asymmetrically
FLOOR = 5e-2


def _model(precision="fp32", ckpt=False, eval_stats=False):
    from pcms_amd.models.unet3d import UNet3D
    torch.manual_seed(0)
    m = UNet3D(n_modalities=5, n_classes=1, precision=precision, checkpoint_decoder=ckpt)
    if eval_stats:
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm3d):
                    mod.running_mean.uniform_(-0.05, 0.05)
                    mod.running_var.uniform_(0.5, 1.5)
    return m


def _data(S, n=2):
    g = torch.Generator().manual_seed(77)
    x = torch.rand(n, 5, *S, generator=g)
    label = (torch.rand(n, 1, *S, generator=g) < 0.4).float()
    return x, label


def _rl2(a, b):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-30)


@functools.lru_cache(maxsize=None)
def _oracle(S, training, n=2, autocast=False):
    """The oracle's x.grad in fp64 and fp32 (and under bf16 autocast), computed once per case
    and shared: {"g64", "g32", "rl_ref", ["gauto", "rl_auto"]}."""
    sd0 = {k: v.detach().clone() for k, v in _model(eval_stats=not training).state_dict().items()}
    x, label = _data(S, n)

    def run(dtype, auto=False):
        sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        xr = x.clone().to(dtype).requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=auto):
            out = ref.forward(sd, xr, training=training)
        out = out.to(dtype)
        loss = ref.bce_dice_loss(out, label.to(dtype)) if training else torch.sigmoid(out).sum()
        loss.backward()
        return xr.grad.detach().clone()

    r = {"g64": run(torch.float64), "g32": run(torch.float32)}
    r["rl_ref"] = _rl2(r["g32"], r["g64"])
    if autocast:
        r["gauto"] = run(torch.float32, auto=True)
        r["rl_auto"] = _rl2(r["gauto"], r["g32"])
    return r


def _gpu(m, S, training, requires_grad=True, n=2):
    """One forward + backward on the GPU model: (x.grad or None, logits, loss)."""
    from pcms_amd.utils.losses import BCEDiceLoss
    x, label = _data(S, n)
    xg = x.cuda().requires_grad_(requires_grad)
    m.train(training)
    m.zero_grad(set_to_none=True)
    logits = m(xg)
    loss = BCEDiceLoss()(logits, label.cuda()) if training else torch.sigmoid(logits).sum()
    loss.backward()
    torch.cuda.synchronize()
    return xg.grad, logits.detach(), loss.detach()


# ---- 1. fp32 build vs the fp64 oracle
@pytest.mark.parametrize("S", [S_HOT, S_ODD])
@pytest.mark.parametrize("training", [True, False])
def test_fp32_input_grad_matches_oracle(training, S):
    o = _oracle(S, training)
    m = _model("fp32", eval_stats=not training).cuda()
    g, logits, _ = _gpu(m, S, training)
    assert g is not None and torch.isfinite(g).all()
    rl = _rl2(g.cpu(), o["g64"])
    bar = max(10 * o["rl_ref"], FLOOR)
    print(f"\n[input grad fp32 {'train' if training else 'eval'} {S}] rl {rl:.3e} rl_ref {o['rl_ref']:.3e} bar {bar:.3e}")
    gu.record_margin(f"input_grad_fp32_{'train' if training else 'eval'}_{'x'.join(map(str, S))}", rl=rl,
                     rl_ref=o["rl_ref"], bar=bar, rl_over_bar=rl / bar)
    if not training:
        # the logits the graph hangs on are the unfolded eval logits of a no_grad call, bit for bit
        eng = m.engine()
        fold = eng.fold_bn_eval
        eng.fold_bn_eval = False
        with torch.no_grad():
            plain = m(_data(S)[0].cuda())
        eng.fold_bn_eval = fold
        assert torch.equal(logits, plain)
    assert rl <= bar, (rl, o["rl_ref"])


# ---- 2. bf16 build vs the fp32 oracle, bar from the oracle's own bf16-autocast run
# (32x32x16 only: at 16^3 BatchNorm runs over two values per channel at the bottleneck and
# autocast alone is 0.94 off)
@pytest.mark.parametrize("training", [True, False])
def test_bf16_input_grad_within_autocast(training):
    o = _oracle(S_HOT, training, autocast=True)
    m = _model("bf16", eval_stats=not training).cuda()
    g, _, _ = _gpu(m, S_HOT, training)
    assert g is not None and torch.isfinite(g).all()
    rl = _rl2(g.cpu(), o["g32"])
    print(f"\n[input grad bf16 {'train' if training else 'eval'}] rl {rl:.3e} autocast {o['rl_auto']:.3e}")
    gu.record_margin(f"input_grad_bf16_{'train' if training else 'eval'}", rl=rl, rl_auto=o["rl_auto"],
                     rl_over_bar=rl / (2 * o["rl_auto"]))
    assert rl <= 2 * o["rl_auto"], (rl, o["rl_auto"])


# ---- 3. asking for the input gradient moves nothing else
@pytest.mark.parametrize("S", [S_HOT, S_ODD])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_training_step_unchanged_by_input_grad(precision, S):
    res = []
    for want in (True, False):
        m = _model(precision).cuda()
        g, logits, loss = _gpu(m, S, True, requires_grad=want)
        assert (g is not None) == want
        res.append((loss, logits, {k: p.grad.clone() for k, p in m.named_parameters()},
                    {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}))
    (l0, lg0, g0, b0), (l1, lg1, g1, b1) = res
    assert torch.equal(l0, l1) and torch.equal(lg0, lg1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


# ---- 4. determinism and decoder checkpointing
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False])
def test_input_grad_deterministic_and_checkpoint_invariant(training, precision):
    m = _model(precision, eval_stats=not training).cuda()
    g0, _, _ = _gpu(m, S_HOT, training)
    m2 = _model(precision, eval_stats=not training).cuda()
    g1, _, _ = _gpu(m2, S_HOT, training)
    assert torch.equal(g0, g1), "two runs differ"
    mc = _model(precision, ckpt=True, eval_stats=not training).cuda()
    gc, _, _ = _gpu(mc, S_HOT, training)
    assert torch.equal(g0, gc), "checkpoint_decoder changes x.grad"


# ---- 5. surface
@pytest.mark.parametrize("training", [True, False])
def test_input_grad_surface(training):
    S = (16, 16, 16)
    m = _model("fp32", eval_stats=not training).cuda()
    x = _data(S)[0].cuda().requires_grad_(True)
    m.train(training)
    fold = m.engine().fold_bn_eval  # (a new engine attaches zeroed gradient views: before zero_grad)
    m.zero_grad(set_to_none=True)
    logits = m(x)
    assert logits.requires_grad
    torch.sigmoid(logits).sum().backward()
    assert x.grad.shape == x.shape and x.grad.device == x.device and x.grad.dtype == torch.float32
    if training:
        assert all(p.grad is not None for p in m.parameters())
        return
    assert all(p.grad is None for p in m.parameters()), "eval mode produces no parameter gradient"
    assert m.engine().fold_bn_eval == fold
    # a second forward before backward(): the saved state is gone
    stale = m(x)
    m(x)
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    with torch.no_grad():  # and a no_grad forward invalidates it too
        kept = m(x.detach().clone().requires_grad_(True))
    assert not kept.requires_grad


def test_predictor_saliency(tmp_path):
    from pcms_amd.predict import ModelPredictor
    S = (16, 16, 16)
    m = _model(eval_stats=True)
    path = str(tmp_path / "model.pth")
    torch.save(m.state_dict(), path)
    pred = ModelPredictor(path, device="cuda", precision="fp32")
    x = _data(S, n=1)[0]
    sal = pred.saliency(x)
    assert isinstance(sal, np.ndarray) and sal.shape == (5,) + S and sal.dtype == np.float32
    # no parameter gradient is written (a new engine's gradient views are zero-filled)
    assert all(p.grad is None or not bool(p.grad.any()) for p in pred.model.parameters())
    o = _oracle(S, False, n=1)
    rl = _rl2(torch.from_numpy(sal), o["g64"][0])
    assert rl <= max(10 * o["rl_ref"], FLOOR), (rl, o["rl_ref"])
