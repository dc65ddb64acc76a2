"""An engine with a history equals a fresh engine with the same weights.

Every kernel weight pack (the general conv pairs, the pack16 forms, the stem's forward and
dgrad packs, the ConvTranspose pairs, the folded eval set) is derived from the fp32 master; a
pack left over from older weights is a silent wrong result.  This test knows nothing of how
the engine keeps them current: it walks one model through every kind of event that changes the
master or moves the packs' buffers, and after each event compares it, bit for bit (the
library's reductions are order-fixed), with a model built new from its ``state_dict()``.
"""
import pytest
import torch

SHAPES = {"16": (2, (16, 16, 16)), "32x64x64": (1, (32, 64, 64))}


def _data(key, seed):
    N, S = SHAPES[key]
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 5, *S, generator=gen).cuda()
    y = (torch.rand(N, 1, *S, generator=gen) < 0.4).float().cuda()
    dl = (torch.rand(N, 1, *S, generator=gen) - 0.5).cuda()
    return x, y, dl


def _observe(m, x, dl):
    """Training logits, the flat gradient of a backward from ``dl``, folded-eval logits and the
    eval input gradient of ``dl`` (the stem dgrad pack) of ``m`` at ``x``."""
    m.train()
    for p in m.parameters():
        p.grad = None
    lg = m(x)
    lg.backward(dl)
    out = [lg.detach().clone(), m.engine().flat_g.clone()]
    m.eval()
    with torch.no_grad():
        out.append(m(x).clone())
    xg = x.clone().requires_grad_(True)
    m(xg).backward(dl)
    out.append(xg.grad.clone())
    m.train()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("precision,shape", [("bf16", "16"), ("fp32", "16"), ("bf16", "32x64x64")])
def test_engine_with_history_equals_fresh_engine(precision, shape, tmp_path):
    """Events: two fused FlatAdam steps; a step with ``fused_packs=False``; an in-place torch
    write to ``flat_p`` (no ``mark_dirty``); a C-ABI write + ``mark_dirty()``; a forward at the
    other shape (re-layout) and back; ``use_b16`` off (the general kernel reads packs the fused
    Adam had skipped) and on again; ``load_checkpoint``; an eval forward that keeps the input
    gradient + its backward around a step (the stem dgrad pack); fp32 only: bf16x3 conv
    arithmetic for a step and back.  After each: training logits, flat gradient, folded-eval
    logits and input gradient equal those of a fresh model loaded from the walked model's
    ``state_dict()``, bit for bit -- first at the other shape, then at the test's own, so each
    check re-lays the walked engine out twice in whatever state the event left it (after a
    fused step the other shape's routes read general packs that step did not write).  The
    shapes: 2x5x16^3, where level 0 runs the split 16x16x32 form (bf16), and 1x5x32x64x64, the
    smallest where its unsplit form takes level 0 in both directions, so the fused Adam leaves
    those convs' general packs unwritten (both asserted on the layout)."""
    from pcms_amd._lib import call
    from pcms_amd.models.unet3d import UNet3D, load_weights
    from pcms_amd.utils.trainer import Trainer
    x, y, dl = _data(shape, 21)
    x_other, _, dl_other = _data(next(k for k in SHAPES if k != shape), 22)
    torch.manual_seed(0)
    m = UNet3D(n_modalities=5, n_classes=1, precision=precision).cuda()
    tr = Trainer({"device": "cuda", "learning_rate": 1e-3, "batch_size": x.shape[0], "num_epochs": 1,
                  "loss": "bce_dice", "precision": precision, "save_dir": str(tmp_path)}, model=m)
    opt, crit = tr.optimizer, tr.criterion
    eng = m.engine()

    def step():
        m.train()
        opt.zero_grad()
        crit(m(x), y).backward()
        opt.step()

    def check(event):
        with torch.device("cuda"):
            fresh = UNet3D(n_modalities=5, n_classes=1, precision=precision)
        load_weights(fresh, m.state_dict())
        fresh.engine().use_b16 = eng.use_b16
        names = ("training logits", "flat gradient", "folded-eval logits", "input gradient")
        for where, xs, dls in (("other", x_other, dl_other), ("own", x, dl)):
            for name, a, b in zip(names, _observe(m, xs, dls), _observe(fresh, xs, dls)):
                assert torch.equal(a, b), f"after {event}, {where} shape: {name} differ from a fresh engine's"

    def fused_steps():
        step()
        step()
        tr.save_checkpoint(0, 0.0)

    def unfused_step():
        opt.fused_packs = False
        step()
        opt.fused_packs = True

    def torch_write():
        step()
        with torch.no_grad():
            eng.flat_p.mul_(1.01)

    def c_abi_write():
        step()
        base = eng.flat_p.data_ptr()
        ws = (eng.convs[0].mod.weight, eng.convs[1].mod.weight, eng.convs[4].mod.weight, eng.ups[3].weight)
        rng = sorted([(w.data_ptr() - base) // 4, (w.data_ptr() - base) // 4 + 96] for w in ws)
        call("pcms_fill_ranges", eng.flat_p, torch.tensor(rng, dtype=torch.int64, device="cuda"), len(rng), 96, 0.02)
        eng.mark_dirty()

    def relayout():
        step()
        with torch.no_grad():
            m(x_other)

    def b16_off():
        step()
        eng.use_b16 = False

    def b16_on_again():
        step()
        eng.use_b16 = True

    def load_checkpoint():
        step()
        tr.load_checkpoint(str(tmp_path / "latest_checkpoint.pth"))

    def input_gradient():
        m.eval()
        xg = x.clone().requires_grad_(True)
        m(xg).backward(dl)
        step()

    def x3_and_back():
        step()
        eng.set_fp32_conv_mode("x3")
        step()
        eng.set_fp32_conv_mode("x6")

    events = [fused_steps, unfused_step, torch_write, c_abi_write, relayout, b16_off, b16_on_again, load_checkpoint,
              input_gradient] + ([x3_and_back] if precision == "fp32" else [])
    for i, ev in enumerate(events):
        ev()
        if i == 0 and precision == "bf16":  # the routes this test relies on
            L = eng.layout
            kinds = [(f.kind, d.kind) for f, d in zip(L.fwd[1:], L.dgrad[1:])]
            want = "b16_split" if shape == "16" else "b16"
            assert L.fwd[1].kind == want and (want, want) in kinds, kinds
            assert L.fwd[1].pack16 and L.dgrad[1].pack16
        check(ev.__name__)
