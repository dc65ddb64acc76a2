"""U-Net execution engine: the forward / backward schedule of the reference model over the
HIP kernels of libpcms_hip.so.

Reference call graph reproduced (models/unet3d.py):
  inc -> down1..down4 (MaxPool3d(2) + DoubleConv) -> up1..up4 (ConvT + pad + cat[skip, up]
  + DoubleConv) -> outc                                   forward @247-296
and its autograd backward (aten convolution_backward / batch_norm_backward / ...).

Layout: activations NDHWC in ``dtype`` (bf16 default, fp32 parity build); parameters live
in ONE flat fp32 master buffer (the module's nn.Parameters are views into it, so
``state_dict()`` keys/shapes are the reference's), gradients in one flat fp32 buffer
(``param.grad`` views), BatchNorm running stats in one flat fp32 buffer.  Kernel weight
packs (bf16 / fp32, MFMA-friendly order) are rebuilt from the master when it changes: they
and the rule that keeps them current live in packs.WeightPacks (``self.packs``).

The engine keeps the activations of the LAST training forward; ``backward`` must follow
that forward (checked).  ``backward(dlogits, want_dx=True)`` also returns the gradient of the
network input (the stem's dgrad, pcms_stem_dgrad).  An eval forward with ``keep_input_grad``
keeps what ``backward_input`` needs for that gradient alone (saliency: no parameter
gradient).  Only device code runs: there is no CPU path.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import BF16, F32, F32X3, call, query
from .dp import module_grad_ranges
from .packs import BN_EPS, WeightPacks, gaps

BN_MOMENTUM = 0.1

_DT = {"bf16": (torch.bfloat16, BF16), "fp32": (torch.float32, F32)}


class Route(NamedTuple):
    """How one 3x3x3 conv launch (a forward, or a dgrad = the forward of the mirrored weights)
    runs at the laid-out shape; decided once by UNetEngine._route."""
    kind: str     # "stem" | "b16" (16x16x32 kernel) | "b16_split" | "gen" (general kernel) | "gen_split"
    splits: int   # split-K request of UNetEngine._splits (the general kernel's argument)
    slabs: int    # slabs the general kernel resolves it to (pcms_conv3_splits; 1: unsplit)
    slabs16: int  # slabs of the 16x16x32 split form (pcms_conv3_fwd16_split_ok; 0: it does not run)
    rows: int     # BatchNorm partial rows the launch writes
    pack16: bool  # a 16x16x32 form runs the layer: its pack16 weights are kept ("b16*" read them,
    #               "gen*" the general kernel's pack)


class Layout(NamedTuple):
    """Everything that shapes one training step, fixed when UNetEngine._alloc lays out the
    buffers for a forward: the backward, the checkpointed recompute and every launch read it,
    never the engine's live attributes (a setting changed after a forward takes effect at the
    next one).  The fields up to ``switches`` are the allocation key (UNetEngine.buf_key)."""
    N: int
    D: int
    H: int
    W: int
    act_ckpt: bool
    side_min_level: int
    convt_wgrad_side: bool
    pool_bn_apply_fused: bool
    wgrad_target: int
    split_target: int
    fuse_bnin: bool
    use_b16: bool
    switches: Tuple[int, ...]           # _lib.switches(): the library's size / route switches
    fwd: Tuple[Route, ...] = ()         # per conv (self.convs order = UNetEngine._sites order)
    dgrad: Tuple[Optional[Route], ...] = ()  # None: the stem (its input needs no gradient)
    bnin: Tuple[bool, ...] = ()         # per block (enc + dec): BN0 + ReLU fused into the second conv
    pool_rows: Tuple[int, ...] = ()     # per level 0-3: partial rows of pcms_maxpool_bwd_bn


class ConvSpec:
    __slots__ = ("mod", "cin", "cout", "cin_store", "fwd", "dgrad", "code", "fwd16", "dgrad16", "i")

    def __init__(self, mod, cin, cout, cin_store):
        self.mod, self.cin, self.cout, self.cin_store = mod, cin, cout, cin_store
        self.i = None  # index in UNetEngine.convs (and in Layout.fwd / .dgrad)
        # the weight packs, allocated and kept current by packs.WeightPacks: the general
        # kernel's pair, and the pcms_conv3_pack16 forms for the 16x16x32 big-box kernel
        # (pcms_conv3_fwd16) where the forward / dgrad can run on it at the allocated shape
        self.fwd = None
        self.dgrad = None
        self.fwd16 = None
        self.dgrad16 = None
        # conv-kernel dtype code: BF16, or for fp32 data F32 (bf16x6 arithmetic, fp32-grade)
        # / F32X3 (bf16x3, faster, ~10x the fp32 rounding error)
        self.code = None


class BNSpec:
    __slots__ = ("mod", "c", "scale", "shift", "mean", "invstd")

    def __init__(self, mod, c):
        self.mod, self.c = mod, c
        self.scale = self.shift = self.mean = self.invstd = None


class BlockSpec:
    """DoubleConv3D: conv0 -> bn0 -> relu -> conv1 -> bn1 -> relu (models/unet3d.py:27-40)."""

    def __init__(self, dc, cin_store):
        seq = dc.conv
        self.c0 = ConvSpec(seq[0], seq[0].in_channels, seq[0].out_channels, cin_store)
        self.b0 = BNSpec(seq[1], seq[1].num_features)
        self.c1 = ConvSpec(seq[3], seq[3].in_channels, seq[3].out_channels, seq[3].in_channels)
        self.b1 = BNSpec(seq[4], seq[4].num_features)
        self.cout = self.c1.cout


def _round8(c: int) -> int:
    return (c + 7) // 8 * 8


class UNetEngine:
    def __init__(self, model, device: torch.device, precision: str = "bf16"):
        if device.type != "cuda":
            raise RuntimeError("pcms_amd runs on a ROCm device only (no CPU path); move the model to 'cuda'")
        _lib.load()
        self.model = model
        self.device = device
        self.precision = precision
        self.tdtype, self.code = _DT[precision]
        self.esize = 2 if self.code == BF16 else 4
        self.ncls = model.n_classes
        self.nmod = model.n_modalities
        self.cp = _round8(self.nmod)
        if self.ncls > 4:
            raise ValueError("the fused output head supports n_classes <= 4")
        m = model
        self.enc = [BlockSpec(m.inc, self.cp)]
        for i in range(1, 5):
            dc = getattr(m, f"down{i}").maxpool_conv[1]
            self.enc.append(BlockSpec(dc, dc.conv[0].in_channels))
        self.ups = []
        self.dec = []
        for i in range(1, 5):
            up = getattr(m, f"up{i}")
            self.ups.append(up.up)
            self.dec.append(BlockSpec(up.conv, up.conv.conv[0].in_channels))
        self.convs: List[ConvSpec] = []
        self.bns: List[BNSpec] = []
        for b in self.enc + self.dec:
            self.convs += [b.c0, b.c1]
            self.bns += [b.b0, b.b1]
        for i, cs in enumerate(self.convs):
            cs.code, cs.i = self.code, i
        # bf16 build: the stem runs on dedicated tap-packed kernels (HBM-bound)
        self.stem_fast = self.code == BF16 and self.cp == 8
        self.stem_sup = 0  # pcms_stem_supported bits for the allocated shape (set by _alloc)
        # PCMS_STEM_DENSE: the K-dense stem forward (9 tap rows of 3 kw x 5 channels) when the
        # weight has <= 5 input channels; 0 selects the 14-tap-pair kernel (A/B)
        self.stem_dense = 16 if self.nmod <= 5 else 0
        # a DoubleConv's first BatchNorm + ReLU applied inside its second conv's staging (forward:
        # pcms_conv3_fwd_bnin, weight gradient: pcms_conv3_wgrad_bnin) instead of a y1 -> a1 HBM
        # pass, on the layers both kernels run (levels 0-1, bf16); bit-identical to the unfused
        # pair (same arithmetic and rounding).  False: the a1 pass (A/B)
        self.fuse_bnin = True
        # the level-0/1 convs (forward and dgrad) on the 16x16x32 big-box kernel
        # (pcms_conv3_fwd16, pack16 weights rebuilt with the other packs); PCMS_B16=0 keeps the
        # 32x32x16 big-box kernel (A/B)
        self.use_b16 = os.environ.get("PCMS_B16", "1") != "0"
        self.packs = WeightPacks(self)
        self._flat_ptrs = None
        # the settings below (with fuse_bnin / use_b16 above) are read once per forward, into the
        # allocation key (forward()); everything after follows self.layout, the plan _alloc made
        # from them, so a change takes effect at the next forward
        self.bufs = None
        self.buf_key = None
        self.layout: Optional[Layout] = None
        self.epoch = 0
        self.saved_epoch = -1
        self.saved_eval_epoch = -1  # the eval forward backward_input may follow (keep_input_grad)
        self._folded = False        # the forward in progress runs the folded eval route
        # decoder activation checkpointing: the decoder blocks'
        # pre-BN conv outputs and first ReLU output (y1, a1, y2) are not kept per level; the
        # forward writes them into one shared level-0-sized set and the backward recomputes
        # them level by level with the forward's BatchNorm coefficients (no statistics pass,
        # running stats untouched).  Every reduction in the library sums in a fixed order (split-K
        # slabs, BN partial rows, weight-gradient partial rows), so the recomputed tensors are
        # bit-identical to the forward's and two identical steps give identical results.
        self.act_ckpt = False
        self.split_target = 512  # split-K conv launches (levels 2-4): workgroups aimed at
        self.wgrad_target = 256  # conv weight-gradient workgroups: one round of 1 WG per CU (fewer partial rows to reduce than 512)
        self.grad_ready = None   # callable(lo, hi) per finished module gradient (dp.GradSync.ready)
        self.kernel_timer = None  # dict name -> [(start, end) events] (bench.py roofline timing)
        # levels >= this run their conv weight gradients on the side stream (the deep levels'
        # small latency-bound launches beside the dgrad chain; the big levels' persistent grids
        # straggle when they share the chip).  99: never; 0: all of them (measured 119.9 vs
        # 121.6 vol/s: off)
        self.wgrad_side_min_level = 99
        # the ConvTranspose weight + bias gradient (HBM-bound: it streams the up-path gradient,
        # 268 MB at level 0) on the side stream beside the same layer's ConvT dgrad (also
        # HBM-bound, reading the same tensor); joined before the next block's backward.  Its
        # partial rows then get their own workspace (ctws_w) instead of sharing ctws.
        self.convt_wgrad_side = False
        # the encoder's MaxPool3d backward + BN-backward reduction without rewriting the block
        # output's gradient (pcms_maxpool_bwd_bn_sums), the pooled part added again in that
        # BatchNorm's apply (pcms_maxpool_bn_apply): the same dy bits, one write + read of the
        # level's tensor fewer.  Measured +0.19 % per step (the per-cell apply streams at ~5.3 TB/s
        # where the per-voxel apply it replaces runs at ~6.2; profiles/r6_pool_bn_apply_fused_ab.txt):
        # off, i.e. pcms_maxpool_bwd_bn + pcms_bn_relu_bwd_finish
        self.pool_bn_apply_fused = False
        self._side_stream = None
        self._side_used = False
        # eval mode: every BatchNorm folded into the conv before it (pcms_bn_fold) and the ReLU
        # applied in the conv epilogue (PCMS_CONV_RELU): conv -> BN -> ReLU is one pass
        # (models/unet3d.py:298-344 predict / inference).  False: the unfolded eval path.
        self.fold_bn_eval = True
        self._bn_epoch = 0     # training forwards so far (each moves the running statistics)
        self._store_ranges = None  # (stem_sup, fill plan) of _store_plan
        self._gstore = False       # this backward writes conv weight gradients (PCMS_GRAD_STORE)
        self._flatten()
        for bn in self.bns:
            c = bn.c
            bn.scale, bn.shift, bn.mean, bn.invstd = (torch.empty(c, device=device) for _ in range(4))

    def set_fp32_conv_mode(self, mode: str, convs=None):
        """fp32 build: the arithmetic of the 3x3x3 convs (all, or the indices ``convs`` of
        self.convs): "x6" (bf16x6, fp32-grade, the default) or "x3" (bf16x3)."""
        if self.code == BF16:
            raise ValueError("the bf16 build has one conv arithmetic")
        code = {"x6": F32, "x3": F32X3}[mode]
        changed = [cs for cs in self.convs if convs is None or cs.i in convs]
        for cs in changed:
            cs.code = code
        self.packs.recoded(changed)
        self.buf_key = None

    # ------------------------------------------------------------------ parameters
    def _flatten(self):
        """One flat fp32 master (params), grad and BN-buffer store; modules hold views."""
        params = list(self.model.parameters())
        total = sum(p.numel() for p in params)
        flat = torch.empty(total, dtype=torch.float32, device=self.device)
        gflat = torch.zeros(total, dtype=torch.float32, device=self.device)
        off = 0
        with torch.no_grad():
            for p in params:
                n = p.numel()
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view_as(p)
                if p.grad is not None:
                    gflat[off:off + n].copy_(p.grad.reshape(-1))
                p.grad = gflat[off:off + n].view_as(p)
                off += n
        bn_total = sum(2 * bn.c for bn in self.bns)
        bflat = torch.empty(bn_total, dtype=torch.float32, device=self.device)
        off = 0
        with torch.no_grad():
            for bn in self.bns:
                for name in ("running_mean", "running_var"):
                    t = getattr(bn.mod, name)
                    bflat[off:off + bn.c].copy_(t.reshape(-1))
                    t.data = bflat[off:off + bn.c]
                    off += bn.c
                nbt = bn.mod.num_batches_tracked
                if nbt.device != self.device:
                    nbt.data = nbt.data.to(self.device)
        self.params = params
        self.flat_p, self.flat_g, self.flat_bn = flat, gflat, bflat
        self._flat_ptrs = [p.data_ptr() for p in params]
        self.packs.rebased()
        self._store_ranges = None  # offsets into the new flat buffer
        self.grad_ranges = module_grad_ranges(self.model)
        # [lo, hi) of every parameter in the flat gradient (per-layer readiness for dp.GradSync)
        self.param_span = {}
        off = 0
        for p in params:
            self.param_span[id(p)] = (off, off + p.numel())
            off += p.numel()

    @contextlib.contextmanager
    def _timed(self, name: str):
        """HIP events around one library call on the current stream when ``kernel_timer`` (a
        dict name -> list) is set: bench.py times the stem kernels inside its timed steps."""
        t = self.kernel_timer
        if t is None:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        t.setdefault(name, []).append((e0, e1))

    def _grads_done(self, *params):
        """The gradients of ``params`` (adjacent in the flat buffer) are final: report their
        flat range to the data-parallel hook (dp.GradSync) -- per layer, as each
        weight-gradient / BatchNorm-backward kernel is enqueued, in descending flat order
        (dp.readiness_groups lists the sequence), so the all-reduce buckets start while the
        backward still runs and only the last layers' bucket waits at the end.  With the
        weight gradients on the side stream the report is made from that stream after it has
        waited for the compute stream's queue, so a bucket's all-reduce is ordered after the
        kernels of both streams that wrote it, and the compute stream itself does not wait for
        the weight gradients (it joins them once per block: _block_bwd)."""
        if self.grad_ready is None:
            return
        spans = [self.param_span[id(p)] for p in params]
        lo, hi = min(a for a, _ in spans), max(b for _, b in spans)
        if self._side_used:
            side = self._side_stream
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                self.grad_ready(lo, hi)
        else:
            self.grad_ready(lo, hi)

    # weight gradients run on a side stream beside the data-gradient chain (dgrad -> BN ->
    # dgrad ...): they only read activations and the dY buffer of their layer, which the main
    # stream does not overwrite before the next _join_side()
    def _side(self, lvl: int, on: Optional[bool] = None):
        if not (lvl >= self.layout.side_min_level if on is None else on):
            return contextlib.nullcontext()
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device)
        self._side_stream.wait_stream(main)
        self._side_used = True
        return torch.cuda.stream(self._side_stream)

    def _join_side(self):
        if self._side_used:
            torch.cuda.current_stream(self.device).wait_stream(self._side_stream)
            self._side_used = False

    def sync_params(self, full: bool = True, fresh_ok: bool = False) -> bool:
        """Re-flatten if a module op (``.to()``, ``.cuda()``, param reassignment) replaced
        storage, and make every ``param.grad`` a view of the flat gradient again.
        ``full=False`` (the calls inside one step after the forward's full check) skips the
        module walk that detects replaced Parameter objects.  ``fresh_ok`` (the backward):
        when EVERY gradient is None (``zero_grad(set_to_none=True)``, torch's default) the views
        are attached without zeroing and True is returned -- the backward then writes the
        gradient instead of accumulating into it (no 361 MB zero fill)."""
        if [p.data_ptr() for p in self.params] != self._flat_ptrs or (
                full and list(self.model.parameters()) != self.params):
            self._flatten()
            return False
        if all(p.grad is None for p in self.params):
            if not fresh_ok:
                return False  # stay None (torch semantics) until a backward attaches them
            off = 0
            for p in self.params:
                n = p.numel()
                p.grad = self.flat_g[off:off + n].view_as(p)
                off += n
            return True
        off = 0
        for p in self.params:
            n = p.numel()
            g = p.grad
            if g is None or g.data_ptr() != self.flat_g.data_ptr() + 4 * off:
                view = self.flat_g[off:off + n].view_as(p)
                with torch.no_grad():
                    if g is None:
                        view.zero_()
                    else:
                        view.copy_(g)
                p.grad = view
            off += n
        return False

    def _store_plan(self):
        """The flat-gradient ranges a fresh backward does NOT write with PCMS_GRAD_STORE (every
        parameter but the weights of the convs that go through pcms_conv3_wgrad): zeroed by one
        pcms_fill_ranges launch before such a backward.  Depends on the stem path (stem_sup)."""
        key = self.stem_sup
        if self._store_ranges is not None and self._store_ranges[0] == key:
            return self._store_ranges[1]
        stored = []
        for i, cs in enumerate(self.convs):
            if i == 0 and self.stem_sup & 2:
                continue  # the stem's streaming kernel accumulates
            w = cs.mod.weight
            stored.append(((w.data_ptr() - self.flat_p.data_ptr()) // 4, w.numel()))
        ranges = gaps(stored, self.flat_g.numel())
        plan = (torch.tensor(ranges, dtype=torch.int64, device=self.device), len(ranges),
                max(e - b for b, e in ranges))
        self._store_ranges = (key, plan)
        return plan

    def mark_dirty(self, packs_fresh: bool = False):
        """The master weights changed.  ``packs_fresh``: by a fused Adam step (adam_plan), which
        already wrote its plan's packs from the new weights."""
        self.packs.changed(by_plan=packs_fresh)

    # ------------------------------------------------------------------ weight packs (packs.WeightPacks)
    stem_pack = property(lambda self: self.packs.stem)
    convt_packs = property(lambda self: self.packs.convt)

    def adam_plan(self):
        return self.packs.adam_plan()

    def _ensure_packs(self):
        self.packs.ensure()

    def _conv_eval(self, i: int, x0, c0, x1, c1, a, N, S):
        """a = relu(conv'(x) + b'): the folded eval conv of self.convs[i] (no statistics)."""
        cs = self.convs[i]
        pack, bias = self.packs.eval[i]
        RELU = 2  # PCMS_CONV_RELU
        r = self.layout.fwd[i]  # the stem kernel or the general one, whatever the training route
        if r.kind == "stem":
            call("pcms_stem_fwd", x0, self.packs.eval["stem"], bias, a, None, N, *S, RELU | self.stem_dense)
        elif r.splits == 1:
            call("pcms_conv3_fwd", cs.code, x0, c0, x1, c1, pack, bias, a, None, cs.cout, None, None, RELU,
                 N, *S, cs.cout, 1)
        else:
            acc = self.bufs["yacc"]
            call("pcms_conv3_fwd", cs.code, x0, c0, x1, c1, pack, bias, a, None, cs.cout, acc, None, 0,
                 N, *S, cs.cout, r.splits)
            call("pcms_split_epilogue", self.code, acc, r.slabs, bias, a, None, cs.cout, None, cs.cout,
                 N * S[0] * S[1] * S[2], RELU)

    # ------------------------------------------------------------------ buffers
    def _levels(self, D, H, W):
        s = [(D, H, W)]
        for _ in range(4):
            d, h, w = s[-1]
            s.append((d // 2, h // 2, w // 2))
        return s

    def _sites(self):
        """The 18 conv call sites in self.convs order: (ConvSpec, level, c0, c1), c0 / c1 the
        channels of the two sources as the block feeds them (the decoder's first conv reads
        the skip and the upsampled halves)."""
        for blk, l in [(bk, i) for i, bk in enumerate(self.enc)] + [(bk, 3 - i) for i, bk in enumerate(self.dec)]:
            c1 = 64 << l if blk in self.dec else 0
            yield blk.c0, l, blk.c0.cin_store - c1, c1
            yield blk.c1, l, blk.c1.cin_store, 0

    def _route(self, N, S, c0, c1, cout, code, b16: bool, dgrad: bool = False, stem: bool = False,
               bnin: bool = False) -> Route:
        """The kernel that runs conv(c0 + c1 -> cout) at N x S, its slab and row counts.  ``b16``:
        the 16x16x32 forms may run it.  ``dgrad``: the dgrad's order of preference (it tries the
        unsplit general kernel before the 16x16x32 split form; the forward after).  ``stem``:
        the dedicated stem forward runs it.  ``bnin``: BN0 + ReLU in the staging (self._bnin):
        the unsplit 16x16x32 kernel where the layer has a pack16 form, else the general one."""
        splits = self._splits(N, S, c0 + c1, cout, code)
        slabs = query("pcms_conv3_splits", code, c0 + c1, splits) if splits > 1 else 1
        ok16 = b16 and bool(query("pcms_conv3_big16_ok", N, *S, c0, c1, cout))
        sp16 = query("pcms_conv3_fwd16_split_ok", N, *S, c0, c1, cout) if b16 else 0
        pack16 = ok16 or sp16 > 0
        if stem:
            kind = "stem"
        elif bnin:
            kind = "b16" if pack16 else "gen"
        else:
            ladder = [("b16", splits == 1 and ok16), ("b16_split", sp16 > 0), ("gen", splits == 1), ("gen_split", True)]
            if dgrad:
                ladder[1], ladder[2] = ladder[2], ladder[1]
            kind = next(k for k, ok in ladder if ok)
        if kind == "stem":
            rows = query("pcms_stem_fwd_rows", N, *S)
        elif kind == "b16":
            rows = query("pcms_conv3_fwd16_rows", N, *S, c0, c1, cout)
        elif kind == "gen":
            rows = query("pcms_conv3_fwd_rows", code, N, *S, c0, c1, cout)
        else:  # the split forms: the epilogue that sums the slabs writes them
            rows = query("pcms_split_epilogue_rows", N * S[0] * S[1] * S[2])
        return Route(kind, splits, slabs, sp16, rows, pack16)

    def _alloc(self, key):
        """Lay out the buffers and the step (self.layout) for ``key``, the Layout fields up to
        ``switches``.  The workspaces are sized for the key's split / weight-gradient workgroup
        targets and library switches: a changed one re-lays them out (a larger one would
        otherwise overrun them)."""
        L = Layout(*key)
        N, D, H, W = key[:4]
        self.bufs = self.layout = self.buf_key = None
        S = self._levels(D, H, W)
        if min(S[4]) < 1:
            raise ValueError(f"spatial size {(D, H, W)} is too small for 4 poolings")
        nv = [N * d * h * w for (d, h, w) in S]
        C = [64 * (1 << l) for l in range(5)]
        T = self.tdtype
        dev = self.device

        def act(l, c):
            return torch.empty(nv[l] * c, dtype=T, device=dev)

        b: Dict[str, object] = {"S": S, "nv": nv, "C": C}
        b["xin"] = act(0, self.cp)
        for l in range(5):
            if l > 0:
                b[f"pool{l}"] = act(l, C[l - 1])
            for k in ("y1", "a1", "y2", "x"):
                b[f"e{l}_{k}"] = act(l, C[l])
        for l in range(4):
            for k in (("u", "a2") if L.act_ckpt else ("u", "y1", "a1", "y2", "a2")):
                # the last decoder block's ReLU output is never stored: the head applies that
                # BatchNorm + ReLU itself (pcms_head_bn_fwd / _bwd)
                b[f"d{l}_{k}"] = act(l, C[l]) if (l, k) != (0, "a2") else None
        if L.act_ckpt:  # shared decoder set (level 0 is the largest: bytes per level ~ 4^-l)
            for k in ("y1", "a1", "y2"):
                b[f"ck_{k}"] = act(0, C[0])
        # gradient buffers
        for l in range(5):
            b[f"gx{l}"] = act(l, C[l])      # grad of encoder output x_l (skip + path)
            b[f"gA{l}"] = act(l, C[l])      # grad of a1 / block outputs (scratch)
            b[f"gY{l}"] = act(l, C[l])      # grad of pre-BN conv outputs (scratch)
            # second one while the side stream may still read gY; else an alias
            b[f"gZ{l}"] = act(l, C[l]) if l >= L.side_min_level else b[f"gY{l}"]
            b[f"gU{l}"] = act(l, C[l])      # grad of up output / pooled input (scratch)
        # dedicated stem kernels where they support the shape (else the general conv kernels)
        self.stem_sup = query("pcms_stem_supported", N, D, H, W) if self.stem_fast else 0
        # the conv call sites: routes, and what each needs of the shared workspaces
        b16 = L.use_b16 and self.code == BF16
        bnin = tuple(self._bnin(blk, N, S[l]) for blk, l in zip(self.enc + self.dec, (0, 1, 2, 3, 4, 3, 2, 1, 0)))
        rows_f = max(max(query("pcms_conv3_mblocks", N, *S[l]) for l in range(5)),
                     query("pcms_stem_fwd_rows", N, *S[0]))
        # weight-gradient workspace: per-split partial rows of the largest conv (and the stem)
        ws = [query("pcms_stem_wgrad_ws_floats", N, *S[0], self.nmod)] if self.stem_fast else [1]
        yacc = 1  # split-K slabs [slabs][nvox][Cout] of every conv (fwd and dgrad) that splits
        fwd, dgrad = [], []
        for cs, l, c0, c1 in self._sites():
            stem = cs.i == 0  # it runs on its own kernels or the general one, and has no dgrad
            rows_f = max(rows_f, query("pcms_conv3_fwd16_rows", N, *S[l], c0, c1, cs.cout))
            ws.append(query("pcms_conv3_wgrad_ws_floats", cs.code, N, *S[l], c0, c1, cs.cout, L.wgrad_target))
            fwd.append(self._route(N, S[l], c0, c1, cs.cout, cs.code, b16 and not stem,
                                   stem=stem and bool(self.stem_sup & 1), bnin=cs.i % 2 == 1 and bnin[cs.i // 2]))
            dgrad.append(None if stem else self._route(N, S[l], cs.cout, 0, cs.cin, cs.code, b16, dgrad=True))
            # both split forms of either direction, whichever the route takes (_conv_eval always
            # takes the general one)
            for r, cout in ((fwd[-1], cs.cout), (dgrad[-1], cs.cin)):
                if r is not None:
                    yacc = max(yacc, (r.slabs if r.splits > 1 else 0) * nv[l] * cout, r.slabs16 * nv[l] * cout)
        rows_s = max(query("pcms_split_epilogue_rows", nv[l]) for l in range(5))
        rows_b = max(query("pcms_bn_bwd_rows", self.code, C[l], nv[l]) for l in range(5))
        # BN partials [rows][C][2] + [rows] voxel counts
        # (also the fused head's BatchNorm partial rows [rows_h][64][2])
        rows_h = query("pcms_head_bn_bwd_rows", D * H * W, N)
        pool_rows = tuple(query("pcms_maxpool_bwd_bn_rows", self.code, N, *S[l], C[l]) for l in range(4))
        rows_b = max(rows_b, *pool_rows)
        b["stats"] = torch.empty(max(max(rows_f, rows_s, rows_b) * (1024 * 2 + 1), rows_h * 64 * 2),
                                 dtype=torch.float32, device=dev)
        b["coef"] = torch.empty(3 * 1024, dtype=torch.float32, device=dev)
        b["bnws"] = torch.empty(query("pcms_bn_ws_doubles", 1024), dtype=torch.float64, device=dev)
        b["dwt"] = torch.empty(max(ws), dtype=torch.float32, device=dev)
        b["yacc"] = torch.empty(yacc, dtype=torch.float32, device=dev)
        # partial rows of the head / ConvT-bias gradient reductions (summed in a fixed order)
        red = [query("pcms_head_bwd_ws_floats", D * H * W, N, self.ncls)]
        for i, up in enumerate(self.ups):
            l = 3 - i
            red.append(query("pcms_convt_wgrad_bias_ws_floats", self.code, N, *S[l + 1], up.in_channels,
                             up.out_channels, 512))
        b["redws"] = torch.empty(max(red), dtype=torch.float32, device=dev)
        ctws = [query("pcms_convt_wgrad_ws_floats", N, *S[4 - i], up.in_channels, up.out_channels, 512)
                for i, up in enumerate(self.ups)]
        if L.convt_wgrad_side:  # the weight gradient's rows apart: the dgrad runs beside it
            b["ctws_w"] = torch.empty(max(ctws), dtype=torch.float32, device=dev)
            ctws = []
        # the ConvT dgrad's K slabs share it (the weight gradient has reduced it by then)
        ctws += [query("pcms_convt_dgrad_ws_floats", N, *S[4 - i], up.in_channels, up.out_channels)
                 for i, up in enumerate(self.ups)]
        # and the forward's K slabs (free in the forward pass)
        ctws += [query("pcms_convt_fwd_ws_floats", N, *S[4 - i], up.in_channels, up.out_channels)
                 for i, up in enumerate(self.ups)]
        b["ctws"] = torch.empty(max(ctws), dtype=torch.float32, device=dev)
        self.packs.relaid(fwd, dgrad)  # the 16x16x32 kernel's weight forms, where it can run the layer
        self.bufs = b
        self.buf_key = key
        self.layout = L._replace(fwd=tuple(fwd), dgrad=tuple(dgrad), bnin=bnin, pool_rows=pool_rows)

    # ------------------------------------------------------------------ primitives
    # _splits and _bnin follow the live split_target / wgrad_target / fuse_bnin: the engine
    # calls them only from _alloc (through _route), within the forward that read those into the
    # key, so Layout's routes are their answers; after that they serve as host-side queries
    def _splits(self, N, S, cin, cout, code):
        mb = query("pcms_conv3_mblocks", N, *S)
        wgs = mb * (cout // 64)
        nch = -(-cin // query("pcms_conv3_chunk", code))
        if wgs >= 192 or nch == 1 or wgs == 0:
            return 1
        return max(1, min(nch, -(-self.split_target // wgs)))

    def _bnin(self, blk: BlockSpec, N, S) -> bool:
        """The block's first BN + ReLU fused into its second conv (forward and weight gradient)?"""
        if not self.fuse_bnin or self.code != BF16:
            return False
        # only where the unfused conv runs unsplit (the same big-box kernel, so the fused step
        # stays bit-identical to the unfused one)
        return bool(query("pcms_conv3_bnin_ok", N, *S, blk.c1.cin, blk.c1.cout, self.wgrad_target)) and \
            self._splits(N, S, blk.c1.cin, blk.c1.cout, self.code) == 1

    def _launch(self, r: Route, cs: ConvSpec, pack16, pack, x0, c0, x1, c1, bias, y0, y1, cy0, cout, st, N, S,
                bnin: Optional[BNSpec] = None):
        """One conv on route ``r``: (y0 | y1, split at channel cy0) = conv(x0 | x1) + bias with
        ``cout`` output channels and BatchNorm partial rows into ``st`` -- a forward (``pack16``
        / ``pack`` = cs.fwd16 / cs.fwd) or a dgrad (cs.dgrad16 / cs.dgrad).  ``bnin``: the input
        is the pre-BN y1 of that BatchNorm; conv(relu(bn(x)))."""
        nvox = N * S[0] * S[1] * S[2]
        isc, ish = (bnin.scale, bnin.shift) if bnin is not None else (None, None)
        if r.kind == "stem":
            with self._timed("stem_fwd"):
                call("pcms_stem_fwd", x0, self.stem_pack, bias, y0, st, N, *S, self.stem_dense)
        elif r.kind == "b16":
            call("pcms_conv3_fwd16", x0, c0, x1, c1, isc, ish, pack16, bias, y0, y1, cy0, st, 0, N, *S, cout)
        elif r.kind == "b16_split":
            acc = self.bufs["yacc"]
            call("pcms_conv3_fwd16_split", x0, c0, x1, c1, pack16, acc, N, *S, cout, r.slabs16)
            call("pcms_split_epilogue", self.code, acc, r.slabs16, bias, y0, y1, cy0, st, cout, nvox, 0)
        else:  # the general kernel and its packs (rebuilt here when the fused Adam skipped them)
            self.packs.general(cs)
            if bnin is not None:
                call("pcms_conv3_fwd_bnin", cs.code, x0, c0, isc, ish, pack, bias, y0, st, N, *S, cout)
            elif r.kind == "gen":
                call("pcms_conv3_fwd", cs.code, x0, c0, x1, c1, pack, bias, y0, y1, cy0, None, st, 0, N, *S, cout, 1)
            else:
                acc = self.bufs["yacc"]
                call("pcms_conv3_fwd", cs.code, x0, c0, x1, c1, pack, bias, y0, y1, cy0, acc, None, 0, N, *S, cout,
                     r.splits)
                call("pcms_split_epilogue", self.code, acc, r.slabs, bias, y0, y1, cy0, st, cout, nvox, 0)

    def _conv(self, cs: ConvSpec, x0, c0, x1, c1, y, N, S, stats: bool, training: bool, bn: BNSpec,
              recompute: bool = False, bnin: Optional[BNSpec] = None):
        """y = conv(x) + b; then BN statistics (train) or eval coefficients.  ``recompute``:
        the conv alone (checkpointed decoder: the forward's BN coefficients are reused).
        ``bnin``: the input is the pre-BN y1 of that BatchNorm; conv(relu(bn(x)))."""
        b = self.bufs
        nvox = N * S[0] * S[1] * S[2]
        r = self.layout.fwd[cs.i]
        st = b["stats"] if training and not recompute else None
        self._launch(r, cs, cs.fwd16, cs.fwd, x0, c0, x1, c1, cs.mod.bias, y, None, cs.cout, cs.cout, st, N, S, bnin)
        if recompute:
            return
        m = bn.mod
        if training:
            if nvox <= 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                                 f"torch.Size([{N}, {bn.c}, {S[0]}, {S[1]}, {S[2]}])")
            call("pcms_bn_finalize", st, r.rows, bn.c, float(nvox), m.weight, m.bias, m.running_mean,
                 m.running_var, m.num_batches_tracked, BN_MOMENTUM, BN_EPS, bn.scale, bn.shift, bn.mean,
                 bn.invstd, b["bnws"])
        else:
            call("pcms_bn_eval_coeffs", m.weight, m.bias, m.running_mean, m.running_var, BN_EPS, bn.c,
                 bn.scale, bn.shift)

    def _block_fwd(self, blk: BlockSpec, x0, c0, x1, c1, out: Dict[str, torch.Tensor], N, S, training,
                   recompute: bool = False, pool_out=None):
        """conv -> BN -> ReLU -> conv -> BN -> ReLU.  ``recompute`` (checkpointed decoder
        backward): y1, a1, y2 again from the same inputs with the forward's BN scale/shift; no
        statistics, no running-stat update, a2 not rewritten.  ``out["a2"] is None``: the
        second BN + ReLU is left to the consumer (the head: pcms_head_bn_fwd).  ``pool_out``
        (encoder blocks 0-3): the output is max-pooled into it in the same pass (the next
        Down3D's MaxPool3d, pcms_bn_relu_pool)."""
        nvox = N * S[0] * S[1] * S[2]
        if not training and self._folded:
            # eval: BN folded, ReLU in the epilogue; the last decoder block's output goes to its
            # y2 buffer, which the plain head then reads (forward(): self._eval_folded)
            i0 = blk.c0.i
            a2 = out["a2"] if out["a2"] is not None else out["y2"]
            self._conv_eval(i0, x0, c0, x1, c1, out["a1"], N, S)
            self._conv_eval(i0 + 1, out["a1"], blk.c0.cout, None, 0, a2, N, S)
            if pool_out is not None:
                call("pcms_maxpool_fwd", self.code, a2, pool_out, N, *S, blk.c1.cout)
            return
        self._conv(blk.c0, x0, c0, x1, c1, out["y1"], N, S, True, training, blk.b0, recompute)
        if self.layout.bnin[blk.c0.i // 2]:  # a1 is never stored: the second conv applies BN0 + ReLU itself
            self._conv(blk.c1, out["y1"], blk.c0.cout, None, 0, out["y2"], N, S, True, training, blk.b1, recompute,
                       bnin=blk.b0)
        else:
            call("pcms_bn_relu", self.code, out["y1"], out["a1"], blk.b0.scale, blk.b0.shift, blk.c0.cout, nvox)
            self._conv(blk.c1, out["a1"], blk.c0.cout, None, 0, out["y2"], N, S, True, training, blk.b1, recompute)
        if recompute or out["a2"] is None:
            return
        if pool_out is not None:
            call("pcms_bn_relu_pool", self.code, out["y2"], out["a2"], pool_out, blk.b1.scale, blk.b1.shift, N, *S,
                 blk.c1.cout)
        else:
            call("pcms_bn_relu", self.code, out["y2"], out["a2"], blk.b1.scale, blk.b1.shift, blk.c1.cout, nvox)

    def _dec_acts(self, l: int) -> Dict[str, torch.Tensor]:
        b = self.bufs
        if not self.layout.act_ckpt:  # the mode the buffers were laid out for
            return {k: b[f"d{l}_{k}"] for k in ("y1", "a1", "y2", "a2")}
        n = b["nv"][l] * b["C"][l]
        return {"y1": b["ck_y1"][:n], "a1": b["ck_a1"][:n], "y2": b["ck_y2"][:n], "a2": b[f"d{l}_a2"]}

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, training: bool, act: int = 0, threshold: float = 0.5,
                keep_input_grad: bool = False) -> torch.Tensor:
        """The network on ``x`` (N, n_modalities, D, H, W).  ``act``: 0 logits, 1 sigmoid
        probabilities (predict), 2 ``sigmoid > threshold`` masks (inference), all produced
        by the head kernel.  ``keep_input_grad`` (eval): the unfolded eval route whatever
        ``fold_bn_eval`` says -- the pre-BN conv outputs are stored and every BatchNorm's
        scale / shift come from pcms_bn_eval_coeffs -- so that ``backward_input`` can follow."""
        if keep_input_grad and training:
            raise ValueError("keep_input_grad is the eval route; a training forward keeps its activations anyway")
        if x.dim() != 5 or x.shape[1] != self.nmod:
            raise ValueError(f"expected input (N, {self.nmod}, D, H, W), got {tuple(x.shape)}")
        if x.device != self.device:
            raise ValueError(f"input on {x.device}, model on {self.device}")
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        N, _, D, H, W = x.shape
        # buffers first: a (re)allocation decides which convs run on the 16x16x32 kernel and
        # gives them new pack16 buffers, which the _ensure_packs below fills.
        # The one read of the step's settings and of the library's switches: the key
        key = (N, D, H, W, self.act_ckpt, self.wgrad_side_min_level, self.convt_wgrad_side, self.pool_bn_apply_fused,
               self.wgrad_target, self.split_target, self.fuse_bnin, self.use_b16, _lib.switches())
        if key != self.buf_key:
            self._alloc(key)
        self._ensure_packs()
        folded = self._folded = not training and self.fold_bn_eval and not keep_input_grad
        if folded:
            self.packs.ensure_eval()
        else:
            self._bn_epoch += training
        b = self.bufs
        S, C = b["S"], b["C"]
        call("pcms_pack_input", self.code, x, b["xin"], N, self.nmod, D * H * W, self.cp)
        # encoder
        inp, cin = b["xin"], self.cp
        for l in range(5):
            if l > 0:  # pool{l} was written by the previous block's fused BN + ReLU + MaxPool pass
                inp, cin = b[f"pool{l}"], C[l - 1]
            out = {"y1": b[f"e{l}_y1"], "a1": b[f"e{l}_a1"], "y2": b[f"e{l}_y2"], "a2": b[f"e{l}_x"]}
            self._block_fwd(self.enc[l], inp, cin, None, 0, out, N, S[l], training,
                            pool_out=b[f"pool{l + 1}"] if l < 4 else None)
        # decoder
        h = b["e4_x"]
        for i in range(4):
            l = 3 - i
            up = self.ups[i]
            fpack, _ = self.convt_packs[i]
            call("pcms_convt_fwd_ws", self.code, h, fpack, up.bias, b[f"d{l}_u"], b["ctws"], N, *S[l + 1],
                 up.in_channels, up.out_channels, *S[l])
            self._block_fwd(self.dec[i], b[f"e{l}_x"], C[l], b[f"d{l}_u"], C[l], self._dec_acts(l), N, S[l],
                            training)
            h = b[f"d{l}_a2"]
        # head = the last decoder block's BN + ReLU + outc 1x1x1 conv in one pass over its y2
        logits = torch.empty((N, self.ncls, D, H, W), dtype=torch.float32, device=self.device)
        oc = self.model.outc
        bn = self.dec[3].b1
        if folded:  # the y2 buffer holds the folded conv's ReLU output
            call("pcms_head_fwd", self.code, self._dec_acts(0)["y2"], oc.weight, oc.bias, logits, D * H * W, N,
                 self.ncls, int(act), float(threshold))
        else:
            call("pcms_head_bn_fwd", self.code, self._dec_acts(0)["y2"], bn.scale, bn.shift, oc.weight, oc.bias,
                 logits, D * H * W, N, self.ncls, int(act), float(threshold))
        self.epoch += 1
        if training:
            self.saved_epoch = self.epoch
        elif keep_input_grad:
            self.saved_eval_epoch = self.epoch
        return logits

    # ------------------------------------------------------------------ backward
    def _stem_dgrad(self, dy1, N, S) -> torch.Tensor:
        """dx (N, n_modalities, D, H, W) fp32 = the stem conv's input gradient of ``dy1`` (the
        gradient of its pre-BN output), on the current stream."""
        dpack = self.packs.stem_dgrad_pack()
        dx = torch.empty((N, self.nmod, *S), dtype=torch.float32, device=self.device)
        with self._timed("stem_dgrad"):
            call("pcms_stem_dgrad", self.code, dy1, dpack, dx, N, *S, self.nmod)
        return dx

    def _block_bwd(self, blk: BlockSpec, ga2, acts, x0, c0, x1, c1, gx_out0, gx_out1, cy0, N, S, lvl,
                   bn1_rows: int = 0, pool_dp=None, want_dx: bool = False):
        """Backward of one DoubleConv block. ga2: grad of block output (None: the second
        BN + ReLU backward was already done by its consumer, gY{lvl} holds dy2).  Writes the
        grad of the block input into gx_out0 (channels [0, cy0)) / gx_out1 (rest); None = skip.
        ``bn1_rows``: the second BatchNorm's backward partial rows are already in the stats
        buffer (written by pcms_maxpool_bwd_bn), only its finish + apply run here.  ``pool_dp``:
        they came from pcms_maxpool_bwd_bn_sums (ga2 holds the skip part only) and the apply
        adds the pooled gradient ``pool_dp`` itself (pcms_maxpool_bn_apply).  ``want_dx`` (the
        stem block): the gradient of the network input is formed too and returned."""
        b = self.bufs
        wt = self.layout.wgrad_target
        nvox = N * S[0] * S[1] * S[2]
        # the previous block's weight gradients (side stream) read this level's buffers until
        # joined (a decoder and an encoder block share gY / gZ / gA at one level)
        self._join_side()
        gY, gZ, gA = b[f"gY{lvl}"], b[f"gZ{lvl}"], b[f"gA{lvl}"]
        # BN1/ReLU backward -> dy2; its weight gradient on the side stream
        if ga2 is not None and bn1_rows:
            m = blk.b1.mod
            call("pcms_bn_relu_bwd_finish", self.code, ga2, acts["y2"], blk.b1.scale, blk.b1.shift, blk.b1.mean,
                 blk.b1.invstd, m.weight, b["stats"], bn1_rows, b["coef"], m.weight.grad, m.bias.grad,
                 gY if pool_dp is None else None, blk.b1.c, nvox, b["bnws"])
            if pool_dp is not None:
                call("pcms_maxpool_bn_apply", self.code, acts["y2"], blk.b1.scale, blk.b1.shift, blk.b1.mean,
                     blk.b1.invstd, b["coef"], pool_dp, ga2, gY, N, *S, blk.b1.c)
        elif ga2 is not None:
            self._bn_bwd(blk.b1, ga2, acts["y2"], gY, nvox)
        if ga2 is not None:
            self._grads_done(blk.b1.mod.weight, blk.b1.mod.bias)
        with self._side(lvl):
            if self.layout.bnin[blk.c0.i // 2]:  # x = relu(bn0(y1)), applied in the kernel's staging (as the forward)
                call("pcms_conv3_wgrad_bnin", blk.c1.code, acts["y1"], blk.c0.cout, blk.b0.scale, blk.b0.shift, gY,
                     blk.c1.mod.weight.grad, b["dwt"], N, *S, blk.c1.cout, blk.c1.cin, wt, int(self._gstore))
            else:
                call("pcms_conv3_wgrad", blk.c1.code, acts["a1"], blk.c0.cout, None, 0, gY, blk.c1.mod.weight.grad,
                     b["dwt"], N, *S, blk.c1.cout, blk.c1.cin, wt, int(self._gstore))
        self._grads_done(blk.c1.mod.weight, blk.c1.mod.bias)
        # dgrad conv1 -> grad of a1
        self._dgrad(blk.c1, gY, gA, None, blk.c1.cin, N, S)
        # BN0/ReLU backward -> dy1 (a second buffer: the side stream may still read gY)
        if blk is self.enc[0] and self.stem_sup & 2:
            # the stem: its BN0 apply runs inside the weight-gradient kernel (dy never stored) --
            # unless the input gradient is wanted: then the apply pass also writes dy1 into gZ.
            # Where gZ is gY's alias this level's weight gradients ran on this stream, so
            # nothing on the side stream reads it (joined all the same)
            bn = blk.b0
            m = bn.mod
            if want_dx and gZ is gY:
                self._join_side()
            call("pcms_bn_relu_bwd", self.code, gA, acts["y1"], bn.scale, bn.shift, bn.mean, bn.invstd, m.weight,
                 b["stats"], b["coef"], m.weight.grad, m.bias.grad, gZ if want_dx else None, bn.c, nvox, b["bnws"])
            self._grads_done(m.weight, m.bias)
            with self._side(lvl), self._timed("stem_wgrad"):
                call("pcms_stem_wgrad_bn", x0, gA, acts["y1"], bn.scale, bn.shift, bn.mean, bn.invstd, b["coef"],
                     blk.c0.mod.weight.grad, b["dwt"], blk.c0.cin, N, *S)
            self._grads_done(blk.c0.mod.weight, blk.c0.mod.bias)
            return self._stem_dgrad(gZ, N, S) if want_dx else None
        self._bn_bwd(blk.b0, gA, acts["y1"], gZ, nvox)
        self._grads_done(blk.b0.mod.weight, blk.b0.mod.bias)
        with self._side(lvl):
            call("pcms_conv3_wgrad", blk.c0.code, x0, c0, x1, c1, gZ, blk.c0.mod.weight.grad, b["dwt"], N,
                 *S, blk.c0.cout, blk.c0.cin, wt, int(self._gstore))
        self._grads_done(blk.c0.mod.weight, blk.c0.mod.bias)
        if gx_out0 is not None:
            self._dgrad(blk.c0, gZ, gx_out0, gx_out1, cy0, N, S)
        if want_dx:  # the stem on the general route: gZ holds dy1
            return self._stem_dgrad(gZ, N, S)
        return None

    def _bn_bwd(self, bn: BNSpec, ga, y, gy, nvox):
        b = self.bufs
        m = bn.mod
        call("pcms_bn_relu_bwd", self.code, ga, y, bn.scale, bn.shift, bn.mean, bn.invstd, m.weight,
             b["stats"], b["coef"], m.weight.grad, m.bias.grad, gy, bn.c, nvox, b["bnws"])

    def _dgrad(self, cs: ConvSpec, gy, out0, out1, cy0, N, S):
        """(out0 | out1, split at channel cy0) = the gradient of the input of conv ``cs``."""
        self._launch(self.layout.dgrad[cs.i], cs, cs.dgrad16, cs.dgrad, gy, cs.cout, None, 0, None, out0, out1, cy0,
                     cs.cin, None, N, S)

    def backward(self, dlogits: torch.Tensor, want_dx: bool = False) -> Optional[torch.Tensor]:
        """The training backward: every parameter gradient into the flat gradient buffer.
        ``want_dx``: also the gradient of the network input, returned as a fresh fp32 tensor
        (N, n_modalities, D, H, W); the parameter gradients are the same bits either way."""
        if self.saved_epoch != self.epoch:
            raise RuntimeError("UNet3D backward must follow its own training forward (the engine keeps "
                               "only the activations of the latest forward)")
        L = self.layout  # the forward's: the buffers were laid out for it, whatever the settings are now
        fresh = self.sync_params(full=False, fresh_ok=True)
        self._gstore = fresh
        if fresh:
            ranges, nr, mx = self._store_plan()
            call("pcms_fill_ranges", self.flat_g, ranges, nr, mx, 0.0)
        b = self.bufs
        S, C = b["S"], b["C"]
        N = L.N
        dlogits = dlogits.contiguous().float()
        oc = self.model.outc
        D, H, W = S[0]
        # head + the last decoder block's BN + ReLU backward in two passes over its y2 (the
        # forward's level-0 y2: under checkpointing the shared set still holds it, and the
        # recompute below rewrites the same bits); dy2 -> gY0
        bn = self.dec[3].b1
        m = bn.mod
        call("pcms_head_bn_bwd", self.code, self._dec_acts(0)["y2"], bn.scale, bn.shift, bn.mean, bn.invstd, m.weight,
             dlogits, oc.weight, oc.weight.grad, oc.bias.grad, b["redws"], b["stats"], b["coef"], m.weight.grad,
             m.bias.grad, b["gY0"], D * H * W, N, self.ncls, b["bnws"])
        self._grads_done(oc.weight, oc.bias)
        self._grads_done(m.weight, m.bias)  # the last decoder block's second BatchNorm (fused above)
        g = None
        # decoder, last block first
        for i in reversed(range(4)):
            l = 3 - i
            blk = self.dec[i]
            acts = self._dec_acts(l)
            self._join_side()  # the recompute rewrites the shared set the side stream may still read
            if L.act_ckpt:
                self._block_fwd(blk, b[f"e{l}_x"], C[l], b[f"d{l}_u"], C[l], acts, N, S[l], True, recompute=True)
            gu = b[f"gU{l}"]
            self._block_bwd(blk, g, acts, b[f"e{l}_x"], C[l], b[f"d{l}_u"], C[l], b[f"gx{l}"], gu, C[l], N,
                            S[l], l)
            up = self.ups[i]
            _, dpack = self.convt_packs[i]
            hin = b["e4_x"] if i == 0 else b[f"d{l + 1}_a2"]
            # weight and bias gradients in one pass over gu (the bias sum over the ConvT output
            # box, F.pad's front offsets floor((S[l] - 2 S[l + 1]) / 2))
            with self._side(l, L.convt_wgrad_side):
                call("pcms_convt_wgrad_bias", self.code, hin, gu, up.weight.grad, up.bias.grad,
                     b["ctws_w"] if L.convt_wgrad_side else b["ctws"], b["redws"], N, *S[l + 1], up.in_channels,
                     up.out_channels, *S[l], 512)
            self._grads_done(up.weight, up.bias)
            gnext = b["gx4"] if i == 0 else b[f"gA{l + 1}"]
            call("pcms_convt_dgrad_ws", self.code, gu, dpack, gnext, b["ctws"], N, *S[l + 1], up.in_channels,
                 up.out_channels, *S[l])
            g = gnext
        # encoder, deepest first; gx{l} holds the skip gradient already (l < 4)
        rows, pool_dp, dx = 0, None, None
        for l in reversed(range(5)):
            blk = self.enc[l]
            acts = {"y1": b[f"e{l}_y1"], "a1": b[f"e{l}_a1"], "y2": b[f"e{l}_y2"]}
            if l == 0:
                dx = self._block_bwd(blk, b["gx0"], acts, b["xin"], self.cp, None, 0, None, None, 0, N, S[0], 0,
                                     bn1_rows=rows, pool_dp=pool_dp, want_dx=want_dx)
            else:
                gp = b[f"gU{l}"]
                self._block_bwd(blk, b[f"gx{l}"], acts, b[f"pool{l}"], C[l - 1], None, 0, gp, None, C[l - 1], N,
                                S[l], l, bn1_rows=rows, pool_dp=pool_dp)
                # MaxPool3d backward + the next block's second BN-backward reduction, one pass
                # (fused form: the pooled gradient is added again by that block's BN apply, so
                # the block output's gradient gx{l-1} is not rewritten)
                bn = self.enc[l - 1].b1
                call("pcms_maxpool_bwd_bn_sums" if L.pool_bn_apply_fused else "pcms_maxpool_bwd_bn", self.code,
                     b[f"e{l - 1}_y2"], bn.scale, bn.shift, bn.mean, bn.invstd, gp, b[f"gx{l - 1}"], b["stats"], N,
                     *S[l - 1], C[l - 1])
                pool_dp = gp if L.pool_bn_apply_fused else None
                rows = L.pool_rows[l - 1]
        self._join_side()  # every weight gradient before the optimizer / all-reduce wait
        self.saved_epoch = -1
        return dx

    # ------------------------------------------------------------------ eval input gradient
    def _block_bwd_input(self, blk: BlockSpec, ga2, acts, gx_out0, gx_out1, cy0, N, S, lvl, stem: bool = False):
        """_block_bwd without the weight gradients and BatchNorm reductions (eval: running
        statistics are constants): BN1 + ReLU backward (``ga2`` None: gY{lvl} holds dy2 already),
        conv1 dgrad, BN0 + ReLU backward, conv0 dgrad -- or, ``stem``, pcms_stem_dgrad, whose
        result is returned."""
        b = self.bufs
        nvox = N * S[0] * S[1] * S[2]
        gY, gZ, gA = b[f"gY{lvl}"], b[f"gZ{lvl}"], b[f"gA{lvl}"]
        if ga2 is not None:
            call("pcms_bn_relu_bwd_eval", self.code, ga2, acts["y2"], blk.b1.scale, blk.b1.shift, gY, blk.b1.c, nvox)
        self._dgrad(blk.c1, gY, gA, None, blk.c1.cin, N, S)
        call("pcms_bn_relu_bwd_eval", self.code, gA, acts["y1"], blk.b0.scale, blk.b0.shift, gZ, blk.b0.c, nvox)
        if stem:
            return self._stem_dgrad(gZ, N, S)
        self._dgrad(blk.c0, gZ, gx_out0, gx_out1, cy0, N, S)
        return None

    def backward_input(self, dlogits: torch.Tensor) -> torch.Tensor:
        """The gradient of the network input after an eval forward with ``keep_input_grad``: the
        training schedule minus every weight gradient and BatchNorm reduction.  No parameter
        gradient is read or written."""
        if self.saved_eval_epoch != self.epoch:
            raise RuntimeError("UNet3D input-gradient backward must follow its own eval forward (the engine "
                               "keeps only the activations of the latest forward)")
        L = self.layout
        b = self.bufs
        S, C = b["S"], b["C"]
        N = L.N
        D, H, W = S[0]
        dlogits = dlogits.contiguous().float()
        self._join_side()
        bn = self.dec[3].b1
        call("pcms_head_bn_bwd_eval", self.code, self._dec_acts(0)["y2"], bn.scale, bn.shift, dlogits,
             self.model.outc.weight, b["gY0"], D * H * W, N, self.ncls)
        g = None
        for i in reversed(range(4)):
            l = 3 - i
            blk = self.dec[i]
            acts = self._dec_acts(l)
            if L.act_ckpt:
                self._block_fwd(blk, b[f"e{l}_x"], C[l], b[f"d{l}_u"], C[l], acts, N, S[l], True, recompute=True)
            gu = b[f"gU{l}"]
            self._block_bwd_input(blk, g, acts, b[f"gx{l}"], gu, C[l], N, S[l], l)
            up = self.ups[i]
            _, dpack = self.convt_packs[i]
            gnext = b["gx4"] if i == 0 else b[f"gA{l + 1}"]
            call("pcms_convt_dgrad_ws", self.code, gu, dpack, gnext, b["ctws"], N, *S[l + 1], up.in_channels,
                 up.out_channels, *S[l])
            g = gnext
        dx = None
        for l in reversed(range(5)):
            acts = {"y1": b[f"e{l}_y1"], "a1": b[f"e{l}_a1"], "y2": b[f"e{l}_y2"]}
            if l == 0:
                dx = self._block_bwd_input(self.enc[0], b["gx0"], acts, None, None, 0, N, S[0], 0, stem=True)
            else:
                gp = b[f"gU{l}"]
                self._block_bwd_input(self.enc[l], b[f"gx{l}"], acts, gp, None, C[l - 1], N, S[l], l)
                # MaxPool3d backward into the skip gradient gx{l-1} (the stored block output
                # e{l-1}_x gives the arg-max)
                call("pcms_maxpool_bwd", self.code, b[f"e{l - 1}_x"], gp, b[f"gx{l - 1}"], N, *S[l - 1], C[l - 1])
        self.saved_eval_epoch = -1
        return dx
