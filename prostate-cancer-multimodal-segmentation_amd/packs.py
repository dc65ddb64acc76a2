"""Kernel weight packs of the U-Net engine, and the one rule that keeps them current.

Every pack (bf16 / fp32, MFMA-friendly order) is derived from the flat fp32 master, whose state
has one name, the weight identity ``(wgen, flat_p._version)``: torch's storage version sees
in-place torch writes, ``wgen`` counts what it does not see (a write through the C ABI reported
by ``changed``, a new flat buffer, a change of conv arithmetic).  Packs come in groups;
``built[group]`` is the identity a group was last built from, and ``_ensure`` rebuilds a group
exactly when that differs from the current one:

  ("gen", i)    ConvSpec.fwd / .dgrad of conv i: the general kernel's pair
  "stem"        the dedicated stem forward's pack (bf16 build)
  "stem_dgrad"  pcms_stem_dgrad's pack
  "p16"         every ConvSpec.fwd16 / .dgrad16 of the layout: one batched pcms_conv3_pack16
  ("convt", i)  the forward / dgrad pair of ConvTranspose i
  "eval"        the folded eval set; its record also carries the BatchNorm buffers' state

Who ensures: ``ensure`` (before every forward) the eager groups; a launch of the general kernel
(``general``) the pair it reads; the stem dgrad pack and the eval set their first use.  One
other party stamps: the fused Adam writes packs in its own pass, and ``changed(by_plan=True)``
records the new identity for exactly the groups its plan wrote.  After such a step ``ensure``
leaves the general pairs the plan did not write (those of convs that run on the 16x16x32
kernel only, and the stem's beside its dedicated kernel) to ``general``; after any other change
it rebuilds every general pair at once.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from ._lib import BF16, F32, call, query

BN_EPS = 1e-5


def gaps(spans, total: int):
    """The [begin, end) ranges of [0, total) that the (offset, length) ``spans`` leave free."""
    out, pos = [], 0
    for off, n in sorted(spans):
        if off > pos:
            out.append([pos, off])
        pos = off + n
    if pos < total:
        out.append([pos, total])
    return out


def pack_general(cs):
    """The general kernel's packs of ``cs`` from its master weight: both directions in one
    launch, or the forward alone (the stem has no dgrad pack)."""
    if cs.dgrad is None:
        call("pcms_conv3_pack", cs.code, cs.mod.weight, cs.fwd, cs.cout, cs.cin, 0)
    else:
        call("pcms_conv3_pack2", cs.code, cs.mod.weight, cs.fwd, cs.dgrad, cs.cout, cs.cin)


class WeightPacks:
    def __init__(self, eng):
        self.e = eng
        self.wgen = 0
        self.built: Dict[object, tuple] = {}
        self.stepped = None  # the identity a complete fused Adam step made (it stamped what it wrote)
        self.read = set()    # convs whose general pair a launch of this layout read
        self.stem = self.stem_dgrad = None
        self.convt: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.eval = None     # {conv index: (fwd pack, folded bias)}, "stem": stem pack
        # cached device tables (adam_plan's, pcms_conv3_pack16's): they hold pointers into the
        # packs and the flat master, and are dropped when either moves
        self._plan = self._table16 = None

    def identity(self):
        return (self.wgen, self.e.flat_p._version)

    def current(self, group) -> bool:
        return self.built.get(group) == self.identity()

    def _ensure(self, group, cur, build, *args):
        if self.built.get(group) != cur:
            build(*args)
            self.built[group] = cur

    def _empty(self, elems: str, *args):
        return torch.empty(query(elems, *args), dtype=self.e.tdtype, device=self.e.device)

    # ------------------------------------------------------------------ what changes the identity or moves pointers
    def changed(self, by_plan: bool = False):
        """The master changed behind torch's back.  ``by_plan``: by a fused Adam step run from
        the cached plan, which wrote the plan's packs from the new weights."""
        self.wgen += 1
        if by_plan and self._plan is not None and self._plan["complete"]:
            self.stepped = cur = self.identity()
            self.built.update((g, cur) for g in self._plan["writes"])

    def rebased(self):
        """A new flat master (UNetEngine._flatten)."""
        self.wgen += 1
        self._plan = self._table16 = None

    def recoded(self, convs):
        """The conv arithmetic of ``convs`` changed: their packs change size and contents."""
        for cs in convs:
            cs.fwd = cs.dgrad = None
        self.eval = None
        self.wgen += 1
        self._plan = self._table16 = None

    def relaid(self, fwd, dgrad):
        """A new layout with the routes ``fwd`` / ``dgrad`` per conv: new pack16 buffers for the
        directions a 16x16x32 form runs, and nothing read through the general kernel yet."""
        for cs, rf, rd in zip(self.e.convs, fwd, dgrad):
            cs.fwd16 = self._empty("pcms_conv3_pack16_elems", cs.cout, cs.cin) if rf.pack16 else None
            cs.dgrad16 = None
            if rd is not None and rd.pack16:
                cs.dgrad16 = self._empty("pcms_conv3_pack16_elems", cs.cin, cs.cout)
        self.read.clear()
        self.built.pop("p16", None)
        self.built.pop("eager", None)
        self._plan = self._table16 = None

    # ------------------------------------------------------------------ ensure
    def ensure(self):
        """The eager groups, before a forward or a plan.  Steady state: one comparison, and
        after a fused Adam step the stem pack's launch."""
        e, cur = self.e, self.identity()
        if self.built.get("eager") == cur:
            return
        lazy = self.stepped == cur
        for cs in e.convs:
            if not lazy or (cs.i == 0 and not e.stem_fast):
                self._ensure(("gen", cs.i), cur, self._build_general, cs)
        if e.stem_fast:
            self._ensure("stem", cur, self._build_stem)
        for i, up in enumerate(e.ups):
            self._ensure(("convt", i), cur, self._build_convt, i, up)
        self._ensure("p16", cur, self._build_pack16)
        self.built["eager"] = cur

    def general(self, cs):
        """Before a launch of the general kernel reads cs.fwd / cs.dgrad: the pair is ensured,
        and a cached Adam plan that does not write it is dropped, so that the next one does."""
        self._ensure(("gen", cs.i), self.identity(), self._build_general, cs)
        if cs.i not in self.read:
            self.read.add(cs.i)
            if self._plan is not None and cs.i in self._plan["skipped"]:
                self._plan = None

    def stem_dgrad_pack(self):
        """pcms_stem_dgrad's weight pack: a step that asks for no input gradient launches and
        allocates nothing for it."""
        self._ensure("stem_dgrad", self.identity(), self._build_stem_dgrad)
        return self.stem_dgrad

    def ensure_eval(self):
        """The folded eval set, current with the parameters and the running statistics (every
        training forward moves those: UNetEngine._bn_epoch)."""
        self.ensure()
        self._ensure("eval", self.identity() + (self.e.flat_bn._version, self.e._bn_epoch), self._build_eval)

    # ------------------------------------------------------------------ builders
    def _build_general(self, cs):
        if cs.fwd is None:
            cs.fwd = self._empty("pcms_conv3_pack_elems", cs.code, cs.cout, cs.cin)
            if cs.i != 0:  # the stem's input gradient has its own kernel and pack
                cs.dgrad = self._empty("pcms_conv3_pack_elems", cs.code, cs.cin, cs.cout)
        pack_general(cs)

    def _build_stem(self):
        if self.stem is None:
            self.stem = self._empty("pcms_stem_pack_elems")
        call("pcms_stem_pack", self.e.convs[0].mod.weight, self.stem, self.e.nmod)

    def _build_stem_dgrad(self):
        e = self.e
        if self.stem_dgrad is None:
            self.stem_dgrad = self._empty("pcms_stem_dgrad_pack_elems", e.code)
        call("pcms_stem_dgrad_pack", e.code, e.convs[0].mod.weight, self.stem_dgrad, e.nmod)

    def _build_convt(self, i, up):
        code, cin, cout = self.e.code, up.in_channels, up.out_channels
        if i not in self.convt:
            self.convt[i] = (self._empty("pcms_convt_pack_elems", code, cin, cout),
                             self._empty("pcms_convt_pack_elems", code, cin, cout))
        f, d = self.convt[i]
        call("pcms_convt_pack", code, up.weight, f, cin, cout, 0)
        call("pcms_convt_pack", code, up.weight, d, cin, cout, 1)

    def _build_pack16(self):
        """One batched pcms_conv3_pack16 launch from the fp32 master."""
        if self._table16 is None:
            rows, tiles = [], 0
            for cs in self.e.convs:
                if cs.fwd16 is None and cs.dgrad16 is None:
                    continue
                rows.append([cs.mod.weight.data_ptr(), cs.cout, cs.cin, 0 if cs.fwd16 is None else cs.fwd16.data_ptr(),
                             0 if cs.dgrad16 is None else cs.dgrad16.data_ptr(), tiles, 0, 0])
                tiles += (cs.cout // 32) * (cs.cin // 32)
            self._table16 = (torch.tensor(rows if rows else [[0] * 8], dtype=torch.int64, device=self.e.device),
                             len(rows), tiles)
        tab, n, tiles = self._table16
        if n:
            call("pcms_conv3_pack16", tab, n, tiles)

    def _build_eval(self):
        """w' = w * gamma / sqrt(rvar + eps), b' = b * sc + beta - rmean * sc per conv
        (pcms_bn_fold), then the forward pack of w'."""
        e = self.e
        if self.eval is None:
            self.eval = {}
            self._eval_tmp = torch.empty(max(cs.cout * cs.cin * 27 for cs in e.convs), dtype=torch.float32,
                                         device=e.device)
        tmp = self._eval_tmp
        for i, (cs, bn) in enumerate(zip(e.convs, e.bns)):
            if i not in self.eval:
                self.eval[i] = (self._empty("pcms_conv3_pack_elems", cs.code, cs.cout, cs.cin),
                                torch.empty(cs.cout, dtype=torch.float32, device=e.device))
            pack, bias = self.eval[i]
            m = bn.mod
            call("pcms_bn_fold", cs.mod.weight, cs.mod.bias, m.weight, m.bias, m.running_mean, m.running_var,
                 BN_EPS, cs.cout, cs.cin * 27, tmp, bias)
            call("pcms_conv3_pack", cs.code, tmp, pack, cs.cout, cs.cin, 0)
            if i == 0 and e.stem_fast:
                if "stem" not in self.eval:
                    self.eval["stem"] = self._empty("pcms_stem_pack_elems")
                call("pcms_stem_pack", tmp, self.eval["stem"], e.nmod)

    # ------------------------------------------------------------------ fused Adam
    def adam_plan(self):
        """Fused Adam + weight-pack plan (FlatAdam.step): device tables of the conv / ConvT
        weights whose packs the Adam kernels write (int64 rows, see include/pcms_hip.h
        pcms_adam_pack_conv3) and the [begin, end) ranges of every other parameter.  The bf16
        build writes bf16 packs, the pack16 forms among them; the fp32 build (``"x6"``: True)
        its bf16x6 packs, for the convs in bf16x6 mode (a conv switched to bf16x3 is repacked
        as before).  ``"writes"``: the groups a step from this plan leaves current;
        ``"skipped"``: the convs whose general pair it does not write, every call of this
        layout having run on the 16x16x32 kernel so far."""
        if self._plan is not None:
            return self._plan
        e = self.e
        x6 = e.code != BF16
        self.ensure()
        base = e.flat_p.data_ptr()

        def offset(t):
            return (t.data_ptr() - base) // 4

        def tab(rows, width=8):
            return torch.tensor(rows if rows else [[0] * width], dtype=torch.int64, device=e.device)

        fused, writes, skipped = [], [], []
        missed = 0  # layers (besides the stem) whose packs the Adam kernels do not write
        conv_rows, tiles = [], 0
        for cs in e.convs[1:]:
            w = cs.mod.weight
            if cs.cin % 32 or cs.cout % 32 or offset(w) % 4 or (x6 and cs.code != F32):
                missed += 1
                continue
            f16 = cs.fwd16.data_ptr() if not x6 and cs.fwd16 is not None else 0
            d16 = cs.dgrad16.data_ptr() if not x6 and cs.dgrad16 is not None else 0
            skip = bool(f16 and d16) and cs.i not in self.read
            conv_rows.append([offset(w), cs.cout, cs.cin, 0 if skip else cs.fwd.data_ptr(),
                              0 if skip else cs.dgrad.data_ptr(), tiles, f16, d16])
            if skip:
                skipped.append(cs.i)
            else:
                writes.append(("gen", cs.i))
            tiles += (cs.cout // 32) * (cs.cin // (16 if x6 else 32))
            fused.append((offset(w), w.numel()))
        ct_rows, ct_tiles = [], 0
        for i, up in enumerate(e.ups):
            w = up.weight
            cin, cout = up.in_channels, up.out_channels
            if cin % 32 or cout % 32 or offset(w) % 4:
                missed += 1
                continue
            f, d = self.convt[i]
            ct_rows.append([offset(w), cin, cout, f.data_ptr(), d.data_ptr(), ct_tiles, 0, 0])
            writes.append(("convt", i))
            ct_tiles += (cin // 32) * (cout // 32)
            fused.append((offset(w), w.numel()))
        ranges = gaps(fused, e.flat_p.numel())
        self._plan = {
            "conv": tab(conv_rows), "nconv": len(conv_rows), "conv_tiles": tiles,
            "convt": tab(ct_rows), "nconvt": len(ct_rows), "convt_tiles": ct_tiles,
            "ranges": tab(ranges, 2), "nranges": len(ranges), "max_len": max([b - a for a, b in ranges], default=0),
            # every conv / ConvT layer but the stem is in the tables (else the step stamps
            # nothing: everything is repacked, as after any other change of the master)
            "complete": missed == 0,
            "x6": x6,
            "p16": not x6,  # the pack16 forms come out of the Adam pass
            "writes": writes + ([] if x6 else ["p16"]), "skipped": skipped,
        }
        return self._plan
