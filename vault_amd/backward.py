"""Backward pass of the HIP engine (what autograd does for ref: vault/models/vault/model.py:151-218 under
vault/tmsc_utils/trainer.py:365): the chain of data gradients layer by layer, top down, and the deferred weight
gradients of a stack packed into full rounds of 256 x 256 tiles."""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import torch

from . import ops
from .params import _in_format, _pad


class BackwardMixin:
    # ---- deferred weight gradients on a second stream -------------------------------------------
    def _wgrads_aside(self, launch, after_layer, items=0):
        """Run ``launch()`` (the batched weight-gradient GEMMs of a group of layers) on the engine's second stream when the
        backward chain leaves CUs idle (few token rows: a chain GEMM of a small batch is a single partial round of tiles).
        Nothing in the chain reads the weight gradients: only the optimizer, which waits for the stream (_join_wgrads).
        Not in data-parallel steps (``after_layer``: the reducer starts on the main stream's events)."""
        if not (self._wgrad_side or items > 0) or after_layer is not None:
            launch()
            return
        if self._wgrad_stream is None:
            self._wgrad_stream = torch.cuda.Stream(self.device)
        side, main, ev = self._wgrad_stream, torch.cuda.current_stream(), torch.cuda.Event()
        ops.pycall(lambda: ev.record(main))
        ops.pycall(lambda: side.wait_event(ev))
        with torch.cuda.stream(side):
            self._wgrad_items = items       # (items per grouped launch of THIS group: _wgrad_group)
            try:
                launch()
            finally:
                self._wgrad_items = 0
        self._wgrad_pending = True

    def _join_wgrads(self):
        if self._wgrad_pending:
            side, main, ev = self._wgrad_stream, torch.cuda.current_stream(), torch.cuda.Event()
            ops.pycall(lambda: ev.record(side))
            ops.pycall(lambda: main.wait_event(ev))
            self._wgrad_pending = False

    def _wgrad(self, dy_bf16, x_bf16, wname, bname, Mtok_pad, Nout, Kin, m_valid, out_rows=0, unsplit=False):
        # dW[Nout,Kin] += dY[Mtok,Nout]^T . X[Mtok,Kin] ; db[Nout] += colsum(dY)
        # (``unsplit``: one pass over the tokens per tile - each element receives ONE float add, so the result does not depend on
        #  the order of atomics: the 256-token contractions of the pruned last ViLT layer, four k-steps long)
        P = self.params
        gw = P.gr(wname, n_elems=Nout * Kin, shape=(Nout, Kin))
        if gw is None:
            return
        nk = Mtok_pad // 64
        # (a WIDE weight with a short contraction - the patch projection's 768 x 3072 at B <= 113: 36 ring tiles x 7 splits fill
        #  the chip; as 144 simple tiles x 3 splits it took 352 us of the B = 64 step, 0.12 PFLOP/s: profiles/r06_small_batch_*)
        wide = Nout % 256 == 0 and Kin % 256 == 0 and (Nout // 256) * (Kin // 256) >= 24
        if Mtok_pad <= 16384 and Nout % 128 == 0 and Kin % 128 == 0 and not wide:
            # short contractions (the LM's 40-token sequences: 10240 rows at B = 256): 128x128 tiles with few splits
            # beat the 256x256 ring kernel, whose tiles x splits cannot fill the chip without very short K ranges
            # (tools/wgrad_sweep.py; in-step A/B on one box: +1.0 % samples/s)
            tiles = (Nout // 128) * (Kin // 128)
            splits = 7 if tiles <= 36 else (4 if tiles <= 108 else 3)
            cfg = 0
        elif Nout % 256 == 0 and Kin % 256 == 0:
            # 256x256 ring kernel; split the token contraction so that tiles x splits fills the 256 CUs once
            tiles = (Nout // 256) * (Kin // 256)
            splits = max(1, min(nk // 2, 256 // tiles, 16))   # >16 partial sums per element: float atomics dominate
            cfg = 3
        else:
            tiles = (Nout // 128) * (Kin // 128)
            splits = max(1, min(nk, (self.WGRAD_TARGET_WGS + tiles - 1) // tiles))
            cfg = 0
        if unsplit:
            splits = 1
        if cfg == 3:
            ops.pycall(lambda: self._prof_begin("wgrad"))
        ops.gemm(dy_bf16, x_bf16, gw, Nout, Kin, Mtok_pad, Nout, Kin, Kin, 1, 1, ops.EPI_F32_ATOMIC, cfg=cfg,
                 splits=splits, accumulate=1, m_valid=out_rows)   # out_rows: rows of dW that exist (0 = all Nout)
        if cfg == 3:
            fl = 2.0 * m_valid * Nout * Kin
            ops.pycall(lambda: self._prof_end("wgrad", fl))
        if bname is not None:
            ops.colsum(dy_bf16, Nout, m_valid, Nout, P.gr(bname, n_elems=Nout, shape=(Nout,)))

    @staticmethod
    def _wgrad_splits(items, per_round, nk, fixed, fixed_unsplit=None):
        """Split count (1 .. 8, two 64-token k-steps each at least) of a persistent weight-gradient launch by a cost model: rounds of
        ``per_round`` blocks over ``items`` tiles x (k-steps at 1.67 us + ``fixed`` us per item; ``fixed_unsplit``: un-split, may store)."""
        def cost(sp):
            fx = fixed_unsplit if (sp == 1 and fixed_unsplit is not None) else fixed
            return -(-items * sp // per_round) * (1.67 * -(-nk // sp) + fx)
        return min((sp for sp in range(1, 9) if nk // sp >= 2), key=cost)

    def _wgrad_batched(self, dY_all, X_all, wnames, i0, Mtok_pad, Nout, Kin, m_valid):
        """dW_l[Nout,Kin] += dY_l[Mtok,Nout]^T . X_l[Mtok,Kin] for the consecutive layers l = i0 .. i0 + len(wnames) - 1 of a
        stack in ONE launch (vault_gemm `batch`): dY_l / X_l are slices of the stacked operand tensors, the dW_l lie
        at a uniform stride in the flat gradient buffer (identical layer layouts)."""
        P = self.params
        G = len(wnames)
        offs = [P.offsets[w][0] for w in wnames]
        stride_o = (offs[1] - offs[0]) if G > 1 else 0
        if any(offs[k + 1] - offs[k] != stride_o for k in range(G - 1)) or Nout % 128 or Kin % 128:
            raise RuntimeError("batched weight gradients need identically laid out layers and 128-multiples")
        gw = P.gr(wnames[0], n_elems=Nout * Kin, shape=(Nout, Kin))
        nk = Mtok_pad // 64
        if Nout % 256 == 0 and Kin % 256 == 0:
            # ring kernel, persistent over (layer, split, tile) items, layer-major: an XCD works on whole layers.  Split
            # count by the cost model of the launch (~40 us fixed per item)
            cfg, tiles = 3, (Nout // 256) * (Kin // 256) * G
            splits = self._wgrad_splits(tiles, 256, nk, 40.0)
        else:
            cfg, tiles = 0, (Nout // 128) * (Kin // 128) * G
            splits = max(1, min(8, Mtok_pad // 512, int(round(512.0 / tiles))))   # ~two resident 128x128 blocks per CU
        st = torch.cuda.current_stream()
        if cfg == 3:
            ops.pycall(lambda: self._prof_begin("wgrad", st))
        # un-split launches whose caller vouches for zero gradients (the fused train step: AdamW cleared them) STORE the
        # tiles instead of adding them with float atomics (memory-side, ~1.3 TB/s against 6 TB/s for stores: 44 -> 10 us
        # of a 216-tile launch's tail)
        acc = 0 if (self._grads_zero and splits == 1) else 1
        ops.gemm(dY_all[i0], X_all[i0], gw, Nout, Kin, Mtok_pad, Nout, Kin, Kin, 1, 1, ops.EPI_F32_ATOMIC, cfg=cfg,
                 splits=splits, accumulate=acc, batch=G, batch_a=dY_all.stride(0), batch_b=X_all.stride(0),
                 batch_o=stride_o)
        if acc == 0:
            self._stored_ranges += [(o, Nout * Kin) for o in offs]
        if cfg == 3:
            fl = 2.0 * m_valid * Nout * Kin * G
            ops.pycall(lambda: self._prof_end("wgrad", fl, st))
    def _wgrad_group_size(self, n_layers, after_layer, stack="lm"):
        """Layers per deferred weight-gradient group.  A single process takes the whole stack (1,296 tiles = five full rounds +
        16 tiles, against two remainders of 136: B = 256, same box, 40.2 -> 39.8 ms per step; equal at B = 64) - so does a
        step that runs the reducer on ONE rank (VAULT_FORCE_DP: nothing goes on a wire, nothing is there to overlap).  With
        more ranks (``dp_world``, set by TrainStep) the LM stack keeps groups of LM_WGRAD_GROUP layers - the upper group's
        gradient range goes on the wire under the backward of the layers below it - and the ViLT stack stays whole when a
        trained LM stack follows: its whole range (half of the gradient bytes) is exchanged under the LM backward."""
        if after_layer is None or self.dp_world <= 1:
            return n_layers
        if stack == "vilt" and self.spec.lm is not None and not self.freeze_lm:
            return n_layers
        g = self.LM_WGRAD_GROUP
        return g if g > 0 else n_layers

    def _wgrad_group(self, kinds, layers, i0, hi, Mtok_pad, m_valid, counts=None):
        """Weight gradients of layers i0 .. hi - 1 of a stack.  ``kinds``: (dY stack, X stack, weight attribute, Nout, Kin) per
        Linear kind.  Every 256 x 256 tile of every kind costs the same (the contraction runs over the tokens), so the tiles
        of all kinds are packed into launches of exactly 256 items - one per CU, un-split, stored (or added) once - and one
        remainder launch whose split count comes from the cost model (vault_wgrad_grouped); one launch per kind leaves 16 %
        of the CUs idle in the 216-tile FFN launches and splits the attention-out / QKV ones 4 / 3 ways with float atomics.
        Falls back to one batched launch per kind when a shape is not a multiple of 256 (the tiny test models).
        ``counts``: layers per kind, i0 .. i0 + count - 1 (default: all of the group; the pruned last ViLT layer contracts its
        FFN and attention-out gradients itself, over its compact rows: those kinds end one layer earlier)."""
        P = self.params
        Gs = [hi - i0] * len(kinds) if counts is None else list(counts)
        kinds, Gs = [k for k, n in zip(kinds, Gs) if n > 0], [n for n in Gs if n > 0]
        hms = [k[5] if len(k) > 5 else 0 for k in kinds]        # rows per plane of a head-major dY (the QKV kind's dqkv), 0 = row-major
        kinds = [k[:5] for k in kinds]
        ok = all(no % 256 == 0 and ki % 256 == 0 for *_, no, ki in kinds)
        strides = []
        for (dY_all, X_all, wsel, Nout, Kin), G in zip(kinds, Gs):
            offs = [P.offsets[getattr(l_, wsel)][0] for l_ in layers[i0:i0 + G]]
            so = (offs[1] - offs[0]) if G > 1 else 0
            ok = ok and all(offs[k + 1] - offs[k] == so for k in range(G - 1))
            strides.append(so)
        if not ok:
            if any(hms):
                raise RuntimeError("head-major dqkv needs the grouped ring weight-gradient launches (_plan_head_major)")
            for (dY_all, X_all, wsel, Nout, Kin), G in zip(kinds, Gs):
                self._wgrad_batched(dY_all, X_all, [getattr(l_, wsel) for l_ in layers[i0:i0 + G]], i0, Mtok_pad, Nout, Kin, m_valid)
            return
        nk = Mtok_pad // 64
        # items per launch: one per CU; beside a backward chain on another stream (small batches) fewer, so that the chain's
        # kernels find free CUs while a launch's persistent blocks hold theirs (WGRAD_SIDE_ITEMS)
        CU = self._wgrad_items or (self.WGRAD_SIDE_ITEMS if self._wgrad_side else 256)
        # items of every kind in list order, cut into launches of CU items (<= 3 segments each)
        remaining = []
        for k, (dY_all, X_all, wsel, Nout, Kin) in enumerate(kinds):
            remaining.append([k, 0, (Nout // 256) * (Kin // 256) * Gs[k]])      # kind, first item, items left
        launches, cur, room = [], [], CU
        for k, first, left in remaining:
            while left > 0:
                take = min(left, room)
                cur.append((k, first, take))
                first, left, room = first + take, left - take, room - take
                if room == 0 or len(cur) == 3:
                    launches.append(cur)
                    cur, room = [], CU
        if cur:
            launches.append(cur)
        st = torch.cuda.current_stream()
        covered: Dict[tuple, int] = {}      # (kind, layer) -> tiles written by store launches
        for segs in launches:
            count = sum(c for _, _, c in segs)
            if count == CU:
                splits = 1
            else:       # remainder: fixed cost per piece ~10 us stored, ~50 us with float atomics
                splits = self._wgrad_splits(count, CU, nk, 50.0, 10.0 if self._grads_zero else 50.0)
            acc = 0 if (self._grads_zero and splits == 1) else 1
            args = []
            for k, first, c in segs:
                dY_all, X_all, wsel, Nout, Kin = kinds[k]
                if acc == 0:
                    tpl = (Nout // 256) * (Kin // 256)
                    for it in range(first, first + c):       # items are (layer-major, tile-minor)
                        covered[(k, it // tpl)] = covered.get((k, it // tpl), 0) + 1
                gw = P.gr(getattr(layers[i0], wsel), n_elems=Nout * Kin, shape=(Nout, Kin))
                args.append(dict(dy=dY_all[i0], x=X_all[i0], dw=gw, n_out=Nout, n_in=Kin, batch=Gs[k], first=first, count=c,
                                 batch_dy=dY_all.stride(0), batch_x=X_all.stride(0), batch_dw=strides[k], dy_hm=hms[k]))
            ops.pycall(lambda: self._prof_begin("wgrad", st))
            ops.wgrad_grouped(args, Mtok_pad, splits=splits, accumulate=acc)
            fl = 2.0 * m_valid * 65536.0 * count
            ops.pycall(lambda fl=fl: self._prof_end("wgrad", fl, st))
        for (k, lay), n in covered.items():
            _, _, wsel, Nout, Kin = kinds[k]
            if n == (Nout // 256) * (Kin // 256):
                self._stored_ranges.append((P.offsets[getattr(layers[i0 + lay], wsel)][0], Nout * Kin))

    def _qkv_bias_grads_batched(self, dqkv_all, layers, i0, hi, ld, rows, N, hm=0, parts=None):
        """QKV bias gradients of layers i0 .. hi - 1 (column sums over the token rows of the first N columns of their dqkv) in
        ONE launch, issued with the group's batched weight gradients: at small batches a single layer's pass is a 4 us read
        behind a 10 us launch + reduction tail, and next to the weight gradients it is off the backward chain."""
        P = self.params
        offs = [P.offsets[l_.qb][0] for l_ in layers[i0:hi]]
        stride_o = (offs[1] - offs[0]) if len(offs) > 1 else 0
        if any(offs[k + 1] - offs[k] != stride_o for k in range(len(offs) - 1)):
            raise RuntimeError("batched bias gradients need identically laid out layers")
        gqb = P.gr(layers[i0].qb, n_elems=ld, shape=(ld,))
        if parts is not None:      # the attention backward left its workgroups' partial column sums: add the rows up
            part_all, nparts = parts
            ops.colsum_partials(part_all[i0], nparts, N, gqb, hi - i0, part_all.stride(0), stride_o)
            return
        if hm:       # head-major dqkv: plane p = columns 64 p .. 64 p + 63
            ops.colsum_hm(dqkv_all[i0], rows, hm, N // 64, gqb, hi - i0, dqkv_all.stride(0), stride_o)
            return
        ops.colsum_batched(dqkv_all[i0], ld, rows, N, gqb, hi - i0, dqkv_all.stride(0), stride_o)
    # ---- backward ---------------------------------------------------------------------------
    @_in_format
    def zero_grad(self):
        if self.params.g is not None:
            self.params.g.zero_()
        self._g_dirty = False
        self._g_stale_key = None

    def backward(self, grad_scale: Optional[float] = None, dlogits: Optional[torch.Tensor] = None,
                 dpooled: Optional[torch.Tensor] = None, dhidden: Optional[torch.Tensor] = None,
                 after_layer=None, ws: Optional[dict] = None):
        """Accumulate parameter gradients of the last train-mode forward into the flat grad buffer.

        Default (VaultForTMSC + labels): d(mean CE)/d(params), scaled by ``grad_scale`` (1/B).
        ``dlogits`` / ``dpooled`` / ``dhidden`` inject external output gradients (autograd bridge).
        ``after_layer(tag)`` is called after each stage so a DP driver can start all-reducing the
        gradient range that just became final.
        """
        self._api_backward_begins()
        with torch.cuda.device(self.device), self._grads_scaled():
            self._backward(grad_scale, dlogits, dpooled, dhidden, after_layer, ws)
            if self.grad_scale != 1.0:      # gradients handed back to the caller's autograd graph
                w_ = self.last if ws is None else ws
                for k in ("d_inputs_embeds", "d_image_embeds"):
                    t = w_.get(k)
                    if t is not None:
                        with ops.operand_format(self.half):
                            ops.scale(t, 1.0 / self.grad_scale, t.numel())

    def _api_backward_begins(self):
        """A backward outside the fused train step ACCUMULATES into the flat gradient buffer: ranges a fused step left un-zeroed
        (its next step would have stored over them) are cleared first; the buffer then holds gradients the fused step must not
        build on (it stores its un-split weight-gradient tiles: TrainStep zeroes when it finds the flag)."""
        if self._g_stale_key is not None:
            self.zero_grad()
        self._g_dirty = True

    @contextlib.contextmanager
    def _grads_scaled(self):
        """Context for a backward outside the fused train step when the operand format carries a gradient scale (fp16): the
        flat gradient buffer may hold earlier, un-scaled contributions (gradient accumulation, several encoder passes): it
        is multiplied by the scale before and by its inverse after the backward - exact, a power of two."""
        def rescale(factor):
            if self.grad_scale != 1.0 and self.params.g is not None:
                with ops.operand_format(self.half):
                    ops.scale(self.params.g, factor, self.params.n_train)
        rescale(self.grad_scale)
        try:
            yield
        finally:
            rescale(1.0 / self.grad_scale)

    def _scaled_in(self, ws, name, t):
        """An externally supplied output gradient (f32) times the gradient scale, in a workspace buffer (identity at 1)."""
        t = t.contiguous()
        if self.grad_scale == 1.0:
            return t
        b = self._buf(ws, name, tuple(t.shape), torch.float32)
        b.copy_(t)
        ops.scale(b.view(-1), self.grad_scale, b.numel())
        return b

    @_in_format
    def _backward(self, grad_scale, dlogits, dpooled, dhidden, after_layer, ws=None, grads_zero=False):
        # grads_zero: the caller vouches that the flat gradient buffer is all zero (TrainStep: the fused optimizer cleared
        # it) - un-split weight-gradient launches may then store instead of accumulate
        self._grads_zero = bool(grads_zero)
        # (element offset, length) of every weight-gradient matrix this backward writes with STORES only (whole matrix covered by
        # un-split launches): the fused optimizer need not zero them for the next step of the same shape (TrainStep)
        self._stored_ranges = []
        ws = self.last if ws is None else ws
        if ws is None or not ws.get("train"):
            raise RuntimeError("backward() needs a preceding forward(train=True)")
        if ws.get("pruned_last") and dhidden is not None:
            raise ValueError("the forward pruned the last layer to the pooler's rows: a gradient of last_hidden_state needs "
                             "forward(need_hidden=True)")
        self.drop_seed = ws["drop_seed"]
        note = (lambda tag: ops.pycall(lambda: after_layer(tag))) if after_layer is not None else (lambda tag: None)
        # deferred weight gradients beside the backward chain when its GEMMs are single partial rounds of tiles (same-box
        # A/B: B = 8 9.76 -> 9.48 ms/step, B = 64 16.12 -> 15.69; B = 256 43.5 -> 43.2: within noise, and concurrent
        # kernels would blur the per-kernel timings the roofline line is built on - serial there)
        self._wgrad_side = ws["Mp"] <= self.WGRAD_STREAM_MAX_ROWS
        vb = self._vilt_grad_buffers(ws, after_layer)
        self._backward_head(ws, vb["top"], grad_scale, dlogits, dpooled, dhidden)
        note("head")
        self._backward_vilt_stack(ws, vb, after_layer, note)
        dvs = self._backward_vilt_embeddings(ws, vb["dx"], after_layer)
        note("vilt_embed")
        if self.spec.lm is None or self.freeze_lm:
            self._join_wgrads()
        else:
            self._backward_lm_stack(ws, dvs, after_layer, note)
        self._run_census(ws, "backward")

    # ---- deferred weight gradients of a stack: groups of layers ------------------------------------
    def _wgrad_groups(self, ws, tag, layers, after_layer, dY, X, rows_pad, rows):
        """A stack's deferred weight gradients (_layer_done): ``dY`` stacks of FFN-out, FFN-in, attention-out, QKV; ``X``: names of theirs."""
        H, FF = ws["H"], ws["FF"]
        kinds = tuple((dy, ws[x], wsel, no, ki) for dy, x, (wsel, no, ki) in
                      zip(dY, X, (("fw", H, FF), ("iw", FF, H), ("ow", H, H), ("qw", 3 * H, H))))
        # (``ends``: one past the last layer of each kind; a pruned last ViLT layer keeps only its QKV kind in the groups)
        n, cut = len(layers), 1 if (tag == "vilt" and ws.get("pruned_last")) else 0
        return dict(layers=layers, size=self._wgrad_group_size(n, after_layer, tag), kinds=kinds, H=H,
                    rows_pad=rows_pad, rows=rows, ends=(n - cut, n - cut, n - cut, n))

    def _layer_done(self, tag, grp, i, note, after_layer, N=None, hm=0, parts=None, items=0, ahead=None):
        """Layer ``i`` of a stack has run its data gradients: report it (per-layer weight gradients: ``grp`` None) or, at the bottom
        layer of a group, launch the group's QKV bias sums (the first ``N`` columns of dqkv, default all 3H; ``hm`` / ``parts``:
        head-major dqkv / the attention backward's partial sums) and weight gradients - ``ahead()`` first, ``items``:
        _wgrads_aside - and report the group's layers top down."""
        if grp is None:
            note(f"{tag}{i}")
        if grp is None or i % grp["size"]:
            return
        layers, kinds, H, hi = grp["layers"], grp["kinds"], grp["H"], min(len(grp["layers"]), i + grp["size"])
        if ahead is not None:
            ahead()

        def launch():
            self._qkv_bias_grads_batched(kinds[3][0], layers, i, hi, 3 * H, grp["rows"], 3 * H if N is None else N, hm=hm, parts=parts)
            self._wgrad_group(kinds[:3] + (kinds[3] + (hm,),), layers, i, hi, grp["rows_pad"], grp["rows"],
                              counts=[max(0, min(hi, e) - i) for e in grp["ends"]])
        self._wgrads_aside(launch, after_layer, items=items)
        for j in reversed(range(i, hi)):
            note(f"{tag}{j}")

    # ---- head / tail ------------------------------------------------------------------------------
    def _backward_head(self, ws, dxb_top, grad_scale, dlogits, dpooled, dhidden):
        """Classifier / pooler / final LayerNorm: the gradient at the top of the ViLT stack into ``dxb_top``."""
        spec, P, x, nv = self.spec, self.params, ws["x"], len(self.vl)
        B, S, M, H = (ws[k] for k in ("B", "S", "M", "H"))
        # (pruned last layer: the stack's output and the gradient at its top are compact, one row per sample - nothing to clear)
        pruned = bool(ws.get("pruned_last"))
        cls_map = (0, 0, 0) if pruned else (1, S, 0)
        if not pruned:
            ops.pycall(dxb_top.zero_)
        if spec.add_pooling_layer and (spec.n_classes > 0 or dpooled is not None):
            Bp = ws["Bp"]
            dpre = self._buf(ws, "dpre", (Bp, H), self.hdt)
            if spec.n_classes > 0 and spec.head == "mlp" and dpooled is None:
                if dlogits is None:
                    raise ValueError("the MLP head has no built-in loss: pass dlogits (the autograd bridge does)")
                ops.tanh_bwd(ws["pooled"], self._mlp_backward(ws, dlogits, B, scale=self.grad_scale), dpre, B * H)
            elif spec.n_classes > 0 and dpooled is None:
                hd = self._drop(self.classifier_dropout, 9001, True)
                gs = ((1.0 / B) if grad_scale is None else grad_scale) * self.grad_scale
                if dlogits is not None:
                    dlogits = self._scaled_in(ws, "dlogits_scaled", dlogits)
                ops.head_bwd(ws["pooled"], ws["logits"], ws.get("labels"), P.w("classifier.1.weight"),
                             P.gr("classifier.1.weight"), P.gr("classifier.1.bias"), dpre, B, H, spec.n_classes, gs,
                             dlogits=dlogits, drop=hd)
            else:
                ops.tanh_bwd(ws["pooled"], self._scaled_in(ws, "dpooled_scaled", dpooled), dpre, B * H)
            self._wgrad(dpre, ws["h0b"], "pooler.dense.weight", "pooler.dense.bias", Bp, H, H, B)
            dh0 = self._buf(ws, "dh0", (Bp, H), self.hdt)
            self._dgrad(dpre, "pooler.dense.weight", dh0, Bp, H, H, ops.EPI_BF16, B)
            ops.layernorm_bwd(ws["pl_xout"] if pruned else x[nv], ws["f_mean"], ws["f_rstd"], P.w("layernorm.weight"), B, H,
                              dy_bf16=dh0, dx_bf16=dxb_top, dgamma=P.gr("layernorm.weight"),
                              dbeta=P.gr("layernorm.bias"), xmap=cls_map, dxmap=cls_map,
                              dbias=None if dhidden is not None else P.gr(self.vl[nv - 1].fb))
        if dhidden is not None:
            # gradient w.r.t. last_hidden_state (all rows): LN backward over all rows, added on top
            ops.layernorm_bwd(x[nv], ws["f_mean_all"], ws["f_rstd_all"], P.w("layernorm.weight"), M, H,
                              dy_f32=self._scaled_in(ws, "dhidden_scaled", dhidden).view(M, H),
                              dres_bf16=dxb_top,        # (in place: every element is read, then written, by one lane)
                              dx_bf16=dxb_top,
                              dgamma=P.gr("layernorm.weight"), dbeta=P.gr("layernorm.bias"),
                              dbias=P.gr(self.vl[nv - 1].fb))

    # ---- encoder layers through the stage-level C ABI ----------------------------------------------
    def _layer_bwd_staged(self, ws, style, layers, i, d, deferred):
        """One C call (csrc/stage.hip: the kernels of _vilt_layer_bwd / _lm_layer_bwd in their order); ``d``: vault_layer_bwd_args members."""
        P, ln, H = self.params, layers[i], ws["H"]
        a = ws[f"stage_{style}{i}"]
        if style == "lm":
            a.drop_seed = self.drop_seed & 0xFFFFFFFF
        gb = ops.layer_bwd_args(
            a, **d, do_wgrad=0 if deferred else 1, g_wqkv=P.gr(ln.qw, n_elems=3 * H * H, shape=(3 * H, H)),
            g_bqkv=None if deferred else P.gr(ln.qb, n_elems=3 * H, shape=(3 * H,)),      # (deferred: with the group's launches)
            g_wo=P.gr(ln.ow), g_bo=P.gr(ln.ob), g_wi=P.gr(ln.iw), g_bi=P.gr(ln.ib), g_wf=P.gr(ln.fw),
            g_ln1w=P.gr(ln.ln1w), g_ln1b=P.gr(ln.ln1b), g_ln2w=P.gr(ln.ln2w), g_ln2b=P.gr(ln.ln2b),
            # (the FFN-out bias gradient: post-LN LM - this layer's, from its LN2 backward; pre-LN ViLT - the layer's below)
            g_bf=P.gr(ln.fb) if style == "lm" else None,
            g_bf_below=P.gr(layers[i - 1].fb) if (style == "vilt" and i > 0) else None)
        ws[f"stage_{style}_bwd{i}"] = gb
        ops.layer_call(f"vault_{style}_layer_bwd", gb, seeded=bool(a.attn_drop_thresh or a.hid_drop_thresh))

    # ---- ViLT stack -------------------------------------------------------------------------------
    def _vilt_grad_buffers(self, ws, after_layer):
        """``dx`` (f32 gradient at the bottom of the stack: the embedding backward reads it), the two 16-bit buffers of the residual-
        gradient stream or - deferred weight gradients - the per-layer ``dY`` stacks with their groups ``grp``, ``top``: the head's."""
        Mp, H, FF, nv, bf = ws["Mp"], ws["H"], ws["FF"], len(self.vl), self.hdt
        vb = dict(dx=self._buf(ws, "dx_a", (Mp, H), torch.float32), grp=None,
                  dxb=(self._buf(ws, "dxb_a", (Mp, H), bf), self._buf(ws, "dxb_b", (Mp, H), bf)))
        if self.LM_WGRAD_BATCHED and "act_all" in ws and self.params.gr(self.vl[0].fw) is not None:
            # dY operands of every ViLT layer stay alive until their group's batched weight-gradient launches:
            # A = gradient at the layer output (FFN-out's dY), B = gradient behind the attention block (attn-out's dY)
            vb["dY"] = (self._stack(ws, "v_dxbA", nv, (Mp, H), bf), self._stack(ws, "v_dU", nv, (Mp, FF), bf),
                        self._stack(ws, "v_dxbB", nv, (Mp, H), bf), self._stack(ws, "v_dqkv", nv, (Mp, 3 * H), bf))
            vb["grp"] = self._wgrad_groups(ws, "vilt", self.vl, after_layer, vb["dY"],
                                           ("act_all", "n2_all", "ctx_all", "n1_all"), Mp, ws["M"])
        vb["top"] = vb["dY"][0][nv - 1] if vb["grp"] else vb["dxb"][0]
        if ws.get("pruned_last"):
            vb["top"] = self._buf(ws, "pl_dtop", (ws["Bp"], H), bf)
        return vb

    def _backward_vilt_stack(self, ws, vb, after_layer, note):
        """The pre-LN ViLT layers, top down.  Residual-gradient stream in bf16 only (GRAD_STREAM_BF16): a layer's incoming
        gradient is ONE bf16 tensor - stream and FFN-out dY at once -, the LayerNorm backward adds it as `dres_bf16` and writes
        only the bf16 result (10 instead of 16 B per element); the bottom layer also writes f32 for the embedding backward."""
        B, S, Mp, H, FF, heads, nv, bf = ws["B"], ws["S"], ws["Mp"], ws["H"], ws["FF"], ws["heads"], len(self.vl), self.hdt
        grp, staged, (dxa, dxb) = vb["grp"], bool(ws.get("vilt_stage")), vb["dxb"]
        d = dict(dN=self._buf(ws, "dN", (Mp, H), bf), dctx=self._buf(ws, "dctx", (Mp, H), bf))
        if not grp:
            d.update(dy_bf16=dxa, dmid_bf16=dxb, dx_bf16=dxa, dU=self._buf(ws, "dU", (Mp, FF), bf), dqkv=self._buf(ws, "dqkv", (Mp, 3 * H), bf))
        # QKV bias gradient from inside the attention backward (vault_attn_args.bias_partials) where the deferred launches would
        # otherwise re-read dqkv for it: the query third (the shortcut covers key / value: no attention dropout here).  The
        # stage call takes neither: the group's launches sum all of (row-major) dqkv
        short, vparts = bool(grp) and self.QKV_BIAS_SHORTCUT and not staged, None
        if short:
            npart = ops.attention_bwd_partials(B, S, H, heads, 1)
            if npart:
                vparts = (self._stack(ws, "v_qbpart", nv, (npart, H), torch.float32), npart)
        # the whole stack's group, launched when the ViLT chain is through, with a trained LM stack's backward next: that
        # chain's GEMMs are partial rounds of tiles at any batch (40 row panels at B = 256) - the group runs beside it
        beside = self.WGRAD_BESIDE_LM_ITEMS if (grp and grp["size"] >= nv and not staged and self.spec.lm is not None
                                                and not self.freeze_lm and not self._wgrad_side) else 0
        ops.pycall(lambda: self._prof_begin("vilt_bwd"))
        for i in reversed(range(nv)):
            if grp:
                d["dy_bf16"], d["dU"], d["dmid_bf16"], d["dqkv"] = (t[i] for t in vb["dY"])
                d["dx_bf16"] = vb["dY"][0][i - 1] if i > 0 else dxa
            d["dx_f32"] = vb["dx"] if i == 0 else None
            if staged:
                self._layer_bwd_staged(ws, "vilt", self.vl, i, d, bool(grp))
            elif i == nv - 1 and ws.get("pruned_last"):
                self._vilt_last_layer_bwd_pruned(ws, i, d, bool(grp), short, vparts, vb["top"])
            else:
                self._vilt_layer_bwd(ws, i, d, bool(grp), short, vparts)
            self._layer_done("vilt", grp, i, note, after_layer, H if short else 3 * H, ws.get("qkv_hm", 0), vparts, beside)
        ops.pycall(lambda: self._prof_end("vilt_bwd"))

    def _vilt_layer_bwd(self, ws, i, d, deferred, short, vparts):
        """The layer backward kernel by kernel (``deferred``: without its weight gradients)."""
        P, ln, vhm = self.params, self.vl[i], ws.get("qkv_hm", 0)
        B, S, M, Mp, H, FF, heads = (ws[k] for k in ("B", "S", "M", "Mp", "H", "FF", "heads"))
        g = lambda k: ws[f"{k}{i}"]  # noqa: E731
        wgrad = (lambda *a: None) if deferred else self._wgrad      # (deferred: with the group's launches, _layer_done)
        dyA, dyB, dU, dqkv, dN, dctx = (d[k] for k in ("dy_bf16", "dmid_bf16", "dU", "dqkv", "dN", "dctx"))
        # FFN
        # (bias gradients are column sums of dY: fused into the kernel that PRODUCES dY - the LayerNorm
        #  backward for the residual-stream gradient, the GEMM epilogue for dU)
        g8 = ws.get("gelu8_active")
        g8kw = dict(cfg=g8, aux_u8=True) if g8 is not None else {}
        self._dgrad(dyA, ln.fw, dU, Mp, FF, H, ops.EPI_BF16_DGELU, M, aux=g("u"), colsum=P.gr(ln.ib), **g8kw)
        wgrad(dyA, g("act"), ln.fw, None, Mp, H, FF, M)
        self._dgrad(dU, ln.iw, dN, Mp, H, FF, ops.EPI_BF16, M)
        wgrad(dU, g("n2"), ln.iw, None, Mp, FF, H, M)
        ops.layernorm_bwd(g("xm"), g("m2"), g("r2"), P.w(ln.ln2w), M, H, dy_bf16=dN, dres_bf16=dyA, dx_bf16=dyB,
                          dgamma=P.gr(ln.ln2w), dbeta=P.gr(ln.ln2b), dbias=P.gr(ln.ob))
        # attention
        # QKV bias gradient without a pass over all of dqkv (``short``: QKV_BIAS_SHORTCUT; the ViLT stack has no attention
        # dropout, D2): softmax rows sum to one, so  sum_keys dV = sum_queries dO  - the value bias gradient is the column sum of
        # dctx, taken in the epilogue of the GEMM that produces dctx; sum_keys dS = 0 for every query, so the key bias
        # gradient is zero (the reference's autograd leaves rounding noise of 1e-9 there); only the query third is summed
        gqb = P.gr(ln.qb, n_elems=3 * H, shape=(3 * H,))
        self._dgrad(dyB, ln.ow, dctx, Mp, H, H, ops.EPI_BF16, M, **(dict(colsum=gqb[2 * H:]) if short else {}))
        wgrad(dyB, g("ctx"), ln.ow, None, Mp, H, H, M)
        ops.attention_bwd(g("qkv"), ws["keymask"], g("ctx"), g("lse"), dctx, dqkv, B, S, H, heads, qkv_hm=vhm,
                          **(dict(bias_partials=vparts[0][i], bias_thirds=1) if vparts else {}))
        self._dgrad(dqkv, ln.qw, dN, Mp, H, 3 * H, ops.EPI_BF16, M, **(dict(a_hm=vhm) if vhm else {}))
        wgrad(dqkv, g("n1"), ln.qw, ln.qb, Mp, 3 * H, H, M)
        # (deferred: the QKV bias gradient's query third - or, without the shortcut, all of it - with the group's launches)
        ops.layernorm_bwd(ws["x"][i], g("m1"), g("r1"), P.w(ln.ln1w), M, H, dy_bf16=dN, dres_bf16=dyB,
                          dx_f32=d["dx_f32"], dx_bf16=d["dx_bf16"], dgamma=P.gr(ln.ln1w), dbeta=P.gr(ln.ln1b),
                          dbias=P.gr(self.vl[i - 1].fb) if i > 0 else None)

    def _vilt_last_layer_bwd_pruned(self, ws, i, d, deferred, short, vparts, dtop):
        """Backward of the last ViLT layer after a pruned forward (engine._vilt_last_layer_pruned): the gradient at the top of
        the stack is non-zero on the CLS rows only, ``dtop`` holds them compact.  The FFN, LayerNorm 2 and attention-out data
        gradients run on those Bp rows, and the three weight gradients are Bp-token contractions, launched here, un-split (one
        add per element into memory the optimizer zeroed - as reproducible as the stored tiles of the grouped launches;
        _stored_ranges does not list them).  Attention backward has one live query
        per item and writes all of dqkv; the QKV data gradient, LayerNorm 1 backward and - deferred or not - the QKV weight
        gradient and bias sums are the full-size layer's.  LayerNorm 1's residual gradient is a full-size buffer that only
        ever holds the CLS rows (``pl_dres``: zero elsewhere from its allocation)."""
        P, ln, vhm = self.params, self.vl[i], ws.get("qkv_hm", 0)
        B, S, M, Mp, H, FF, heads, Bp = (ws[k] for k in ("B", "S", "M", "Mp", "H", "FF", "heads", "Bp"))
        bf = self.hdt
        g, c = (lambda k: ws[f"{k}{i}"]), (lambda k: ws[f"pl_{k}"])  # noqa: E731
        dU, dNc, dmid, dctx = (self._buf(ws, f"pl_{k}", (Bp, w), bf) for k, w in (("dU", FF), ("dN", H), ("dmid", H), ("dctx", H)))
        dres, dqkv, dN = self._buf(ws, "pl_dres", (Mp, H), bf), d["dqkv"], d["dN"]
        g8 = ws.get("pl_gelu8")
        g8kw = dict(cfg=g8, aux_u8=True) if g8 is not None else {}
        self._dgrad(dtop, ln.fw, dU, Bp, FF, H, ops.EPI_BF16_DGELU, B, aux=c("u"), colsum=P.gr(ln.ib), like=Mp, **g8kw)
        self._wgrad(dtop, c("act"), ln.fw, None, Bp, H, FF, B, unsplit=True)
        self._dgrad(dU, ln.iw, dNc, Bp, H, FF, ops.EPI_BF16, B, like=Mp)
        self._wgrad(dU, c("n2"), ln.iw, None, Bp, FF, H, B, unsplit=True)
        ops.layernorm_bwd(c("xm"), c("m2"), c("r2"), P.w(ln.ln2w), B, H, dy_bf16=dNc, dres_bf16=dtop, dx_bf16=dmid,
                          dgamma=P.gr(ln.ln2w), dbeta=P.gr(ln.ln2b), dbias=P.gr(ln.ob))
        ops.rows_scatter_h16(dmid, dres, B, H, 1, S, 0)          # dres[b S] = dmid[b]
        # (the value-bias shortcut holds: the only queries with dO != 0 are the CLS rows, and softmax rows still sum to one)
        gqb = P.gr(ln.qb, n_elems=3 * H, shape=(3 * H,))
        self._dgrad(dmid, ln.ow, dctx, Bp, H, H, ops.EPI_BF16, B, like=Mp, **(dict(colsum=gqb[2 * H:]) if short else {}))
        self._wgrad(dmid, c("ctx"), ln.ow, None, Bp, H, H, B, unsplit=True)
        ops.attention_bwd(g("qkv"), ws["keymask"], c("ctx"), g("lse"), dctx, dqkv, B, S, H, heads, qkv_hm=vhm, q_rows=1,
                          **(dict(bias_partials=vparts[0][i], bias_thirds=1) if vparts else {}))
        self._dgrad(dqkv, ln.qw, dN, Mp, H, 3 * H, ops.EPI_BF16, M, **(dict(a_hm=vhm) if vhm else {}))
        if not deferred:
            self._wgrad(dqkv, g("n1"), ln.qw, ln.qb, Mp, 3 * H, H, M)
        ops.layernorm_bwd(ws["x"][i], g("m1"), g("r1"), P.w(ln.ln1w), M, H, dy_bf16=dN, dres_bf16=dres,
                          dx_f32=d["dx_f32"], dx_bf16=d["dx_bf16"], dgamma=P.gr(ln.ln1w), dbeta=P.gr(ln.ln1b),
                          dbias=P.gr(self.vl[i - 1].fb) if i > 0 else None)

    # ---- ViLT embeddings --------------------------------------------------------------------------
    def _backward_vilt_embeddings(self, ws, dx0, after_layer):
        """Image rows (patch projection with its weight gradient) and text rows; returns the f32 gradient of the text embedding sum."""
        spec, P, v = self.spec, self.params, self.spec.vilt
        B, T, S, H, NP, Ml, Mlp, Kp, Mpp = (ws[k] for k in ("B", "T", "S", "H", "NP", "Ml", "Mlp", "Kp", "Mpp"))
        buf = lambda name, shape, dtype=torch.float32: self._buf(ws, name, shape, dtype)  # noqa: E731
        dyp = buf("dyp", (Mpp, H), self.hdt)
        gpos = P.gr("embeddings.position_embeddings", shape=(v.num_patches + 1, H))
        gmt = P.gr("embeddings.token_type_embeddings.weight")
        if ws.get("img_embeds") is not None:
            # externally supplied image embeddings: their gradient (for the caller's autograd) and the modality type's
            die = buf("d_iemb", (_pad(B * NP), H))
            ops.rows_gather_bwd(dx0, die, gmt[ws.get("img_type", 1)], B * NP, H, NP, S, T)
            ws["d_image_embeds"] = die[:B * NP].view(B, NP, H)
        elif ws["ragged"]:
            ops.image_sel_bwd(dx0, gpos, gmt[ws.get("img_type", 1)], P.gr("embeddings.cls_token", shape=(H,)),
                              P.gr("embeddings.patch_embeddings.projection.bias"), dyp, ws["sel"], ws["hw"], B, NP, S, T, H,
                              ws["gw"], v.image_size // v.patch_size)
        else:
            ops.image_rows_bwd(dx0, gpos, gmt[ws.get("img_type", 1)], P.gr("embeddings.cls_token", shape=(H,)),
                               P.gr("embeddings.patch_embeddings.projection.bias"), dyp, NP, H, B, S, T)
        if ws.get("img_embeds") is None:
            # (small batches: beside the chain, like the stack's deferred launches - nothing below reads this gradient)
            self._wgrads_aside(lambda: self._wgrad(dyp, ws["apatch_in"] if ws.get("patches_in") else ws["apatch"],
                                                   "embeddings.patch_embeddings.projection.weight", None,
                                                   Mpp, H, Kp, B * NP), after_layer)
        dvs = buf("d_vt_sum", (Mlp, H))
        # text rows: out = LN(.) + mtype[0]  =>  d mtype[0] = sum dy = THIS backward's d beta: taken through a scratch
        # vector (the gradient buffers accumulate across backward passes: multi-image heads, gradient accumulation)
        dbeta_now = buf("d_vt_beta", (H,))
        ops.pycall(dbeta_now.zero_)
        ops.layernorm_bwd(ws["vt_sum"], ws["vt_mean"], ws["vt_rstd"], P.w("embeddings.text_embeddings.LayerNorm.weight"),
                          Ml, H, dy_f32=dx0, dymap=(T, S, 0), dx_f32=dvs,
                          dgamma=P.gr("embeddings.text_embeddings.LayerNorm.weight"), dbeta=dbeta_now)
        ops.axpy(P.gr("embeddings.text_embeddings.LayerNorm.bias"), dbeta_now, 1.0, H)
        ops.axpy(gmt[0], dbeta_now, 1.0, H)
        tt = ws["tt"]
        gt = [(P.gr("embeddings.text_embeddings.token_type_embeddings.weight"), tt if tt is not None else 0)]
        if spec.lm is None:
            if ws.get("txt_embeds") is not None:
                ws["d_inputs_embeds"] = dvs[:Ml].view(B, T, H)     # inputs_embeds stood in for the word embeddings
            else:
                gt.append((P.gr("embeddings.text_embeddings.word_embeddings.weight"), ws["ids"]))
        if ws["use_pos"]:
            gt.append((P.gr("embeddings.text_embeddings.position_embeddings.weight"), "mod"))
        ops.scatter_add(dvs, gt, Ml, H, period=T)
        return dvs

    # ---- language model ---------------------------------------------------------------------------
    def _backward_lm_stack(self, ws, dvs, after_layer, note):
        """The post-LN LM layers, top down, from ``dvs`` (f32 gradient of the stack's output), then its embeddings."""
        B, T, H, FF, heads, Ml, Mlp = (ws[k] for k in ("B", "T", "H", "FF", "heads", "Ml", "Mlp"))
        nl, bf, staged = len(self.ll), self.hdt, bool(ws.get("lm_stage"))
        buf = lambda name, shape, dtype=torch.float32: self._buf(ws, name, shape, dtype)  # noqa: E731
        # gradient at a layer's output: bf16 part (the QKV data gradient of the layer above, left in dN) + f32 part (its dx_f32):
        # consumed by the layer's LN2 backward before either is overwritten
        dN, grp = buf("lm_dN", (Mlp, H), bf), None
        d = dict(dy_bf16=None, dy_f32=dvs, dmid_f32=buf("lm_dh", (Mlp, H)), dx_f32=buf("lm_dh1", (Mlp, H)), dN=dN, dx_bf16=dN,
                 dctx=buf("lm_dctx", (Mlp, H), bf))
        if self.LM_WGRAD_BATCHED and "lm_act_all" in ws and self.params.gr(self.ll[0].fw) is not None:
            # dY operands of every layer stay alive until their group's batched weight-gradient launches
            dY = (self._stack(ws, "lm_dhb", nl, (Mlp, H), bf), self._stack(ws, "lm_dU", nl, (Mlp, FF), bf),
                  self._stack(ws, "lm_dh1b", nl, (Mlp, H), bf), self._stack(ws, "lm_dqkv", nl, (Mlp, 3 * H), bf))
            grp = self._wgrad_groups(ws, "lm", self.ll, after_layer, dY,
                                     ("lm_act_all", "lm_y1b_all", "lm_ctx_all", "lm_yb_all"), Mlp, Ml)
        else:
            d.update(dmid_bf16=buf("lm_dhb", (Mlp, H), bf), dh1_bf16=buf("lm_dh1b", (Mlp, H), bf),
                     dU=buf("lm_dU", (Mlp, FF), bf), dqkv=buf("lm_dqkv", (Mlp, 3 * H), bf))
        # (the LM has attention dropout: it needs all three thirds of the QKV bias gradient - in-kernel partial sums of three
        #  tiles per wave cost the S <= 64 kernel 11 us per launch against the 10 us per layer of the batched pass over dqkv:
        #  LM_BIAS_PARTIALS stays off; the form is exercised by tests/test_gpu_ops.py)
        lparts = None
        if self.LM_BIAS_PARTIALS and grp and not staged:
            npart = ops.attention_bwd_partials(B, T, H, heads, 3)
            if npart:
                lparts = (self._stack(ws, "lm_qbpart", nl, (npart, 3 * H), torch.float32), npart)
        embed_done = []

        def embed_ahead():
            # data-parallel step: the embedding tables' gradient (a third of the bytes on the wire) first, so that its
            # all-reduce runs under the last group's weight-gradient launches (exchange.BucketReducer)
            self._lm_embed_backward(ws, d["dy_bf16"], d["dy_f32"])
            embed_done.append(True)
            note("lm_embed")
        ops.pycall(lambda: self._prof_begin("lm_bwd"))
        for i in reversed(range(nl)):
            if grp:
                d["dmid_bf16"], d["dU"], d["dh1_bf16"], d["dqkv"] = (t[i] for t in dY)
            if staged:
                self._layer_bwd_staged(ws, "lm", self.ll, i, d, bool(grp))
            else:
                self._lm_layer_bwd(ws, i, d, bool(grp), lparts)
            d["dy_bf16"], d["dy_f32"] = d["dN"], d["dx_f32"]
            # (the stage calls keep dqkv row-major: lm_qkv_hm is 0 there)
            self._layer_done("lm", grp, i, note, after_layer, hm=ws.get("lm_qkv_hm", 0), parts=lparts,
                             ahead=embed_ahead if (i == 0 and after_layer is not None) else None)
        ops.pycall(lambda: self._prof_end("lm_bwd"))
        if not embed_done:
            self._lm_embed_backward(ws, d["dy_bf16"], d["dy_f32"])
        self._join_wgrads()
        if not embed_done:
            note("lm_embed")

    def _lm_embed_backward(self, ws, dyb, dyf):
        # embeddings: y0 = dropout(LN(esum))
        P = self.params
        B, T, H, Ml, Mlp = (ws[k] for k in ("B", "T", "H", "Ml", "Mlp"))
        desum = self._buf(ws, "lm_desum", (Mlp, H), torch.float32)
        ops.layernorm_bwd(ws["lm_esum"], ws["lm_emean"], ws["lm_erstd"], P.w("bert.embeddings.LayerNorm.weight"), Ml, H,
                          dy_bf16=dyb, dy_f32=dyf, dx_f32=desum, dgamma=P.gr("bert.embeddings.LayerNorm.weight"),
                          dbeta=P.gr("bert.embeddings.LayerNorm.bias"),
                          drop=self._drop(self.spec.lm.hidden_dropout_prob, 1, True), drop_on_dy=True)
        if ws.get("txt_embeds") is not None:
            ws["d_inputs_embeds"] = desum[:Ml].view(B, T, H)
        ops.scatter_add(desum, [None if ws.get("txt_embeds") is not None else
                                (P.gr("bert.embeddings.word_embeddings.weight"), ws["ids"]),
                                (P.gr("bert.embeddings.position_embeddings.weight"), ws["lm_pos"]),
                                (P.gr("bert.embeddings.token_type_embeddings.weight"), ws["lm_tt"])], Ml, H,
                        rowmask=ws["amf"])   # padded positions are masked keys everywhere: their gradient is exactly 0

    def _lm_layer_bwd(self, ws, i, d, deferred, lparts):
        """The layer backward kernel by kernel (``deferred``: without its weight gradients)."""
        P, ln, lm, lhm = self.params, self.ll[i], self.spec.lm, ws.get("lm_qkv_hm", 0)
        B, T, H, FF, heads, Ml, Mlp = (ws[k] for k in ("B", "T", "H", "FF", "heads", "Ml", "Mlp"))
        pdh, pda = lm.hidden_dropout_prob, lm.attention_probs_dropout_prob
        g = lambda k: ws[f"lm_{k}{i}"]  # noqa: E731
        wgrad = (lambda *a: None) if deferred else self._wgrad      # (deferred: with the group's launches, _layer_done)
        dh, dh1, dhb, dh1b, dU, dqkv, dN, dctx = (d[k] for k in ("dmid_f32", "dx_f32", "dmid_bf16", "dh1_bf16", "dU", "dqkv", "dN", "dctx"))
        # y2 = LN2(h2)
        ops.layernorm_bwd(g("h2"), g("m2"), g("r2"), P.w(ln.ln2w), Ml, H, dy_bf16=d["dy_bf16"], dy_f32=d["dy_f32"], dx_f32=dh,
                          dx_bf16=dhb, dgamma=P.gr(ln.ln2w), dbeta=P.gr(ln.ln2b),
                          drop=self._drop(pdh, 16 * i + 4, True), dbias=P.gr(ln.fb))
        self._dgrad(dhb, ln.fw, dU, Mlp, FF, H, ops.EPI_BF16_DGELU, Ml, aux=g("u"), colsum=P.gr(ln.ib))
        wgrad(dhb, g("act"), ln.fw, None, Mlp, H, FF, Ml)
        self._dgrad(dU, ln.iw, dN, Mlp, H, FF, ops.EPI_BF16, Ml)
        wgrad(dU, g("y1b"), ln.iw, None, Mlp, FF, H, Ml)
        # y1 = LN1(h1) ; d y1 = dgrad(bf16) + dh (residual)
        ops.layernorm_bwd(g("h1"), g("m1"), g("r1"), P.w(ln.ln1w), Ml, H, dy_bf16=dN, dy_f32=dh, dx_f32=dh1,
                          dx_bf16=dh1b, dgamma=P.gr(ln.ln1w), dbeta=P.gr(ln.ln1b),
                          drop=self._drop(pdh, 16 * i + 3, True), dbias=P.gr(ln.ob))
        self._dgrad(dh1b, ln.ow, dctx, Mlp, H, H, ops.EPI_BF16, Ml)
        wgrad(dh1b, g("ctx"), ln.ow, None, Mlp, H, H, Ml)
        ops.attention_bwd(g("qkv"), ws["amf"], g("ctx"), g("lse"), dctx, dqkv, B, T, H, heads,
                          drop=self._drop(pda, 16 * i + 2, True), qkv_hm=lhm,
                          **(dict(bias_partials=lparts[0][i], bias_thirds=3) if lparts else {}))
        self._dgrad(dqkv, ln.qw, dN, Mlp, H, 3 * H, ops.EPI_BF16, Ml, **(dict(a_hm=lhm) if lhm else {}))
        wgrad(dqkv, ws["lm_yb"][i], ln.qw, ln.qb, Mlp, 3 * H, H, Ml)
