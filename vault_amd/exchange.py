"""The data-parallel gradient exchange of the train step: the bucket ranges of the flat gradient buffer, the row-sparse
exchange of the word-embedding table, the bf16 wire format, and the reducer that launches each range from the backward pass as
soon as it is final.  Device-agnostic on purpose: HIP tensors + RCCL in production, host tensors + gloo in the tests.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .engine import VaultEngine


class GradBuckets:
    """Contiguous ranges of the flat gradient buffer in the order backward finalises them.

    The flat layout is [LM embeddings, LM layers 0.., ViLT embeddings, ViLT layers 0.., head], and
    backward runs head -> ViLT layers (top down) -> ViLT embeddings -> LM layers (top down) -> LM
    embeddings, i.e. strictly descending addresses: after stage ``tag`` every gradient at or above
    ``stage_lo[tag]`` is final.
    """

    def __init__(self, engine: VaultEngine, bucket_mb: float = 64.0):
        P = engine.params
        self.engine = engine
        self.bucket_elems = int(bucket_mb * 1024 * 1024 / 4)
        lo: Dict[str, int] = {}

        def first(prefix_or_names) -> int:
            offs = [P.offsets[n][0] for n in P.trainable
                    if (n.startswith(prefix_or_names) if isinstance(prefix_or_names, str) else n in prefix_or_names)]
            return min(offs) if offs else P.n_train

        spec = engine.spec
        lo["head"] = first(("layernorm.weight", "layernorm.bias", "pooler.dense.weight", "pooler.dense.bias",
                            "classifier.1.weight", "classifier.1.bias"))
        for i in range(spec.vilt.num_hidden_layers):
            lo[f"vilt{i}"] = first(f"encoder.layer.{i}.")
        lo["vilt_embed"] = first("embeddings.")
        if spec.lm is not None and not engine.freeze_lm:
            for i in range(spec.lm.num_hidden_layers):
                lo[f"lm{i}"] = first(f"bert.encoder.layer.{i}.")
            lo["lm_embed"] = 0
        self.stage_lo = lo
        self.last_tag = "lm_embed" if (spec.lm is not None and not engine.freeze_lm) else "vilt_embed"
        self.n = P.n_train


class SparseTable:
    """An embedding table inside the flat gradient buffer whose gradient is exchanged row-sparse: rows x H floats at
    element offset ``lo``; only the rows named by some rank's token ids of the step are non-zero."""

    def __init__(self, lo: int, rows: int, H: int):
        self.lo, self.rows, self.H = int(lo), int(rows), int(H)
        self.hi = self.lo + self.rows * self.H


def _on_bf16_library(fn):
    """The wire format of the exchange is bf16 whatever the engine's operand format (f32 range: no gradient scale to
    respect): these kernels always run on libvault_hip.so."""
    def run(*a):
        with ops.operand_format("bf16"):
            return fn(*a)
    return staticmethod(run)


class ExchangeKernels:
    """Pack / unpack kernels of the exchange on DEVICE tensors (csrc/exchange.hip).  The reducer takes them as an object so
    that its bucket logic can be driven with host tensors over gloo in the CPU tests (which bring their own stand-ins)."""
    narrow = _on_bf16_library(ops.cast_bf16)              # (src_f32, dst_bf16, n)
    widen = _on_bf16_library(ops.widen_bf16)              # (src_bf16, dst_f32, n)
    sum_chunks = _on_bf16_library(ops.sum_chunks_bf16)    # (src_bf16, n_src, chunk, out_bf16)
    rows_union = staticmethod(ops.rows_union)         # (keys, n_keys, V, flags, uniq, count)
    rows_gather = staticmethod(ops.rows_gather)       # (table, idx, n_rows, H, out)
    rows_scatter = staticmethod(ops.rows_scatter)     # (src, idx, n_rows, H, table)


class BucketReducer:
    """Sums each contiguous gradient range over the ranks as soon as it is final.

    ``on_stage(tag)`` is the engine's ``after_layer`` callback, ``finish()`` waits for everything.  Two things keep the
    bytes on the wire down:
      * ``sparse``: the word-embedding table (a fifth of the gradient elements, of which a step touches at most
        world x B x T rows) is exchanged as the union of the touched rows: all-gather of the token ids at the START of the
        step (``begin_step``), sorted union on every rank, gather -> all-reduce of the compact [U, H] rows -> scatter.
        Exact: untouched rows are zero on every rank.
      * ``wire="bf16"``: reduce-scatter + all-gather with bf16 on the wire and f32 accumulation - all-to-all of the
        bf16 chunks (every peer link carries its own chunk: point-to-point xGMI, no ring), f32 sum in rank order,
        rounded to bf16 once, all-gather, widened back into the f32 gradient.  Half the bytes of the f32 all-reduce;
        every rank ends with the same bits.  ``wire="fp32"`` is a plain sum all-reduce.
    Device-agnostic on purpose (CPU tensors + gloo in the tests, HIP tensors + RCCL in production).
    """

    WIRE_PIECE = 1 << 25      # bf16 wire: elements per reduce-scatter / all-gather round (64 MiB of bf16 scratch x 2)
    # One rank (VAULT_FORCE_DP=1 on a single GPU): run the transport's collectives anyway - the tests that exercise the RCCL calls
    # with one process set this; by default the identity sum is skipped, so that the one-rank line of bench.py shows what the
    # data-parallel CODE PATH costs (buckets, events, stage notes, split optimizer pass), not RCCL's degenerate copy kernels
    SINGLE_RANK_COLLECTIVES = False

    def __init__(self, flat_grad: torch.Tensor, stage_lo: Dict[str, int], last_tag: str, bucket_elems: int,
                 dist, group=None, comm_stream=None, compute_device=None, wire: str = "fp32",
                 sparse: Optional[SparseTable] = None, kernels=ExchangeKernels):
        if wire not in ("fp32", "bf16"):
            raise ValueError("wire must be 'fp32' or 'bf16'")
        self.g, self.stage_lo, self.last_tag, self.bucket_elems = flat_grad, stage_lo, last_tag, bucket_elems
        self.dist, self.group, self.comm_stream, self.device = dist, group, comm_stream, compute_device
        self.wire, self.sparse, self.k = wire, sparse, kernels
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self.native_a2a = dist.get_backend(group) != "gloo"      # gloo has no all-to-all: emulated with all-gather (tests)
        self.n = flat_grad.numel()
        self.hi = self.n          # everything at or above is launched (top-down frontier)
        self.bottom = 0           # everything below is launched (the lowest stage may finish ahead of the one above it)
        above = [v for t, v in stage_lo.items() if t != last_tag and v > stage_lo.get(last_tag, 0)]
        self.above_last = min(above) if above else self.n      # where the stage above the lowest one starts
        self.min_seen = self.n    # lowest stage_lo among the stages noted in this step
        self.done: List = []      # per launch: event on the communication stream (None on the host)
        self.launched: List[Tuple[int, int]] = []
        self.wire_bytes = 0       # bytes this rank put on the wire in the current step (diagnostics)
        self._scratch: Dict[str, torch.Tensor] = {}
        self._union_ready = None
        self._n_keys = 0
        self._key_capacity = None   # per-rank key count agreed on in the first step (begin_step)
        self._keys_given = None
        self.union_waits = 0        # steps in which the host had to WAIT for the union (diagnostics: expected 0)
        # VAULT_DP_CHECK_SPARSE=N (debug): in the first N steps the row-sparse result is compared with a dense f32 all-reduce of
        # the whole table (a host sync per step): a gradient row that some rank holds outside the union of the step's token
        # ids - a second source of gradient on the table - would otherwise stay un-reduced without an error
        self._check_sparse_left = int(os.environ.get("VAULT_DP_CHECK_SPARSE", "0") or 0)
        self.sparse_checks = 0

    # ---- plumbing -------------------------------------------------------------------------------------------
    def _buf(self, name: str, n: int, dtype) -> torch.Tensor:
        t = self._scratch.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = torch.zeros(n, dtype=dtype, device=self.g.device)
            self._scratch[name] = t
        return t[:n]

    def _host_buf(self, name: str, n: int, dtype) -> torch.Tensor:
        """The host image of a device word the exchange reads back (pinned when the copy runs on a stream), made once."""
        t = self._scratch.get(name)
        if t is None:
            t = torch.zeros(n, dtype=dtype)
            if self.comm_stream is not None:
                t = t.pin_memory()
            self._scratch[name] = t
        return t

    def _on_comm_stream(self, fn):
        """Run ``fn`` with the communication stream current, ordered behind everything enqueued on the compute stream so
        far; returns the event that marks its end (None on the host).  Collectives inside ``fn`` are waited for on the
        stream (``Work.wait()`` blocks the stream, not the host, with RCCL; it blocks the host with gloo)."""
        if self.comm_stream is None:
            fn()
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            fn()
            end = torch.cuda.Event()
            end.record(self.comm_stream)
        return end

    def _all_to_all(self, recv: torch.Tensor, send: torch.Tensor, chunk: int):
        if self.native_a2a:
            self.dist.all_to_all_single(recv, send, group=self.group, async_op=True).wait()
            return
        parts = [torch.empty_like(send) for _ in range(self.world)]
        self.dist.all_gather(parts, send, group=self.group)
        for k in range(self.world):
            recv[k * chunk:(k + 1) * chunk].copy_(parts[k][self.rank * chunk:(self.rank + 1) * chunk])

    def _all_gather(self, full: torch.Tensor, part: torch.Tensor):
        if self.native_a2a:
            self.dist.all_gather_into_tensor(full, part, group=self.group, async_op=True).wait()
            return
        parts = [torch.empty_like(part) for _ in range(self.world)]
        self.dist.all_gather(parts, part, group=self.group)
        n = part.numel()
        for k in range(self.world):
            full[k * n:(k + 1) * n].copy_(parts[k])

    def _sum_over_ranks(self, view: torch.Tensor):
        """view (contiguous f32, 4-element aligned) <- its sum over the ranks, in the configured wire format."""
        n = view.numel()
        if n == 0 or (self.world == 1 and not self.SINGLE_RANK_COLLECTIVES):
            return      # (one rank - VAULT_FORCE_DP on a single GPU: the sum is the identity, nothing goes on a wire)
        if self.wire == "fp32":
            self.dist.all_reduce(view, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True).wait()
            self.wire_bytes += 2 * 4 * n * (self.world - 1) // self.world
            return
        W = self.world
        for p0 in range(0, n, self.WIRE_PIECE):
            m = min(self.WIRE_PIECE, n - p0)
            chunk = -(-m // (8 * W)) * 8                      # elements per rank, 16-byte multiples
            send = self._buf("send", chunk * W, torch.bfloat16)
            recv = self._buf("recv", chunk * W, torch.bfloat16)
            red = self._buf("red", chunk, torch.bfloat16)
            if chunk * W > m:
                send[m - (m % 4):].zero_()                    # the padding behind the range (and a ragged tail) adds zeros
            m4 = m - (m % 4)
            if m4:
                self.k.narrow(view[p0:p0 + m4], send, m4)
            if m % 4:                                         # (never for the engine's 64-aligned ranges)
                send[m4:m].copy_(view[p0 + m4:p0 + m])
            self._all_to_all(recv, send, chunk)               # recv[k] = rank k's bf16 image of MY chunk
            self.k.sum_chunks(recv, W, chunk, red)            # f32 accumulation in rank order, one rounding
            self._all_gather(send, red)                       # (the send buffer is free again: it takes the result)
            if m4:
                self.k.widen(send, view[p0:p0 + m4], m4)
            if m % 4:
                view[p0 + m4:p0 + m].copy_(send[m4:m])
            self.wire_bytes += 2 * 2 * chunk * (W - 1)

    # ---- row-sparse table -----------------------------------------------------------------------------------
    def begin_step(self, keys: Optional[torch.Tensor]):
        """Start of a step: ``keys`` = this rank's token ids (int64, any shape; None: this step touches no row of the table,
        on EVERY rank alike).  Their all-gather and the union run on the communication stream at once; the host reads the
        union's size only when the table's gradient is final (``_exchange_table``).

        The all-gather needs the SAME key count on every rank and every rank to agree on ids-or-none: the first step
        exchanges (count, has-keys) between the ranks and raises on a mismatch (one host synchronisation, once).  The count
        of that step - the first step's B x T - is the CAPACITY afterwards: a later, smaller batch is padded with -1 (ignored
        by the union).  Every later step carries a two-word header (token count, ids given) per rank in the same all-gather:
        a rank with more ids than the capacity, or one that switched between ids and ``inputs_embeds``, makes EVERY rank raise
        when the table is exchanged (``_check_headers``) - a decision taken on one rank only would leave the others waiting
        in their next collective until it times out.

        The bucket frontier starts over here as well: a step that raised from inside the exchange (the header / id checks run
        under ``_launch``) never reached ``finish()``, and a frontier left at its position would make ``on_stage`` skip every
        upper range of the next step without an error (the replicas would diverge silently)."""
        self.reset(wait=True)
        self.wire_bytes = 0
        self._union_ready, self._n_keys = None, 0
        if self.sparse is None:
            return
        n_local = 0 if keys is None else int(keys.numel())
        if self._key_capacity is None:
            hdr = torch.tensor([n_local, 0 if keys is None else 1], dtype=torch.int64, device=self.g.device)
            allh = [torch.zeros_like(hdr) for _ in range(self.world)]
            self.dist.all_gather(allh, hdr, group=self.group)
            rows = [tuple(int(v) for v in h.cpu()) for h in allh]
            if any(r != rows[0] for r in rows):
                raise RuntimeError(f"row-sparse embedding exchange: the ranks disagree on (token count, ids given): {rows} - "
                                   "every rank must step the same per-rank batch shape (or pass sparse_embedding=False)")
            self._key_capacity, self._keys_given = n_local, keys is not None
        n = self._key_capacity
        W, V = self.world, self.sparse.rows
        # this rank's slice of the all-gather: [token count, ids given, keys (capacity n; short batches padded with -1, a
        # batch beyond the capacity truncated - its header makes every rank raise)]
        mine = self._buf("keys_local", n + 2, torch.int64)
        mine[0], mine[1] = n_local, (0 if keys is None else 1)
        if n:
            m = min(n_local, n)
            if m:
                mine[2:2 + m].copy_(keys.reshape(-1)[:m])
            if m < n:
                mine[2 + m:].fill_(-1)
        allk = self._buf("keys", (n + 2) * W, torch.int64)
        hdrs = self._buf("headers", 2 * W, torch.int64)
        host_h = self._host_buf("headers_host", 2 * W, torch.int64)
        if n:
            flags = self._buf("flags", V, torch.int32)
            uniq = self._buf("uniq", min(V, n * W), torch.int64)
            cnt = self._buf("count", 2, torch.int32)               # [distinct rows, keys outside the table]
            host = self._host_buf("count_host", 2, torch.int32)

        def go():
            self._all_gather(allk, mine)
            slots = allk.view(W, n + 2)[:, :2]
            hdrs.view(W, 2).copy_(slots)
            host_h.copy_(hdrs, non_blocking=True)
            if n:
                slots.fill_(-1)                                   # (the header words are no keys: padding for the union)
                self.k.rows_union(allk, (n + 2) * W, V, flags, uniq, cnt)
                host.copy_(cnt, non_blocking=True)

        self._union_ready = self._on_comm_stream(go)
        self._n_keys = n * W if (keys is not None and self._keys_given) else 0
        self.wire_bytes += 8 * (n + 2) * (W - 1)

    def _check_headers(self):
        """Every rank reads the same (token count, ids given) words of all ranks and takes the same decision."""
        if self._union_ready is not None and not self._union_ready.query():
            # (enqueued at the start of the step: normally long done - the host only blocks, and counts it, when the
            #  first collective of the step was slow)
            self.union_waits += 1
            self._union_ready.synchronize()
        h = self._scratch["headers_host"].view(self.world, 2).tolist()
        over = [(r, int(c)) for r, (c, _) in enumerate(h) if c > self._key_capacity]
        if over:
            raise RuntimeError(f"row-sparse embedding exchange: rank(s) {over} stepped more token ids than the "
                               f"{self._key_capacity} per rank agreed on in the first step (the capacity is the first step's "
                               "B x T: start with the largest batch, or pass sparse_embedding=False)")
        switched = [r for r, (_, g_) in enumerate(h) if bool(g_) != self._keys_given]
        if switched:
            raise RuntimeError(f"row-sparse embedding exchange: rank(s) {switched} switched between token ids and inputs_embeds "
                               "(construct the TrainStep with sparse_embedding=False)")

    def _exchange_table(self):
        sp = self.sparse
        self._check_headers()
        U = 0
        if self._n_keys:
            U, bad = int(self._scratch["count_host"][0]), int(self._scratch["count_host"][1])
            if bad:
                raise RuntimeError(f"row-sparse embedding exchange: {bad} token ids lie outside the table's {sp.rows} rows - their "
                                   "gradient rows would be left un-reduced (replicas would diverge)")
        table = self.g[sp.lo:sp.hi]
        dense = None
        if self._check_sparse_left > 0:
            # (debug; VAULT_DP_CHECK_SPARSE must be set identically on every rank - the comparison is a collective.  It runs in
            #  the steps without any touched row too - inputs_embeds steps, an empty union: exactly the steps in which a second
            #  source of gradient on the table would go un-reduced altogether)
            dense = table.clone()
            self.dist.all_reduce(dense, op=self.dist.ReduceOp.SUM, group=self.group)
        if U > 0:
            uniq = self._scratch["uniq"]
            compact = self._buf("rows", min(sp.rows, self._n_keys) * sp.H, torch.float32)[:U * sp.H]
            self.k.rows_gather(table, uniq, U, sp.H, compact)
            self._sum_over_ranks(compact)
            self.k.rows_scatter(compact, uniq, U, sp.H, table)
        if dense is not None:
            self._check_sparse_left -= 1
            self.sparse_checks += 1
            both = torch.stack([(table - dense).abs().max(), dense.abs().max()])
            self.dist.all_reduce(both, op=self.dist.ReduceOp.MAX, group=self.group)   # (every rank takes the same decision)
            err, ref = float(both[0]), float(both[1])
            tol = (1e-2 if self.wire == "bf16" else 1e-5) * ref + 1e-30
            if not err <= tol:
                raise RuntimeError(f"row-sparse embedding exchange differs from the dense all-reduce of the table: max |diff| "
                                   f"{err:.3e} against max |gradient| {ref:.3e} (VAULT_DP_CHECK_SPARSE) - some rank holds "
                                   "gradient rows outside the union of this step's token ids")

    # ---- bucket logic ---------------------------------------------------------------------------------------
    def reset(self, wait: bool = False):
        """Forget the ranges launched so far: top-down frontier at the end of the buffer, nothing launched, no events.
        ``wait``: the compute stream first waits for exchanges still in flight (a step that raised left them behind: whatever
        the caller does to the gradient buffer next must not race with them)."""
        if wait:
            self._wait(self.done)
        self.hi, self.bottom, self.min_seen = self.n, 0, self.n
        self.done.clear()
        self.launched.clear()

    def on_stage(self, tag: str):
        lo = self.stage_lo.get(tag)
        if lo is None:
            return
        early = tag == self.last_tag and self.min_seen > self.above_last and self.bottom == 0 and self.above_last < self.hi
        self.min_seen = min(self.min_seen, lo)
        if early:
            # the lowest stage (the embedding tables) became final BEFORE the stage above it was noted - the engine runs the
            # embedding backward ahead of the deferred weight gradients of the last group of layers in data-parallel
            # steps, so that this exchange runs under them: reduce [0, above_last) now
            self._launch(0, self.above_last)
            self.bottom = self.above_last
            return
        final = lo <= self.bottom
        if final:
            lo = self.bottom
        if self.hi <= lo or (not final and (self.hi - lo) < self.bucket_elems):
            return
        self._launch(lo, self.hi)
        self.hi = lo

    def _launch(self, lo: int, hi: int):
        sp = self.sparse

        def go():
            if sp is not None and lo < sp.hi and hi > sp.lo:
                self._sum_over_ranks(self.g[lo:max(lo, sp.lo)])
                self._exchange_table()
                self._sum_over_ranks(self.g[min(hi, sp.hi):hi])
            else:
                self._sum_over_ranks(self.g[lo:hi])

        self.done.append(self._on_comm_stream(go))
        self.launched.append((lo, hi))

    def _wait(self, events):
        for ev in events:
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)

    def finish_upper(self) -> int:
        """Make the compute stream wait for every launched range except the LAST one (the lowest addresses: launched when
        backward ends, nothing is left to hide it behind) and return its upper bound x: gradients in [x, n) are final
        and reduced, so the optimizer can already run on them while [0, x) is still on the wire."""
        if len(self.done) < 2:
            return self.n if not self.done else self.launched[-1][1]
        self._wait(self.done[:-1])
        del self.done[:-1]
        return self.launched[-1][1]

    def finish(self):
        self._wait(self.done)
        missing = (self.bottom, self.hi) if self.hi != self.bottom else None
        self.reset()      # (first: the reducer stays usable after the error)
        if missing is not None:
            raise RuntimeError("gradient range [%d, %d) was never reduced" % missing)



def make_reducer(engine: VaultEngine, dist, process_group, bucket_mb: float, wire: str, sparse_embedding: Optional[bool]):
    """The reducer of a data-parallel train step over ``engine``'s flat gradient buffer, its collectives on a side stream, and
    the name of the table it exchanges row-sparse (None: every range goes dense).  ``wire``: the format of the dense ranges
    ("fp32": sum all-reduce; "bf16": reduce-scatter + all-gather with bf16 on the wire and f32 accumulation);
    ``sparse_embedding`` (None: on): the row-sparse exchange of the word-embedding table."""
    b = GradBuckets(engine, bucket_mb)
    sparse = sparse_name = None
    if sparse_embedding is None or sparse_embedding:
        P = engine.params
        name = ("bert.embeddings.word_embeddings.weight" if engine.spec.lm is not None
                else "embeddings.text_embeddings.word_embeddings.weight")
        # (a tied MLM decoder puts a DENSE gradient on ViLT's own table)
        if P.has_grad(name) and not (engine.spec.lm is None and engine.spec.head == "mlm"):
            o, shp = P.offsets[name]
            sparse = SparseTable(o, shp[0], shp[1])
            sparse_name = name
    reducer = BucketReducer(engine.params.g[:engine.params.n_train], b.stage_lo, b.last_tag, b.bucket_elems, dist, process_group,
                            torch.cuda.Stream(device=engine.device), engine.device, wire=wire, sparse=sparse)
    return reducer, sparse_name
