"""Data-parallel fine-tune step around the HIP engine.

Restates the per-step body of the reference's loop, ref: vault/tmsc_utils/trainer.py:353-369
(forward -> CrossEntropy -> zero_grad/backward -> AdamW step -> scheduler step) with
  * the optimizer of trainer.py:244-254 (transformers-4.48 ``AdamW``, ``correct_bias=False`` by
    default, eps 1e-8, decoupled weight decay on all parameters) as ONE fused HIP kernel over the
    flat parameter buffer,
  * the schedule of trainer.py:256-280 (linear warm-up over ``warmup_ratio`` of the steps, then
    linear decay to 0),
  * and - absent from the reference, which is single-device - data parallelism: one process per
    GPU, each rank runs the step on its shard of the batch, gradients are summed with RCCL
    all-reduce (``torch.distributed`` backend "nccl" on ROCm) over xGMI and averaged inside the
    optimizer kernel.  The flat gradient buffer is reduced in contiguous buckets that are launched
    from the backward pass as soon as the stages that write them have been enqueued, on a side
    stream, so the exchange overlaps the remaining backward kernels.

No loss.item() per step: the loss stays on the device (the reference syncs every step at
trainer.py:369); read ``TrainStep.loss`` when needed.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from .engine import VaultEngine
from .exchange import BucketReducer, ExchangeKernels, GradBuckets, SparseTable, make_reducer
from .optim import (LR_SCHEDULES, MAX_PARAM_GROUPS, NO_DECAY_PATTERNS, OPTIMIZER_STATE_KEYS, OPTIMIZERS, adam_bias_corrections,
                    build_param_groups, check_optimizer_state, constant_with_warmup_schedule, cosine_schedule, ema_decay_at,
                    hf_no_decay_groups, linear_schedule, no_decay_parameter_names, pass_call, scheduled)

# (the schedules, the parameter groups and the state check live in optim.py, the gradient exchange in exchange.py: their names
#  stay importable from here)
__all__ = ["TrainStep", "BucketReducer", "SparseTable", "ExchangeKernels", "GradBuckets", "linear_schedule", "cosine_schedule",
           "constant_with_warmup_schedule", "LR_SCHEDULES", "OPTIMIZERS", "adam_bias_corrections", "build_param_groups",
           "no_decay_parameter_names", "hf_no_decay_groups", "NO_DECAY_PATTERNS", "MAX_PARAM_GROUPS", "ema_decay_at",
           "check_optimizer_state", "OPTIMIZER_STATE_KEYS", "evaluate", "evaluation_metrics"]


class TrainStep:
    def __init__(self, engine: VaultEngine, learning_rate: float = 2e-5, adam_beta1: float = 0.9,
                 adam_beta2: float = 0.999, adam_epsilon: float = 1e-8, weight_decay: float = 0.0,
                 correct_bias: bool = False, warmup_ratio: float = 0.1, total_steps: int = 1000,
                 process_group=None, bucket_mb: float = 64.0, constant_lr: bool = False, use_tape: bool = True,
                 assume_full_pixel_mask: bool = False, wire: Optional[str] = None, sparse_embedding: Optional[bool] = None,
                 precise_forward: bool = False, max_grad_norm: Optional[float] = None,
                 param_groups: Optional[Sequence[dict]] = None, track_grad_norm: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False, optimizer: str = "hf",
                 lr_schedule: str = "linear"):
        """``max_grad_norm``: clip the global L2 norm of the gradient before AdamW (torch.nn.utils.clip_grad_norm_, HF
        ``TrainingArguments.max_grad_norm``); ``param_groups``: ``[{"params": [names], "lr": .., "weight_decay": ..}, ..]``
        (engine parameter names = state_dict keys; unnamed parameters form the default group at ``learning_rate`` /
        ``weight_decay``; every group follows the schedule from its own base lr); ``track_grad_norm``: keep the norm without
        clipping.  With either norm option ``grad_norm`` holds the step's pre-clip norm on the device.
        ``ema_decay`` (0 <= d < 1; None: no average): keep an exponential moving average of the trainable weights in ``ema``,
        moved inside the optimizer's own pass (``ema <- ema + (1 - d_t)(p - ema)``, d_t = :func:`ema_decay_at` with
        ``ema_warmup``); :meth:`ema_weights` evaluates or saves the averaged model.
        ``optimizer``: ``"hf"`` (the reference's transformers-4.48 AdamW, ``correct_bias`` its flag) or ``"torch"``, the
        arithmetic of ``torch.optim.AdamW`` (a current HF ``Trainer``'s ``adamw_torch``): always bias-corrected, eps added to
        the corrected root, the weights decayed before the update.  ``lr_schedule``: ``"linear"``, ``"cosine"`` or
        ``"constant_with_warmup"`` (HF ``lr_scheduler_type``; ``constant_lr=True`` overrides it)."""
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {optimizer!r}")
        if optimizer == "torch" and correct_bias:
            raise ValueError("optimizer='torch' always corrects the bias: correct_bias belongs to optimizer='hf'")
        if lr_schedule not in LR_SCHEDULES:
            raise ValueError(f"lr_schedule must be one of {tuple(LR_SCHEDULES)}, not {lr_schedule!r}")
        self.optimizer, self.lr_schedule = optimizer, lr_schedule
        self.engine = engine
        self.lr, self.b1, self.b2, self.eps, self.wd = learning_rate, adam_beta1, adam_beta2, adam_epsilon, weight_decay
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0):
            raise ValueError("max_grad_norm must be positive (None: no clipping)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.track_grad_norm = bool(track_grad_norm)
        # the step's gradient norm (0-dim f32 on the device, written by the kernel: no host sync), None without the options
        self.grad_norm: Optional[torch.Tensor] = None
        self._group_map = self._group_table = self._norm_partials = None
        if ema_decay is not None and not (0.0 <= float(ema_decay) < 1.0):
            raise ValueError("ema_decay must lie in [0, 1) (None: no weight average)")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        # the average of P.p[:n_train] (f32 on the device; frozen parameters lie behind n_train and need none), None without
        # the option
        self.ema: Optional[torch.Tensor] = None
        self._ema_swapped = False      # inside ema_weights(): P.p holds the average, self.ema the trained weights
        if param_groups is not None or self.max_grad_norm is not None or self.ema_decay is not None or optimizer == "torch":
            # the grouped AdamW (one group when only clipping or the average is asked for: it reads the clip factor from the
            # device, and its sibling with the average takes the same group map, as does the torch form)
            gmap, table = build_param_groups(engine.params, param_groups, learning_rate, weight_decay)
            self._group_map = torch.from_numpy(gmap).to(engine.device)
            self._group_table = torch.from_numpy(table).to(engine.device)
        if self.ema_decay is not None:
            self.ema = torch.empty(engine.params.n_train, dtype=torch.float32, device=engine.device)
            self.reset_ema()
        if self._needs_norm:
            self._norm_partials = torch.empty(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device=engine.device)
        self.correct_bias = correct_bias
        self.total_steps = int(total_steps)
        self.warmup_steps = int(warmup_ratio * self.total_steps)
        self.constant_lr = constant_lr
        self.step_idx = 0
        self.loss: Optional[torch.Tensor] = None
        self.use_tape = use_tape
        # split-bf16 ("bf16x3") forward GEMMs: logits / loss of the training step at fp32 class (inside the 1e-3 of the reference),
        # bf16 backward as in the fast mode; ~3x the forward GEMM time
        self.precise_forward = bool(precise_forward)
        self._tape = None
        self._tape_key = None
        self._tape_ws = None
        self._zero_mask = None      # see _build_zero_mask
        # True: the caller vouches that every pixel_mask is all ones on the square pre-training canvas (no device
        # sync per step); False: the mask is checked each step and padded batches take the general image path
        self.assume_full_pixel_mask = assume_full_pixel_mask
        self._loss_buf = None
        self.world = 1
        self.wire = None
        self.reducer: Optional[BucketReducer] = None
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            self.world = dist.get_world_size(process_group)
        engine.dp_world = self.world
        # VAULT_FORCE_DP=1 exercises the bucketed all-reduce path even with a single rank (debug/testing)
        if self.world > 1:
            # every rank draws its own dropout masks: the keep/drop hash takes (seed, stream, LOCAL element index), so
            # equal seeds would give sample j of every rank the same pattern
            engine.drop_seed = (engine.drop_seed + dist.get_rank(process_group) * 0x9E3779B1) & 0xFFFFFFFF
            # the gradient all-reduce (RCCL kernels on a side stream) shares the CUs with the backward GEMMs: hand the
            # GEMM tiles out dynamically so that a CU held by the collective does not stall a static tile walk.
            # (The tape records the argument structs: this must be set before the first step is recorded.)
            ops.GEMM_SCHED = 3
            # (the deferred, batched weight gradients already come in groups of 6 layers - engine.LM_WGRAD_GROUP - so the
            # upper group's gradient range is all-reduced under the backward of the layers below it)
        if self.world > 1 or (os.environ.get("VAULT_FORCE_DP") == "1" and dist.is_available() and dist.is_initialized()):
            self.wire = wire or "fp32"
            self.reducer, self._sparse_name = make_reducer(engine, dist, process_group, bucket_mb, self.wire, sparse_embedding)

    @property
    def _needs_norm(self) -> bool:
        return self.max_grad_norm is not None or self.track_grad_norm

    def current_lr(self) -> float:
        return scheduled(self.lr, self.lr_schedule, self.constant_lr, self.step_idx, self.warmup_steps, self.total_steps)

    def lr_factor(self) -> float:
        """The schedule's multiplier of every group's base lr at the current step (LambdaLR)."""
        return scheduled(1.0, self.lr_schedule, self.constant_lr, self.step_idx, self.warmup_steps, self.total_steps)

    def __call__(self, batch: Dict[str, torch.Tensor], labels: torch.Tensor) -> torch.Tensor:
        """One optimisation step.  The first call for a (B, T) shape runs eagerly and records the call
        tape (ops.Tape); later calls copy the batch into the persistent input buffers and replay it."""
        eng = self.engine
        self._refuse_inside_ema_weights("a training step")
        B, T = batch["input_ids"].shape
        if self.reducer:
            # (a step that raised inside the exchange never reached finish(): its frontier and its events are dropped here,
            #  before anything below touches the gradient buffer)
            self.reducer.reset(wait=True)
        if eng._g_dirty:
            # gradients of an API-level backward (loss.backward() through the module) are still in the flat buffer: the fused step
            # starts from zeros (it STORES its un-split weight-gradient tiles and lets AdamW clear the buffer afterwards)
            eng.zero_grad()
        with torch.cuda.device(eng.device), ops.operand_format(eng.half):
            # staging decides the image geometry (square all-valid canvas, or a padded batch of differently sized
            # images: host-side patch selection); every geometry has its own workspace, hence its own tape
            ws = eng.stage_inputs(batch, True, labels, validate=not self.assume_full_pixel_mask)
            # what the recorded launches bake in besides the buffers of the (B, T, geometry) workspace: whether token
            # types were given, the launch stream, the GEMM scheduling mode and the forward number format
            key = ws["key"] + (ws["tt"] is None, torch.cuda.current_stream().cuda_stream, ops.GEMM_SCHED,
                               bool(eng.fp8_forward), labels.dtype.is_floating_point, bool(ws.get("patches_in")), self.precise_forward,
                               eng.half, eng.grad_scale, bool(ws.get("patches_in") and ws.get("patch_adopted")))
            # from here to the enqueued AdamW (which clears it) the flat gradient buffer holds this step's partial gradients: an
            # exception in between (the reducer's checks raise and stay usable) must not leave them for the next step, which
            # STORES its un-split weight-gradient tiles but atomically ADDS bias / LayerNorm / embedding / split-K gradients
            if eng._g_stale_key is not None and eng._g_stale_key != key:
                # the previous fused step (another shape / mode: another tape) left the ranges ITS successor would have stored
                # un-zeroed; this step may accumulate there
                eng.zero_grad()
            eng._g_dirty = True        # (after the zeroing above, which clears the flag)
            if self.reducer:
                # the token ids of every rank name the rows of the word-embedding table this step touches: their
                # all-gather + union start now on the communication stream (inputs_embeds: no row is touched)
                self.reducer.begin_step(ws["ids"] if ws.get("txt_embeds") is None else None)
            if self.use_tape and self._tape is not None and self._tape_key == key and self._tape_ws is ws:
                eng.drop_seed = (eng.drop_seed + 1) & 0xFFFFFFFF
                if self._tape.rebinds:       # (the adopted pixel_patches tensor of THIS step: VaultEngine.adopt_pixel_patches)
                    self._tape.rebind(ws["apatch_in"].data_ptr())
                self._tape.replay(seed=eng.drop_seed)
            else:
                eng.drop_seed = (eng.drop_seed + 1) & 0xFFFFFFFF
                tape = ops.start_tape() if self.use_tape else None
                adopted = bool(ws.get("patches_in") and ws.get("patch_adopted"))
                if tape is not None and adopted:
                    ap_in = ws["apatch_in"]
                    tape.rebind_range = (ap_in.data_ptr(), ap_in.data_ptr() + ap_in.numel() * ap_in.element_size())
                try:
                    out = eng.forward_staged(ws, need_hidden=False, loss_scale=1.0 / B, precise=self.precise_forward)
                    # gradients are zero here: the fused optimizer clears them after use (they start at 0)
                    eng._backward(1.0 / B, None, None, None, self.reducer.on_stage if self.reducer else None, grads_zero=True)
                finally:
                    if self.use_tape:
                        ops.stop_tape()
                if tape is not None and adopted and len(tape.rebinds) < 2:
                    raise RuntimeError("adopted pixel_patches: the recorded step does not show the operand's two uses "
                                       "(patch-embedding GEMM, its weight gradient)")
                self._tape, self._tape_key, self._tape_ws, self._loss_buf = tape, key, ws, out["loss"]
                self._zero_mask = self._build_zero_mask(eng._stored_ranges)
            if self.reducer and self._needs_norm:
                # the gradient norm needs the whole reduced gradient: no optimizer pass under the last bucket's exchange
                self.reducer.finish()
                self.optimizer_step(zero_mask=self._zero_mask)
            elif self.reducer:
                # optimizer on the already reduced upper part of the flat buffer while the last bucket (LM / ViLT
                # embeddings: the lowest addresses) is still being all-reduced, then on the rest
                x = self.reducer.finish_upper()
                if 0 < x < eng.params.n_train:
                    self.optimizer_step(lo=x, hi=eng.params.n_train, advance=False, zero_mask=self._zero_mask)
                    self.reducer.finish()
                    self.optimizer_step(lo=0, hi=x, zero_mask=self._zero_mask)
                else:
                    self.reducer.finish()
                    self.optimizer_step(zero_mask=self._zero_mask)
            else:
                self.optimizer_step(zero_mask=self._zero_mask)
            eng._g_dirty = False       # (the optimizer pass over [0, n_train) is enqueued: it zeroes what it reads ...)
            eng._g_stale_key = key if self._zero_mask is not None else None     # (... but for the ranges the next step stores)
        self.loss = self._loss_buf
        return self.loss

    def _build_zero_mask(self, stored):
        """One byte per 64 gradient elements: 0 over the weight-gradient matrices the recorded backward writes with stores only
        (engine._stored_ranges: every tensor is 64-element aligned) - the optimizer skips their zeroing (4 of its 34 B/param);
        None when nothing is stored (small batches: split-K launches accumulate) or with VAULT_ADAMW_ZERO_MASK=0."""
        if not stored or os.environ.get("VAULT_ADAMW_ZERO_MASK", "1") == "0":
            return None
        key = tuple(sorted(stored))
        if getattr(self, "_zero_mask_key", None) == key:
            return self._zero_mask
        n64 = self.engine.params.n_train // 64
        m = np.ones(n64, np.uint8)
        for o, n in key:
            assert o % 64 == 0 and n % 64 == 0
            m[o // 64:(o + n) // 64] = 0
        self._zero_mask_key = key
        return torch.from_numpy(m).to(self.engine.device)

    def optimizer_step(self, lo: int = 0, hi: Optional[int] = None, advance: bool = True,
                       zero_mask: Optional[torch.Tensor] = None):
        """Fused AdamW (``optimizer``) over elements [lo, hi) of the flat parameter buffer (default: all trainable ones);
        ``advance=False`` leaves the step counter alone (first part of a split update).  ``zero_mask`` (one byte per 64
        elements of the WHOLE buffer, 0 = leave the gradient un-zeroed) is the fused step's own: a caller that steps the
        optimizer by hand (gradient accumulation, a manual loop) gets every gradient it read cleared.
        With ``max_grad_norm`` / ``track_grad_norm`` a pass over the whole range first measures the gradient norm (and
        clips); clipping refuses a partial range.  With parameter groups ``lo`` must be 64-aligned."""
        eng = self.engine
        self._refuse_inside_ema_weights("optimizer_step")
        P = eng.params
        hi = P.n_train if hi is None else hi
        full = lo == 0 and hi == P.n_train
        if hi > lo and not full and self.max_grad_norm is not None:
            raise ValueError("max_grad_norm: the optimizer step must cover every trainable element (the norm needs the "
                             "whole gradient)")
        if hi > lo and self._group_map is not None and lo % 64:
            raise ValueError("parameter groups: the optimizer range must start at a multiple of 64 elements")
        with torch.cuda.device(eng.device), ops.operand_format(eng.half):
            if hi > lo:
                # (the gradients carry the operand format's power-of-two scale - fp16: engine.grad_scale - and the sum
                #  over the ranks: both are divided out here)
                gscale = 1.0 / (self.world * eng.grad_scale)
                zm = zero_mask
                if zm is not None and (lo % 64 or (hi - lo) % 64):
                    zm = None          # (never for the engine's 64-aligned stage boundaries)
                coef = None
                if full and self._needs_norm:
                    # norm of the reduced, unscaled gradient and the clip factor, both left on the device for AdamW
                    out = torch.empty(2, dtype=torch.float32, device=eng.device)
                    ops.grad_norm(P.g, P.n_train, self._norm_partials, out,
                                  self.max_grad_norm if self.max_grad_norm is not None else math.inf, gscale)
                    self.grad_norm = out[0]
                    coef = out[1:] if self.max_grad_norm is not None else None
                # one call: pass_call names the entry point and its scalars (both halves of a split pass run at the same t: the
                # counter advances behind the second); the tensors are the same ranges of the flat buffers for every form
                name, scalars, kw = pass_call(
                    optimizer=self.optimizer, grouped=self._group_map is not None, averaged=self.ema is not None, lr=self.lr,
                    beta1=self.b1, beta2=self.b2, eps=self.eps, weight_decay=self.wd, correct_bias=self.correct_bias,
                    ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, lr_schedule=self.lr_schedule,
                    constant_lr=self.constant_lr, warmup_steps=self.warmup_steps, total_steps=self.total_steps,
                    step_idx=self.step_idx)
                tensors = [P.p[lo:hi], P.g[lo:hi], P.m[lo:hi], P.v[lo:hi], P.pb[lo:hi], hi - lo]
                ema = None if self.ema is None else self.ema[lo:hi]
                if name == "adamw_step_ema":
                    tensors.insert(5, ema)      # (this form takes the average in front of the count ...)
                elif name == "adamw_step_torch":
                    kw["ema"] = ema             # (... this one by keyword: None without an average)
                if self._group_map is not None:
                    tensors += [self._group_map[lo // 64:(hi + 63) // 64], self._group_table]
                    kw["coef"] = coef
                # (looked up on the module at call time: the tests put stand-ins there)
                getattr(ops, name)(*tensors, *scalars, grad_scale=gscale, zero_grad=True,
                                   zero_mask=None if zm is None else zm[lo // 64:hi // 64], **kw)
        if advance:
            with torch.cuda.device(eng.device):
                P.refresh_transposed()   # W^T shadow of the data-gradient GEMMs, from the bf16 shadow just written
            P._pb3_fresh = False   # the split-bf16 (precise inference) shadow is stale now
            self.step_idx += 1

    # ---- weight average ---------------------------------------------------------------------------------------------
    def _refuse_inside_ema_weights(self, what: str):
        if self._ema_swapped:
            raise RuntimeError(f"{what} inside ema_weights(): the parameter buffer holds the averaged weights")

    def reset_ema(self):
        """Start the average over from the current weights (for a caller who loaded weights after building the step)."""
        if self.ema is None:
            raise RuntimeError("this TrainStep keeps no weight average (ema_decay=None)")
        self._refuse_inside_ema_weights("reset_ema")
        self.ema.copy_(self.engine.params.p[:self.engine.params.n_train])

    def _swap_ema(self):
        eng = self.engine
        P = eng.params
        with torch.cuda.device(eng.device), ops.operand_format(eng.half):
            ops.ema_swap(P.p, self.ema, P.pb, P.n_train)
            P.refresh_transposed()
        P._pb3_fresh = False

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the engine runs on the averaged weights: the average and the trainable part of the flat
        parameter buffer change places ON the device (recorded tapes and the model classes' ``nn.Parameter`` views point
        into that buffer), with the 16-bit, transposed and split shadows following - ``engine.forward(..., train=False)``,
        :func:`evaluate`, ``ParamStore.state_dict_numpy()`` and a model's ``state_dict()`` / ``save_pretrained`` all see
        the average.  Leaving the block, also by an exception, swaps back: every buffer has its old bits again.  Training
        steps, ``optimizer_step`` and a nested ``ema_weights()`` inside the block raise RuntimeError."""
        if self.ema is None:
            raise RuntimeError("this TrainStep keeps no weight average (ema_decay=None)")
        self._refuse_inside_ema_weights("ema_weights()")
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swapped = False
            self._swap_ema()

    # ---- optimizer state --------------------------------------------------------------------------------------------
    def _named(self, buf: torch.Tensor) -> Dict[str, torch.Tensor]:
        P = self.engine.params
        host = buf[:P.n_train].detach().cpu()
        return {n: P._view(host, n).clone() for n in P.trainable}

    def state_dict(self) -> dict:
        """What a run needs besides the weights to continue where it stopped, as CPU tensors by parameter name: the AdamW
        moments (``exp_avg``, ``exp_avg_sq``), the weight average (``ema``, None without one), the step counter (the
        schedule's position) and the engine's dropout seed; ``hyper`` records the step's settings for the reader.  The
        weights themselves are saved by the model (``state_dict()`` / ``save_pretrained``), as before.  To resume: load the
        weights, build the step, then :meth:`load_state_dict`."""
        self._refuse_inside_ema_weights("state_dict")
        P = self.engine.params
        return {"step_idx": int(self.step_idx), "drop_seed": int(self.engine.drop_seed),
                "exp_avg": self._named(P.m), "exp_avg_sq": self._named(P.v),
                "ema": None if self.ema is None else self._named(self.ema),
                "hyper": dict(lr=self.lr, betas=(self.b1, self.b2), eps=self.eps, weight_decay=self.wd,
                              correct_bias=self.correct_bias, total_steps=self.total_steps, warmup_steps=self.warmup_steps,
                              ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, optimizer=self.optimizer)}

    def load_state_dict(self, sd: dict):
        """Write a :meth:`state_dict` into the moments, the average, the step counter and the engine's dropout seed
        (checked first by :func:`check_optimizer_state`: nothing is written when it raises).  Hyper-parameters are not
        taken over: this step's own hold."""
        self._refuse_inside_ema_weights("load_state_dict")
        P = self.engine.params
        check_optimizer_state(P, sd, self.ema is not None)
        for key, buf in (("exp_avg", P.m), ("exp_avg_sq", P.v), ("ema", self.ema)):
            if buf is None:
                continue
            host = buf[:P.n_train].detach().cpu()           # (the padding between tensors keeps what it holds)
            for n in P.trainable:
                P._view(host, n).copy_(torch.as_tensor(sd[key][n], dtype=torch.float32))
            buf[:P.n_train].copy_(host)
        self.step_idx = int(sd["step_idx"])
        self.engine.drop_seed = int(sd["drop_seed"]) & 0xFFFFFFFF


def evaluation_metrics(eval_true, eval_preds) -> Dict[str, float]:
    """``eval_accuracy`` and ``macro_f1_score`` as the reference computes them (ref: vault/tmsc_utils/trainer.py:513-549:
    sklearn ``precision_recall_fscore_support(average="macro", zero_division=0)`` over the union of the labels that
    occur in truth or predictions, and the plain match rate)."""
    t = np.asarray(list(eval_true)).reshape(-1)
    p = np.asarray(list(eval_preds)).reshape(-1)
    f1s = []
    for c in np.union1d(t, p):
        tp = float(np.sum((p == c) & (t == c)))
        fp = float(np.sum((p == c) & (t != c)))
        fn = float(np.sum((p != c) & (t == c)))
        prec = tp / (tp + fp) if tp + fp > 0 else 0.0
        rec = tp / (tp + fn) if tp + fn > 0 else 0.0
        f1s.append(2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0)
    return dict(eval_accuracy=float(np.mean(p == t)) if t.size else 0.0,
                macro_f1_score=float(np.mean(f1s)) if f1s else 0.0)


def evaluate(engine: VaultEngine, batches) -> Dict[str, float]:
    """The reference's evaluation pass (ref: vault/tmsc_utils/trainer.py:429-484): eval-mode forward per batch (all
    dropouts off), mean cross-entropy weighted by batch size, argmax predictions, accuracy and macro-F1.
    ``batches`` yields ``(batch_dict_on_device, labels_on_device)``."""
    preds, true = [], []
    loss_sum, n = 0.0, 0
    for batch, labels in batches:
        out = engine.forward(batch, train=False, labels=labels, need_hidden=False)
        B = int(labels.shape[0])
        loss_sum += float(out["loss"].item()) * B
        n += B
        preds.extend(out["logits"].view(B, -1).argmax(dim=-1).tolist())
        true.extend(labels.view(-1).tolist())
    res = evaluation_metrics(true, preds)
    res["eval_loss"] = loss_sum / max(n, 1)
    return res
