"""Host side of the fused train step's optimizer: learning-rate schedules, bias corrections, parameter groups, the decay of
the weight average, the check of a saved optimizer state - and :func:`pass_call`, the one place that decides which AdamW entry
point of ``ops`` an optimizer pass uses and with which scalars.  Pure functions of numbers and names: no tensor on a device, no
engine, no ``ops``.
"""
from __future__ import annotations

import math
import re
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .spec import VaultSpec, param_entries

if TYPE_CHECKING:
    from .engine import VaultEngine


def linear_schedule(base_lr: float, step: int, warmup_steps: int, total_steps: int) -> float:
    """lr used by optimizer step number ``step`` (0-based) under get_linear_schedule_with_warmup."""
    if step < warmup_steps:
        return base_lr * float(step) / float(max(1, warmup_steps))
    return base_lr * max(0.0, float(total_steps - step) / float(max(1, total_steps - warmup_steps)))


def cosine_schedule(base_lr: float, step: int, warmup_steps: int, total_steps: int) -> float:
    """lr used by optimizer step number ``step`` (0-based) under get_cosine_schedule_with_warmup (half a cosine period: num_cycles
    0.5, multiplied in HF's order so that the factors agree to the last bit)."""
    if step < warmup_steps:
        return base_lr * float(step) / float(max(1, warmup_steps))
    progress = float(step - warmup_steps) / float(max(1, total_steps - warmup_steps))
    return base_lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))


def constant_with_warmup_schedule(base_lr: float, step: int, warmup_steps: int, total_steps: int) -> float:
    """lr used by optimizer step number ``step`` (0-based) under get_constant_schedule_with_warmup (``total_steps`` plays no
    part: the signature is the other schedules')."""
    if step < warmup_steps:
        return base_lr * float(step) / float(max(1.0, warmup_steps))
    return base_lr


LR_SCHEDULES = {"linear": linear_schedule, "cosine": cosine_schedule, "constant_with_warmup": constant_with_warmup_schedule}
OPTIMIZERS = ("hf", "torch")      # transformers-4.48 AdamW (the reference's), torch.optim.AdamW


def scheduled(base: float, lr_schedule: str, constant_lr: bool, step: int, warmup_steps: int, total_steps: int) -> float:
    """``base`` under the named schedule at optimizer step ``step`` (0-based); ``constant_lr`` overrides the schedule."""
    return base if constant_lr else LR_SCHEDULES[lr_schedule](base, step, warmup_steps, total_steps)


def adam_bias_corrections(beta1: float, beta2: float, t: int) -> Tuple[float, float]:
    """(1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) at optimizer step ``t`` (1-based) in double precision: what
    torch.optim.AdamW divides its step size and the root of the second moment by (vault_adamw_step_torch takes them as
    factors)."""
    return 1.0 / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t)


# ---- parameter groups ------------------------------------------------------------------------------------------------
# transformers' Trainer.get_decay_parameter_names: no weight decay on parameters whose lower-cased name matches one of these,
# nor on any parameter of an nn.LayerNorm module
NO_DECAY_PATTERNS = (r"bias", r"layernorm", r"rmsnorm", r"(?:^|\.)norm(?:$|\.)", r"_norm(?:$|\.)")
MAX_PARAM_GROUPS = 256       # one byte per 64 elements in the group map (vault_adamw_step_grouped)


def no_decay_parameter_names(spec: VaultSpec, names: Sequence[str]) -> List[str]:
    """The names among ``names`` that an HF ``Trainer`` keeps out of weight decay: biases, every LayerNorm (BERT
    ``LayerNorm``, ViLT ``layernorm_before`` / ``layernorm_after`` / the final ``layernorm``, the embedding LayerNorms - and the
    MLP head's ``classifier.1``, a LayerNorm by module type, not by name)."""
    ln_modules = {n for n, _, init in param_entries(spec) if init == "ln_w"}
    pats = [re.compile(p_) for p_ in NO_DECAY_PATTERNS]
    return [n for n in names if n in ln_modules or any(p_.search(n.lower()) for p_ in pats)]


def hf_no_decay_groups(engine: VaultEngine) -> List[dict]:
    """``param_groups`` for :class:`TrainStep` as an HF ``Trainer`` builds its optimizer: the no-decay parameters in one group
    at weight decay 0, every other trainable parameter in the default group (the step's own ``weight_decay``)."""
    return [{"params": no_decay_parameter_names(engine.spec, engine.params.trainable), "weight_decay": 0.0}]


def build_param_groups(layout, param_groups: Optional[Sequence[dict]], lr: float, weight_decay: float):
    """Check ``param_groups`` against a parameter layout (``offsets``, ``trainable``, ``n_train``: a ParamStore or
    ParamStore.layout()) and return (group map: uint8 [n_train // 64], one group index per 64 elements; table: float32
    [n_groups, 2] of base (lr, weight_decay)).  Group 0 is the default group - every trainable parameter no group names,
    at (lr, weight_decay) - and group k + 1 is ``param_groups[k]``; its missing ``lr`` / ``weight_decay`` fall back to the
    step's.  ValueError for a name that is unknown, not trainable or in two groups, and for any key but those three."""
    groups = [] if param_groups is None else param_groups
    if isinstance(groups, (dict, str)) or not isinstance(groups, Sequence):
        raise ValueError("param_groups must be a sequence of dicts")
    if len(groups) + 1 > MAX_PARAM_GROUPS:
        raise ValueError(f"at most {MAX_PARAM_GROUPS - 1} parameter groups (besides the default group)")
    trainable = set(layout.trainable)
    table = [(float(lr), float(weight_decay))]
    gmap = np.zeros(layout.n_train // 64, np.uint8)
    owner: Dict[str, int] = {}
    for k, grp in enumerate(groups):
        if not isinstance(grp, dict):
            raise ValueError(f"param_groups[{k}] is not a dict")
        extra = set(grp) - {"params", "lr", "weight_decay"}
        if extra:
            raise ValueError(f"param_groups[{k}]: unsupported key(s) {sorted(extra)} (only params, lr and weight_decay "
                             "are per group; betas and eps are the step's)")
        names = grp.get("params")
        if names is None or isinstance(names, str):
            raise ValueError(f"param_groups[{k}]['params'] must be a list of parameter names")
        vals = []
        for key, default in (("lr", lr), ("weight_decay", weight_decay)):
            try:
                val = float(grp.get(key, default))
            except (TypeError, ValueError):
                raise ValueError(f"param_groups[{k}]['{key}'] is not a number") from None
            if not math.isfinite(val):
                raise ValueError(f"param_groups[{k}]['{key}'] is not finite")
            vals.append(val)
        table.append(tuple(vals))
        for n in names:
            if n not in layout.offsets:
                raise ValueError(f"param_groups[{k}]: unknown parameter {n!r}")
            if n not in trainable:
                raise ValueError(f"param_groups[{k}]: {n!r} is not trained by this engine (frozen or without gradient)")
            if n in owner:
                raise ValueError(f"{n!r} is in param_groups[{owner[n]}] and param_groups[{k}]")
            owner[n] = k
            o, shp = layout.offsets[n]
            gmap[o // 64:(o + int(np.prod(shp)) + 63) // 64] = k + 1      # (every tensor starts 64-aligned)
    return gmap, np.asarray(table, np.float32).reshape(-1, 2)


# ---- weight average and optimizer state ------------------------------------------------------------------------------
def ema_decay_at(decay: float, t: int, warmup: bool = False) -> float:
    """Decay of the weight average at optimizer step ``t`` (1-based): ``decay``, or with the usual EMA warm-up
    ``min(decay, (1 + t) / (10 + t))`` - the first steps weigh the fresh weights more, so that the average leaves the
    initial weights quickly (2 / 11 at t = 1)."""
    decay = float(decay)
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


OPTIMIZER_STATE_KEYS = ("step_idx", "drop_seed", "exp_avg", "exp_avg_sq", "ema", "hyper")


def check_optimizer_state(layout, sd, want_ema: bool) -> None:
    """Check a ``TrainStep.state_dict()`` against a parameter layout (``offsets``, ``trainable``: a ParamStore or
    ParamStore.layout()) before anything is written.  ``exp_avg``, ``exp_avg_sq`` (and ``ema`` when ``want_ema``) must name
    every trainable parameter exactly once with its shape: ValueError for a name that is unknown, not trainable or missing,
    for a tensor of the wrong shape, and for an ``ema`` entry that is there without ``want_ema`` or absent with it.  The
    ``hyper`` entries are not compared: the receiving step's own values hold."""
    if not isinstance(sd, dict):
        raise ValueError("optimizer state must be a dict (TrainStep.state_dict())")
    lost = [k for k in OPTIMIZER_STATE_KEYS if k not in sd and k != "hyper"]
    if lost:
        raise ValueError(f"optimizer state lacks {lost}")
    if sd["ema"] is not None and not want_ema:
        raise ValueError("optimizer state carries a weight average, this step keeps none (ema_decay=None)")
    if sd["ema"] is None and want_ema:
        raise ValueError("optimizer state carries no weight average, this step keeps one (ema_decay)")
    trainable = set(layout.trainable)
    for key in ("exp_avg", "exp_avg_sq") + (("ema",) if want_ema else ()):
        part = sd[key]
        if not isinstance(part, dict):
            raise ValueError(f"optimizer state [{key!r}] must be a dict of tensors by parameter name")
        for n, t in part.items():
            if n not in layout.offsets:
                raise ValueError(f"optimizer state [{key!r}]: unknown parameter {n!r}")
            if n not in trainable:
                raise ValueError(f"optimizer state [{key!r}]: {n!r} is not trained by this engine (frozen or without gradient)")
            if tuple(t.shape) != tuple(layout.offsets[n][1]):
                raise ValueError(f"optimizer state [{key!r}][{n!r}] has shape {tuple(t.shape)}, the parameter "
                                 f"{tuple(layout.offsets[n][1])}")
        missing = [n for n in layout.trainable if n not in part]
        if missing:
            raise ValueError(f"optimizer state [{key!r}] lacks {len(missing)} trainable parameter(s), the first: {missing[0]!r}")


# ---- one optimizer pass -----------------------------------------------------------------------------------------------
def pass_call(*, optimizer: str, grouped: bool, averaged: bool, lr: float, beta1: float, beta2: float, eps: float,
              weight_decay: float, correct_bias: bool, ema_decay: Optional[float], ema_warmup: bool, lr_schedule: str,
              constant_lr: bool, warmup_steps: int, total_steps: int, step_idx: int) -> Tuple[str, tuple, dict]:
    """Which AdamW entry point of ``ops`` the optimizer pass of step number ``step_idx`` (0-based) uses, and its scalars:
    (name, the scalars the entry point takes by position - they follow its tensors -, those it takes by keyword).
    ``grouped``: the step holds a group map (parameter groups, clipping, the average or the torch form asked for one);
    ``averaged``: it keeps a weight average.  Both halves of a split pass get the same answer: the step counter advances
    behind the second."""
    t = step_idx + 1
    when = (lr_schedule, constant_lr, step_idx, warmup_steps, total_steps)
    lr_factor = scheduled(1.0, *when)        # (LambdaLR: the grouped forms scale every group's base lr by it)
    bc = math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t) if correct_bias else 1.0
    if optimizer == "torch":
        omd = 1.0 - ema_decay_at(ema_decay, t, ema_warmup) if averaged else 1.0
        return ("adamw_step_torch", (lr_factor, beta1, beta2, eps) + adam_bias_corrections(beta1, beta2, t),
                dict(one_minus_decay=omd))
    if averaged:
        return ("adamw_step_ema", (lr_factor, beta1, beta2, eps, 1.0 - ema_decay_at(ema_decay, t, ema_warmup)),
                dict(bias_corr_factor=bc))
    if grouped:
        return "adamw_step_grouped", (lr_factor, beta1, beta2, eps), dict(bias_corr_factor=bc)
    return "adamw_step", (scheduled(lr, *when), beta1, beta2, eps, weight_decay), dict(bias_corr_factor=bc)
