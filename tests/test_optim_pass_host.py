"""``optim.pass_call``: which AdamW entry point an optimizer pass of the train step takes and every scalar it hands over, against
formulas written out here (no GPU, no ``ops``).  Floats are compared with ``==``: the kernels must see the bits they saw before
the choice had a function of its own."""
import itertools
import math

import pytest

from tests.optim_common import _stub_engine
from vault_amd.optim import pass_call
from vault_amd.train import TrainStep

LR, B1, B2, EPS, WD, DECAY, WARMUP, TOTAL = 3e-4, 0.9, 0.999, 1e-8, 0.05, 0.999, 3, 2000
STEPS = (0, 1, 999)


def _schedule(name, base, s, w=WARMUP, total=TOTAL):
    """get_{linear,cosine,constant}_schedule_with_warmup x base at 0-based step s, multiplied in the order the step uses."""
    if s < w:
        return base * float(s) / float(max(1, w))
    if name == "linear":
        return base * max(0.0, float(total - s) / float(max(1, total - w)))
    if name == "cosine":
        return base * max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * (float(s - w) / float(max(1, total - w))))))
    assert name == "constant_with_warmup"
    return base


def _call(step_idx, optimizer="hf", grouped=False, averaged=False, correct_bias=False, ema_warmup=False, lr_schedule="linear",
          constant_lr=False):
    return pass_call(optimizer=optimizer, grouped=grouped, averaged=averaged, lr=LR, beta1=B1, beta2=B2, eps=EPS, weight_decay=WD,
                     correct_bias=correct_bias, ema_decay=DECAY if averaged else None, ema_warmup=ema_warmup,
                     lr_schedule=lr_schedule, constant_lr=constant_lr, warmup_steps=WARMUP, total_steps=TOTAL, step_idx=step_idx)


def _bc(t, correct_bias):
    return math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t) if correct_bias else 1.0


def _one_minus_decay(t, warmup):
    return 1.0 - (min(DECAY, (1.0 + t) / (10.0 + t)) if warmup else DECAY)


@pytest.mark.parametrize("step_idx,correct_bias", itertools.product(STEPS, (False, True)))
def test_plain_form(step_idx, correct_bias):
    t = step_idx + 1
    assert _call(step_idx, correct_bias=correct_bias) == \
        ("adamw_step", (_schedule("linear", LR, step_idx), B1, B2, EPS, WD), {"bias_corr_factor": _bc(t, correct_bias)})


@pytest.mark.parametrize("step_idx,correct_bias", itertools.product(STEPS, (False, True)))
def test_grouped_form(step_idx, correct_bias):
    t = step_idx + 1
    assert _call(step_idx, grouped=True, correct_bias=correct_bias) == \
        ("adamw_step_grouped", (_schedule("linear", 1.0, step_idx), B1, B2, EPS), {"bias_corr_factor": _bc(t, correct_bias)})


@pytest.mark.parametrize("step_idx,correct_bias,ema_warmup", itertools.product(STEPS, (False, True), (False, True)))
def test_ema_form(step_idx, correct_bias, ema_warmup):
    t = step_idx + 1
    assert _call(step_idx, grouped=True, averaged=True, correct_bias=correct_bias, ema_warmup=ema_warmup) == \
        ("adamw_step_ema", (_schedule("linear", 1.0, step_idx), B1, B2, EPS, _one_minus_decay(t, ema_warmup)),
         {"bias_corr_factor": _bc(t, correct_bias)})


@pytest.mark.parametrize("step_idx,averaged,ema_warmup", itertools.product(STEPS, (False, True), (False, True)))
def test_torch_forms(step_idx, averaged, ema_warmup):
    t = step_idx + 1
    omd = _one_minus_decay(t, ema_warmup) if averaged else 1.0
    assert _call(step_idx, optimizer="torch", grouped=True, averaged=averaged, ema_warmup=ema_warmup) == \
        ("adamw_step_torch", (_schedule("linear", 1.0, step_idx), B1, B2, EPS, 1.0 / (1.0 - B1 ** t), 1.0 / math.sqrt(1.0 - B2 ** t)),
         {"one_minus_decay": omd})


def test_selection_order():
    name = lambda **kw: _call(5, **kw)[0]  # noqa: E731
    assert name() == "adamw_step"
    assert name(grouped=True) == "adamw_step_grouped"
    assert name(grouped=True, averaged=True) == "adamw_step_ema"
    assert name(optimizer="torch", grouped=True) == name(optimizer="torch", grouped=True, averaged=True) == "adamw_step_torch"


def test_track_grad_norm_alone_takes_the_plain_entry_point():
    """The group map is what ``grouped`` is read from: the norm alone builds none, every other option does."""
    step = TrainStep(_stub_engine(), track_grad_norm=True)
    assert step._needs_norm and step._group_map is None and step.ema is None and step.optimizer == "hf"
    assert _call(0, grouped=step._group_map is not None, averaged=step.ema is not None)[0] == "adamw_step"
    for kw in (dict(max_grad_norm=1.0), dict(param_groups=[]), dict(optimizer="torch")):
        assert TrainStep(_stub_engine(), **kw)._group_map is not None, kw


@pytest.mark.parametrize("lr_schedule", ["linear", "cosine", "constant_with_warmup"])
def test_the_schedule_in_use_is_the_one_named(lr_schedule):
    seen = set()
    for s in (0, 1, 2, 3, 500, 999, 1999, 2000, 2500):
        assert _call(s, lr_schedule=lr_schedule)[1][0] == _schedule(lr_schedule, LR, s)
        for kw in (dict(grouped=True), dict(grouped=True, averaged=True), dict(optimizer="torch", grouped=True)):
            assert _call(s, lr_schedule=lr_schedule, **kw)[1][0] == _schedule(lr_schedule, 1.0, s)
        # constant_lr overrides the named schedule, warm-up included
        assert _call(s, lr_schedule=lr_schedule, constant_lr=True)[1][0] == LR
        assert _call(s, lr_schedule=lr_schedule, constant_lr=True, grouped=True)[1][0] == 1.0
        seen.add(_call(s, lr_schedule=lr_schedule, grouped=True)[1][0])
    assert len(seen) > 3                                   # (the steps chosen tell the three schedules apart ...)
    others = {"linear", "cosine", "constant_with_warmup"} - {lr_schedule}
    assert all(_schedule(o, 1.0, 999) != _schedule(lr_schedule, 1.0, 999) for o in others)      # (... at step 999 pairwise)
