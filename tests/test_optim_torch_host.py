"""Host side of the train step's torch.optim.AdamW option: the inputs, the float64 reference (``torch.optim.AdamW`` itself,
single-tensor, on the CPU) and the error bounds that tests/test_gpu_optim_torch.py holds the kernel to - calibrated here without
a GPU - plus the option's argument checks, the bias corrections and the warm-up schedules.

The bounds, with u = 2^-24, after t steps, per element i:
  weights  |p - p64| <= t u (4 P_i + 32 S_i): P_i the largest |p_i| of the float64 run so far (the start included) - the roundings
           of p itself: the decay product, the subtraction, slack for an fma; S_i = lr_group(i) max_{s<=t} factor_s / (1 - b1^s) -
           the update, whose quotient m / denom is O(1) after bias correction;
  moments  |m - m64| <= t u G_i and |v - v64| <= 8 t u V_i, G_i = max_s |g_i| (the gradient the optimizer sees), V_i = max_s v64_i.
The weights and gradients are smaller than the workload's on purpose: that is what puts the eps placement and the decay order
above ulp(p)."""
import math
import types

import numpy as np
import pytest
import torch

from tests.optim_common import U, _f32, _stub_engine
from vault_amd.train import (LR_SCHEDULES, TrainStep, adam_bias_corrections, constant_with_warmup_schedule, cosine_schedule,
                             linear_schedule)

GROUPS = [(2e-3, 0.1), (1e-2, 0.0), (5e-3, 0.5)]
FACTORS = [1.0, 0.75, 0.5, 0.25]
B1, B2, EPS, T = 0.9, 0.999, 1e-8, 4
COEF = 0.37                        # the clip factor the kernel reads from the device


def make_case(n64=210, seed=3, steps=T):
    """p0 = N(0,1) 10^U(-4,0); a group per 64-block; four never-touched blocks per group; a random zero mask; per step
    g = N(0,1) 10^U(-6,0) (f32 values, zero on the never-touched blocks)."""
    rng = np.random.default_rng(seed)
    n = 64 * n64
    p0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32)
    gid = rng.integers(0, 3, n64).astype(np.uint8)
    idle = np.zeros(n64, bool)
    for k in range(3):
        idle[np.flatnonzero(gid == k)[:4]] = True
    zmask = (rng.random(n64) > 0.3).astype(np.uint8)
    grads = []
    for _ in range(steps):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        g[np.repeat(idle, 64)] = 0.0
        grads.append(g)
    return types.SimpleNamespace(n=n, n64=n64, p0=p0, gid=gid, idle=idle, zmask=zmask, grads=grads)


def torch_adamw_run(p0, el_group, grads, factors, groups=GROUPS, betas=(B1, B2), eps=EPS, dtype=torch.float64):
    """The reference: ``torch.optim.AdamW(foreach=False, fused=False)`` on CPU tensors of ``dtype``, one nn.Parameter per group
    gathered from the flat buffer by ``el_group`` (group index per element), stepped with LambdaLR over ``factors``.  Yields the
    flat (p, m, v) as float64 numpy arrays after every step; ``grads`` are the gradients the optimizer sees."""
    idx = [torch.from_numpy(np.flatnonzero(el_group == k)) for k in range(len(groups))]
    flat = torch.from_numpy(np.asarray(p0))
    params = [torch.nn.Parameter(flat[ix].to(dtype)) for ix in idx]
    opt = torch.optim.AdamW([{"params": [q], "lr": lr, "weight_decay": wd} for q, (lr, wd) in zip(params, groups)],
                            betas=betas, eps=eps, foreach=False, fused=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: factors[min(s, len(factors) - 1)])
    for g in grads:
        g = torch.from_numpy(np.asarray(g))
        for q, ix in zip(params, idx):
            q.grad = g[ix].to(dtype)
        opt.step()
        sched.step()
        out = [np.zeros(len(el_group)) for _ in range(3)]
        for q, ix in zip(params, idx):
            st = opt.state[q]
            for o, x in zip(out, (q.detach(), st["exp_avg"], st["exp_avg_sq"])):
                o[ix.numpy()] = x.double().numpy()
        yield tuple(out)


class Bounds:
    """The tolerances of the module docstring, gathered along the float64 run."""

    def __init__(self, p0, el_group, groups=GROUPS, b1=B1):
        self.lr = np.asarray([lr for lr, _ in groups])[el_group]
        self.P = np.abs(np.asarray(p0, np.float64))
        self.G = np.zeros_like(self.P)
        self.V = np.zeros_like(self.P)
        self.s, self.t, self.b1 = 0.0, 0, b1

    def update(self, p64, g64, v64, factor):
        self.t += 1
        self.P = np.maximum(self.P, np.abs(p64))
        self.G = np.maximum(self.G, np.abs(g64))
        self.V = np.maximum(self.V, v64)
        self.s = max(self.s, factor / (1.0 - self.b1 ** self.t))
        return self

    @property
    def p(self):
        return self.t * U * (4.0 * self.P + 32.0 * self.lr * self.s)

    @property
    def m(self):
        return self.t * U * self.G

    @property
    def v(self):
        return 8.0 * self.t * U * self.V

    def worst(self, got, want, which):
        """max |got - want| / bound (0 / 0 counts as 0: never-touched elements keep exact zeros)."""
        err, tol = np.abs(np.asarray(got, np.float64) - want), getattr(self, which)
        return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))))


def short_decimal(x):
    """optim_torch.hip's short_decimal: the shortest decimal that rounds to the f32 ``x``."""
    x = np.float32(x)
    s = 10.0
    while s <= 1e9:
        r = float(np.rint(float(x) * s)) / s
        if np.float32(r) == x:
            return r
        s *= 10.0
    return float(x)


def numpy_adamw_run(p0, el_group, grads, factors, dtype=np.float64, mutant=None, groups=GROUPS, naive_betas=False):
    """AdamW written out in the kernel's operation order in ``dtype`` (float32: a restatement of the kernel without its fused
    multiply-adds; float64 with ``mutant``: one of the three places in which the HF form differs from torch's)."""
    f = dtype
    p = np.asarray(p0).astype(f)
    m, v = np.zeros_like(p), np.zeros_like(p)
    lr0 = np.asarray([lr for lr, _ in groups], np.float32).astype(f)[el_group]
    wd = np.asarray([w for _, w in groups], np.float32).astype(f)[el_group]
    if dtype == np.float64:
        lr0, wd = np.asarray([lr for lr, _ in groups])[el_group], np.asarray([w for _, w in groups])[el_group]
        b1, b2, omb1, omb2 = B1, B2, 1.0 - B1, 1.0 - B2
    else:
        b1, b2 = f(B1), f(B2)
        omb1, omb2 = (f(1) - b1, f(1) - b2) if naive_betas else (f(1.0 - short_decimal(b1)), f(1.0 - short_decimal(b2)))
    for t, g in enumerate(grads, 1):
        inv_bc1, inv_sqrt_bc2 = adam_bias_corrections(B1, B2, t)
        if mutant == "no_bias_correction":
            inv_bc1 = inv_sqrt_bc2 = 1.0
        lr = f(factors[t - 1]) * lr0
        ge = np.asarray(g).astype(f)
        decay = f(1) - lr * wd
        if mutant != "decay_after":
            p = p * decay
        m = m * b1 + omb1 * ge
        v = v * b2 + omb2 * ge * ge
        if mutant == "hf_eps":
            p = p - (lr * f(inv_bc1) / f(inv_sqrt_bc2)) * (m / (np.sqrt(v) + f(EPS)))
        else:
            p = p - (lr * f(inv_bc1)) * (m / (np.sqrt(v) * f(inv_sqrt_bc2) + f(EPS)))
        if mutant == "decay_after":
            p = p - lr * wd * p
        yield p.copy(), m.copy(), v.copy()


# ---- tolerance calibration ----------------------------------------------------------------------------------------------
def test_bounds_hold_for_float32_adamw_and_catch_the_three_hf_differences():
    """What keeps the GPU test from hiding a wrong formula, for the reference alone: torch's own float32 run stays within
    half of every bound, and each float64 mutant - HF eps placement, decay after the update, no bias correction - leaves the
    weight bound on more than half of the elements of the groups it can affect, at every step.  Then the GPU test's own
    situation, in which the float64 run sees g x float(f32(0.37)) and a float32 run that product rounded: torch's float32 run and
    a float32 restatement in the kernel's operation order stay within the bounds."""
    case = make_case()
    el = np.repeat(case.gid, 64).astype(np.int64)
    g64 = [g.astype(np.float64) for g in case.grads]
    ref = list(torch_adamw_run(case.p0, el, g64, FACTORS))
    t32 = list(torch_adamw_run(case.p0, el, case.grads, FACTORS, dtype=torch.float32))
    mutants = {name: list(numpy_adamw_run(case.p0, el, g64, FACTORS, mutant=name))
               for name in ("hf_eps", "decay_after", "no_bias_correction")}
    plain = list(numpy_adamw_run(case.p0, el, g64, FACTORS))
    affected = {"hf_eps": np.ones(case.n, bool), "no_bias_correction": np.ones(case.n, bool),
                "decay_after": (el == 0) | (el == 2)}
    bnd = Bounds(case.p0, el)
    for t in range(T):
        p64, m64, v64 = ref[t]
        bnd.update(p64, g64[t], v64, FACTORS[t])
        w = [bnd.worst(x, y, which) for x, y, which in zip(t32[t], ref[t], "pmv")]
        print(f"step {t + 1} torch float32: err / bound p {w[0]:.3f} m {w[1]:.3f} v {w[2]:.3f}")
        assert max(w) <= 0.5, (t + 1, w)
        # the float64 restatement is the reference's formula: the mutants differ from it by their mutation alone
        assert bnd.worst(plain[t][0], p64, "p") < 1e-6
        for name, run in mutants.items():
            sel = affected[name]
            out = float(np.mean(np.abs(run[t][0] - p64)[sel] > bnd.p[sel]))
            print(f"step {t + 1} mutant {name}: outside the weight bound on {100 * out:.1f} % of its elements")
            assert out > 0.5, (name, t + 1, out)
    # the GPU test's situation
    c = _f32(COEF)
    g64 = [g.astype(np.float64) * c for g in case.grads]
    g32 = [g.astype(np.float32) for g in g64]
    ref = list(torch_adamw_run(case.p0, el, g64, FACTORS))
    runs = {"torch float32": list(torch_adamw_run(case.p0, el, g32, FACTORS, dtype=torch.float32)),
            "kernel order float32": list(numpy_adamw_run(case.p0, el, g32, FACTORS, dtype=np.float32))}
    naive = list(numpy_adamw_run(case.p0, el, g32, FACTORS, dtype=np.float32, naive_betas=True))
    bnd = Bounds(case.p0, el)
    for t in range(T):
        bnd.update(ref[t][0], g64[t], ref[t][2], FACTORS[t])
        for name, run in runs.items():
            w = [bnd.worst(x, y, which) for x, y, which in zip(run[t], ref[t], "pmv")]
            print(f"step {t + 1} {name}, gradient x f32(0.37): err / bound p {w[0]:.3f} m {w[1]:.3f} v {w[2]:.3f}")
            assert max(w) <= 1.0, (name, t + 1, w)
        # 1 - beta2 taken from the f32 beta2 is 216 u from 0.001: the second moment leaves its bound (why optim_torch.hip does
        # not compute it that way)
        wv = bnd.worst(naive[t][2], ref[t][2], "v")
        print(f"step {t + 1} float32 with 1.f - beta2f: v err / bound {wv:.1f}")
        assert wv > 1.0


def test_short_decimal_recovers_the_usual_betas():
    for b in (0.9, 0.999, 0.8, 0.99, 0.95, 0.98, 0.9999, 0.5, 0.0):
        assert short_decimal(np.float32(b)) == b
    x = np.float32(0.9) * np.float32(0.987654321)                   # no short decimal: the f32 itself
    assert np.float32(short_decimal(x)) == x


# ---- options ---------------------------------------------------------------------------------------------------------------
def test_option_checks_come_before_any_allocation():
    with pytest.raises(ValueError, match="optimizer"):
        TrainStep(_stub_engine(), optimizer="adam")
    with pytest.raises(ValueError, match="correct_bias"):
        TrainStep(_stub_engine(), optimizer="torch", correct_bias=True)
    with pytest.raises(ValueError, match="lr_schedule"):
        TrainStep(_stub_engine(), lr_schedule="nope")
    # (an engine without any attribute: the checks ran before the step looked at it)
    for bad in (dict(optimizer="adam"), dict(optimizer="torch", correct_bias=True), dict(lr_schedule="nope")):
        with pytest.raises(ValueError):
            TrainStep(object(), **bad)


def test_torch_option_builds_one_group_and_default_builds_none():
    step = TrainStep(_stub_engine(), optimizer="torch", learning_rate=3e-4, weight_decay=0.25)
    assert step.optimizer == "torch" and step._group_map is not None and not step._group_map.any()
    assert step._group_table.tolist() == [[_f32(3e-4), 0.25]]
    assert step.ema is None and step._norm_partials is None
    plain = TrainStep(_stub_engine())
    assert plain.optimizer == "hf" and plain.lr_schedule == "linear" and plain._group_map is None


def test_adam_bias_corrections():
    for b1, b2 in ((0.9, 0.999), (0.8, 0.99)):
        for t in range(1, 2001):
            assert adam_bias_corrections(b1, b2, t) == (1 / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t)), (b1, b2, t)


# ---- schedules ---------------------------------------------------------------------------------------------------------------
def _hf_factors(make, steps, **kw):
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sched = make(opt, **kw)
    out = []
    for _ in range(steps):
        out.append(sched.get_last_lr()[0])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("warmup,total", [(3, 25), (0, 25)])
def test_schedules_equal_the_transformers_functions(warmup, total):
    import transformers.optimization as HO
    cases = ((cosine_schedule, HO.get_cosine_schedule_with_warmup, dict(num_warmup_steps=warmup, num_training_steps=total)),
             (constant_with_warmup_schedule, HO.get_constant_schedule_with_warmup, dict(num_warmup_steps=warmup)),
             (linear_schedule, HO.get_linear_schedule_with_warmup, dict(num_warmup_steps=warmup, num_training_steps=total)))
    for ours, make, kw in cases:
        want = _hf_factors(make, 30, **kw)
        for s in range(30):
            got = ours(1.0, s, warmup, total)
            assert abs(got - want[s]) <= 1e-15 * abs(want[s]), (ours.__name__, s, got, want[s])
            assert abs(ours(2e-5, s, warmup, total) - 2e-5 * want[s]) <= 2e-15 * 2e-5 * abs(want[s])


def test_train_step_uses_the_chosen_schedule():
    assert LR_SCHEDULES["linear"] is linear_schedule
    for name, fn in LR_SCHEDULES.items():
        step = TrainStep(_stub_engine(), learning_rate=2e-5, warmup_ratio=0.12, total_steps=25, lr_schedule=name)
        assert step.warmup_steps == 3
        flat = TrainStep(_stub_engine(), learning_rate=2e-5, warmup_ratio=0.12, total_steps=25, lr_schedule=name, constant_lr=True)
        for s in range(30):
            step.step_idx = flat.step_idx = s
            assert step.current_lr() == fn(2e-5, s, 3, 25) and step.lr_factor() == fn(1.0, s, 3, 25)
            assert flat.current_lr() == 2e-5 and flat.lr_factor() == 1.0          # constant_lr wins
    step = TrainStep(_stub_engine(), learning_rate=2e-5, warmup_ratio=0.12, total_steps=25)
    step.step_idx = 10
    assert step.current_lr() == linear_schedule(2e-5, 10, 3, 25)                  # the default is today's
