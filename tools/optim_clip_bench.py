"""Cost of gradient clipping and parameter groups in the fused train step (informational, not a gate).

Part 1, at the full trainable size of ViLT-B/32 + BERTweet (222.4 M f32 elements, HF no-decay groups from the real layout):
vault_grad_norm, vault_adamw_step_grouped (with and without the device clip factor) and vault_adamw_step, interleaved rounds,
device events around 10 launches each, the median round reported.
Part 2 (unless --kernels-only): the B = 256 train step of bench.py, plain against max_grad_norm + HF decay groups, on one
engine, alternating rounds of --steps steps; prints one JSON line per part.
    python tools/optim_clip_bench.py [--steps 10] [--rounds 3] [--kernels-only]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vault_amd import ops                                                             # noqa: E402
from vault_amd.params import ParamStore                                               # noqa: E402
from vault_amd.spec import LMSpec, VaultSpec, ViltSpec, synthetic_batch               # noqa: E402
from vault_amd.train import TrainStep, build_param_groups, hf_no_decay_groups, no_decay_parameter_names   # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def time_launches(fn, reps=10):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3      # us per launch


def kernels(rounds):
    spec = VaultSpec(vilt=ViltSpec(), lm=LMSpec.bertweet_base(), n_classes=3)
    lay = ParamStore.layout(spec)
    n = lay.n_train
    nd = no_decay_parameter_names(spec, lay.trainable)
    gmap, table = build_param_groups(lay, [{"params": nd, "weight_decay": 0.0}], 2e-5, 0.01)
    dev = "cuda"
    p = torch.randn(n, device=dev); g = torch.randn(n, device=dev) * 1e-3
    m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); pb = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    dmap, dtab = torch.from_numpy(gmap).to(dev), torch.from_numpy(table).to(dev)
    parts = torch.empty(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device=dev)
    out = torch.empty(2, device=dev)
    fns = {
        "adamw_step": lambda: ops.adamw_step(p, g, m, v, pb, n, 2e-5, 0.9, 0.999, 1e-8, 0.01, grad_scale=1.0, zero_grad=True),
        "adamw_step_grouped": lambda: ops.adamw_step_grouped(p, g, m, v, pb, n, dmap, dtab, 1.0, 0.9, 0.999, 1e-8,
                                                             grad_scale=1.0, zero_grad=True),
        "adamw_step_grouped+coef": lambda: ops.adamw_step_grouped(p, g, m, v, pb, n, dmap, dtab, 1.0, 0.9, 0.999, 1e-8,
                                                                  grad_scale=1.0, coef=out[1:], zero_grad=True),
        "grad_norm": lambda: ops.grad_norm(g, n, parts, out, 1.0, 1.0),
    }
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            g.normal_(std=1e-3)          # (the AdamW passes zero it; the norm pass reads the same bytes either way)
            torch.cuda.synchronize()
            res[k].append(time_launches(f))
    us = {k: round(median(x), 1) for k, x in res.items()}
    bytes_ = {"adamw_step": 34 * n, "adamw_step_grouped": 34 * n + n // 64, "adamw_step_grouped+coef": 34 * n + n // 64,
              "grad_norm": 4 * n}
    return {"what": "optimizer kernels at the full trainable size (median of rounds, us per launch)", "n_elements": n,
            "no_decay_elements": int(sum(int(torch.tensor(lay.offsets[k][1]).prod()) for k in nd)),
            "us": us, "TB_per_s": {k: round(bytes_[k] / (us[k] * 1e-6) / 1e12, 2) for k in us},
            "spread_us": {k: [round(min(x), 1), round(max(x), 1)] for k, x in res.items()}}


def train_step(steps, rounds):
    import bench
    dev = torch.device("cuda:0")
    from vault_amd.engine import VaultEngine
    spec = VaultSpec(vilt=ViltSpec(), lm=LMSpec.bertweet_base(), n_classes=3)
    eng = VaultEngine(spec, dev, seed=0, classifier_dropout=0.1, half="bf16")
    B = 256
    bn = synthetic_batch(spec, B, seed=1234, n_classes=3)
    batch, _, labels = bench.resident_inputs(eng, spec, bn, dev)
    kw = dict(learning_rate=2e-5, warmup_ratio=0.1, total_steps=1000, assume_full_pixel_mask=True, weight_decay=0.01)
    steppers = {"plain": TrainStep(eng, **kw),
                "max_grad_norm+hf_groups": TrainStep(eng, max_grad_norm=1.0, param_groups=hf_no_decay_groups(eng), **kw)}
    for st in steppers.values():
        for _ in range(3):
            st(batch, labels)
    torch.cuda.synchronize()
    res = {k: [] for k in steppers}
    for _ in range(rounds):
        for k, st in steppers.items():
            evs = []
            for _ in range(steps):
                e0 = torch.cuda.Event(enable_timing=True); e0.record()
                st(batch, labels)
                e1 = torch.cuda.Event(enable_timing=True); e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            res[k].append(median([a.elapsed_time(b) for a, b in evs]))
    ms = {k: round(median(x), 3) for k, x in res.items()}
    return {"what": "B = 256 train step, bf16, one GPU (median step of each round, median of rounds, ms)", "ms": ms,
            "rounds_ms": {k: [round(x, 3) for x in v] for k, v in res.items()},
            "delta_pct": round(100.0 * (ms["max_grad_norm+hf_groups"] / ms["plain"] - 1.0), 2),
            "grad_norm_last_step": float(steppers["max_grad_norm+hf_groups"].grad_norm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_clip_bench.py times GPU kernels: no GPU visible")
    print(json.dumps(kernels(max(a.rounds, 5))), flush=True)
    torch.cuda.empty_cache()
    if not a.kernels_only:
        print(json.dumps(train_step(a.steps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
