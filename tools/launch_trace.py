#!/usr/bin/env python3
"""The engine's recorded launch sequence (ops.Tape) of one named configuration as text: one line per recorded call - the C
function's name (`py` for a host callback), then every argument and every member of a struct argument; integers and floats as
they are, pointers as the index of their first appearance in the trace (addresses differ between runs, their pattern of reuse
does not) - and a SHA-256 of the lines.  Two trees that print the same hash enqueue the same device work.  Reads the tape
only: launches nothing of its own.

    python tools/launch_trace.py CONFIG [--lm roberta|bert] [--quiet]      (CONFIG: see CONFIGS; one process per configuration)
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vault_amd import ops  # noqa: E402
from vault_amd.engine import VaultEngine  # noqa: E402
from vault_amd.spec import LMSpec, VaultSpec, ViltSpec, synthetic_batch, synthetic_ragged_batch  # noqa: E402
from vault_amd.train import TrainStep, hf_no_decay_groups  # noqa: E402

PER_KERNEL = dict(STAGE_MAX_ROWS=0)
LISTEN = dict(dp_world=2, LM_WGRAD_GROUP=1)
# name -> engine attributes, then options: `listen` (forward + backward with a stage listener instead of a TrainStep call),
# `eng` (constructor keywords), `step` (TrainStep keywords), `spec` / `batch` (what runs), `optim` (TrainStep keywords of an
# optimizer configuration: four un-taped steps under one outer tape, so that the norm pass, the AdamW entry point with every
# scalar of every step and the shadow refresh are on it; `hf_groups`: param_groups=hf_no_decay_groups(engine))
CONFIGS = {
    "stage": ({}, {}),
    "per_kernel": (PER_KERNEL, {}),
    "per_layer_wgrad": (dict(PER_KERNEL, LM_WGRAD_BATCHED=False), {}),
    "listener": (dict(PER_KERNEL, **LISTEN), dict(listen=True)),
    "stage_listener": (LISTEN, dict(listen=True)),
    "freeze_lm": ({}, dict(eng=dict(freeze_lm=True))),
    "no_lm": ({}, dict(spec="no_lm")),
    "ragged": ({}, dict(batch="ragged")),
    "precise": ({}, dict(step=dict(precise_forward=True))),
    "fp8": ({}, dict(eng=dict(fp8_forward=True))),
    "embeds": ({}, dict(batch="embeds")),
    "full": ({}, dict(spec="full")),
    "optim_hf": ({}, dict(optim=dict(weight_decay=0.01, correct_bias=True, track_grad_norm=True))),
    "optim_grouped_clip": ({}, dict(optim=dict(weight_decay=0.01, max_grad_norm=1.0, lr_schedule="cosine"), hf_groups=True)),
    "optim_ema": ({}, dict(optim=dict(weight_decay=0.01, ema_decay=0.999, ema_warmup=True, correct_bias=True))),
    "optim_torch": ({}, dict(optim=dict(weight_decay=0.01, optimizer="torch", lr_schedule="constant_with_warmup"))),
    "optim_torch_ema": ({}, dict(optim=dict(weight_decay=0.01, optimizer="torch", ema_decay=0.99, max_grad_norm=1.0))),
}
OPTIM_STEPS = 4


def record(name, lm):
    attrs, opt = CONFIGS[name]
    spec = VaultSpec.tiny(3, lm)
    B = 5
    if opt.get("spec") == "no_lm":
        spec = VaultSpec(vilt=spec.vilt, lm=None, n_classes=3)
    elif opt.get("spec") == "full":     # 96 x 185 = 17,760 ViLT token rows: head-major qkv, 8-bit gelu', grouped ring launches
        spec = VaultSpec(vilt=ViltSpec(), lm=LMSpec.bertweet_base() if lm == "roberta" else LMSpec.bert_base_uncased(), n_classes=3)
        B = 96
    if opt.get("batch") == "ragged":
        bn = synthetic_ragged_batch(spec, [(192, 128), (96, 160), (160, 192)], (192, 192), seed=7)
    else:
        bn = synthetic_batch(spec, B, seed=7)
    eng = VaultEngine(spec, "cuda:0", seed=0, classifier_dropout=0.1, half="bf16", **opt.get("eng", {}))
    for k, v in attrs.items():
        setattr(eng, k, v)
    b = {k: torch.from_numpy(v).cuda() for k, v in bn.items()}
    if opt.get("batch") == "embeds":     # inputs_embeds + image_embeds, external dhidden / dpooled through backward()
        g = torch.Generator().manual_seed(7)
        H, L = spec.vilt.hidden_size, 24
        b = dict(inputs_embeds=torch.randn(B, 40, H, generator=g).cuda(), image_embeds=torch.randn(B, L, H, generator=g).cuda(),
                 attention_mask=b["attention_mask"])
        tape = ops.start_tape()
        try:
            eng.forward(b, train=True)
            eng.zero_grad()
            eng.backward(dhidden=torch.randn(B, 40 + L, H, generator=g).cuda(), dpooled=torch.randn(B, H, generator=g).cuda())
        finally:
            ops.stop_tape()
    elif opt.get("listen"):
        tape = ops.start_tape()
        try:
            eng.forward(b, train=True, labels=b["labels"], need_hidden=False)
            eng.zero_grad()
            eng.backward(after_layer=lambda tag: None)
        finally:
            ops.stop_tape()
    elif "optim" in opt:
        kw = dict(opt["optim"], param_groups=hf_no_decay_groups(eng)) if opt.get("hf_groups") else opt["optim"]
        step = TrainStep(eng, use_tape=False, total_steps=10, warmup_ratio=0.3, **kw)
        tape = ops.start_tape()
        try:
            for _ in range(OPTIM_STEPS):
                step(b, b["labels"])
        finally:
            ops.stop_tape()
    else:       # the fused step records its forward + backward itself (between ops.start_tape() and ops.stop_tape())
        step = TrainStep(eng, total_steps=10, **opt.get("step", {}))
        step(b, b["labels"])
        tape = step._tape
    torch.cuda.synchronize()
    return tape


def lines_of(tape):
    seen = {}

    def ptr(p):
        return "-" if not p else "p%d" % seen.setdefault(p, len(seen))

    def show(v, t=None):        # t: the declared type of a struct member / array element (ctypes hands pointers back as integers)
        v = getattr(v, "_obj", v)       # byref(struct)
        if isinstance(v, C.Structure):
            return "{" + " ".join(f"{n}={show(getattr(v, n), ft)}" for n, ft in v._fields_) + "}"
        if isinstance(v, C.Array):
            return "[" + " ".join(show(x, v._type_) for x in v) + "]"
        if t is C.c_void_p or isinstance(v, (C.c_void_p, C._Pointer)):
            return ptr(v if (v is None or isinstance(v, int)) else C.cast(v, C.c_void_p).value)
        return repr(v.value if isinstance(v, C._SimpleCData) else v)

    for fn, args in tape.calls:
        yield " ".join([fn.__name__] + [show(a) for a in args]) if args else "py"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--lm", default="roberta", choices=["roberta", "bert"])
    ap.add_argument("--quiet", action="store_true", help="print the hash only")
    a = ap.parse_args()
    lines = list(lines_of(record(a.config, a.lm)))
    if not a.quiet:
        print("\n".join(lines))
    print(f"{a.config} {a.lm} calls={len(lines)} sha256={hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
