#!/usr/bin/env python
"""Headline benchmark: train samples/sec (image+text pairs) of the ViLT-B32 + BERTweet-base
fine-tune step (forward + backward + fused AdamW, bf16 MFMA compute / fp32 master weights), per-GPU
batch 256, synthetic 384x384 images + 40-token captions, on N GPUs of one node (data parallel,
RCCL all-reduce of gradients).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W
  python bench.py --gpus N ...          (no torchrun environment: starts the N ranks itself, fails when the node has < N GPUs)
  python bench.py --config {2,3,4,5}    (BASELINE.json configs: per-GPU batch 64 | 64 x N ranks | frozen bert-base-uncased,
                                         batch 128 | MXFP8 forward, batch 256)
  python bench.py --gpus N --scaling strong   (global batch 256 = 256 / N per GPU; default weak: 256 per GPU)
  python bench.py ... --dump-outputs DIR      (after the timed steps: what the last one computed, DIR/<name>.npy)
  python bench.py ... --full                  (the measurements below besides the headline)

Rank 0 prints ONE JSON line (see DESIGN.md "Measurement").  A plain run sets up, warms up, times the K steps and prints
`value` / `ms_per_step` and the fields that need no further run.  `--full` adds what takes work of its own: the live
kernel timing below (`roofline`, `roofline_ffn1`, `blocks`), the golden-batch `parity` with the precise mode and the fp16
operand line, the f32-pixel / host->device / uint8 input loops, the other wire format, the other BASELINE configurations
and `cpu_baseline` (the `--no-*` options leave parts of it out).  `roofline` is the dominant kernel of the
step by GPU time (rocprofv3 --stats, profiles/): the weight-gradient instantiation of the bf16 MFMA ring
GEMM, gemm256_kernel<1,1,EPI_F32_ATOMIC,4>, timed live with events on the launch stream around all of its
launches (ViLT layers + patch projection) in every 4th timed step; `roofline_ffn1` is the same for the FFN-in forward GEMM (the
largest single GEMM call site; 8-wave kernel gemm8w_kernel<EPI_BF16_GELU,4>); `step_mfma_frac` is the whole step against the 2.5 PFLOP/s dense bf16 peak
with BASELINE.md's 120.67 GFLOP/sample.  `cpu_baseline` times the CPU oracle (plain fp32 torch
restatement of the reference path) on the host cores, on a bounded sample.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from vault_amd.engine import VaultEngine  # noqa: E402
from vault_amd.spec import LMSpec, VaultSpec, ViltSpec, build_state, synthetic_batch  # noqa: E402
from vault_amd.train import TrainStep  # noqa: E402

FLOP_PER_SAMPLE_TRAIN = 120.67e9      # BASELINE.md §2 (fwd 40.22 GF x 3)
FLOP_VILT_BLOCK_FWD = 32.687493120e9  # 12 ViLT layers (GEMMs + attention, S = 185 unpadded), forward, per sample
FLOP_LM_BLOCK_FWD = 6.853754880e9     # 12 LM layers (S = 40), forward, per sample
PEAK_BF16 = 2.5e15                    # MI355X dense bf16 MFMA, MI355X_MICROARCH.md


def _physical_cores() -> int:
    try:
        import psutil
        return int(psutil.cpu_count(logical=False) or os.cpu_count() or 1)
    except Exception:
        return int(os.cpu_count() or 1)


def cpu_baseline(spec, seconds_budget: float = 36.0):
    """Oracle (fp32 torch restatement of the reference path) fwd + bwd + HF-AdamW on the host cores.

    Bounded samples: batch 8 at 32 threads, batch 8 at every physical core, batch 32 at 32 threads - a
    third of `seconds_budget` each (one un-timed step first: allocator / thread-pool warm-up).  Eager torch CPU ops on
    this model stop scaling far below the core count of the GPU box, so `value` / `cores` are the FASTEST point; every
    point is listed in `runs`."""
    from oracle import vault_oracle as O
    state = build_state(spec, 0)
    phys = _physical_cores()
    points = [(min(32, phys), 8), (phys, 8), (min(32, phys), 32)]
    runs = []
    for cores, batch in points:
        if any(r["cores"] == cores and r["batch"] == batch for r in runs):
            continue
        torch.set_num_threads(cores)
        P = O.to_torch_state(state, requires_grad=True)
        names = [k for k in P]
        m = {k: torch.zeros_like(v) for k, v in P.items()}
        v2 = {k: torch.zeros_like(v) for k, v in P.items()}
        tb = O.torch_batch(synthetic_batch(spec, batch, seed=99, n_classes=3))

        def step(t):
            for p in P.values():
                p.grad = None
            loss, _ = O.vault_loss(P, spec, tb)
            loss.backward()
            with torch.no_grad():
                for k in names:
                    g = P[k].grad
                    if g is not None:
                        O.hf_adamw_step(P[k], g, m[k], v2[k], 2e-5, t)

        t0 = time.time()
        step(1)
        warm = time.time() - t0
        if warm > seconds_budget:   # a pathological host: keep the warm-up step as the sample
            runs.append({"cores": cores, "batch": batch, "value": round(batch / warm, 3), "steps": 1, "seconds": round(warm, 1)})
            continue
        t0 = time.time()
        n = 0
        while True:
            step(n + 2)
            n += 1
            if time.time() - t0 > seconds_budget / 3.0 or n >= 16:
                break
        dt = time.time() - t0
        runs.append({"cores": cores, "batch": batch, "value": round(batch * n / dt, 3), "steps": n, "seconds": round(dt, 1)})
        del P, m, v2
    best = max(runs, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "samples/s", "cores": best["cores"], "kind": "port",
            "sample": f"{best['steps']} full fine-tune steps (fwd+bwd+AdamW, fp32) of the CPU oracle at batch {best['batch']}, same "
                      f"model shape and synthetic inputs; {best['seconds']} s on {best['cores']} threads "
                      f"({phys} physical cores on the box; the optimizer part is formula-pinned only: no reference AdamW "
                      f"under transformers 5.15)",
            "runs": runs}


def resident_inputs(eng, spec, bn, dev):
    """The synthetic batch `bn` resident in HBM where a data loader's copies would land - the engine's own staging buffers (no
    device-to-device re-copy per step) - with the image in the form the input pipeline delivers it: the patch-embedding GEMM's
    16-bit operand (`pixel_patches`: the unfold [B x 144, 3 x 32 x 32] that vault_image_preprocess writes straight from its
    resize kernel, here produced once from the f32 pixels by vault_im2col BEFORE the timed region).  Returns (batch with
    pixel_patches, the same batch with f32 pixel_values, labels)."""
    from vault_amd import ops
    B, T = bn["input_ids"].shape
    v = spec.vilt
    stage = eng.input_buffers(B, T, True)
    for k in ("input_ids", "pixel_values", "labels"):
        stage[k].copy_(torch.from_numpy(bn[k]).to(dev))
    with torch.cuda.device(dev), ops.operand_format(eng.half):
        ops.im2col(stage["pixel_values"], stage["pixel_patches"], B, v.num_channels, v.image_size, v.patch_size)
    rest = {k: torch.from_numpy(x).to(dev) for k, x in bn.items() if k not in ("labels", "input_ids", "pixel_values", "pixel_mask")}
    with_patches = dict(rest, input_ids=stage["input_ids"], pixel_patches=stage["pixel_patches"])
    with_pixels = dict(rest, input_ids=stage["input_ids"], pixel_values=stage["pixel_values"],
                       pixel_mask=torch.from_numpy(bn["pixel_mask"]).to(dev))
    return with_patches, with_pixels, stage["labels"]


DUMP_SAMPLE_PER_PARAM = 4096   # fp32 master-weight elements per parameter in params_sample.npy (seeded by the name)


def dump_outputs(out_dir, stepper, spec, B, T):
    """What the last timed step handed its caller, as float32 .npy files in `out_dir`: `loss` (the mean loss, [1]), `logits`
    ([B, n_classes], the step's workspace) and `params_sample` - the fp32 master weights after the step's AdamW, per parameter
    of the HF inventory in its order (vault_amd.spec.param_entries) all elements up to DUMP_SAMPLE_PER_PARAM, else that many drawn with
    a generator seeded by the parameter's name (the same elements under any flat layout; 3.5 MB at the bench shape)."""
    import zlib
    from vault_amd.spec import param_entries
    eng = stepper.engine
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize(eng.device)
    np.save(os.path.join(out_dir, "loss.npy"), stepper.loss.detach().float().cpu().numpy().reshape(1))
    np.save(os.path.join(out_dir, "logits.npy"), eng.workspace(B, T, True)["logits"].float().cpu().numpy())
    parts = []
    for name, _, _ in param_entries(spec):
        w = eng.params.w(name).reshape(-1)
        n = w.numel()
        if n > DUMP_SAMPLE_PER_PARAM:
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).integers(0, n, DUMP_SAMPLE_PER_PARAM))
            w = w[torch.from_numpy(idx).to(w.device)]
        parts.append(w.float().cpu().numpy())
    np.save(os.path.join(out_dir, "params_sample.npy"), np.concatenate(parts))


def measure_parity(eng, spec, args, dev):
    """Logits / loss of the eval-mode forward on the reference-generated golden batch (tests/golden/, B = 2, the same
    deterministic weights the bench engine holds: seed 0) - in the number format the timed steps use, and in the
    precise (split-bf16) inference mode with its throughput at the bench batch."""
    name = "full_bert_base_frozen_b2" if args.lm == "bert-base-uncased" else "full_bertweet_b2"
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    bn = synthetic_batch(spec, int(g["meta_batch"]), seed=int(g["meta_data_seed"]), n_classes=3)
    db = {k: torch.from_numpy(v).to(dev) for k, v in bn.items()}
    out = {}
    for mode, precise in (("fast", False), ("precise", True)):
        o = eng.forward(db, train=False, labels=db["labels"], need_hidden=False, precise=precise)
        torch.cuda.synchronize(dev)
        out[mode] = {"max_abs_dlogits": float(np.abs(o["logits"].cpu().numpy() - g["logits"]).max()),
                     "dloss": abs(float(o["loss"]) - float(g["loss"]))}
    return name, out


def measure_fp16(spec, args, dev, bn_bench, B, steps: int = 10, warmup: int = 3):
    """The fp16 operand build (libvault_hip_f16.so, VaultEngine(half="fp16")) on this box: (1) TRAIN-mode forward on the
    reference golden batch - the logits / loss a training step computes - against the reference's numbers; (2) the training
    throughput of that mode at the bench batch (same steps as the headline loop: tape, fused AdamW dividing the gradient
    scale out)."""
    name = "full_bert_base_frozen_b2" if args.lm == "bert-base-uncased" else "full_bertweet_b2"
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    e16 = VaultEngine(spec, dev, seed=0, freeze_lm=args.freeze_lm, classifier_dropout=0.0, half="fp16")
    import copy
    spec0 = copy.deepcopy(spec)
    spec0.lm.hidden_dropout_prob = 0.0
    spec0.lm.attention_probs_dropout_prob = 0.0
    e16.spec = spec0
    bn = synthetic_batch(spec, int(g["meta_batch"]), seed=int(g["meta_data_seed"]), n_classes=3)
    db = {k: torch.from_numpy(v).to(dev) for k, v in bn.items()}
    o = e16.forward(db, train=True, labels=db["labels"], need_hidden=False)
    torch.cuda.synchronize(dev)
    res = {"what": "IEEE fp16 MFMA operands (v_mfma_f32_16x16x32_f16, the bf16 instruction's rate), fp32 accumulate / residual / "
                   "statistics / master weights; 16-bit gradients under a static 2^12 scale divided out inside the fused AdamW; "
                   "conversions saturate at 65504 (VaultEngine(half='fp16'), bench.py --half fp16)",
           "golden": f"tests/golden/{name}.npz (reference-generated, B = 2), TRAIN-mode forward, dropout off",
           "max_abs_dlogits": round(float(np.abs(o["logits"].cpu().numpy() - g["logits"]).max()), 6),
           "dloss": round(abs(float(o["loss"]) - float(g["loss"])), 6), "north_star_tolerance": 1e-3}
    e16.spec = spec
    e16.classifier_dropout = 0.1
    e16._ws.clear()
    st = TrainStep(e16, learning_rate=2e-5, warmup_ratio=0.1, total_steps=100, assume_full_pixel_mask=True)
    b16, _, lab16 = resident_inputs(e16, spec, bn_bench, dev)
    for _ in range(warmup):
        st(b16, lab16)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        st(b16, lab16)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    res.update(train_samples_per_s=round(B * steps / dt, 2), ms_per_step=round(dt / steps * 1e3, 3), steps=steps,
               final_loss=round(float(st.loss.item()), 5))
    del st, e16, b16, lab16
    torch.cuda.empty_cache()
    return res


CONFIGS = {   # BASELINE.json `configs` (1 is the CPU plumbing case: a test, not a bench line)
    2: dict(batch=64, what="config 2: bf16 fine-tune, batch 64, 1 GPU"),
    3: dict(batch=64, what="config 3: bf16 fine-tune, global batch 64 x ranks (512 at DP = 8)"),
    4: dict(batch=128, lm="bert-base-uncased", freeze_lm=True, what="config 4: frozen bert-base-uncased LM, batch 128"),
    5: dict(batch=256, fp8_forward=True, what="config 5: MXFP8 forward GEMMs, bf16 backward, batch 256"),
    # not a BASELINE config: the single-GPU anchor of the strong-scaling reading of the metric (global batch 256
    # = 256 / N per GPU; N = 8 -> 32) - what one rank of `--scaling strong --gpus 8` computes, without the exchange
    "b32": dict(batch=32, what="per-GPU batch 32 on one GPU: the per-rank shape of --scaling strong at 8 GPUs (global batch 256)"),
}


def count_gpus_sysfs() -> int:
    """GPUs of this node WITHOUT touching the HIP runtime: KFD topology nodes with SIMDs (CPU nodes have simd_count 0),
    capped by the visibility variables.  The launcher parent forks the ranks: it must not have initialised a runtime."""
    import glob
    n = 0
    for p in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            props = dict(l.split()[:2] for l in open(p) if len(l.split()) >= 2)
        except OSError:
            continue
        if int(props.get("simd_count", "0")) > 0:
            n += 1
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip()]))
    return n


def _self_launch(n: int, argv):
    """`--gpus N` outside a torchrun environment: this process has made no GPU call (the devices are counted from sysfs) -
    it starts N fresh ranks through torch.distributed.run and exits with their code."""
    import socket
    import subprocess
    have = count_gpus_sysfs()
    if have < n:
        print(f"bench.py: --gpus {n} needs {n} devices, this node shows {have}: refusing to measure fewer ranks than asked for",
              file=sys.stderr)
        sys.exit(2)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *argv]
    sys.exit(subprocess.run(cmd).returncode)


def quick_config(cfg: int, dev, world: int, steps: int = 10, warmup: int = 3):
    """A short timed loop of another BASELINE configuration on its own engine (freed afterwards): the same step,
    inputs resident, barrier + synchronize on both sides, max over ranks."""
    c = CONFIGS[cfg]
    lm = LMSpec.bert_base_uncased() if c.get("lm") == "bert-base-uncased" else LMSpec.bertweet_base()
    spec = VaultSpec(vilt=ViltSpec(), lm=lm, n_classes=3)
    B = c["batch"]
    eng = VaultEngine(spec, dev, seed=0, freeze_lm=c.get("freeze_lm", False), classifier_dropout=0.1,
                      fp8_forward=c.get("fp8_forward", False), half="bf16")
    stepper = TrainStep(eng, learning_rate=2e-5, warmup_ratio=0.1, total_steps=steps + warmup, assume_full_pixel_mask=True)
    rank = int(os.environ.get("RANK", "0"))
    bn = synthetic_batch(spec, B, seed=1234 + rank, n_classes=3)
    batch, _, labels = resident_inputs(eng, spec, bn, dev)

    def sync_all():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(warmup):
        stepper(batch, labels)
    sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        stepper(batch, labels)
    sync_all()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    flop = 106.96e9 if c.get("freeze_lm") else FLOP_PER_SAMPLE_TRAIN
    sps = B * world * steps / dt
    out = {"what": c["what"], "value": round(sps, 2), "unit": "samples/s", "ms_per_step": round(dt / steps * 1e3, 3),
           "per_gpu_batch": B, "global_batch": B * world, "steps": steps, "warmup": warmup,
           "step_mfma_frac": round(sps / world * flop / PEAK_BF16, 4), "final_loss": round(float(stepper.loss.item()), 5)}
    del stepper, eng, batch, labels
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default 256: the metric's)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak (default, the headline): per-GPU batch fixed at --batch, global = batch x ranks; strong: GLOBAL batch "
                         "fixed at --batch (256), per-GPU batch = batch / ranks (BASELINE.md §4's second reading of 'bs256')")
    ap.add_argument("--config", type=int, default=None, choices=sorted(k for k in CONFIGS if isinstance(k, int)),
                    help="a BASELINE.json configuration as the timed workload (sets batch / LM / freeze / fp8 as it states)")
    ap.add_argument("--wire", default=None, choices=["fp32", "bf16"],
                    help="data-parallel gradient wire format (default fp32 all-reduce; bf16 = reduce-scatter + all-gather "
                         "with bf16 on the wire, f32 accumulation)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short loops of the other BASELINE configurations (`other_configs`)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--freeze-lm", action="store_true")
    ap.add_argument("--fp8-forward", action="store_true",
                    help="BASELINE config 5: MXFP8 forward Linear GEMMs (block-scaled fp8 MFMA), bf16 backward")
    ap.add_argument("--lm", default="bertweet", choices=["bertweet", "bert-base-uncased"])
    ap.add_argument("--half", default="bf16", choices=["bf16", "fp16"],
                    help="16-bit operand format of the timed steps (default bf16: BASELINE's; fp16 = libvault_hip_f16.so, the "
                         "format whose training step is inside the 1e-3 tolerance - also measured beside the bf16 line, "
                         "`parity.fp16_operands`)")
    ap.add_argument("--no-parity", action="store_true", help="skip the golden-batch parity measurement and the precise-mode timing")
    ap.add_argument("--no-h2d", action="store_true", help="skip the second timed loop with pipelined host->device input copies")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: live kernel timing (roofline, blocks), parity, the other input forms, wire format "
                         "and configurations, cpu_baseline (the --no-* options apply to this); off: the timed steps only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32, rank 0)")
    args = ap.parse_args()
    if args.config is not None:
        c = CONFIGS[args.config]
        args.batch = args.batch or c["batch"]
        args.lm = c.get("lm", args.lm)
        args.freeze_lm = args.freeze_lm or c.get("freeze_lm", False)
        args.fp8_forward = args.fp8_forward or c.get("fp8_forward", False)
    args.batch = args.batch or 256

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        _self_launch(args.gpus, sys.argv[1:])          # (never returns)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    if local_rank >= torch.cuda.device_count():
        print(f"bench.py: rank {rank} needs device {local_rank}, this node shows {torch.cuda.device_count()}", file=sys.stderr)
        sys.exit(2)
    dev = torch.device(f"cuda:{local_rank}")
    torch.cuda.set_device(dev)
    pg = None
    if world > 1 or os.environ.get("VAULT_FORCE_DP") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        if dist.get_world_size() != world:
            raise RuntimeError(f"RCCL reports {dist.get_world_size()} ranks, expected {world}")

    lm = LMSpec.bertweet_base() if args.lm == "bertweet" else LMSpec.bert_base_uncased()
    spec = VaultSpec(vilt=ViltSpec(), lm=lm, n_classes=3)
    eng = VaultEngine(spec, dev, seed=0, freeze_lm=args.freeze_lm, classifier_dropout=0.1, fp8_forward=args.fp8_forward,
                      half=args.half)
    total = args.steps + args.warmup
    stepper = TrainStep(eng, learning_rate=2e-5, warmup_ratio=0.1, total_steps=max(total, 10), process_group=pg,
                       assume_full_pixel_mask=True,   # synthetic 384x384 images, all-ones masks: no per-step mask check
                       wire=args.wire)

    B = args.batch
    if args.scaling == "strong":
        if args.batch % world:
            raise SystemExit(f"--scaling strong: the global batch {args.batch} does not divide over {world} ranks")
        B = args.batch // world
    parity = None
    if args.full and rank == 0 and not args.no_parity:
        gname, par = measure_parity(eng, spec, args, dev)
        parity = {"golden": f"tests/golden/{gname}.npz (reference-generated, B = 2, eval mode)",
                  "mode": ("mxfp8 forward GEMMs" if args.fp8_forward else f"{args.half} MFMA operands, fp32 accumulate (the timed mode)"),
                  "max_abs_dlogits": round(par["fast"]["max_abs_dlogits"], 6), "dloss": round(par["fast"]["dloss"], 6),
                  "north_star_tolerance": 1e-3,
                  "precise_mode": {"what": "split-bf16 (bf16x3) forward GEMMs: fp32-class products on the bf16 MFMA path - as an inference "
                                           "mode, and as a training mode (TrainStep(precise_forward=True): this forward + the bf16 "
                                           "backward; precise_forward_train_samples_per_s)",
                                   "max_abs_dlogits": round(par["precise"]["max_abs_dlogits"], 6),
                                   "dloss": round(par["precise"]["dloss"], 6)}}
    bn = synthetic_batch(spec, B, seed=1234 + rank, n_classes=3)
    # inputs are resident in HBM before the timed region, the image as the patch-embedding GEMM's operand (resident_inputs);
    # `with_f32_pixel_values` below times the same steps from f32 pixels (the unfold pass inside the step)
    batch, batch_pix, labels = resident_inputs(eng, spec, bn, dev)

    # live timing of the dominant kernels: event pairs on the launch stream around their launches, in every 4th
    # timed step (an event pair costs ~1-2 us of stream time: sampling keeps `value` undisturbed)
    # ... and of the two encoder stacks as blocks (the north star's own target metric): one pair around each stack's forward
    # layer loop, one around its backward layer loop including the stack's weight-gradient launches
    evs = {"wgrad": [], "ffn1": [], "vilt_fwd": [], "vilt_bwd": [], "lm_fwd": [], "lm_bwd": []}
    eng.profile_events = None

    def sync_all():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        stepper(batch, labels)
    sync_all()
    step_ev = []          # one event pair per timed step on the launch stream: the median beside the mean
    t0 = time.perf_counter()
    for k in range(args.steps):
        eng.profile_events = evs if (args.full and k % 4 == 0) else None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        stepper(batch, labels)
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        step_ev.append((e0, e1))
    sync_all()
    dt = time.perf_counter() - t0
    eng.profile_events = None
    loss = float(stepper.loss.item())
    step_ms = sorted(a.elapsed_time(b) for a, b in step_ev)
    ms_median = step_ms[len(step_ms) // 2] if len(step_ms) % 2 else 0.5 * (step_ms[len(step_ms) // 2 - 1] + step_ms[len(step_ms) // 2])
    if args.dump_outputs and rank == 0:
        # (before the --full loops below step the same weights further)
        dump_outputs(args.dump_outputs, stepper, spec, B, int(bn["input_ids"].shape[1]))

    ms_by_rank = [round(dt / args.steps * 1e3, 3)]
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        allt = [torch.zeros_like(t) for _ in range(world)]
        torch.distributed.all_gather(allt, t)
        ms_by_rank = [round(float(x.item()) / args.steps * 1e3, 3) for x in allt]
        dt = max(float(x.item()) for x in allt)          # MAX over ranks
    exchange = None
    if stepper.reducer is not None:
        dense = 2 * 4 * eng.params.n_train * (world - 1) // max(world, 1)
        exchange = {"wire": stepper.wire, "sparse_word_embedding": stepper.reducer.sparse is not None,
                    "bytes_sent_per_rank_and_step": int(stepper.reducer.wire_bytes),
                    "dense_f32_all_reduce_would_send": int(dense), "rccl_world_size": torch.distributed.get_world_size()}
        if args.full and (world > 1 or os.environ.get("VAULT_FORCE_DP") == "1"):
            # the OTHER wire format on the same ranks, a short loop (the reducer reads its format at every launch: no
            # re-recording): informational - `value` above is the configured format's
            other = "bf16" if stepper.wire == "fp32" else "fp32"
            stepper.reducer.wire = other
            for _ in range(3):
                stepper(batch, labels)
            sync_all()
            t0 = time.perf_counter()
            n_o = max(4, args.steps // 2)
            for _ in range(n_o):
                stepper(batch, labels)
            sync_all()
            t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            exchange["other_wire"] = {"wire": other, "ms_per_step": round(float(t.item()) / n_o * 1e3, 3),
                                      "value": round(B * world * n_o / float(t.item()), 2),
                                      "bytes_sent_per_rank_and_step": int(stepper.reducer.wire_bytes)}
            stepper.reducer.wire = stepper.wire

    # ---- the same steps from f32 pixel_values resident in HBM (the reference's input tensor: the unfold pass - 0.68 GB of HBM
    #      traffic at batch 256 - runs inside the step); a short loop, informational
    f32pix = None
    if args.full and not args.no_h2d:
        n_p = max(4, args.steps // 2)
        for _ in range(2):
            stepper(batch_pix, labels)
        sync_all()
        t0 = time.perf_counter()
        for _ in range(n_p):
            stepper(batch_pix, labels)
        sync_all()
        tpx = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        if world > 1:
            torch.distributed.all_reduce(tpx, op=torch.distributed.ReduceOp.MAX)
        f32pix = {"value": round(B * world * n_p / float(tpx.item()), 2), "ms_per_step": round(float(tpx.item()) / n_p * 1e3, 3),
                  "steps": n_p, "what": "the same steps fed from f32 pixel_values [B, 3, 384, 384] resident in HBM: vault_im2col "
                  "(f32 -> 16-bit unfold) runs inside every step"}

    # ---- second loop: the same K steps with the input copies inside the loop (ref: tmsc_utils/trainer.py:183-202,353
    #      batch_to_device): a fresh host batch per step from pinned memory.  Round 6: the f32 pixels (453 MB, all but 30 KB of a
    #      batch) are copied host -> device on a side stream STRAIGHT INTO the engine's staging buffer (input_buffers(): staging
    #      then copies nothing) as soon as the running step has unfolded them - the engine records `pixels_consumed` behind its
    #      im2col - so the next batch travels under the rest of the current step; ids / masks / labels (read until the end of a
    #      step) go through two small device buffers and the engine's own restage
    h2d = None
    if args.full and not args.no_h2d:
        nb = 2
        host = []
        for i in range(nb):
            hb = synthetic_batch(spec, B, seed=4321 + 7 * rank + i, n_classes=3)
            host.append({k: torch.from_numpy(v).pin_memory() for k, v in hb.items() if k in ("input_ids", "attention_mask", "pixel_values", "pixel_mask", "labels")})
        small = ("input_ids", "attention_mask", "pixel_mask", "labels")
        devb = [{k: torch.empty_like(host[0][k], device=dev) for k in small} for _ in range(nb)]
        T = int(bn["input_ids"].shape[1])
        pix_stage = eng.input_buffers(B, T)["pixel_values"]
        copy_stream = torch.cuda.Stream(device=dev)
        ready = [torch.cuda.Event() for _ in range(nb)]
        consumed = [torch.cuda.Event() for _ in range(nb)]

        def prefetch(k, pix_free):
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(consumed[k % nb])
                for name in small:
                    devb[k % nb][name].copy_(host[k % nb][name], non_blocking=True)
                copy_stream.wait_event(pix_free)          # (the step that reads the staging buffer has unfolded its pixels)
                pix_stage.copy_(host[k % nb]["pixel_values"], non_blocking=True)
                ready[k % nb].record(copy_stream)

        def run(k):
            d = devb[k % nb]
            stepper({"input_ids": d["input_ids"], "attention_mask": d["attention_mask"], "pixel_values": pix_stage,
                     "pixel_mask": d["pixel_mask"]}, d["labels"])
            consumed[k % nb].record(torch.cuda.current_stream(dev))

        for i in range(nb):
            consumed[i].record(torch.cuda.current_stream(dev))
        start = torch.cuda.Event(); start.record(torch.cuda.current_stream(dev))
        prefetch(0, start)
        torch.cuda.current_stream(dev).wait_event(ready[0])
        run(0)                                            # (untimed: records / finds the tape of the pixel_values form)
        pix_free = eng.workspace(B, T, True)["pixels_consumed"]
        prefetch(1, pix_free)
        sync_all()
        t0 = time.perf_counter()
        for k in range(1, args.steps + 1):
            torch.cuda.current_stream(dev).wait_event(ready[k % nb])
            run(k)                                        # (enqueues the step: its im2col is followed by the event's record)
            if k < args.steps:
                prefetch(k + 1, pix_free)                 # the next batch: waits for THAT record on the copy stream
        sync_all()
        dt2 = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt2], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt2 = float(t.item())
        h2d = {"value": round(B * world * args.steps / dt2, 2), "ms_per_step": round(dt2 / args.steps * 1e3, 3),
               "what": "the same steps with a fresh pinned host batch per step: the f32 pixels copied host->device on a side stream "
                       "straight into the engine's staging buffer behind the running step's unfold (no device-to-device restage; "
                       "overlapped with the rest of that step), ids / masks / labels through two small buffers; the unfold "
                       "(vault_im2col) runs inside every step"}

    # ---- third loop: the input pipeline from uint8 images: per step a pinned host batch of 8-bit RGB images
    #      (480 x 480, what a JPEG decoder leaves) is copied host->device on the side stream (177 MB instead of 453 MB of
    #      float pixels) and resized / normalised / padded THERE by vault_image_preprocess straight into the double-buffered
    #      device batch - what HuggingFace's processor does per item on CPU workers in the reference
    #      (ref: vault/models/vault/dataset.py:337-341), bit-identically (tests/test_gpu_preprocess.py)
    u8 = None
    if args.full and not args.no_h2d and not args.fp8_forward:
        from vault_amd.preprocess import DeviceImageProcessor
        proc = DeviceImageProcessor(dev)
        HW = 480
        rng = np.random.default_rng(99 + rank)
        himg = [torch.from_numpy(rng.integers(0, 256, size=(B, HW, HW, 3), dtype=np.uint8)).pin_memory() for _ in range(nb)]
        sizes = [(HW, HW)] * B

        # the resize kernel writes the patch-embedding GEMM's bf16 operand itself (no f32 pixel tensor, no unfold pass)
        Kp = spec.vilt.num_channels * spec.vilt.patch_size ** 2
        devp = [torch.empty(B * spec.vilt.num_patches, Kp, dtype=eng.hdt, device=dev) for _ in range(nb)]

        def prefetch_u8(k):
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(consumed[k % nb])
                for name in ("input_ids", "attention_mask", "labels"):
                    devb[k % nb][name].copy_(host[k % nb][name], non_blocking=True)
                proc.from_packed(himg[k % nb].view(-1), sizes, patch_out=devp[k % nb], patch_size=spec.vilt.patch_size,
                                 want_mask=False)           # (fully valid 384 x 384 canvases: the engine needs no mask)
                ready[k % nb].record(copy_stream)

        for i in range(nb):
            consumed[i].record(torch.cuda.current_stream(dev))
        # the resize kernel's output IS the patch GEMM's operand: the recorded step re-points its two launches at this step's
        # tensor instead of copying it into the engine's buffer (VaultEngine.adopt_pixel_patches)
        eng.adopt_pixel_patches = True
        prefetch_u8(0)
        d = devb[0]
        for k in range(2):            # (the step with this input form records its own tape: outside the timed region)
            torch.cuda.current_stream(dev).wait_event(ready[0])
            stepper({"input_ids": d["input_ids"], "attention_mask": d["attention_mask"], "pixel_patches": devp[0]}, d["labels"])
        sync_all()
        t0 = time.perf_counter()
        for k in range(args.steps):
            if k + 1 < args.steps:
                prefetch_u8(k + 1)
            torch.cuda.current_stream(dev).wait_event(ready[k % nb])
            d = devb[k % nb]
            stepper({"input_ids": d["input_ids"], "attention_mask": d["attention_mask"], "pixel_patches": devp[k % nb]}, d["labels"])
            consumed[k % nb].record(torch.cuda.current_stream(dev))
        sync_all()
        dt3 = time.perf_counter() - t0
        eng.adopt_pixel_patches = False
        if world > 1:
            t = torch.tensor([dt3], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt3 = float(t.item())
        u8 = {"value": round(B * world * args.steps / dt3, 2), "ms_per_step": round(dt3 / args.steps * 1e3, 3),
              "what": f"the same steps fed from pinned uint8 images ({HW} x {HW} x 3 per sample, {B * HW * HW * 3 / 1e6:.0f} MB per step): "
                      "host->device copy + GPU resize / normalise / pad (vault_image_preprocess, bit-identical to the HF ViLT "
                      "processor; both passes in one launch, the 8-bit intermediate in LDS) on a side stream, double-buffered, "
                      "overlapped with the previous step; the resize kernel writes the patch-embedding GEMM's bf16 operand directly "
                      "(no f32 pixel tensor, no unfold pass, no pixel mask) and the step's GEMMs read it where it was written "
                      "(no restage copy)"}

    precise_fwd = None
    if args.full and rank == 0 and not args.no_parity and not args.fp8_forward:
        # throughput of the mode that meets the north star's 1e-3: eval forward, split-bf16 GEMMs, at the bench batch
        ev = dict(batch_pix)       # (the split-bf16 mode splits f32 pixels: it takes pixel_values)
        for _ in range(2):
            eng.forward(ev, train=False, need_hidden=False, precise=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(5):
            eng.forward(ev, train=False, need_hidden=False, precise=True)
        torch.cuda.synchronize(dev)
        tp = (time.perf_counter() - t0) / 5
        for _ in range(2):
            eng.forward(ev, train=False, need_hidden=False)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(5):
            eng.forward(ev, train=False, need_hidden=False)
        torch.cuda.synchronize(dev)
        tf = (time.perf_counter() - t0) / 5
        precise_fwd = {"precise_forward_samples_per_s": round(B / tp, 1), "fast_forward_samples_per_s": round(B / tf, 1),
                       "batch": B}
        if world == 1:
            # ... and as a TRAINING mode: split-bf16 forward GEMMs (logits / loss of the step inside 1e-3), bf16 backward
            pstep = TrainStep(eng, learning_rate=2e-5, warmup_ratio=0.1, total_steps=100, assume_full_pixel_mask=True,
                              precise_forward=True)
            for _ in range(2):
                pstep(batch_pix, labels)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(5):
                pstep(batch_pix, labels)
            torch.cuda.synchronize(dev)
            precise_fwd["precise_forward_train_samples_per_s"] = round(B * 5 / (time.perf_counter() - t0), 1)
            del pstep

    # ---- the fp16 operand build beside the bf16 line (same box, same batch, same steps): TRAIN-mode logits / loss on the
    #      reference golden and the training throughput of that mode
    fp16_line = None
    if args.full and rank == 0 and world == 1 and not args.no_parity and not args.fp8_forward and args.half == "bf16":
        try:
            fp16_line = measure_fp16(spec, args, dev, bn, B, steps=args.steps, warmup=args.warmup)
            # the bf16 steps once more, right behind the fp16 loop (same clock / thermal state of the box: the headline loop ran
            # minutes earlier, and a box's clock under load drifts by 1-2 % over a bench run)
            for _ in range(args.warmup):
                stepper(batch, labels)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                stepper(batch, labels)
            torch.cuda.synchronize(dev)
            fp16_line["bf16_right_after_samples_per_s"] = round(B * args.steps / (time.perf_counter() - t0), 2)
            fp16_line["ratio_to_bf16_right_after"] = round(fp16_line["train_samples_per_s"] / fp16_line["bf16_right_after_samples_per_s"], 4)
        except Exception as e:  # pragma: no cover
            fp16_line = {"error": repr(e)}

    # ---- the other BASELINE configurations, each a short loop on its own engine (rank 0 prints them in `other_configs`):
    #      per-GPU batch 64 (config 2 on one GPU, config 3's per-GPU shape on N), and on one GPU the frozen-LM and fp8-forward ones
    others = None
    if args.full and not args.no_other_configs and args.config is None and B == 256 and args.lm == "bertweet" \
            and not args.freeze_lm and not args.fp8_forward:
        del stepper
        eng._ws.clear()
        torch.cuda.empty_cache()
        others = {}
        for cfg in ((2, 4, 5, "b32") if world == 1 else (3,)):
            okey = f"config{cfg}" if isinstance(cfg, int) else f"batch_{cfg[1:]}"
            try:
                others[okey] = quick_config(cfg, dev, world)
            except Exception as e:  # pragma: no cover
                others[okey] = {"error": repr(e)}

    if rank == 0:
        sps = B * world * args.steps / dt
        v = spec.vilt
        M = B * (40 + 1 + v.num_patches)
        flop_per_sample = FLOP_PER_SAMPLE_TRAIN if not args.freeze_lm else 106.96e9

        def roof(site, kernel, pmc_file):
            """achieved = algorithmic FLOPs of all timed launches / the sum of their durations"""
            ms = [s_.elapsed_time(e_) for s_, e_, _ in evs[site]]
            fl = [f for _, _, f in evs[site]]
            if not ms:
                return {"bound": "mfma", "kernel": kernel, "achieved": None, "peak": 2500.0, "unit": "TFLOP/s",
                        "frac": None, "traffic": None, "launches_timed": 0}
            achieved = sum(fl) / (sum(ms) * 1e-3) / 1e12
            # HBM/fabric bytes of that kernel from PMC counters (separate rocprofv3 --pmc passes, committed under
            # profiles/: FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE), average per launch; only for the profiled batch
            traffic = None
            traffic_src = None
            try:
                pm = json.load(open(os.path.join(ROOT, "profiles", pmc_file)))
                if pm.get("batch") == B and pm.get("lm") == args.lm and not args.freeze_lm:
                    traffic = pm["traffic_bytes_per_launch_avg"]
                    traffic_src = f"profiles/{pmc_file} (separate rocprofv3 --pmc passes of this workload; not measured in this run)"
            except Exception:
                traffic = None
            return {"bound": "mfma", "kernel": kernel, "flop_per_launch_avg": round(float(np.mean(fl)) / 1e9, 2),
                    "achieved": round(achieved, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(achieved / 2500.0, 4),
                    "traffic": traffic, "traffic_source": traffic_src, "launches_timed": len(ms),
                    "avg_launch_ms": round(float(np.mean(ms)), 4)}

        def block(fwd_site, bwd_site, flop_fwd, what):
            """A stack's layers as one block: algorithmic FLOPs (forward x 3 when its backward runs) over the event-timed
            duration of its forward + backward layer loops (backward: data gradients, attention / LayerNorm backward AND the
            stack's weight-gradient launches), against the dense bf16 peak."""
            tf = [a.elapsed_time(b) for a, b, _ in evs[fwd_site]]
            tb = [a.elapsed_time(b) for a, b, _ in evs[bwd_site]]
            if not tf:
                return None
            trained = bool(tb)
            if trained and eng._wgrad_side:       # (small batches: weight gradients on a second stream - the pair would miss them)
                return {"what": what, "frac": None, "why": "deferred weight gradients run on a second stream at this batch"}
            ms_f, ms_b = float(np.mean(tf)), (float(np.mean(tb)) if trained else 0.0)
            fl = B * flop_fwd * (3.0 if trained else 1.0)
            return {"what": what, "ms_forward": round(ms_f, 3), "ms_backward": round(ms_b, 3) if trained else None,
                    "gflop_per_sample": round(fl / B / 1e9, 2), "achieved_tflops": round(fl / ((ms_f + ms_b) * 1e-3) / 1e12, 1),
                    "frac": round(fl / ((ms_f + ms_b) * 1e-3) / PEAK_BF16, 4), "steps_timed": len(tf)}

        live = {}           # (--full: the kernels and blocks timed live in every 4th step)
        if args.full:
            blk_vilt = block("vilt_fwd", "vilt_bwd", FLOP_VILT_BLOCK_FWD,
                             f"12 ViLT layers (HF modeling_vilt.py:303-451), {M} token rows: LayerNorms, QKV / attention-out / FFN GEMMs, "
                             "attention, their data gradients, attention / LayerNorm backward and the stack's weight-gradient launches")
            blk_lm = block("lm_fwd", "lm_bwd", FLOP_LM_BLOCK_FWD,
                           f"12 LM layers (HF modeling_roberta.py:222-398), {B * 40} token rows, "
                           + ("forward only (frozen LM)" if args.freeze_lm else "forward + backward + weight gradients"))
            r_wgrad = roof("wgrad", "gemm256_kernel<1,1,5,4,false,false> (static tile walk, no split-K form; A[K][M]^T B[K][N], EPI_F32_ATOMIC): the weight-gradient GEMMs, "
                                    f"dW[N x K] += dY[tokens][N]^T X[tokens][K] - grouped launches (vault_wgrad_grouped): the 256 x 256 tiles "
                                    f"of all four Linear kinds (FFN-out, FFN-in, attention-out, QKV) of a stack's layers packed into "
                                    f"rounds of 256 ({M} ViLT tokens / {B * 40} LM tokens per layer), and the patch projection",
                           "r06_pmc_gemm_wgrad.json")
            r_ffn1 = roof("ffn1", "gemm8w_kernel<7,4,true> / <1,4,true> (GELU epilogue with the 8-bit tile-native / bf16 gelu', 256-wide tiles, register-direct): FFN-in forward, ViLT "
                                  f"[{M}x{v.intermediate_size}x{v.hidden_size}] + LM [{B * 40}x{v.intermediate_size}x{v.hidden_size}]",
                          "r06_pmc_gemm_ffn1.json")
            live = {"roofline": r_wgrad, "roofline_ffn1": r_ffn1,
                    "vilt_block_frac": None if blk_vilt is None else blk_vilt["frac"],
                    "lm_block_frac": None if blk_lm is None else blk_lm["frac"],
                    "blocks": {"vilt": blk_vilt, "lm": blk_lm}}
        out = {
            "metric": "train samples/sec (img+text pairs) ViLT-B32+BERTweet, bs256, 1/2/4/8 MI355X",
            "value": round(sps, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "ms_per_step_median": round(ms_median, 3),
            "ms_per_step_min_max": [round(step_ms[0], 3), round(step_ms[-1], 3)],
            "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "mxfp8 forward GEMMs / bf16 backward" if args.fp8_forward else args.half,
            "value_input_form": "since round 5 the image is resident as `pixel_patches` (the patch-embedding operand, what the input "
                                "pipeline writes); rounds 1-4 timed f32 `pixel_values` with the unfold inside the step - that form is "
                                "`with_f32_pixel_values` in the --full line (0.3 % apart)",
            "data": "synthetic",
            "config": {"workload": f"ViLT-B32 + {args.lm} fine-tune step (fwd+bwd+AdamW), per-GPU batch {B}, "
                                   f"40 text tokens + 384x384 image (185-token fused sequence; resident as the patch-embedding "
                                   f"operand `pixel_patches`, the input pipeline's output), "
                                   f"{'frozen LM' if args.freeze_lm else 'all weights trained'}"
                                   f"{', MXFP8 forward Linears' if args.fp8_forward else ''}",
                       "global_batch": B * world, "seq_len": 185, "parallelism": f"dp{world}",
                       **({"baseline_config": args.config} if args.config is not None else {})},
            "ms_per_step_by_rank": ms_by_rank,
            "step_mfma_frac": round(sps / world * flop_per_sample / PEAK_BF16, 4),
            **live,
            "final_loss": round(loss, 5),
        }
        if exchange is not None:
            out["gradient_exchange"] = exchange
        if others is not None:
            out["other_configs"] = others
        if parity is not None:
            if fp16_line is not None:
                if "train_samples_per_s" in fp16_line:
                    fp16_line["ratio_to_the_bf16_line"] = round(fp16_line["train_samples_per_s"] / sps, 4)
                parity["fp16_operands"] = fp16_line
            if precise_fwd is not None:
                parity["precise_mode"].update(precise_fwd)
            out["parity"] = parity
        if f32pix is not None:
            out["with_f32_pixel_values"] = f32pix
        if h2d is not None:
            out["with_h2d_input_copies"] = h2d
        if u8 is not None:
            out["with_uint8_input_pipeline"] = u8
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                out["cpu_baseline"] = cpu_baseline(spec)
            except Exception as e:  # pragma: no cover
                out["cpu_baseline"] = {"error": repr(e)}
        # librccl prints its version banner through C stdio, which a redirected stdout only flushes at exit - after
        # this line.  Flush it first: the JSON line must be the last thing on stdout.
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:  # pragma: no cover
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
