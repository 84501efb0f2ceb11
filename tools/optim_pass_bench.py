"""Cost of an optimizer option inside the optimizer's pass (a record, not a gate).

    python tools/optim_pass_bench.py {ema,torch} [--launches 30] [--warmup 5] [--half bf16] [--out profiles/<form's file>]

``ema``: vault_adamw_step_ema, ``torch``: vault_adamw_step_torch (without the weight average) - each against
vault_adamw_step_grouped of the same build, in one process on one device, on flat buffers of the full trainable size of
ViLT-B/32 + BERTweet-base (ParamStore.layout: about 222 M f32 elements), one group with weight decay.  Every timed launch gets a
fresh non-zero gradient first (a device copy outside the timed window), so no element is idle and both kernels store everything
they can: 34 B per parameter for the grouped kernel and the torch form (which adds two multiplies per element - the decay factor,
the corrected root - to a pass bound by memory), 42 B with the average (+1 B per 64 elements of group map).  The two kernels
alternate launch by launch; each launch is timed by its own pair of device events; the medians, their ratio and the achieved
bytes per second go to --out.  The allowance: ``ema`` 1.1 times the byte ratio (the sixth stream), ``torch`` 1.05 times the grouped
kernel's median.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vault_amd import ops                                                             # noqa: E402
from vault_amd.optim import adam_bias_corrections                                     # noqa: E402
from vault_amd.params import ParamStore                                               # noqa: E402
from vault_amd.spec import LMSpec, VaultSpec, ViltSpec                                # noqa: E402

BYTES_GROUPED = 34      # per parameter: loads p g m v, stores p m v, the gradient's zero, the shadow
# form -> (kernel, its bytes per parameter (ema: + load and store of e), output file, what the header says of the group)
FORMS = {"ema": ("adamw_step_ema", 42, "ema_optimizer_pass.txt", "one group"),
         "torch": ("adamw_step_torch", 34, "torch_adamw_optimizer_pass.txt", "one group with decay")}
TORCH_ALLOWANCE = 1.05


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("form", choices=sorted(FORMS))
    ap.add_argument("--launches", type=int, default=30, help="timed launches per kernel (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--half", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--out", default=None, help="default: the form's file under profiles/")
    a = ap.parse_args()
    kernel, kbytes, out_name, group_text = FORMS[a.form]
    out = a.out or os.path.join(ROOT, "profiles", out_name)
    if not torch.cuda.is_available():
        raise SystemExit("optim_pass_bench.py times GPU kernels: no GPU visible")
    launches = max(20, a.launches)
    spec = VaultSpec(vilt=ViltSpec(), lm=LMSpec.bertweet_base(), n_classes=3)
    n = ParamStore.layout(spec).n_train
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=gen) * 0.02
    g_src = torch.randn(n, device=dev, generator=gen) * 1e-3
    g_src[g_src == 0] = 1e-3
    g = torch.empty_like(g_src)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = p.to(ops.HALF_DTYPE[a.half])
    gmap = torch.zeros(n // 64, dtype=torch.uint8, device=dev)
    table = torch.tensor([[2e-5, 0.01]], dtype=torch.float32, device=dev)
    fns = {"adamw_step_grouped": lambda: ops.adamw_step_grouped(p, g, m, v, pb, n, gmap, table, 1.0, 0.9, 0.999, 1e-8,
                                                                 grad_scale=1.0, zero_grad=True)}
    if a.form == "ema":
        ema = p.clone()
        omd = 1.0 - 0.999
        fns[kernel] = lambda: ops.adamw_step_ema(p, g, m, v, pb, ema, n, gmap, table, 1.0, 0.9, 0.999, 1e-8, omd,
                                                 grad_scale=1.0, zero_grad=True)
    else:
        inv_bc1, inv_sqrt_bc2 = adam_bias_corrections(0.9, 0.999, 100)
        fns[kernel] = lambda: ops.adamw_step_torch(p, g, m, v, pb, n, gmap, table, 1.0, 0.9, 0.999, 1e-8, inv_bc1,
                                                   inv_sqrt_bc2, grad_scale=1.0, zero_grad=True)
    times = {k: [] for k in fns}
    with ops.operand_format(a.half):
        for it in range(a.warmup + launches):
            for k, f in fns.items():
                g.copy_(g_src)                                   # (the pass zeroes it: fresh gradients, outside the window)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)   # us
    assert not bool(g.any()) and bool(torch.isfinite(p).all())
    assert not torch.equal(ema, p) if a.form == "ema" else bool(v.all())
    us = {k: median(x) for k, x in times.items()}
    per_param = {"adamw_step_grouped": BYTES_GROUPED, kernel: kbytes}
    nbytes = {k: b * n + n // 64 for k, b in per_param.items()}
    ratio = us[kernel] / us["adamw_step_grouped"]
    lines = [f"tools/optim_pass_bench.py {a.form}: {torch.cuda.get_device_name(0)}, {a.half} build, n = {n:,} f32 parameters, "
             f"{group_text}, no idle element, {launches} alternating launches per kernel after {a.warmup} warm-up rounds, one event "
             "pair per launch",
             f"{'kernel':<22}{'median us':>12}{'min us':>10}{'max us':>10}{'B/param':>9}{'GB moved':>10}{'TB/s':>8}"]
    for k in fns:
        lines.append(f"{k:<22}{us[k]:>12.1f}{min(times[k]):>10.1f}{max(times[k]):>10.1f}{per_param[k]:>9}{nbytes[k] / 1e9:>10.3f}"
                     f"{nbytes[k] / (us[k] * 1e-6) / 1e12:>8.2f}")
    if a.form == "ema":
        byte_ratio = nbytes[kernel] / nbytes["adamw_step_grouped"]
        lines.append(f"time ratio ema / grouped = {ratio:.3f}; byte ratio = {byte_ratio:.3f}; time ratio / byte ratio = "
                     f"{ratio / byte_ratio:.3f} ({'within' if ratio <= 1.1 * byte_ratio else 'ABOVE'} the 1.1 allowance for the sixth "
                     "stream)")
    else:
        lines.append(f"time ratio torch / grouped = {ratio:.3f} at the same bytes ({'within' if ratio <= TORCH_ALLOWANCE else 'ABOVE'} "
                     f"the {TORCH_ALLOWANCE} allowance)")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
