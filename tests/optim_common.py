"""What the optimizer tests share (tests/test_*optim*_host.py, test_ema_host.py and their test_gpu_* counterparts): the float32
helpers, the float64 recurrence of the weight average with its bound, the tiny model's spec / engine / batch, and the stub engine
of the host tests.  A plain module: no fixtures, no hooks."""
import types

import numpy as np
import torch

from vault_amd.engine import VaultEngine
from vault_amd.params import ParamStore
from vault_amd.spec import VaultSpec, build_state, synthetic_batch

U = 2.0 ** -24                     # unit roundoff of f32


def _f32(x: float) -> float:
    return float(np.float32(x))


class _Recurrence:
    """e <- e + (1 - d)(p - e) in float64 over the device's own p after each step, and the bound on the kernel's f32 result:
    a step rounds the subtraction (|p - e| <= 2 max(|p|, |e|), weighted by 1 - d <= 1), the product and the add - at most
    4 x 2^-24 x max(|p|, |e|) with the slack of a whole rounding - and carries the earlier error on at weight d <= 1:
    atol = 4 T 2^-24 max(|p|, |e|) after T steps, the magnitudes taken over all steps so far."""

    def __init__(self, e0: torch.Tensor):
        self.e = e0.double().clone()
        self.mag = self.e.abs()
        self.T = 0

    def step(self, p: torch.Tensor, one_minus_decay: float):
        p = p.double()
        self.mag = torch.maximum(self.mag, p.abs())
        self.e = self.e + one_minus_decay * (p - self.e)
        self.mag = torch.maximum(self.mag, self.e.abs())
        self.T += 1

    def check(self, ema: torch.Tensor, what=""):
        err = (ema.double() - self.e).abs()
        tol = 4.0 * self.T * U * self.mag
        over = err > tol
        worst = float((err / tol.clamp_min(1e-300)).max())
        print(f"ema vs float64 recurrence {what}: T = {self.T}, max err {float(err.max()):.3e}, max err / bound {worst:.3f}")
        assert not bool(over.any()), (what, int(over.sum()), worst)


def _tiny():
    spec = VaultSpec.tiny(3, "roberta")
    spec.lm.hidden_dropout_prob = 0.0; spec.lm.attention_probs_dropout_prob = 0.0
    return spec


def _engine(spec, state=None, half="bf16"):
    return VaultEngine(spec, "cuda:0", state=build_state(spec, 0) if state is None else state, classifier_dropout=0.0,
                       half=half)


def _batch(spec, seed, B=4):
    bn = synthetic_batch(spec, B, seed=seed, n_classes=3)
    return bn, {k: torch.from_numpy(v).cuda() for k, v in bn.items() if k != "labels"}, torch.from_numpy(bn["labels"]).cuda()


def _stub_engine(layout=None):
    """What TrainStep reads before it touches a device: the parameter layout (its checks run first); the tiny RoBERTa model's
    by default."""
    layout = ParamStore.layout(VaultSpec.tiny(3, "roberta")) if layout is None else layout
    return types.SimpleNamespace(params=layout, device="cpu", spec=None)
