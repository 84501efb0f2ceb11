"""Gradient-norm clipping and parameter groups of the fused train step on the GPU: the norm kernel, the grouped AdamW kernel
(both operand formats), TrainStep against the fp32 oracle, data parallelism, and the unchanged default path."""
import math

import numpy as np
import pytest
import torch

from oracle import vault_oracle as O
from tests.optim_common import _tiny
from vault_amd import ops
from vault_amd.engine import VaultEngine
from vault_amd.spec import VaultSpec, build_state, synthetic_batch
from vault_amd.train import TrainStep, hf_no_decay_groups, no_decay_parameter_names

pytestmark = pytest.mark.gpu


def _norm(g, max_norm=math.inf, unscale=1.0):
    out = torch.full((2,), -1.0, device="cuda")
    parts = torch.empty(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device="cuda")
    ops.grad_norm(g, g.numel(), parts, out, max_norm, unscale)
    return out


def _torch_coef(norm32, max_norm):
    """torch.nn.utils.clip_grad_norm_'s factor from a float32 norm, with torch's own f32 arithmetic."""
    return torch.clamp(max_norm / (norm32 + 1e-6), max=1.0)


@pytest.mark.parametrize("n", [4, 1024, 2048 * 256 * 4 + 4 * 37, 2048 * 256 * 4 * 4 * 3 + 1028])
def test_grad_norm_matches_float64_and_repeats_bit_for_bit(n):
    gen = torch.Generator(device="cuda").manual_seed(n)
    mag = 10.0 ** (torch.rand(n, device="cuda", generator=gen) * 10.0 - 8.0)        # 1e-8 .. 1e2
    g = torch.randn(n, device="cuda", generator=gen) * mag
    unscale = 0.25
    a = _norm(g, unscale=unscale)
    b = _norm(g, unscale=unscale)
    torch.cuda.synchronize()
    assert torch.equal(a, b)                                                 # fixed grid, fixed order: the same bits
    ref = float(torch.linalg.vector_norm(g.double())) * unscale
    assert abs(float(a[0]) - ref) <= 1e-6 * ref, (float(a[0]), ref)
    assert float(a[1]) == 1.0                                                # max_norm = inf: the norm alone, no clipping


def test_clip_factor_follows_clip_grad_norm():
    g = torch.randn(1 << 20, device="cuda") * 5e-4        # (norm ~0.5: the 1e-6 of the denominator shows in f32)
    norm = _norm(g)[0:1].clone()
    nv = float(norm)
    for max_norm in (2.0 * nv, nv / 4.0, nv, float(np.float32(nv))):           # no clip, clip, the exact threshold
        out = _norm(g, max_norm)
        assert torch.equal(out[0:1], norm)
        want = _torch_coef(norm.cpu(), max_norm)
        assert torch.equal(out[1:2].cpu(), want), (max_norm, float(out[1]), float(want))
    assert float(_norm(g, 2.0 * nv)[1]) == 1.0 and float(_norm(g, nv)[1]) < 1.0
    # against torch.nn.utils.clip_grad_norm_ itself (the unscale factor applied to the gradient first)
    w = torch.zeros_like(g, requires_grad=True)
    w.grad = g * 0.5
    total = torch.nn.utils.clip_grad_norm_([w], 0.3 * nv)
    out = _norm(g, 0.3 * nv, 0.5)
    assert abs(float(out[0]) - float(total)) <= 1e-6 * float(total)
    assert abs(float(out[1]) * float(g[7]) * 0.5 - float(w.grad[7])) <= 1e-5 * abs(float(w.grad[7])) + 1e-30
    # non-finite gradients propagate as torch does: NaN norm -> NaN factor, infinite norm -> factor 0
    gn = g.clone(); gn[12345] = float("nan")
    o = _norm(gn, 1.0)
    assert math.isnan(float(o[0])) and math.isnan(float(o[1]))
    gi = g.clone(); gi[99] = float("inf")
    o = _norm(gi, 1.0)
    assert math.isinf(float(o[0])) and float(o[1]) == 0.0
    with pytest.raises(RuntimeError, match="EINVAL"):
        ops.grad_norm(g, 6, torch.empty(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device="cuda"), out, 1.0, 1.0)


def _adam_case(n64, seed):
    rng = np.random.default_rng(seed)
    n = 64 * n64
    p = rng.standard_normal(n).astype(np.float32)
    return n, rng, p


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_grouped_adamw_matches_hf_formula_per_group(fmt):
    """Three groups with their own lr / weight decay, idle 64-blocks in each (they move only in the group with decay), a
    zero_mask, the clip factor read from the device and a schedule multiplier, on the library of either operand format."""
    n64 = 3 * 70
    n, rng, p = _adam_case(n64, 3)
    groups = [(2e-5, 0.01), (1e-4, 0.0), (5e-4, 0.1)]
    gid = rng.integers(0, 3, n64).astype(np.uint8)
    idle = np.zeros(n64, bool)
    for k in range(3):                                       # four never-touched 64-blocks per group
        idle[np.flatnonzero(gid == k)[:4]] = True
    zmask = (rng.random(n64) > 0.3).astype(np.uint8)
    coef = 0.37
    hdt = ops.HALF_DTYPE[fmt]
    gscale = 1.0 / 4096.0 if fmt == "fp16" else 0.5
    dp = torch.from_numpy(p).cuda(); dm = torch.zeros(n, device="cuda"); dv = torch.zeros(n, device="cuda")
    pb = dp.to(hdt)
    gmap = torch.from_numpy(gid).cuda()
    table = torch.tensor(groups, dtype=torch.float32, device="cuda")
    dcoef = torch.tensor([coef], dtype=torch.float32, device="cuda")
    p_ref = p.astype(np.float64); m_ref = np.zeros(n); v_ref = np.zeros(n)
    el_gid = np.repeat(gid, 64); el_idle = np.repeat(idle, 64)
    for t in range(1, 5):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        g[el_idle] = 0.0
        factor = [1.0, 0.75, 0.5, 0.25][t - 1]
        bc = math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        dg = torch.from_numpy(g / gscale).cuda()
        with ops.operand_format(fmt):
            ops.adamw_step_grouped(dp, dg, dm, dv, pb, n, gmap, table, factor, 0.9, 0.999, 1e-8, bias_corr_factor=bc,
                                   grad_scale=gscale, coef=dcoef, zero_grad=True, zero_mask=torch.from_numpy(zmask).cuda())
        for k, (lr, wd) in enumerate(groups):
            s = el_gid == k
            pk, mk, vk = p_ref[s], m_ref[s], v_ref[s]
            O.hf_adamw_step(pk, coef * g[s].astype(np.float64), mk, vk, lr * factor, t, weight_decay=wd, correct_bias=True)
            p_ref[s], m_ref[s], v_ref[s] = pk, mk, vk
        torch.cuda.synchronize()
        gz = dg.cpu().numpy().reshape(n64, 64)
        assert not gz[zmask == 1].any()                                  # cleared where the mask says so ...
        busy = ~idle & (zmask == 0)
        np.testing.assert_array_equal(gz[busy], (g / gscale).reshape(n64, 64)[busy])     # ... left alone elsewhere
    np.testing.assert_allclose(dp.cpu().numpy(), p_ref, atol=2e-7, rtol=1e-6)
    np.testing.assert_allclose(dm.cpu().numpy(), m_ref, atol=1e-8, rtol=1e-4)
    np.testing.assert_allclose(dv.cpu().numpy(), v_ref, atol=1e-14, rtol=1e-4)
    assert torch.equal(pb, dp.to(hdt))
    pf = dp.cpu().numpy()
    for k, (_, wd) in enumerate(groups):
        s = el_idle & (el_gid == k)
        if wd == 0.0:      # idle, no decay: bit-identical to where they started, moments untouched
            assert np.array_equal(pf[s], p[s]) and float(dm.cpu().numpy()[s].max()) == 0.0
        else:              # idle with decay: they shrink
            assert (np.abs(pf[s]) < np.abs(p[s])).mean() > 0.99


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_one_group_without_clipping_is_bit_identical_to_adamw_step(fmt, wd):
    n64 = 300
    n, rng, p = _adam_case(n64, 11)
    hdt = ops.HALF_DTYPE[fmt]
    a = [torch.from_numpy(p).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    b = [x.clone() for x in a]
    pba, pbb = a[0].to(hdt), a[0].to(hdt)
    zmask = torch.from_numpy((rng.random(n64) > 0.5).astype(np.uint8)).cuda()
    gmap = torch.zeros(n64, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[3e-4, wd]], dtype=torch.float32, device="cuda")
    one = torch.ones(1, device="cuda")
    for t in range(1, 4):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        g[: n // 4] = 0.0                                                 # idle quarter (skipped without decay)
        ga, gb = torch.from_numpy(g).cuda(), torch.from_numpy(g).cuda()
        bc = math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        with ops.operand_format(fmt):
            ops.adamw_step(a[0], ga, a[1], a[2], pba, n, 3e-4, 0.9, 0.999, 1e-8, wd, bias_corr_factor=bc, grad_scale=0.25,
                           zero_grad=True, zero_mask=zmask)
            ops.adamw_step_grouped(b[0], gb, b[1], b[2], pbb, n, gmap, table, 1.0, 0.9, 0.999, 1e-8, bias_corr_factor=bc,
                                   grad_scale=0.25, coef=one if t % 2 else None, zero_grad=True, zero_mask=zmask)
        torch.cuda.synchronize()
        assert torch.equal(ga, gb)
    for x, y in zip(a + [pba], b + [pbb]):
        assert torch.equal(x, y)


# ---- TrainStep ------------------------------------------------------------------------------------------------------
def _oracle_steps(spec, state, bn, nsteps, lr, wd, no_decay, max_norm):
    """O.vault_loss -> clip_grad_norm_ -> per-group hf_adamw_step; returns per step (loss, pre-clip norm, coef) and the state
    after step 1 (p, m, and the unclipped gradient)."""
    P = O.to_torch_state(state, requires_grad=True)
    m = {k: torch.zeros_like(v) for k, v in P.items()}; v2 = {k: torch.zeros_like(v) for k, v in P.items()}
    tb = O.torch_batch(bn)
    hist, first = [], None
    for t in range(1, nsteps + 1):
        for p in P.values():
            p.grad = None
        loss, _ = O.vault_loss(P, spec, tb)
        loss.backward()
        g1 = {k: p.grad.clone() for k, p in P.items() if p.grad is not None}
        params = [p for p in P.values() if p.grad is not None]
        total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        coef = min(1.0, max_norm / (total + 1e-6))
        hist.append((float(loss.detach()), total, coef))
        with torch.no_grad():
            for k, p in P.items():
                if p.grad is not None:
                    O.hf_adamw_step(p, p.grad, m[k], v2[k], O.linear_schedule_lr(lr, t - 1, 0, 10), t,
                                    weight_decay=0.0 if k in no_decay else wd)
        if t == 1:
            first = ({k: p.detach().clone() for k, p in P.items()}, {k: x.clone() for k, x in m.items()}, g1)
    return hist, first


@pytest.mark.parametrize("half", ["fp16", "bf16"])
def test_clipped_grouped_train_step_vs_oracle(half):
    spec = _tiny()
    bn = synthetic_batch(spec, 4, seed=21, n_classes=3)
    state = build_state(spec, 0)
    lr, wd = 5e-5, 0.01
    eng = VaultEngine(spec, "cuda:0", state=state, classifier_dropout=0.0, half=half)
    no_decay = set(hf_no_decay_groups(eng)[0]["params"])
    assert no_decay == set(no_decay_parameter_names(spec, eng.params.trainable)) and "layernorm.weight" in no_decay
    # the step-1 norm of the oracle, then a threshold that really clips (about half of it)
    (_, norm1, _), = _oracle_steps(spec, state, bn, 1, lr, wd, no_decay, 1e9)[0]
    max_norm = 0.5 * norm1
    hist, (p1_ref, m1_ref, g1_ref) = _oracle_steps(spec, state, bn, 3, lr, wd, no_decay, max_norm)
    step = TrainStep(eng, learning_rate=lr, weight_decay=wd, warmup_ratio=0.0, total_steps=10, max_grad_norm=max_norm,
                     param_groups=hf_no_decay_groups(eng))
    db = {k: torch.from_numpy(v).cuda() for k, v in bn.items() if k != "labels"}
    labels = torch.from_numpy(bn["labels"]).cuda()
    losses, norms = [], []
    P = eng.params
    for i in range(3):
        losses.append(float(step(db, labels)))          # (the loss buffer is the step's own: read it per step)
        norms.append(step.grad_norm)
        if i == 0:
            torch.cuda.synchronize()
            p1, m1 = P.p.clone(), P.m.clone()
    assert len({x.data_ptr() for x in norms}) == 3          # a tensor of its own per step
    assert step.grad_norm.dim() == 0 and step.grad_norm.dtype == torch.float32 and step.grad_norm.is_cuda
    norms = [float(x) for x in norms]
    tol = 3e-2 if half == "bf16" else 1e-2
    for (lref, nref, _), l, nm in zip(hist, losses, norms):
        assert abs(l - lref) < 5e-3, (losses, hist)
        assert abs(nm - nref) < tol * nref, (norms, hist)
    coef_ref = hist[0][2]
    assert coef_ref < 0.55
    # moments after step 1: m = (1 - b1) coef g  (Adam's update itself barely sees a constant factor at step 1)
    names = [k for k in g1_ref if P.has_grad(k)]
    mine = torch.cat([P._view(m1, k).reshape(-1).cpu() for k in names])
    ref = torch.cat([m1_ref[k].reshape(-1) for k in names])
    unclipped = torch.cat([0.1 * g1_ref[k].reshape(-1) for k in names])
    assert float((mine - ref).norm() / ref.norm()) < (5e-2 if half == "bf16" else 1e-2)
    assert abs(float(mine.norm() / unclipped.norm()) - coef_ref) < tol * coef_ref
    # decay on the decay group only, after step 1: LayerNorm weights (~1) sit where the no-decay update puts them (5e-7 of
    # decay would be visible there), the untouched rows of the LM's word table (g = m = v = 0) shrank by lr x wd exactly
    for k in ("layernorm.weight", "bert.encoder.layer.1.output.LayerNorm.weight", "encoder.layer.0.layernorm_before.weight"):
        w1 = P._view(p1, k).cpu(); w0 = torch.from_numpy(state[k])
        d_groups = float((w1 - p1_ref[k]).abs().median())
        d_decayed = float((w1 - (p1_ref[k] - lr * wd * p1_ref[k])).abs().median())
        assert d_groups < 2e-7 < d_decayed, (k, d_groups, d_decayed)
        assert not torch.equal(w1, w0)
    k = "bert.embeddings.word_embeddings.weight"
    rows = np.setdiff1d(np.arange(spec.lm.vocab_size), bn["input_ids"].reshape(-1))
    assert len(rows) > 10 and float(g1_ref[k][rows].abs().max()) == 0.0
    w0 = torch.from_numpy(state[k])[rows]
    w1 = P._view(p1, k).cpu()[rows]
    torch.testing.assert_close(w1, w0 * (1 - lr * wd), rtol=3e-7, atol=0)
    assert not torch.equal(w1, w0)


def test_clipped_grouped_tape_replay_matches_eager():
    """The recorded step with clipping and groups against eager steps (use_tape=False).  Float atomics of the backward make
    two eager runs differ in the last bits already (tests/test_gpu_train.py::test_tape_replay_matches_eager_steps): the same
    bounds as there, and the same norms."""
    spec = VaultSpec.tiny(3, "roberta")
    state = build_state(spec, 0)
    batches = [synthetic_batch(spec, 4, seed=40 + i, n_classes=3) for i in range(4)]
    res = {}
    for use_tape in (False, True):
        eng = VaultEngine(spec, "cuda:0", state=state, classifier_dropout=0.1, half="bf16")
        step = TrainStep(eng, learning_rate=5e-5, weight_decay=0.01, warmup_ratio=0.0, total_steps=10, use_tape=use_tape,
                         max_grad_norm=0.5, param_groups=hf_no_decay_groups(eng))
        losses, norms = [], []
        for bn in batches:
            db = {k: torch.from_numpy(v).cuda() for k, v in bn.items() if k != "labels"}
            losses.append(float(step(db, torch.from_numpy(bn["labels"]).cuda())))
            norms.append(step.grad_norm)
        assert (step._tape is not None) == use_tape
        res[use_tape] = (losses, [float(x) for x in norms], eng.params.p.clone())
    (la, na, pa), (lb, nb, pb) = res[False], res[True]
    assert min(na) > 0.5                                                 # it clipped in every step
    assert abs(la[0] - lb[0]) < 1e-6 and max(abs(a - b) for a, b in zip(la, lb)) < 5e-4, (la, lb)
    assert max(abs(a - b) / a for a, b in zip(na, nb)) < 1e-3, (na, nb)
    d = (pa - pb).abs()
    assert float(d.mean()) < 1e-6 and float((d > 1e-5).float().mean()) < 0.02


def test_default_train_step_issues_only_the_plain_adamw(monkeypatch):
    calls = {"adamw_step": 0}
    real, real_grouped, real_norm = ops.adamw_step, ops.adamw_step_grouped, ops.grad_norm

    def counted(*a, **kw):
        calls["adamw_step"] += 1
        return real(*a, **kw)

    def forbidden(*a, **kw):
        raise AssertionError("the default TrainStep launched a clipping / group kernel")

    monkeypatch.setattr(ops, "adamw_step", counted)
    monkeypatch.setattr(ops, "adamw_step_grouped", forbidden)
    monkeypatch.setattr(ops, "grad_norm", forbidden)
    spec = _tiny()
    eng = VaultEngine(spec, "cuda:0", state=build_state(spec, 0), classifier_dropout=0.0, half="bf16")
    step = TrainStep(eng, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10)
    bn = synthetic_batch(spec, 4, seed=5, n_classes=3)
    db = {k: torch.from_numpy(v).cuda() for k, v in bn.items() if k != "labels"}
    for _ in range(2):                                                   # eager + recorded, then a replay
        step(db, torch.from_numpy(bn["labels"]).cuda())
    torch.cuda.synchronize()
    assert calls["adamw_step"] == 2 and step.grad_norm is None
    # and with the options on, the plain pass is never taken
    monkeypatch.setattr(ops, "adamw_step_grouped", real_grouped)
    monkeypatch.setattr(ops, "grad_norm", real_norm)
    calls["adamw_step"] = 0
    step = TrainStep(eng, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    step(db, torch.from_numpy(bn["labels"]).cuda())
    assert calls["adamw_step"] == 0 and step.grad_norm is not None
    step = TrainStep(eng, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10, track_grad_norm=True)
    step(db, torch.from_numpy(bn["labels"]).cuda())
    assert calls["adamw_step"] == 1 and float(step.grad_norm) > 0.0
    # a manual optimizer step over a part of the buffer cannot clip
    step = TrainStep(eng, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        step.optimizer_step(lo=0, hi=1024)


# ---- data parallel --------------------------------------------------------------------------------------------------
def _dp_clip_worker(rank, world, port, out_path, nsteps, clip):
    """One data-parallel rank with clipping (optional) and the HF groups; both ranks share cuda:0, gloo carries the
    device tensors; its half of every global batch of 8."""
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        spec = _tiny()
        eng = VaultEngine(spec, "cuda:0", state=build_state(spec, 0), classifier_dropout=0.0, half="bf16")
        step = TrainStep(eng, learning_rate=5e-5, weight_decay=0.01, warmup_ratio=0.0, total_steps=10, bucket_mb=0.25,
                         wire="fp32", sparse_embedding=True, max_grad_norm=0.5 if clip else None,
                         param_groups=hf_no_decay_groups(eng))
        assert step.world == world and step.reducer is not None
        losses, norms = [], []
        for i in range(nsteps):
            bn = synthetic_batch(spec, 8, seed=90 + i, n_classes=3)
            lo, hi = rank * (8 // world), (rank + 1) * (8 // world)
            db = {k: torch.from_numpy(v[lo:hi]).cuda() for k, v in bn.items() if k != "labels"}
            losses.append(float(step(db, torch.from_numpy(bn["labels"][lo:hi]).cuda())))
            norms.append(step.grad_norm.cpu() if clip else None)
        torch.cuda.synchronize()
        torch.save({"p": eng.params.p.cpu(), "losses": losses, "norms": norms}, f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("clip", [True, False])
def test_data_parallel_clipping_and_groups_equal_one_rank(tmp_path, clip):
    """Two ranks with the norm on (clipping: no optimizer pass under the last bucket; groups only: the split pass over the
    sliced group map) stay bit-identical and land where one rank stepping the global batch lands."""
    import torch.multiprocessing as mp
    world, nsteps = 2, 3
    out = str(tmp_path / "dpclip")
    mp.spawn(_dp_clip_worker, args=(world, 29810 + int(clip), out, nsteps, clip), nprocs=world, join=True)
    r0, r1 = [torch.load(out + f".{r}") for r in range(world)]
    assert torch.equal(r0["p"], r1["p"])
    if clip:
        assert all(torch.equal(a, b) for a, b in zip(r0["norms"], r1["norms"]))      # the same reduced gradient, same bits
    spec = _tiny()
    eng = VaultEngine(spec, "cuda:0", state=build_state(spec, 0), classifier_dropout=0.0, half="bf16")
    step = TrainStep(eng, learning_rate=5e-5, weight_decay=0.01, warmup_ratio=0.0, total_steps=10, use_tape=False,
                     max_grad_norm=0.5 if clip else None, param_groups=hf_no_decay_groups(eng), track_grad_norm=not clip)
    ref_losses, ref_norms = [], []
    for i in range(nsteps):
        bn = synthetic_batch(spec, 8, seed=90 + i, n_classes=3)
        db = {k: torch.from_numpy(v).cuda() for k, v in bn.items() if k != "labels"}
        ref_losses.append(float(step(db, torch.from_numpy(bn["labels"]).cuda())))
        ref_norms.append(float(step.grad_norm))
    torch.cuda.synchronize()
    if clip:
        assert min(ref_norms) > 0.5
    for i, c in enumerate(ref_losses):
        assert abs((r0["losses"][i] + r1["losses"][i]) / 2 - c) < 5e-4
        if clip:       # (step 1 from the same weights; later steps inherit the float-atomic spread of the trajectories)
            assert abs(float(r0["norms"][i]) - ref_norms[i]) < (1e-4 if i == 0 else 1e-3) * ref_norms[i], (r0["norms"], ref_norms)
    d = (r0["p"] - eng.params.p.cpu()).abs()
    assert float(d.mean()) < 2e-6 and float((d > 1e-5).float().mean()) < 0.03
