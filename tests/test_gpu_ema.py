"""Weight average (EMA) of the fused train step and its resumable optimizer state on the GPU: the AdamW kernel with the
average against the grouped kernel (bit for bit) and a float64 recurrence, the in-place swap, TrainStep's option, the
``ema_weights()`` block, the state round trip, the split data-parallel pass and the unchanged default path."""
import math

import numpy as np
import pytest
import torch

from oracle import vault_oracle as O
from tests.optim_common import U, _Recurrence, _batch, _engine, _f32, _tiny
from vault_amd import ops
from vault_amd.train import TrainStep, ema_decay_at, hf_no_decay_groups

pytestmark = pytest.mark.gpu

GRID_CAP_N = 8192 * 256 * 4 + 64 * 37      # the grid-stride loop takes a second, ragged trip


def _three_group_case(n64, seed):
    rng = np.random.default_rng(seed)
    n = 64 * n64
    p = rng.standard_normal(n).astype(np.float32)
    gid = rng.integers(0, 3, n64).astype(np.uint8)
    idle = np.zeros(n64, bool)
    for k in range(3):                                       # four never-touched 64-blocks per group
        idle[np.flatnonzero(gid == k)[:4]] = True
    zmask = (rng.random(n64) > 0.3).astype(np.uint8)
    return n, rng, p, gid, idle, zmask


GROUPS = [(2e-5, 0.01), (1e-4, 0.0), (5e-4, 0.1)]


# ---- kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_adamw_ema_equals_grouped_adamw_and_follows_the_recurrence(fmt):
    n64 = 3 * 70
    n, rng, p, gid, idle, zmask = _three_group_case(n64, 3)
    hdt = ops.HALF_DTYPE[fmt]
    gscale = 1.0 / 4096.0 if fmt == "fp16" else 0.5
    omd = _f32(1.0 - 0.9)
    A = [torch.from_numpy(p).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    B = [x.clone() for x in A]
    pba, pbb = A[0].to(hdt), B[0].to(hdt)
    ema = B[0].clone()
    rec = _Recurrence(ema)
    gmap = torch.from_numpy(gid).cuda()
    zm = torch.from_numpy(zmask).cuda()
    table = torch.tensor(GROUPS, dtype=torch.float32, device="cuda")
    dcoef = torch.tensor([0.37], dtype=torch.float32, device="cuda")
    el_idle = np.repeat(idle, 64)
    for t in range(1, 5):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        g[el_idle] = 0.0
        factor = [1.0, 0.75, 0.5, 0.25][t - 1]
        bc = math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        ga, gb = torch.from_numpy(g / gscale).cuda(), torch.from_numpy(g / gscale).cuda()
        with ops.operand_format(fmt):
            ops.adamw_step_grouped(A[0], ga, A[1], A[2], pba, n, gmap, table, factor, 0.9, 0.999, 1e-8, bias_corr_factor=bc,
                                   grad_scale=gscale, coef=dcoef, zero_grad=True, zero_mask=zm)
            ops.adamw_step_ema(B[0], gb, B[1], B[2], pbb, ema, n, gmap, table, factor, 0.9, 0.999, 1e-8, omd,
                               bias_corr_factor=bc, grad_scale=gscale, coef=dcoef, zero_grad=True, zero_mask=zm)
        torch.cuda.synchronize()
        for name, x, y in zip(("p", "m", "v", "shadow", "g"), A + [pba, ga], B + [pbb, gb]):
            assert torch.equal(x, y), (name, t)
        rec.step(B[0], omd)                                  # (the device's own p of this step)
        rec.check(ema, f"{fmt} step {t}")
    assert torch.equal(pbb, B[0].to(hdt))
    assert not torch.equal(ema, B[0])
    # never-touched blocks without decay: the average still holds the bits of p
    s = torch.from_numpy(el_idle & (np.repeat(gid, 64) == 1)).cuda()
    assert torch.equal(ema[s], torch.from_numpy(p).cuda()[s]) and torch.equal(B[0][s], ema[s])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_idle_blocks_skip_only_when_the_average_holds_the_weights(fmt):
    """64-blocks 0..5: [busy | idle, e == p | idle, e apart from p | idle in the group with decay | busy | idle, one element of e
    apart]; groups (lr, 0) and (lr, 0.1)."""
    n64, n = 6, 64 * 6
    hdt = ops.HALF_DTYPE[fmt]
    gen = torch.Generator(device="cuda").manual_seed(5)
    p0 = torch.randn(n, device="cuda", generator=gen)
    g = torch.randn(n, device="cuda", generator=gen) * 1e-2
    blk = lambda x, k: x[64 * k:64 * (k + 1)]  # noqa: E731
    for k in (1, 2, 3, 5):
        blk(g, k).zero_()
    p, m, v = p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pb0 = torch.full((n,), 3.0, dtype=hdt, device="cuda")   # (not p's image: a skipped block must leave the shadow alone)
    pb = pb0.clone()
    e0 = p0.clone()
    blk(e0, 2).add_(torch.randn(64, device="cuda", generator=gen) * 0.1)
    blk(e0, 5)[17] += 0.25                                  # one element of one f32x4: the whole block's others keep their bits
    ema = e0.clone()
    gmap = torch.tensor([0, 0, 0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    table = torch.tensor([[1e-3, 0.0], [1e-3, 0.1]], dtype=torch.float32, device="cuda")
    omd = _f32(1.0 - 0.75)
    rec = _Recurrence(e0)
    with ops.operand_format(fmt):
        ops.adamw_step_ema(p, g, m, v, pb, ema, n, gmap, table, 1.0, 0.9, 0.999, 1e-8, omd)
    torch.cuda.synchronize()
    rec.step(p, omd)
    rec.check(ema, fmt)
    # idle, no decay, e == p: nothing moves
    for x, x0 in ((p, p0), (ema, e0), (pb, pb0)):
        assert torch.equal(blk(x, 1), blk(x0, 1))
    assert not blk(m, 1).any() and not blk(v, 1).any()
    # idle, no decay, e apart: p, m, v and the shadow keep their bits, the average moves by (1 - d)(p - e)
    for k in (2, 5):
        assert torch.equal(blk(p, k), blk(p0, k)) and torch.equal(blk(pb, k), blk(pb0, k))
        assert not blk(m, k).any() and not blk(v, k).any()
    assert not bool((blk(ema, 2) == blk(e0, 2)).any())
    want = blk(e0, 2).double() + omd * (blk(p0, 2).double() - blk(e0, 2).double())
    assert float((blk(ema, 2).double() - want).abs().max()) <= 4 * U * float(torch.maximum(blk(p0, 2).abs(), blk(e0, 2).abs()).max())
    moved = blk(ema, 5) != blk(e0, 5)
    assert moved.nonzero().flatten().tolist() == [17]
    # idle in the group with decay: p shrinks (and is stored with its shadow), the average follows
    assert bool((blk(p, 3).abs() < blk(p0, 3).abs()).all())
    assert torch.equal(blk(pb, 3), blk(p, 3).to(hdt))
    assert not bool((blk(ema, 3) == blk(e0, 3)).any())
    # busy blocks moved everything
    for k in (0, 4):
        assert not torch.equal(blk(p, k), blk(p0, k)) and torch.equal(blk(pb, k), blk(p, k).to(hdt))
        assert bool(blk(m, k).any()) and not blk(g, k).any()


def test_adamw_ema_beyond_the_grid_cap():
    n = GRID_CAP_N
    n64 = n // 64
    gen = torch.Generator(device="cuda").manual_seed(9)
    p0 = torch.randn(n, device="cuda", generator=gen)
    g0 = torch.randn(n, device="cuda", generator=gen) * 1e-2
    gmap = torch.randint(0, 3, (n64,), device="cuda", generator=gen).to(torch.uint8)
    zm = (torch.rand(n64, device="cuda", generator=gen) > 0.3).to(torch.uint8)
    idle = torch.rand(n64, device="cuda", generator=gen) < 0.05
    idle[-3:] = True                                         # (the ragged end too)
    g0.view(n64, 64)[idle] = 0.0
    table = torch.tensor(GROUPS, dtype=torch.float32, device="cuda")
    dcoef = torch.tensor([0.37], dtype=torch.float32, device="cuda")
    A = [p0.clone(), g0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    B = [x.clone() for x in A]
    pba, pbb = p0.to(torch.bfloat16), p0.to(torch.bfloat16)
    ema = p0 + 0.01 * torch.randn(n, device="cuda", generator=gen)
    rec = _Recurrence(ema)
    omd = _f32(1.0 - 0.9)
    with ops.operand_format("bf16"):
        ops.adamw_step_grouped(A[0], A[1], A[2], A[3], pba, n, gmap, table, 0.75, 0.9, 0.999, 1e-8, grad_scale=0.5, coef=dcoef,
                               zero_grad=True, zero_mask=zm)
        ops.adamw_step_ema(B[0], B[1], B[2], B[3], pbb, ema, n, gmap, table, 0.75, 0.9, 0.999, 1e-8, omd, grad_scale=0.5,
                           coef=dcoef, zero_grad=True, zero_mask=zm)
    torch.cuda.synchronize()
    for name, x, y in zip(("p", "g", "m", "v", "shadow"), A + [pba], B + [pbb]):
        assert torch.equal(x, y), name
    assert not torch.equal(B[0][-64 * 37:], p0[-64 * 37:])                # the tail was reached
    rec.step(B[0], omd)
    rec.check(ema, "grid cap")


def test_adamw_ema_argument_errors():
    n = 64
    z = lambda: torch.zeros(n, device="cuda")  # noqa: E731
    p, g, m, v, ema = z(), z(), z(), z(), z()
    pb = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    gmap = torch.zeros(1, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[1e-3, 0.0]], dtype=torch.float32, device="cuda")
    args = lambda e, k, omd: (p, g, m, v, pb, e, k, gmap, table, 1.0, 0.9, 0.999, 1e-8, omd)  # noqa: E731
    with ops.operand_format("bf16"):
        for bad in (args(ema, n, 0.0), args(ema, n, 1.5), args(None, n, 0.1), args(ema, 6, 0.1)):
            with pytest.raises(RuntimeError, match="EINVAL"):
                ops.adamw_step_ema(*bad)
        ops.adamw_step_ema(*args(ema, n, 1.0))               # decay 0: the upper end of (0, 1] is valid
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [64 * 300, GRID_CAP_N])
def test_ema_swap_exchanges_in_place_and_twice_is_the_identity(fmt, n):
    hdt = ops.HALF_DTYPE[fmt]
    gen = torch.Generator(device="cuda").manual_seed(n % 1000)
    p0 = torch.randn(n, device="cuda", generator=gen) * 10.0 ** (torch.rand(n, device="cuda", generator=gen) * 8.0 - 4.0)
    e0 = torch.randn(n, device="cuda", generator=gen)
    pb0 = p0.to(hdt)
    p, e, pb = p0.clone(), e0.clone(), pb0.clone()
    with ops.operand_format(fmt):
        ops.ema_swap(p, e, pb, n)
        torch.cuda.synchronize()
        assert torch.equal(p, e0) and torch.equal(e, p0) and torch.equal(pb, p.to(hdt))
        assert not torch.equal(pb, pb0)
        ops.ema_swap(p, e, pb, n)
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and torch.equal(e, e0) and torch.equal(pb, pb0)


# ---- TrainStep ------------------------------------------------------------------------------------------------------

def _steps_against_recurrence(step, db, labels, nsteps, decay, warmup):
    P = step.engine.params
    rec = _Recurrence(step.ema)
    for t in range(1, nsteps + 1):
        step(db, labels)
        torch.cuda.synchronize()
        rec.step(P.p[:P.n_train].clone(), _f32(1.0 - ema_decay_at(decay, t, warmup)))
        rec.check(step.ema, f"train step {t}")
    assert step.step_idx == nsteps
    assert not torch.equal(step.ema, P.p[:P.n_train])
    return rec


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("warmup", [False, True])
def test_train_step_moves_the_average_by_the_recurrence(warmup, clipped):
    spec = _tiny()
    eng = _engine(spec)
    _, db, labels = _batch(spec, 21)
    opts = dict(max_grad_norm=1e-2, param_groups=hf_no_decay_groups(eng)) if clipped else {}
    step = TrainStep(eng, learning_rate=5e-5, weight_decay=0.01, warmup_ratio=0.0, total_steps=10, ema_decay=0.9,
                     ema_warmup=warmup, **opts)
    P = eng.params
    assert step.ema.dtype == torch.float32 and step.ema.numel() == P.n_train and step.ema.is_cuda
    assert torch.equal(step.ema, P.p[:P.n_train]) and step.ema.data_ptr() != P.p.data_ptr()
    _steps_against_recurrence(step, db, labels, 3, 0.9, warmup)
    if clipped:
        assert float(step.grad_norm) > 1e-2                               # it clipped
    step.reset_ema()
    assert torch.equal(step.ema, P.p[:P.n_train])
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="ema_decay"):
            TrainStep(eng, ema_decay=bad)


def test_ema_weights_block_swaps_the_engine_onto_the_average_and_back():
    spec = _tiny()
    eng = _engine(spec)
    bn, db, labels = _batch(spec, 22)
    step = TrainStep(eng, learning_rate=1e-3, weight_decay=0.01, warmup_ratio=0.0, total_steps=10, ema_decay=0.9)
    P = eng.params
    for _ in range(3):
        step(db, labels)
    torch.cuda.synchronize()
    nt = P.n_train
    p0, pb0, e0 = P.p.clone(), P.pb.clone(), step.ema.clone()
    tname = eng.vl[0].ow
    pbT0 = P.pbT[tname].clone()
    out_logits = eng.forward(db, train=False, need_hidden=False)["logits"].clone()

    def inside():
        assert torch.equal(P.p[:nt], e0) and torch.equal(step.ema, p0[:nt])
        assert torch.equal(P.p[nt:], p0[nt:])                             # frozen parameters stay
        fresh = torch.zeros_like(P.pb)
        with ops.operand_format("bf16"):
            ops.cast_bf16(P.p, fresh, P.n_total)
        assert torch.equal(P.pb[:P.n_total], fresh[:P.n_total])
        rows = P.offsets[tname][1][0]
        assert torch.equal(P.pbT[tname], P.wb(tname).reshape(rows, -1).t())
        assert not torch.equal(P.pbT[tname], pbT0)

    with step.ema_weights() as inner:
        assert inner is step
        inside()
        lg = eng.forward(db, train=False, need_hidden=False)["logits"].clone()
        assert not torch.equal(lg, out_logits)
        sd = P.state_dict_numpy()
        np.testing.assert_array_equal(sd["pooler.dense.weight"], P._view(e0, "pooler.dense.weight").cpu().numpy())
        ref = O.vault_forward(O.to_torch_state(sd), spec, O.torch_batch(bn))
        d = float((lg.cpu() - ref["logits"].detach()).abs().max())
        print(f"eval logits on the averaged weights vs the fp32 oracle: max |diff| {d:.3e}")
        assert d < 3e-3                                                   # tests/test_gpu_model.py: tiny forward, bf16
        with pytest.raises(RuntimeError, match="ema_weights"):
            step(db, labels)
        with pytest.raises(RuntimeError, match="ema_weights"):
            step.optimizer_step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            with step.ema_weights():
                pass
        inside()                                                          # (the refused calls touched nothing)
    torch.cuda.synchronize()
    assert torch.equal(P.p, p0) and torch.equal(P.pb, pb0) and torch.equal(step.ema, e0) and torch.equal(P.pbT[tname], pbT0)
    assert torch.equal(eng.forward(db, train=False, need_hidden=False)["logits"], out_logits)
    with pytest.raises(KeyError, match="boom"):
        with step.ema_weights():
            assert torch.equal(P.p[:nt], e0)
            raise KeyError("boom")
    torch.cuda.synchronize()
    assert torch.equal(P.p, p0) and torch.equal(P.pb, pb0) and torch.equal(step.ema, e0) and torch.equal(P.pbT[tname], pbT0)
    step(db, labels)                                                      # and training goes on
    torch.cuda.synchronize()
    assert step.step_idx == 4 and not torch.equal(P.p, p0)
    with pytest.raises(RuntimeError, match="no weight average"):
        with TrainStep(eng, warmup_ratio=0.0, total_steps=10).ema_weights():
            pass


def test_optimizer_state_round_trip_resumes_bit_for_bit():
    spec = _tiny()
    eng = _engine(spec)
    _, db, labels = _batch(spec, 23)
    opts = dict(learning_rate=5e-5, weight_decay=0.01, warmup_ratio=0.3, total_steps=10, ema_decay=0.9, ema_warmup=True)
    step = TrainStep(eng, param_groups=hf_no_decay_groups(eng), **opts)
    for _ in range(2):
        step(db, labels)
    torch.cuda.synchronize()
    sd = step.state_dict()
    P = eng.params
    assert sd["step_idx"] == 2 and sd["drop_seed"] == eng.drop_seed and set(sd["exp_avg"]) == set(P.trainable)
    assert all(not t.is_cuda and tuple(t.shape) == tuple(P.offsets[n][1]) for n, t in sd["ema"].items())
    assert sd["hyper"]["ema_decay"] == 0.9 and sd["hyper"]["total_steps"] == 10 and sd["hyper"]["warmup_steps"] == 3
    eng2 = _engine(spec, state=P.state_dict_numpy())
    step2 = TrainStep(eng2, param_groups=hf_no_decay_groups(eng2), **opts)
    P2 = eng2.params
    assert step2.step_idx == 0 and not P2.m.any()
    with pytest.raises(ValueError, match="weight average"):
        TrainStep(eng2, **{**opts, "ema_decay": None}).load_state_dict(sd)
    step2.load_state_dict(sd)
    for n in P.trainable:
        for a, b in ((P.m, P2.m), (P.v, P2.v), (step.ema, step2.ema), (P.p, P2.p)):
            assert torch.equal(P._view(a, n), P2._view(b, n)), n
    assert step2.step_idx == step.step_idx == 2 and eng2.drop_seed == eng.drop_seed
    assert step2.current_lr() == step.current_lr() and step2.current_lr() != TrainStep(eng2, **opts).current_lr()
    # the same gradient through both optimizers: everything the pass writes comes out with the same bits
    nt = P.n_train
    g = torch.randn(nt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 1e-3
    before = P.p.clone()
    for s_, P_ in ((step, P), (step2, P2)):
        P_.g[:nt].copy_(g)
        s_.optimizer_step()
    torch.cuda.synchronize()
    assert not torch.equal(P.p, before) and step.step_idx == step2.step_idx == 3
    for name, a, b in (("p", P.p, P2.p), ("m", P.m, P2.m), ("v", P.v, P2.v), ("ema", step.ema, step2.ema),
                       ("shadow", P.pb[:nt], P2.pb[:nt]), ("g", P.g[:nt], P2.g[:nt])):
        assert torch.equal(a, b), name
    # a state without the average loads into a step without one, and not into one with it
    plain = TrainStep(eng2, **{**opts, "ema_decay": None})
    sd_plain = plain.state_dict()
    assert sd_plain["ema"] is None
    plain.load_state_dict(sd_plain)
    with pytest.raises(ValueError, match="no weight average"):
        step2.load_state_dict(sd_plain)


def test_default_train_step_launches_no_ema_kernel(monkeypatch):
    def forbidden(*a, **kw):
        raise AssertionError("the default TrainStep launched a weight-average kernel")

    monkeypatch.setattr(ops, "adamw_step_ema", forbidden)
    monkeypatch.setattr(ops, "ema_swap", forbidden)
    spec = _tiny()
    eng = _engine(spec)
    _, db, labels = _batch(spec, 5)
    free = torch.cuda.memory_allocated()
    step = TrainStep(eng, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10)
    assert step.ema is None and step._group_map is None and torch.cuda.memory_allocated() == free
    for _ in range(2):
        step(db, labels)
    torch.cuda.synchronize()
    assert step.ema is None and step.step_idx == 2
    with pytest.raises(RuntimeError, match="no weight average"):
        step.reset_ema()


def test_ema_in_the_split_pass_over_rccl_single_rank(monkeypatch):
    """One rank over RCCL with VAULT_FORCE_DP=1 and no clipping: the optimizer runs on the reduced upper range while the last
    bucket is on the wire, then on the rest - two launches per step at the same decay."""
    import os
    import torch.distributed as dist
    from vault_amd.train import BucketReducer
    monkeypatch.setattr(BucketReducer, "SINGLE_RANK_COLLECTIVES", True)
    calls = []
    real = ops.adamw_step_ema

    def counted(*a, **kw):
        calls.append((int(a[6]), float(a[13])))                          # (n, one_minus_decay)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "adamw_step_ema", counted)
    spec = _tiny()
    _, db, labels = _batch(spec, 41, B=8)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29647", VAULT_FORCE_DP="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        eng = _engine(spec)
        step = TrainStep(eng, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10, bucket_mb=0.05, wire="fp32",
                         ema_decay=0.9, ema_warmup=True)
        assert step.reducer is not None and step.reducer.native_a2a
        _steps_against_recurrence(step, db, labels, 3, 0.9, True)
    finally:
        dist.destroy_process_group()
        os.environ.pop("VAULT_FORCE_DP", None)
    nt = eng.params.n_train
    assert len(calls) == 6, calls                                        # two ranges per step ...
    for t in range(3):
        (n_hi, d_hi), (n_lo, d_lo) = calls[2 * t], calls[2 * t + 1]
        assert n_hi + n_lo == nt and 0 < n_lo < nt                       # ... that tile [0, n_train) ...
        assert d_hi == d_lo == 1.0 - ema_decay_at(0.9, t + 1, True)      # ... at the same t
