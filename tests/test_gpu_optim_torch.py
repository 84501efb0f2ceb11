"""torch.optim.AdamW semantics of the fused train step on the GPU: vault_adamw_step_torch against ``torch.optim.AdamW`` itself
(CPU, float64, single-tensor) within the bounds derived and calibrated in tests/test_optim_torch_host.py, its two forms (with
and without the weight average) against each other, the grid cap, the argument checks, ``TrainStep(optimizer="torch")`` end to
end, the state, the split data-parallel pass and the unchanged default path."""
import numpy as np
import pytest
import torch

from tests import test_optim_torch_host as H
from tests.optim_common import _Recurrence, _batch, _engine, _f32, _tiny
from vault_amd import ops
from vault_amd.train import TrainStep, adam_bias_corrections, ema_decay_at, hf_no_decay_groups, linear_schedule

pytestmark = pytest.mark.gpu

GRID_CAP_N = 8192 * 256 * 4 + 64 * 37      # the grid-stride loop takes a second, ragged trip
B1, B2, EPS = H.B1, H.B2, H.EPS


def _within(bnd, got, want, what):
    """p, m, v of the device against the float64 run, each figure printed before it is asserted."""
    worst = [bnd.worst(x.detach().cpu().numpy(), y, which) for x, y, which in zip(got, want, "pmv")]
    print(f"{what}: err / bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    for x, y, which in zip(got, want, "pmv"):
        err = np.abs(x.detach().cpu().numpy().astype(np.float64) - y)
        assert not (err > getattr(bnd, which)).any(), (what, which, int((err > getattr(bnd, which)).sum()), worst)


@pytest.fixture(scope="module")
def case():
    """The inputs of tests/test_optim_torch_host.py and the float64 reference for both gradient scales (the scales are powers
    of two: g / grad_scale is exact, and both formats see the same effective gradient g x float(f32(grad_scale) x f32(0.37)))."""
    c = H.make_case()
    c.el = np.repeat(c.gid, 64).astype(np.int64)
    c.ref, c.g64 = {}, {}
    for fmt, gscale in (("bf16", 0.5), ("fp16", 2.0 ** -12)):
        k = float(np.float32(gscale) * np.float32(H.COEF))
        c.g64[fmt] = [(g / np.float32(gscale)).astype(np.float32).astype(np.float64) * k for g in c.grads]
        c.ref[fmt] = list(H.torch_adamw_run(c.p0, c.el, c.g64[fmt], H.FACTORS))
    return c


def _launch(fmt, bufs, g, pb, case, t, gscale, dcoef, gmap, table, zm, ema=None, omd=1.0):
    inv_bc1, inv_sqrt_bc2 = adam_bias_corrections(B1, B2, t)
    with ops.operand_format(fmt):
        ops.adamw_step_torch(bufs[0], g, bufs[1], bufs[2], pb, case.n, gmap, table, H.FACTORS[t - 1], B1, B2, EPS, inv_bc1,
                             inv_sqrt_bc2, ema=ema, one_minus_decay=omd, grad_scale=gscale, coef=dcoef, zero_grad=True,
                             zero_mask=zm)


# ---- kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_kernel_follows_torch_adamw_in_float64(fmt, case):
    hdt = ops.HALF_DTYPE[fmt]
    gscale = 2.0 ** -12 if fmt == "fp16" else 0.5
    n = case.n
    p0 = torch.from_numpy(case.p0).cuda()
    bufs = [p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    pb0 = torch.full((n,), 3.0, dtype=hdt, device="cuda")    # (not p's image: a skipped block must leave the shadow alone)
    pb = pb0.clone()
    gmap = torch.from_numpy(case.gid).cuda()
    zm = torch.from_numpy(case.zmask).cuda()
    table = torch.tensor(H.GROUPS, dtype=torch.float32, device="cuda")
    dcoef = torch.tensor([H.COEF], dtype=torch.float32, device="cuda")
    el_idle = torch.from_numpy(np.repeat(case.idle, 64)).cuda()
    el_zero = torch.from_numpy(np.repeat(case.zmask.astype(bool), 64)).cuda()
    keep = el_idle & torch.from_numpy(case.el == 1).cuda()   # never touched, in the group without decay
    bnd = H.Bounds(case.p0, case.el)
    for t in range(1, H.T + 1):
        g0 = torch.from_numpy((case.grads[t - 1] / np.float32(gscale)).astype(np.float32)).cuda()
        g = g0.clone()
        _launch(fmt, bufs, g, pb, case, t, gscale, dcoef, gmap, table, zm)
        torch.cuda.synchronize()
        p64, m64, v64 = case.ref[fmt][t - 1]
        bnd.update(p64, case.g64[fmt][t - 1], v64, H.FACTORS[t - 1])
        _within(bnd, bufs, (p64, m64, v64), f"{fmt} step {t}")
        written = ~keep
        assert torch.equal(pb[written], bufs[0].to(hdt)[written]), t
        cleared = el_zero & ~keep
        assert not g[cleared].any() and torch.equal(g[~cleared], g0[~cleared]), t
        assert bool(g0[cleared].any())
        assert torch.equal(bufs[0][keep], p0[keep]) and torch.equal(pb[keep], pb0[keep]), t
        assert not bufs[1][keep].any() and not bufs[2][keep].any(), t
    # never-touched blocks of the groups WITH decay shrank, and their shadow followed
    dec = el_idle & ~keep
    assert bool((bufs[0][dec].abs() < p0[dec].abs()).all()) and int(keep.sum()) == 4 * 64 and int(dec.sum()) == 8 * 64


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_the_two_forms_agree_and_the_average_follows_the_recurrence(fmt, case):
    hdt = ops.HALF_DTYPE[fmt]
    gscale = 2.0 ** -12 if fmt == "fp16" else 0.5
    n = case.n
    p0 = torch.from_numpy(case.p0).cuda()
    A = [p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    Bf = [x.clone() for x in A]
    pba, pbb = p0.to(hdt), p0.to(hdt)
    gmap = torch.from_numpy(case.gid).cuda()
    zm = torch.from_numpy(case.zmask).cuda()
    table = torch.tensor(H.GROUPS, dtype=torch.float32, device="cuda")
    dcoef = torch.tensor([H.COEF], dtype=torch.float32, device="cuda")
    blocks = np.flatnonzero(case.idle & (case.gid == 1))    # the never-touched blocks without decay: 0, 1 start equal, 2, 3 apart
    el = lambda ks: torch.from_numpy(np.repeat(np.isin(np.arange(case.n64), ks), 64)).cuda()  # noqa: E731
    same, apart = el(blocks[:2]), el(blocks[2:])
    e0 = p0.clone()
    e0[apart] += 0.25
    ema = e0.clone()
    rec = _Recurrence(ema)
    omd = _f32(1.0 - 0.9)
    for t in range(1, H.T + 1):
        g0 = torch.from_numpy((case.grads[t - 1] / np.float32(gscale)).astype(np.float32)).cuda()
        ga, gb = g0.clone(), g0.clone()
        _launch(fmt, A, ga, pba, case, t, gscale, dcoef, gmap, table, zm)
        _launch(fmt, Bf, gb, pbb, case, t, gscale, dcoef, gmap, table, zm, ema=ema, omd=omd)
        torch.cuda.synchronize()
        for name, x, y in zip(("p", "m", "v", "shadow", "g"), A + [pba, ga], Bf + [pbb, gb]):
            assert torch.equal(x, y), (name, t)
        rec.step(Bf[0], omd)                                 # (the device's own p of this step)
        rec.check(ema, f"{fmt} step {t}")
        assert torch.equal(ema[same], p0[same]) and torch.equal(Bf[0][same], p0[same]), t
        assert torch.equal(Bf[0][apart], p0[apart]), t
    assert not torch.equal(A[0], p0) and not torch.equal(ema, Bf[0])
    assert not bool((ema[apart] == e0[apart]).any())         # the average moved where it started apart


def test_kernel_beyond_the_grid_cap():
    n = GRID_CAP_N
    n64 = n // 64
    rng = np.random.default_rng(9)
    p0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32)
    g0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    gid = rng.integers(0, 3, n64).astype(np.uint8)
    zmask = (rng.random(n64) > 0.3).astype(np.uint8)
    idle = rng.random(n64) < 0.05
    idle[-3:] = True                                         # (the ragged end too)
    g0[np.repeat(idle, 64)] = 0.0
    gid[-3:] = (0, 1, 2)
    el = np.repeat(gid, 64).astype(np.int64)
    k = float(np.float32(0.5) * np.float32(H.COEF))
    g64 = g0.astype(np.float64) * k
    (p64, m64, v64), = H.torch_adamw_run(p0, el, [g64], [0.75])
    bnd = H.Bounds(p0, el).update(p64, g64, v64, 0.75)
    bufs = [torch.from_numpy(p0).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    g = torch.from_numpy(g0).cuda()
    pb = bufs[0].to(torch.bfloat16)
    inv_bc1, inv_sqrt_bc2 = adam_bias_corrections(B1, B2, 1)
    with ops.operand_format("bf16"):
        ops.adamw_step_torch(bufs[0], g, bufs[1], bufs[2], pb, n, torch.from_numpy(gid).cuda(),
                             torch.tensor(H.GROUPS, dtype=torch.float32, device="cuda"), 0.75, B1, B2, EPS, inv_bc1, inv_sqrt_bc2,
                             grad_scale=0.5, coef=torch.tensor([H.COEF], dtype=torch.float32, device="cuda"), zero_grad=True,
                             zero_mask=torch.from_numpy(zmask).cuda())
    torch.cuda.synchronize()
    _within(bnd, bufs, (p64, m64, v64), "grid cap")
    tail = slice(n - 64 * 37, n)
    busy = torch.from_numpy(~np.repeat(idle, 64)[tail]).cuda()
    assert int(busy.sum()) >= 64 * 20 and bool((bufs[1][tail][busy] != 0).all())      # the ragged second trip ran ...
    assert bool((bufs[0][tail][busy] != torch.from_numpy(p0[tail]).cuda()[busy]).any())  # ... and moved the weights
    assert torch.equal(pb, bufs[0].to(torch.bfloat16))       # (the shadow started as p's image: skipped blocks agree too)
    keep = torch.from_numpy(np.repeat(idle & (gid == 1), 64)).cuda()
    assert torch.equal(bufs[0][keep], torch.from_numpy(p0).cuda()[keep]) and bool(keep[-128:-64].all())


def test_argument_errors():
    n = 64
    z = lambda: torch.zeros(n, device="cuda")  # noqa: E731
    p, g, m, v, ema = z(), z(), z(), z(), z()
    pb = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    gmap = torch.zeros(1, dtype=torch.uint8, device="cuda")
    zm = torch.ones(1, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[1e-3, 0.0]], dtype=torch.float32, device="cuda")
    wide = torch.zeros(257, 2, dtype=torch.float32, device="cuda")
    none = torch.zeros(0, 2, dtype=torch.float32, device="cuda")
    nan = float("nan")

    def call(p=p, g=g, m=m, v=v, n=n, gmap=gmap, table=table, bc1=1.5, bc2=2.0, ema=None, omd=1.0, zm=None):
        ops.adamw_step_torch(p, g, m, v, pb, n, gmap, table, 1.0, B1, B2, EPS, bc1, bc2, ema=ema, one_minus_decay=omd,
                             zero_mask=zm)

    bad = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-4), dict(n=6), dict(n=60, zm=zm),
           dict(table=wide), dict(table=none), dict(bc1=0.99), dict(bc2=0.5), dict(bc1=nan), dict(bc2=nan),
           dict(ema=ema, omd=0.0), dict(ema=ema, omd=1.5), dict(ema=ema, omd=nan), dict(ema=p)]
    with ops.operand_format("bf16"):
        for kw in bad:
            with pytest.raises(RuntimeError, match="EINVAL"):
                call(**kw)
        # a null map or table cannot pass the wrapper's own dtype checks: straight at the C entry point
        import ctypes as C
        from vault_amd import lib as L
        fn = L.load("bf16").vault_adamw_step_torch
        ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())  # noqa: E731
        for mp, tb in ((None, table), (gmap, None)):
            code = fn(ptr(p), ptr(g), ptr(m), ptr(v), ptr(pb), ptr(None), C.c_longlong(n), ptr(mp), ptr(tb), C.c_int(1),
                      C.c_float(1.0), C.c_float(B1), C.c_float(B2), C.c_float(EPS), C.c_float(1.5), C.c_float(2.0), C.c_float(1.0),
                      ptr(None), C.c_float(1.0), C.c_int(1), ptr(None), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            with pytest.raises(RuntimeError, match="EINVAL"):
                L.check(code, "vault_adamw_step_torch")
        torch.cuda.synchronize()
        assert not p.any() and not m.any() and not v.any()   # (nothing was launched)
        call(ema=ema, omd=1.0)                               # decay 0: the upper end of (0, 1] is valid
        call(omd=0.0)                                        # without an average one_minus_decay is not looked at
        call(bc1=1.0, bc2=1.0, zm=zm)
    torch.cuda.synchronize()


# ---- TrainStep ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ema_decay", [None, 0.9])
def test_train_step_with_the_torch_optimizer_end_to_end(monkeypatch, ema_decay):
    spec = _tiny()
    eng = _engine(spec)
    _, db, labels = _batch(spec, 21)
    seen = []
    real = ops.adamw_step_torch

    def recording(*a, **kw):
        n = int(a[5])
        seen.append(dict(g=a[1][:n].clone(), n=n, lr_factor=float(a[8]), bc=(float(a[12]), float(a[13])),
                         grad_scale=float(kw["grad_scale"]), coef=kw["coef"].clone()))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "adamw_step_torch", recording)
    step = TrainStep(eng, learning_rate=5e-4, weight_decay=0.1, warmup_ratio=0.3, total_steps=10,
                     param_groups=hf_no_decay_groups(eng), max_grad_norm=1e-2, optimizer="torch", ema_decay=ema_decay)
    P = eng.params
    nt = P.n_train
    p0 = P.p[:nt].clone()
    rec = None if ema_decay is None else _Recurrence(step.ema)
    for t in range(1, 4):
        step(db, labels)
        torch.cuda.synchronize()
        assert float(step.grad_norm) > 1e-2                  # it clipped
        if rec is not None:
            rec.step(P.p[:nt].clone(), _f32(1.0 - ema_decay_at(ema_decay, t, False)))
            rec.check(step.ema, f"train step {t}")
    assert step.step_idx == 3 and len(seen) == 3 and all(s["n"] == nt for s in seen)
    factors = [linear_schedule(1.0, s, 3, 10) for s in range(3)]
    assert factors == [0.0, 1.0 / 3.0, 2.0 / 3.0]
    for t, s in enumerate(seen, 1):
        assert s["bc"] == adam_bias_corrections(0.9, 0.999, t) and s["lr_factor"] == factors[t - 1], t
    # torch.optim.AdamW in float64 on the gradients the kernel read, scaled as the kernel scales them, with the same two groups
    el = np.repeat(step._group_map.cpu().numpy(), 64).astype(np.int64)
    assert el.size == nt and set(np.unique(el)) == {0, 1}
    groups = [(5e-4, 0.1), (5e-4, 0.0)]
    g64 = [s["g"].cpu().numpy().astype(np.float64) * float(np.float32(s["grad_scale"]) * np.float32(float(s["coef"][0])))
           for s in seen]
    p0_host = p0.cpu().numpy()
    bnd = H.Bounds(p0_host, el, groups=groups)
    for t, out in enumerate(H.torch_adamw_run(p0_host, el, g64, factors, groups=groups), 1):
        bnd.update(out[0], g64[t - 1], out[2], factors[t - 1])
    _within(bnd, (P.p[:nt], P.m[:nt], P.v[:nt]), out, f"TrainStep, ema_decay={ema_decay}, t = 3")
    assert not torch.equal(P.p[:nt], p0) and torch.equal(P.pb[:nt], P.p[:nt].to(torch.bfloat16))


def test_torch_optimizer_state_resumes_bit_for_bit_and_loads_into_the_hf_form():
    spec = _tiny()
    eng = _engine(spec)
    _, db, labels = _batch(spec, 23)
    opts = dict(learning_rate=5e-4, weight_decay=0.1, warmup_ratio=0.3, total_steps=10)
    step = TrainStep(eng, param_groups=hf_no_decay_groups(eng), optimizer="torch", **opts)
    for _ in range(2):
        step(db, labels)
    torch.cuda.synchronize()
    sd = step.state_dict()
    assert sd["hyper"]["optimizer"] == "torch" and sd["step_idx"] == 2
    P = eng.params
    eng2 = _engine(spec, state=P.state_dict_numpy())
    step2 = TrainStep(eng2, param_groups=hf_no_decay_groups(eng2), optimizer="torch", **opts)
    P2 = eng2.params
    step2.load_state_dict(sd)
    assert step2.step_idx == 2
    nt = P.n_train
    g = torch.randn(nt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 1e-3
    before = P.p.clone()
    for s_, P_ in ((step, P), (step2, P2)):
        P_.g[:nt].copy_(g)
        s_.optimizer_step()
    torch.cuda.synchronize()
    assert not torch.equal(P.p, before) and step.step_idx == step2.step_idx == 3
    for n in P.trainable:
        for name, a, b in (("p", P.p, P2.p), ("m", P.m, P2.m), ("v", P.v, P2.v), ("shadow", P.pb, P2.pb)):
            assert torch.equal(P._view(a, n), P2._view(b, n)), (name, n)
    # the moments mean the same in both forms: the state loads into an "hf" step, whose own arithmetic then holds
    hf = TrainStep(eng2, param_groups=hf_no_decay_groups(eng2), **opts)
    assert hf.state_dict()["hyper"]["optimizer"] == "hf"
    hf.load_state_dict(sd)
    assert hf.step_idx == 2
    for n in P.trainable:
        assert torch.equal(P2._view(P2.m, n).cpu(), sd["exp_avg"][n]) and torch.equal(P2._view(P2.v, n).cpu(), sd["exp_avg_sq"][n])


def test_default_train_step_never_reaches_the_torch_entry_point(monkeypatch):
    def forbidden(*a, **kw):
        raise AssertionError("the default TrainStep launched the torch-form AdamW")

    monkeypatch.setattr(ops, "adamw_step_torch", forbidden)
    spec = _tiny()
    eng = _engine(spec)
    _, db, labels = _batch(spec, 5)
    free = torch.cuda.memory_allocated()
    step = TrainStep(eng, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10)
    assert torch.cuda.memory_allocated() == free and step._group_map is None and step.optimizer == "hf"
    for _ in range(2):
        step(db, labels)
    torch.cuda.synchronize()
    assert step.step_idx == 2


def test_torch_optimizer_in_the_split_pass_over_rccl_single_rank(monkeypatch):
    """One rank over RCCL with VAULT_FORCE_DP=1 and no clipping: the optimizer runs on the reduced upper range while the last
    bucket is on the wire, then on the rest - two launches per step at the same t."""
    import os
    import torch.distributed as dist
    from vault_amd.train import BucketReducer
    monkeypatch.setattr(BucketReducer, "SINGLE_RANK_COLLECTIVES", True)
    calls = []
    real = ops.adamw_step_torch

    def counted(*a, **kw):
        calls.append((a[0].data_ptr(), int(a[5]), float(a[12]), float(a[13])))     # (p, n, both bias corrections)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "adamw_step_torch", counted)
    spec = _tiny()
    _, db, labels = _batch(spec, 41, B=8)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29653", VAULT_FORCE_DP="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        eng = _engine(spec)
        step = TrainStep(eng, learning_rate=5e-4, weight_decay=0.1, warmup_ratio=0.0, total_steps=10, bucket_mb=0.05, wire="fp32",
                         optimizer="torch")
        assert step.reducer is not None and step.reducer.native_a2a
        p0 = eng.params.p[:eng.params.n_train].clone()
        for _ in range(3):
            step(db, labels)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
        os.environ.pop("VAULT_FORCE_DP", None)
    P = eng.params
    nt = P.n_train
    assert step.step_idx == 3 and not torch.equal(P.p[:nt], p0)
    assert len(calls) == 6, calls                                        # two ranges per step ...
    base = P.p.data_ptr()
    for t in range(3):
        (p_hi, n_hi, *bc_hi), (p_lo, n_lo, *bc_lo) = calls[2 * t], calls[2 * t + 1]
        assert p_lo == base and p_hi == base + 4 * n_lo and n_hi + n_lo == nt and 0 < n_lo < nt   # ... that tile [0, n_train) ...
        assert tuple(bc_hi) == tuple(bc_lo) == adam_bias_corrections(0.9, 0.999, t + 1)          # ... at the same t
