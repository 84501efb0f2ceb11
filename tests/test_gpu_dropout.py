"""Every train-mode dropout site against the host restatement of its mask (tests/dropout_common.py).

No mask is stored: forward and backward each regenerate keep / drop from (seed, stream, element index), and every site computes
that index on its own.  Each test here has two parts:
  a. the kernel's mask is READ BACK from its outputs (zeros, or the untouched residual) and compared with the restatement for
     exact equality, in both operand formats (bf16 and fp16 builds);
  b. the values are compared with a float64 reference that applies the restated mask, under the bound the project already
     asserts for the same kernel without dropout (or one derived in the test's docstring).
The exact mask checks run at p = 0.5, where a transposed or mis-strided index agrees with the right one on half of the
positions only (tests/test_dropout_host.py).  Every test prints what it measured."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import dropout_common as D
from vault_amd import lib as L, ops
from vault_amd.spec import LMSpec, VaultSpec, ViltSpec, build_state

pytestmark = pytest.mark.gpu

FMTS = ["bf16", "fp16"]
MANT = {"bf16": 7, "fp16": 10}              # stored significand bits of the 16-bit formats
EMIN = {"bf16": -126, "fp16": -14}          # smallest normal exponent
F32 = np.float32


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _ulp16(x, fmt):
    """Spacing of the 16-bit format at |x| (float64 tensor)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -200))).clamp_min(EMIN[fmt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x.device), e - MANT[fmt])


def _scale(drop):
    return float(F32(drop.scale))               # the kernels receive the scale as a float


def _ln64(x, g, b, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double()


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
ROWS = 37                                       # not a multiple of the forward kernel's four rows per block
LN_CASES = [(256, (0, 0, 0)), (768, (0, 0, 0)), (256, (10, 13, 2)), (768, (10, 13, 2))]       # (H, row map with T = 10 < S = 13)
EPS = 1e-5


def _ln_inputs(H):
    x = _rand(ROWS, H, seed=1) * 2 + 0.3
    gam = 1 + 0.1 * _rand(H, seed=2)
    bet = 0.5 + 0.1 * _rand(H, seed=3)           # beta != 0: a kept output is never exactly 0
    return x, gam, bet


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("H,ymap", LN_CASES)
def test_layernorm_forward(H, ymap, p, fmt):
    """y = dropout(LN(x)) (+ post_add), keyed by the OUTPUT row: orow * H + c.  The zero pattern of the f32 and of the 16-bit
    output equals the restated mask exactly; with post_add the dropped elements are post_add bit for bit; kept elements against
    float64 LN(x) * scale (+ post) within 1e-4 * scale (the bound of test_layernorm_fwd_bwd, scaled); mean / rstd are those of
    the dropout-off launch bit for bit.
    Measured (MI355X, all cases, both formats): kept elements at most 7.3e-7 off at p = 0.1 (bound 1.1e-4), 1.3e-6 at p = 0.5
    (bound 2e-4)."""
    dt = ops.HALF_DTYPE[fmt]
    x, gam, bet = _ln_inputs(H)
    post = _rand(H, seed=4)
    drop = ops.Drop(p, seed=7, stream=3)
    phys = D.mapped_rows(ROWS, ymap)
    nphys = int(phys.max()) + 4
    pidx = torch.from_numpy(phys).cuda()
    new = lambda dtype=torch.float32: torch.full((nphys, H), 7.0, dtype=dtype, device="cuda")   # noqa: E731
    stat = lambda: torch.zeros(ROWS, device="cuda")                                              # noqa: E731
    y0, y0h, m0, r0 = new(), new(dt), stat(), stat()
    y1, y1h, m1, r1 = new(), new(dt), stat(), stat()
    y2 = new()
    with ops.operand_format(fmt):
        ops.layernorm_fwd(x, gam, bet, EPS, ROWS, H, y_bf16=y0h, y_f32=y0, mean=m0, rstd=r0, ymap=ymap)
        ops.layernorm_fwd(x, gam, bet, EPS, ROWS, H, y_bf16=y1h, y_f32=y1, mean=m1, rstd=r1, ymap=ymap, drop=drop)
        ops.layernorm_fwd(x, gam, bet, EPS, ROWS, H, y_f32=y2, ymap=ymap, drop=drop, post_add=post)
    torch.cuda.synchronize()
    keep = D.keep_rows(drop, ROWS, H, row_index=phys).cuda()
    assert not bool((y0[pidx] == 0).any()) and not bool((y0h[pidx] == 0).any())          # (nothing is 0 without dropout)
    assert torch.equal(y1[pidx] == 0, ~keep)
    assert torch.equal(y1h[pidx] == 0, ~keep)
    assert torch.equal(y2[pidx][~keep], post.expand(ROWS, H)[~keep])
    assert torch.equal(m1, m0) and torch.equal(r1, r0)
    other = torch.ones(nphys, dtype=torch.bool, device="cuda")
    other[pidx] = False
    for t in (y0, y1, y2, y0h, y1h):                                                      # rows outside the map: untouched
        assert bool((t[other] == 7.0).all())
    s = _scale(drop)
    ref = _ln64(x, gam, bet, EPS) * s
    e1 = float((y1[pidx].double() - ref)[keep].abs().max())
    e2 = float((y2[pidx].double() - ref - post.double())[keep].abs().max())
    print(f"LayerNorm forward H = {H} ymap = {ymap} p = {p} {fmt}: kept elements max |err| {e1:.2e} (with post_add {e2:.2e}), "
          f"bound {1e-4 * s:.2e}")
    assert e1 < 1e-4 * s and e2 < 1e-4 * s
    assert float((y1h[pidx].double() - y1[pidx].double()).abs().max()) <= float(ref.abs().max()) * 2.0 ** -(MANT[fmt] + 1)


def _ln_stats(x, gam, bet, H):
    mean = torch.zeros(ROWS, device="cuda"); rstd = torch.zeros(ROWS, device="cuda")
    y = torch.zeros(ROWS, H, device="cuda")
    ops.layernorm_fwd(x, gam, bet, EPS, ROWS, H, y_f32=y, mean=mean, rstd=rstd)
    return mean, rstd


def _spread(t, phys, nphys, fill=7.0):
    """Logical rows -> the physical rows of a row map, other rows = fill."""
    out = torch.full((nphys,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    out[torch.from_numpy(phys).to(t.device)] = t
    return out


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("H,dymap", LN_CASES)
def test_layernorm_backward_with_the_mask_on_the_incoming_gradient(H, dymap, p, fmt):
    """drop_on_dy (the embedding LayerNorm, y = dropout(LN(x))): the mask is keyed by the dy row.  dx, dgamma, dbeta against
    float64 autograd of mask * scale * LN(x) under the restated mask, bounds of test_layernorm_fwd_bwd.  At p = 0.5 a mask keyed
    by another row is wrong on half of the elements: errors of the size of the gradient itself.
    Measured (MI355X, all cases, both formats): dx at most 9.8e-7 (bounds 1.6e-4 .. 3.0e-4), dgamma 6.3e-6 (bounds 5.6e-3 or
    more), dbeta 3.9e-6 (bounds 4.7e-3 or more)."""
    dt = ops.HALF_DTYPE[fmt]
    x, gam, bet = _ln_inputs(H)
    drop = ops.Drop(p, seed=12345, stream=18)
    phys = D.mapped_rows(ROWS, dymap)
    nphys = int(phys.max()) + 4
    dy16 = _rand(ROWS, H, seed=5).to(dt)
    dy32 = _rand(ROWS, H, seed=6)
    dx = torch.zeros(ROWS, H, device="cuda"); dg = torch.zeros(H, device="cuda"); db = torch.zeros(H, device="cuda")
    with ops.operand_format(fmt):
        mean, rstd = _ln_stats(x, gam, bet, H)
        ops.layernorm_bwd(x, mean, rstd, gam, ROWS, H, dy_bf16=_spread(dy16, phys, nphys), dy_f32=_spread(dy32, phys, nphys),
                          dx_f32=dx, dgamma=dg, dbeta=db, dymap=dymap, drop=drop, drop_on_dy=True)
    torch.cuda.synchronize()
    keep = D.keep_rows(drop, ROWS, H, row_index=phys).cuda()
    xr = x.double().requires_grad_(True); gr = gam.double().requires_grad_(True); br = bet.double().requires_grad_(True)
    y = keep.double() * _scale(drop) * _ln64(xr, gr, br, EPS)
    y.backward(dy16.double() + dy32.double())
    ex = float((dx.double() - xr.grad).abs().max())
    eg = float((dg.double() - gr.grad).abs().max())
    eb = float((db.double() - br.grad).abs().max())
    tx = 5e-5 * max(1.0, float(xr.grad.abs().max()))
    tg = 2e-4 * float(gr.grad.abs().max()) + 1e-4
    tb = 2e-4 * float(br.grad.abs().max()) + 1e-4
    print(f"LayerNorm backward (mask on dy) H = {H} dymap = {dymap} p = {p} {fmt}: dx {ex:.2e} (bound {tx:.2e}), "
          f"dgamma {eg:.2e} ({tg:.2e}), dbeta {eb:.2e} ({tb:.2e})")
    assert ex < tx and eg < tg and eb < tb


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("H,dxmap", LN_CASES)
def test_layernorm_backward_with_the_mask_on_the_16_bit_branch(H, dxmap, p, fmt):
    """drop_on_dy = 0 (the partner of a residual GEMM with dropout: the 16-bit copy of dx is that GEMM's dY): keyed by the dx
    row.  dx_f32 equals the dropout-off launch bit for bit (and the float64 LayerNorm backward within the bound of
    test_layernorm_fwd_bwd); the zero pattern of the 16-bit dx is the restated mask exactly; kept elements lie within one 16-bit
    ulp of dx_f32 * scale; dbias = initial value + column sums of the masked branch within 2e-3 (the kernel adds the f32 values
    in front of the 16-bit rounding, as the dropout-off test's reference does).
    Measured (MI355X, all cases, both formats): dx_f32 at most 5.4e-7 from float64; kept 16-bit elements 0.500 ulp from
    dx_f32 * scale; dbias at most 2.5e-6 off."""
    dt = ops.HALF_DTYPE[fmt]
    x, gam, bet = _ln_inputs(H)
    drop = ops.Drop(p, seed=7, stream=3)
    phys = D.mapped_rows(ROWS, dxmap)
    nphys = int(phys.max()) + 4
    pidx = torch.from_numpy(phys).cuda()
    dy16 = _rand(ROWS, H, seed=5).to(dt)
    dy32 = _rand(ROWS, H, seed=6)
    out = {}
    with ops.operand_format(fmt):
        mean, rstd = _ln_stats(x, gam, bet, H)
        for name, d in (("off", ops.NO_DROP), ("on", drop)):
            dx32 = torch.full((nphys, H), 7.0, device="cuda")
            dx16 = torch.full((nphys, H), 7.0, dtype=dt, device="cuda")
            dbias = torch.ones(H, device="cuda")
            ops.layernorm_bwd(x, mean, rstd, gam, ROWS, H, dy_bf16=dy16, dy_f32=dy32, dx_f32=dx32, dx_bf16=dx16, dxmap=dxmap, drop=d,
                              drop_on_dy=False, dbias=dbias)
            out[name] = (dx32, dx16, dbias)
    torch.cuda.synchronize()
    keep = D.keep_rows(drop, ROWS, H, row_index=phys).cuda()
    dx32, dx16, dbias = out["on"]
    assert torch.equal(dx32, out["off"][0])
    assert not bool((out["off"][1][pidx] == 0).any())
    assert torch.equal(dx16[pidx] == 0, ~keep)
    other = torch.ones(nphys, dtype=torch.bool, device="cuda")
    other[pidx] = False
    assert bool((dx16[other] == 7.0).all()) and bool((dx32[other] == 7.0).all())
    xr = x.double().requires_grad_(True)
    _ln64(xr, gam, bet, EPS).backward(dy16.double() + dy32.double())
    e32 = float((dx32[pidx].double() - xr.grad).abs().max())
    assert e32 < 5e-5 * max(1.0, float(xr.grad.abs().max()))
    want = dx32[pidx].double() * _scale(drop)
    ulps = float(((dx16[pidx].double() - want).abs() / _ulp16(want, fmt))[keep].max())
    refb = 1.0 + (want * keep.double()).sum(0)
    eb = float((dbias.double() - refb).abs().max())
    print(f"LayerNorm backward (mask on the 16-bit dx) H = {H} dxmap = {dxmap} p = {p} {fmt}: dx_f32 {e32:.2e}, kept 16-bit dx "
          f"{ulps:.3f} ulp from dx_f32 * scale (bound 1), dbias {eb:.2e} (bound 2e-3)")
    assert ulps <= 1.0
    assert eb < 2e-3


# ------------------------------------------------------------------------------------------------------------ residual GEMM
EPI_RES = ops.EPI_F32_RES


def _gemm_inputs(M, N, K, fmt, seed):
    dt = ops.HALF_DTYPE[fmt]
    A = _rand(M, K, seed=seed).to(dt)
    W = _rand(N, K, scale=K ** -0.5, seed=seed + 1).to(dt)
    bias, res = _rand(N, seed=seed + 2), _rand(M, N, seed=seed + 3)
    z = A.double() @ W.double().t() + bias.double()
    return A, W, bias, res, z


def _gemm_check(launch, M, N, m_valid, drop, res, z, what):
    """Two launches of one configuration: on a zero residual the zero pattern of the output IS the mask (all elements, exact);
    on a random residual the dropped elements are the residual bit for bit, rows >= m_valid are untouched and the kept elements
    are (A W^T + bias) * scale + res within 2e-4 max|z| scale (the bound of test_forward_gelu_and_residual, scaled).  Returns
    the measured error / bound."""
    keep = D.keep_rows(drop, M, N).cuda()[:m_valid]
    zero = torch.zeros(M, N, device="cuda")
    out = torch.full((M, N), 7.0, device="cuda")
    launch(out, zero)
    torch.cuda.synchronize()
    assert torch.equal(out[:m_valid] == 0, ~keep), f"{what}: the zero pattern is not the restated mask"
    assert bool((out[m_valid:] == 7.0).all()), what
    out = torch.full((M, N), 7.0, device="cuda")
    launch(out, res)
    torch.cuda.synchronize()
    assert torch.equal(out[:m_valid][~keep], res[:m_valid][~keep]), f"{what}: a dropped element is not the residual"
    assert bool((out[m_valid:] == 7.0).all()), what
    s = _scale(drop)
    err = float(((out[:m_valid].double() - res[:m_valid].double()) - z[:m_valid] * s)[keep].abs().max())
    tol = 2e-4 * float(z.abs().max()) * s
    assert err <= tol, (what, err, tol)
    return err, tol


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 768, 192), (256, 768, 320)])
def test_residual_gemm_every_configuration(M, N, K, fmt):
    """out = dropout(A W^T + bias) + res, keyed by m * N + n (ldo == N), with the automatic choice and every explicit cfg 0..8:
    a configuration whose plan refuses must raise, one that launches must obey the mask (_gemm_check) - never an undropped
    output.  On MI355X, all three shapes, both formats: cfg -1 (plan 7), 0, 1, 2, 3, 7, 8 launch and obey; cfg 4 does so at
    N = 768 and refuses N = 256 (no 192-wide tiles) at launch, after a plan of 4, `out` untouched; cfg 5 / 6 (8-wave kernel: no
    dropout in its residual epilogue) refuse in the plan.  Measured: kept elements at most 2.4e-6 off, bounds 2.3e-3 or more."""
    A, W, bias, res, z = _gemm_inputs(M, N, K, fmt, seed=50)
    drop = ops.Drop(0.5, seed=12345, stream=18)
    m_valid = M - 37
    log = []
    with ops.operand_format(fmt):
        for cfg in range(-1, 9):
            def launch(out, r, **kw):
                return ops.gemm(A, W, out, M, N, K, K, K, N, 0, 0, EPI_RES, cfg=cfg, m_valid=m_valid, bias=bias, res=r, drop=drop, **kw)
            plan = launch(res, res, plan_only=True)
            probe = torch.full((M, N), 7.0, device="cuda")
            if plan < 0:
                with pytest.raises(RuntimeError):
                    launch(probe, res)
                log.append(f"cfg {cfg}: refused by the plan")
            else:
                try:
                    launch(probe, res)
                except RuntimeError:
                    log.append(f"cfg {cfg}: plan {plan}, refused at launch")
                else:
                    err, tol = _gemm_check(launch, M, N, m_valid, drop, res, z, f"cfg {cfg} (plan {plan})")
                    log.append(f"cfg {cfg}: plan {plan}, mask exact, kept max |err| {err:.2e} (bound {tol:.2e})")
                    continue
            torch.cuda.synchronize()
            assert bool((probe == 7.0).all()), f"cfg {cfg}: a refused launch wrote to out"
    print(f"residual GEMM with dropout ({M}, {N}, {K}) {fmt}:\n  " + "\n  ".join(log))
    assert log[0].startswith("cfg -1: plan") and "mask exact" in log[0]          # the automatic choice always has a kernel


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("panels,K,want_plan", [(70, 64, None), (86, 512, 4)])
def test_residual_gemm_keeps_the_global_offset_where_the_tail_cut_would_split(panels, K, want_plan, fmt):
    """N = 768 with more 256 x 192 tiles than one round of 256, automatic choice.  vault_gemm moves the row panels behind the
    last full round of a cfg 4 launch to a second launch on another `out` pointer (gemm.hip, tail of the last round); masks are
    keyed by the offset from `out`, so dropout must switch that cut off: every row panel obeys the one global mask.
    (256 x 70, 768, 64) is the case as first stated: 280 tiles, but its plan is a configuration that never cuts.
    (256 x 86, 768, 512) is the smallest row count whose plan WITHOUT dropout is cfg 4 with a cut (344 tiles: 64 panels in the
    full round, 22 behind it).
    Measured (MI355X): plans 2 and 4, the same with and without dropout; kept elements at most 1.9e-6 / 4.3e-6 off (bound 3.1e-3)."""
    M, N = 256 * panels, 768
    A, W, bias, res, z = _gemm_inputs(M, N, K, fmt, seed=60)
    drop = ops.Drop(0.5, seed=7, stream=3)
    m_valid = M - 37
    with ops.operand_format(fmt):
        def launch(out, r, **kw):
            return ops.gemm(A, W, out, M, N, K, K, K, N, 0, 0, EPI_RES, cfg=-1, m_valid=m_valid, bias=bias, res=r, **kw)
        plan_off, plan = launch(res, res, plan_only=True), launch(res, res, plan_only=True, drop=drop)
        assert plan >= 0 and (want_plan is None or plan_off == want_plan)
        err, tol = _gemm_check(lambda o, r: launch(o, r, drop=drop), M, N, m_valid, drop, res, z, f"plan {plan}")
    print(f"residual GEMM with dropout ({M}, {N}, {K}) {fmt}: plan {plan} (without dropout {plan_off}), mask exact over all {panels} "
          f"row panels, kept max |err| {err:.2e} (bound {tol:.2e})")


@pytest.mark.parametrize("fmt", FMTS)
def test_residual_gemm_split_k_inside_the_launch(fmt):
    """(768, 768, 1536), cfg 4 with three K splits and a workspace (the LM stack's FFN-out at small batches, stage.hip): the
    split that draws the last ticket runs the epilogue, and with it the dropout - it must obey the mask or refuse.
    On MI355X it launches and obeys, in both formats: kept elements at most 2.2e-6 off (bound 2.7e-3); the tile counters are
    zero again afterwards."""
    M, N, K, splits = 768, 768, 1536, 3
    A, W, bias, res, z = _gemm_inputs(M, N, K, fmt, seed=70)
    drop = ops.Drop(0.5, seed=0, stream=1)
    m_valid = M - 37
    ws = torch.zeros(16384 + (M // 256) * (N // 192) * splits * 256 * 192 * 4, dtype=torch.uint8, device="cuda")
    with ops.operand_format(fmt):
        def launch(out, r, **kw):
            return ops.gemm(A, W, out, M, N, K, K, K, N, 0, 0, EPI_RES, cfg=4, splits=splits, splitk_ws=ws, m_valid=m_valid, bias=bias,
                            res=r, drop=drop, **kw)
        plan = launch(res, res, plan_only=True)
        if plan < 0:
            with pytest.raises(RuntimeError):
                launch(torch.zeros(M, N, device="cuda"), res)
            print(f"split-K residual GEMM with dropout {fmt}: refused by the plan")
            return
        err, tol = _gemm_check(launch, M, N, m_valid, drop, res, z, "cfg 4, 3 splits")
    assert int(ws[:16384].view(torch.int32).abs().max()) == 0
    print(f"split-K residual GEMM with dropout {fmt}: plan {plan}, mask exact, kept max |err| {err:.2e} (bound {tol:.2e})")


def test_residual_gemm_mxfp8_zero_pattern():
    """vault_gemm_mxfp8 takes the dropout members with the residual epilogue (the shared epilogue of gemm_epi.h): (256, 768, 256),
    the zero pattern on a zero residual is the restated mask; the dropout-off launch has no zero at all."""
    M, N, K = 256, 768, 256
    A = _rand(M, K, seed=80).bfloat16(); W = _rand(N, K, scale=K ** -0.5, seed=81).bfloat16()
    bias = _rand(N, seed=82)
    drop = ops.Drop(0.5, seed=12345, stream=18)
    q = lambda t: (torch.empty(t.shape, dtype=torch.uint8, device="cuda"), torch.empty(t.shape[0], K // 32, dtype=torch.uint8, device="cuda"))   # noqa: E731
    (qa, sa), (qw, sw) = q(A), q(W)
    ops.quant_mxfp8(A, M, K, K, qa, sa)
    ops.quant_mxfp8(W, N, K, K, qw, sw)
    zero = torch.zeros(M, N, device="cuda")
    plan = ops.gemm_mxfp8(qa, sa, qw, sw, zero, M, N, K, N, EPI_RES, bias=bias, res=zero, drop=drop, plan_only=True)
    assert plan >= 0
    o0 = torch.full((M, N), 7.0, device="cuda"); o1 = torch.full((M, N), 7.0, device="cuda")
    ops.gemm_mxfp8(qa, sa, qw, sw, o0, M, N, K, N, EPI_RES, bias=bias, res=zero)
    ops.gemm_mxfp8(qa, sa, qw, sw, o1, M, N, K, N, EPI_RES, bias=bias, res=zero, drop=drop)
    torch.cuda.synchronize()
    keep = D.keep_rows(drop, M, N).cuda()
    assert not bool((o0 == 0).any())
    assert torch.equal(o1 == 0, ~keep)
    assert torch.equal(o1[keep], (o0 * F32(drop.scale))[keep])           # kept: the same f32 value times the scale, one rounding
    print(f"MXFP8 residual GEMM with dropout: plan {plan}, mask exact")


# --------------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("H", [256, 768])
def test_head_forward_and_backward(H, fmt):
    """logits = dropout(tanh(pre)) Wc^T + bc, keyed by b * H + n, the mask applied behind the tanh: pooled equals the dropout-off
    launch bit for bit, the zero pattern of dpre is the restated mask exactly.  logits, dWc, dbc, dpre against float64 computed
    FROM THE KERNEL'S OWN pooled (tanhf's accuracy stays out), bounds of f32 summation:
      logits   2 H 2^-24 sum_n |z_n W_cn| + 2^-23 |logit|      (H products and adds per wave-reduced sum)
      dWc, dbc 2 B 2^-24 sum_b |term_b| + 2^-23 |result|       (zero-initialised, one launch: atomicAdds over B terms)
      dpre     one 16-bit ulp; Wc and dlogits are positive, so that the three-term f32 sum Wc^T dlogits cannot cancel.
    Measured (MI355X), error / bound at most: logits below 5e-4, dWc 0.15, dbc 0.073, dpre 0.500 ulp."""
    B, Cn, p = 5, 3, 0.5
    dt = ops.HALF_DTYPE[fmt]
    pre = _rand(B, H, seed=90) * 0.7
    Wc = 0.02 + 0.05 * _rand(Cn, H, seed=91).abs()
    bc = _rand(Cn, seed=92)
    dlog = 0.3 + _rand(B, Cn, seed=93).abs()
    drop = ops.Drop(p, seed=7, stream=3)
    z = lambda *s, d=torch.float32: torch.zeros(*s, dtype=d, device="cuda")   # noqa: E731
    pooled0, logits0, pooled, logits = z(B, H), z(B, Cn), z(B, H), z(B, Cn)
    dWc, dbc, dpre = z(Cn, H), z(Cn), torch.full((B, H), 7.0, dtype=dt, device="cuda")
    with ops.operand_format(fmt):
        ops.head_fwd(pre, Wc, bc, None, pooled0, logits0, None, B, H, Cn, 1.0)
        ops.head_fwd(pre, Wc, bc, None, pooled, logits, None, B, H, Cn, 1.0, drop=drop)
        ops.head_bwd(pooled, logits, None, Wc, dWc, dbc, dpre, B, H, Cn, 1.0, dlogits=dlog, drop=drop)
    torch.cuda.synchronize()
    keep = D.keep_rows(drop, B, H).cuda()
    assert torch.equal(pooled, pooled0) and not torch.equal(logits, logits0)
    assert torch.equal(dpre == 0, ~keep)
    u = 2.0 ** -24
    t = pooled.double()
    zz = t * keep.double() * _scale(drop)                                     # [B, H]
    W64, dl = Wc.double(), dlog.double()
    ref = zz @ W64.t() + bc.double()
    bound = 2 * H * u * (zz.abs() @ W64.abs().t()) + 2 * u * ref.abs()
    r_log = float(((logits.double() - ref).abs() / bound).max())
    ref = dl.t() @ zz
    bound = 2 * B * u * (dl.abs().t() @ zz.abs()) + 2 * u * ref.abs()
    live = bound > 0                                                          # (a column every sample dropped: exactly 0)
    assert bool((dWc[~live] == 0).all())
    r_w = float(((dWc.double() - ref).abs()[live] / bound[live]).max())
    ref = dl.sum(0)
    bound = 2 * B * u * dl.abs().sum(0) + 2 * u * ref.abs()
    r_b = float(((dbc.double() - ref).abs() / bound).max())
    ref = (dl @ W64) * keep.double() * _scale(drop) * (1.0 - t * t)
    r_p = float(((dpre.double() - ref).abs() / _ulp16(ref, fmt))[keep].max())
    print(f"head H = {H} {fmt}: error / bound: logits {r_log:.3f}, dWc {r_w:.3f}, dbc {r_b:.3f}, dpre {r_p:.3f} ulp")
    assert r_log <= 1.0 and r_w <= 1.0 and r_b <= 1.0 and r_p <= 1.0


# ---------------------------------------------------------------------------------------------------------------- attention
ATT_B, ATT_HEADS = 2, 3                       # bh = b * heads + h with both factors > 1
# the two edges of each kernel family (S <= 64, <= 192, <= 288, <= 320) and a partial tile; p = 0.1 on two shapes
ATT_CASES = [(S, 0.5) for S in (17, 40, 64, 70, 129, 192, 193, 288, 289, 320)] + [(40, 0.1), (185, 0.1)]
REL16 = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}


@lru_cache(maxsize=4)
def _attn_case(S, fmt):
    """qkv [M, 3H] (q, k ~ 0.5 N(0, 1): every probability far above the 16-bit underflow), the key mask (one masked span on
    sample 1) and the float64 probabilities."""
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    dt = ops.HALF_DTYPE[fmt]
    qkv = _rand(M, 3 * H, seed=100 + S)
    qkv[:, :2 * H] *= 0.5
    qkv = qkv.to(dt)
    keymask = torch.ones(B, S, device="cuda")
    keymask[1, 5:min(17, S - 1)] = 0
    q, k, v = qkv.double().view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    s = s.masked_fill(keymask[:, None, None, :] == 0, float("-inf"))
    P = torch.softmax(s, dim=-1)
    live = (keymask != 0)[:, None, None, :].expand(B, heads, S, S)
    assert float(P[live].min()) > 2.0 ** -13
    return qkv, keymask, P, live


def _fwd(qkv, keymask, S, drop, fmt, pad=16, **kw):
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    ctx = torch.full((M + pad, H), 7.0, dtype=ops.HALF_DTYPE[fmt], device="cuda")
    lse = torch.zeros(B, heads, S, device="cuda")
    ops.attention_fwd(qkv, keymask, ctx, lse, B, S, H, heads, drop=drop, **kw)
    return ctx, lse


def _one_hot_block(S, j, dt):
    """[S, 64]: row r has a one in column r - 64 j for the rows of block j (64 j <= r < 64 j + 64), zeros elsewhere."""
    t = torch.zeros(S, 64, dtype=dt, device="cuda")
    r = torch.arange(64 * j, min(S, 64 * j + 64), device="cuda")
    t[r, r - 64 * j] = 1
    return t


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("S,p", ATT_CASES)
def test_attention_forward_probabilities_read_through_one_hot_values(S, p, fmt):
    """With V one-hot over key block j (V[k, k - 64 j] = 1), ctx[q, c] IS the dropped, scaled probability of (q, 64 j + c):
    ceil(S / 64) launches read the whole [B, heads, S, S] matrix out of the kernel.  Its zero pattern on live keys equals the
    restated mask (index ((b heads + h) S + q) S + k) exactly, masked keys are 0, the kept values are float64 softmax * scale
    within 2^-7 (bf16) / 2^-10 (fp16) relative - two 16-bit roundings (un-normalised p, then ctx), factor 2 of margin - and lse
    equals the dropout-off launch bit for bit.
    Measured (MI355X), worst over the shapes: 2^-7.05 (bf16), 2^-10.05 (fp16) - the two roundings at their worst at once."""
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    dt = ops.HALF_DTYPE[fmt]
    qkv, keymask, P, live = _attn_case(S, fmt)
    drop = ops.Drop(p, seed=12345, stream=18)
    Pt = torch.zeros(B, heads, S, S, dtype=torch.float64, device="cuda")
    with ops.operand_format(fmt):
        _, lse0 = _fwd(qkv, keymask, S, ops.NO_DROP, fmt)
        for j in range((S + 63) // 64):
            qj = qkv.clone()
            qj.view(B, S, 3, heads, 64)[:, :, 2] = _one_hot_block(S, j, dt)[None, :, None, :]
            ctx, lse = _fwd(qj, keymask, S, drop, fmt)
            torch.cuda.synchronize()
            assert torch.equal(lse, lse0)
            assert bool((ctx[M:] == 7.0).all())                                  # nothing is written behind the last sequence
            w = min(64, S - 64 * j)
            Pt[:, :, :, 64 * j:64 * j + w] = ctx[:M].double().view(B, S, heads, 64).permute(0, 2, 1, 3)[..., :w]
            assert bool((ctx[:M].view(B, S, heads, 64)[..., w:] == 0).all())     # columns of keys >= S
    keep = D.keep_attn(drop, B, heads, S).cuda()
    assert bool((Pt[~live] == 0).all())
    assert torch.equal((Pt == 0)[live], (~keep)[live])
    want = P * _scale(drop)
    sel = live & keep
    rel = float(((Pt - want).abs() / want)[sel].max())
    print(f"attention forward S = {S} p = {p} {fmt}: mask exact over {int(live.sum())} probabilities, kept values within "
          f"2^{math.log2(rel):.2f} relative (bound 2^{math.log2(REL16[fmt]):.0f})")
    assert rel <= REL16[fmt]


def _bwd(qkv, keymask, ctx, lse, dctx, S, drop, fmt, **kw):
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    dqkv = torch.full((M + 16, 3 * H), 7.0, dtype=ops.HALF_DTYPE[fmt], device="cuda")
    ops.attention_bwd(qkv, keymask, ctx, lse, dctx, dqkv, B, S, H, heads, drop=drop, **kw)
    return dqkv


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("S,p", ATT_CASES)
def test_attention_backward_mask_read_through_one_hot_gradients(S, p, fmt):
    """The same trick on the dV path: with dctx one-hot over query block j (dctx[q, q - 64 j] = 1), dV[k, c] is the dropped
    probability of (64 j + c, k) - the mask as the BACKWARD regenerates it, from its transposed tile walk.  Zero pattern on live
    keys == the restated mask, exactly; masked keys receive 0.
    Measured (MI355X): kept values within 2^-8.01 (bf16) / 2^-11.00 (fp16) relative of float64 softmax * scale."""
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    dt = ops.HALF_DTYPE[fmt]
    qkv, keymask, P, live = _attn_case(S, fmt)
    drop = ops.Drop(p, seed=12345, stream=18)
    Pt = torch.zeros(B, heads, S, S, dtype=torch.float64, device="cuda")
    with ops.operand_format(fmt):
        ctx, lse = _fwd(qkv, keymask, S, drop, fmt)
        for j in range((S + 63) // 64):
            dctx = torch.zeros(M, H, dtype=dt, device="cuda")
            dctx.view(B, S, heads, 64)[:] = _one_hot_block(S, j, dt)[None, :, None, :]
            dqkv = _bwd(qkv, keymask, ctx, lse, dctx, S, drop, fmt)
            torch.cuda.synchronize()
            assert bool((dqkv[M:] == 7.0).all())
            dv = dqkv[:M].double().view(B, S, 3, heads, 64)[:, :, 2].permute(0, 2, 3, 1)        # [B, heads, c, k]
            w = min(64, S - 64 * j)
            Pt[:, :, 64 * j:64 * j + w, :] = dv[:, :, :w]
            assert bool((dv[:, :, w:] == 0).all())                              # no query behind the sequence contributes
    keep = D.keep_attn(drop, B, heads, S).cuda()
    assert bool((Pt[~live] == 0).all())
    assert torch.equal((Pt == 0)[live], (~keep)[live])
    sel = live & keep
    rel = float(((Pt - P * _scale(drop)).abs() / (P * _scale(drop)))[sel].max())
    print(f"attention backward (dV path) S = {S} p = {p} {fmt}: mask exact, kept values within 2^{math.log2(rel):.2f} relative")
    assert rel <= 2 * REL16[fmt]          # (not a bound of the issue: the recomputed probabilities are sane, nothing more)


def _attn_grad64(qkv, keymask, keep, scale, dctx, S, rows=None):
    """float64 autograd of softmax -> mask * scale -> @ V; ``rows``: only these query rows of every item receive a gradient."""
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    s = s.masked_fill(keymask[:, None, None, :] == 0, float("-inf"))
    o = (torch.softmax(s, dim=-1) * keep.double() * scale) @ v
    o = o.permute(0, 2, 1, 3).reshape(M, H)
    g = dctx.double()
    if rows is not None:
        m = torch.zeros(B, S, 1, dtype=torch.float64, device="cuda")
        m[:, rows] = 1
        g = (g.view(B, S, H) * m).view(M, H)
    o.backward(g)
    return x.grad


def _grad_errors(d, g, what):
    B = ATT_B
    e_max = float((d - g).abs().max() / g.abs().max())
    e_fro = float((d - g).norm() / g.norm())
    e_per = float(((d - g).view(B, -1).norm(dim=1) / g.view(B, -1).norm(dim=1)).max())
    print(f"{what}: max |err| / max |g| {e_max:.2e} (bound 3e-2), Frobenius {e_fro:.2e} (1e-2), worst sample {e_per:.2e} (1.5e-2)")
    assert e_max < 3e-2 and e_fro < 1e-2 and e_per < 1.5e-2


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("S,p", ATT_CASES)
def test_attention_backward_gradient(S, p, fmt):
    """dq, dk, dv for random dctx and V against float64 autograd of softmax -> mask * scale -> @ V under the restated mask:
    the three bounds the project applies to these kernels without dropout.  A wrong index on the dP path at p = 0.5 errs by
    tens of percent.
    Measured (MI355X), worst over the shapes: bf16 max 3.4e-3, Frobenius 2.4e-3, per sample 2.4e-3; fp16 5.0e-4, 3.0e-4, 3.0e-4."""
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    dt = ops.HALF_DTYPE[fmt]
    qkv, keymask, P, live = _attn_case(S, fmt)
    drop = ops.Drop(p, seed=7, stream=3)
    dctx = _rand(M, H, seed=11).to(dt)
    with ops.operand_format(fmt):
        ctx, lse = _fwd(qkv, keymask, S, drop, fmt)
        dqkv = _bwd(qkv, keymask, ctx, lse, dctx, S, drop, fmt)
    torch.cuda.synchronize()
    keep = D.keep_attn(drop, B, heads, S).cuda()
    g = _attn_grad64(qkv, keymask, keep, _scale(drop), dctx, S)
    _grad_errors(dqkv[:M].double(), g, f"attention backward S = {S} p = {p} {fmt}")
    # and the forward values of the same launch, as test_attention_fwd_bwd bounds them
    q, k, v = qkv.double().view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref = ((P * keep.double() * _scale(drop)) @ v).permute(0, 2, 1, 3).reshape(M, H)
    assert float((ctx[:M].double() - ref).abs().max()) < 2e-2 * float(ref.abs().max())


def _to_head_major(x, R):
    M, N = x.shape
    out = torch.zeros(N // 64, R, 64, dtype=x.dtype, device=x.device)
    out[:, :M] = x.view(M, N // 64, 64).permute(1, 0, 2)
    return out


def _from_head_major(y, M):
    Pn, R, _ = y.shape
    return y[:, :M].permute(1, 0, 2).reshape(M, Pn * 64)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("S", [40, 129])
def test_attention_head_major_layout_with_dropout(S, fmt):
    """``qkv_hm`` at p = 0.5: context, log-sum-exp and the gradient equal the row-major run (itself pinned above) bit for bit."""
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    R = ((M + 255) // 256) * 256 + 256
    dt = ops.HALF_DTYPE[fmt]
    qkv, keymask, _, _ = _attn_case(S, fmt)
    drop = ops.Drop(0.5, seed=7, stream=3)
    dctx = _rand(M, H, seed=11).to(dt)
    with ops.operand_format(fmt):
        ctx, lse = _fwd(qkv, keymask, S, drop, fmt)
        dqkv = _bwd(qkv, keymask, ctx, lse, dctx, S, drop, fmt)
        qh = _to_head_major(qkv, R)
        ctx2, lse2 = _fwd(qh, keymask, S, drop, fmt, qkv_hm=R)
        dqh = torch.full((3 * heads, R, 64), 7.0, dtype=dt, device="cuda")
        ops.attention_bwd(qh, keymask, ctx2, lse2, dctx, dqh, B, S, H, heads, drop=drop, qkv_hm=R)
    torch.cuda.synchronize()
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2)
    assert torch.equal(_from_head_major(dqh, M), dqkv[:M])
    assert bool((dqh[:, M:] == 7.0).all())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("S", [40, 129])
def test_attention_one_live_query_with_dropout(S, fmt):
    """``q_rows = 1`` at p = 0.5 (compact ctx / dctx, [B][H]): row 0 of the mask read through one-hot V is exact, and the
    backward matches the float64 reference in which only query 0 of every item receives a gradient.
    Measured (MI355X), worst: bf16 max 2.4e-3, Frobenius 2.3e-3, per sample 2.4e-3; fp16 3.5e-4, 2.9e-4, 3.0e-4."""
    B, heads = ATT_B, ATT_HEADS
    H, M, Bp = heads * 64, B * S, 256
    dt = ops.HALF_DTYPE[fmt]
    qkv, keymask, P, live = _attn_case(S, fmt)
    drop = ops.Drop(0.5, seed=12345, stream=18)
    keep = D.keep_attn(drop, B, heads, S).cuda()
    P0 = torch.zeros(B, heads, S, dtype=torch.float64, device="cuda")
    lse = torch.full((B, heads, S), 5.0, device="cuda")
    with ops.operand_format(fmt):
        for j in range((S + 63) // 64):
            qj = qkv.clone()
            qj.view(B, S, 3, heads, 64)[:, :, 2] = _one_hot_block(S, j, dt)[None, :, None, :]
            c = torch.full((Bp, H), 7.0, dtype=dt, device="cuda")
            ops.attention_fwd(qj, keymask, c, lse, B, S, H, heads, drop=drop, q_rows=1)
            torch.cuda.synchronize()
            assert bool((c[B:] == 7.0).all())
            w = min(64, S - 64 * j)
            P0[:, :, 64 * j:64 * j + w] = c[:B].double().view(B, heads, 64)[..., :w]
        live0, keep0 = live[:, :, 0], keep[:, :, 0]
        assert bool((P0[~live0] == 0).all())
        assert torch.equal((P0 == 0)[live0], (~keep0)[live0])
        want = P[:, :, 0] * _scale(drop)
        assert float(((P0 - want).abs() / want)[live0 & keep0].max()) <= REL16[fmt]
        # backward: compact ctx / lse of the real V, compact dctx
        ctx_c = torch.zeros(Bp, H, dtype=dt, device="cuda")
        ops.attention_fwd(qkv, keymask, ctx_c, lse, B, S, H, heads, drop=drop, q_rows=1)
        dctx_c = _rand(Bp, H, seed=12).to(dt)
        dqkv = _bwd(qkv, keymask, ctx_c, lse, dctx_c, S, drop, fmt, q_rows=1)
    torch.cuda.synchronize()
    dctx = torch.zeros(M, H, dtype=dt, device="cuda")
    dctx.view(B, S, H)[:, 0] = dctx_c[:B]
    g = _attn_grad64(qkv, keymask, keep, _scale(drop), dctx, S, rows=[0])
    d = dqkv[:M].double()
    assert float(d.view(B, S, 3 * H)[:, 1:, :H].abs().max()) == 0.0              # dq of the other queries
    _grad_errors(d, g, f"attention backward, one live query, S = {S} {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("S,thirds", [(40, 3), (129, 1)])
def test_attention_bias_partials_with_dropout(S, thirds, fmt):
    """``bias_partials`` at p = 0.5: dqkv is bit-identical to the launch without them and the partial sums add up to the
    column sums of the stored dqkv, within the tolerance of
    test_attention_backward_leaves_the_qkv_bias_gradient_as_partial_sums (un-rounded sums against sums of 16-bit values).
    Measured (MI355X): bf16 1.7e-2 (bound 4.2e-2) and 4.5e-3 (3.7e-2); fp16 1.4e-3 (5.3e-3) and 6.8e-4 (4.7e-3)."""
    B, heads = ATT_B, ATT_HEADS
    H, M = heads * 64, B * S
    dt = ops.HALF_DTYPE[fmt]
    qkv, keymask, _, _ = _attn_case(S, fmt)
    drop = ops.Drop(0.5, seed=7, stream=3)
    dctx = _rand(M, H, seed=11).to(dt)
    with ops.operand_format(fmt):
        ctx, lse = _fwd(qkv, keymask, S, drop, fmt)
        d0 = _bwd(qkv, keymask, ctx, lse, dctx, S, drop, fmt)
        n = ops.attention_bwd_partials(B, S, H, heads, thirds)
        assert n == B * heads
        part = torch.full((n, thirds * H), 3.0, device="cuda")
        d1 = _bwd(qkv, keymask, ctx, lse, dctx, S, drop, fmt, bias_partials=part, bias_thirds=thirds)
        out = torch.full((thirds * H + 64,), 0.25, device="cuda")
        ops.colsum_partials(part, n, thirds * H, out)
    torch.cuda.synchronize()
    assert torch.equal(d0, d1)
    dq = d1[:M].float()
    ref, got = dq[:, :thirds * H].sum(0), out[:thirds * H] - 0.25
    tol = 2.0 ** -(MANT[fmt] + 1) * float(dq.abs().max()) * M ** 0.5 + 1e-4
    err = float((got - ref).abs().max())
    print(f"attention bias partials S = {S} thirds = {thirds} {fmt}: {err:.2e} (bound {tol:.2e})")
    assert err <= tol
    assert float((got - ref).norm() / ref.norm()) < 5e-3
    assert float((out[thirds * H:] - 0.25).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------- one LM layer, end to end
def _pad(n, m=256):
    return (n + m - 1) // m * m


@pytest.mark.parametrize("fmt", FMTS)
def test_lm_layer_one_c_call_forward_and_backward_with_dropout(fmt):
    """The dropout-on twin of test_gpu_stage.py::test_lm_layer_one_c_call_forward_and_backward: the same tiny layer (B = 5,
    S = 40, H = 256, FF = 512, 4 heads) with attention and hidden dropout at p = 0.1, seed 1234, stream base 16.  The float64
    reference is the post-LN layer written out below, with keep_attn on stream base + 2 and keep_rows (key m * H + n of the
    padded [Mp, H] buffers) on base + 3 (attention-out) and base + 4 (FFN-out); the assertions and bounds are the twin's - 2e-2
    on the output, 2e-2 / 3e-2 on gradient norms - and the weight gradients include g_wqkv, which depends on the attention mask.
    Measured (MI355X): output 2.4e-4 (bf16) / 2.9e-5 (fp16) of max |y|; dx 3.0e-4 / 3.7e-5; worst weight gradient (g_wqkv)
    3.7e-3 / 4.6e-4."""
    dt = ops.HALF_DTYPE[fmt]
    lm = LMSpec(vocab_size=64, max_position_embeddings=50, hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                intermediate_size=512, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    spec = VaultSpec(vilt=ViltSpec(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=512,
                                   vocab_size=64), lm=lm, n_classes=0)
    state = build_state(spec, 5)
    B, S, H, FF, heads = 5, 40, 256, 512, 4
    M, Mp = B * S, _pad(B * S)
    dev = "cuda"
    pre = "bert.encoder.layer.0"
    w = lambda n: torch.from_numpy(state[f"{pre}.{n}"]).to(dev)  # noqa: E731
    att = "attention.self"
    W = dict(wqkv=torch.cat([w(f"{att}.query.weight"), w(f"{att}.key.weight"), w(f"{att}.value.weight")], 0).to(dt).contiguous(),
             bqkv=torch.cat([w(f"{att}.query.bias"), w(f"{att}.key.bias"), w(f"{att}.value.bias")], 0).contiguous(),
             wo=w("attention.output.dense.weight").to(dt), bo=w("attention.output.dense.bias"),
             wi=w("intermediate.dense.weight").to(dt), bi=w("intermediate.dense.bias"),
             wf=w("output.dense.weight").to(dt), bf=w("output.dense.bias"))
    lnp = dict(ln1w=w("attention.output.LayerNorm.weight"), ln1b=w("attention.output.LayerNorm.bias"),
               ln2w=w("output.LayerNorm.weight"), ln2b=w("output.LayerNorm.bias"))
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(Mp, H); x[:M] = torch.randn(M, H, generator=g)
    keymask = torch.ones(B, S); keymask[0, 25:] = 0; keymask[3, 9:] = 0
    z = lambda *s, d=torch.float32: torch.zeros(*s, dtype=d, device=dev)  # noqa: E731
    x_d, x_h, km_d = x.to(dev), x.to(dev).to(dt), keymask.to(dev)         # (held: the argument structs keep raw pointers)
    bufs = dict(x_out=z(Mp, H), x_out_bf16=z(Mp, H, d=dt), qkv=z(Mp, 3 * H, d=dt), ctx=z(Mp, H, d=dt), lse=z(B, heads, S),
                xm=z(Mp, H), y1=z(Mp, H), n2=z(Mp, H, d=dt), act=z(Mp, FF, d=dt), u=z(Mp, FF, d=dt), h2=z(Mp, H),
                m1=z(Mp), r1=z(Mp), m2=z(Mp), r2=z(Mp))
    seed, base = 1234, 16
    d_att, d3, d4 = ops.Drop(0.1, seed, base + 2), ops.Drop(0.1, seed, base + 3), ops.Drop(0.1, seed, base + 4)
    a = ops.layer_args(B=B, S=S, H=H, FF=FF, heads=heads, rows=M, rows_pad=Mp, eps=lm.layer_norm_eps, x_in=x_d,
                       x_in_bf16=x_h, keymask=km_d, attn_drop_thresh=d_att.thresh, hid_drop_thresh=d3.thresh,
                       drop_seed=seed, drop_stream_base=base, attn_drop_scale=d_att.scale, hid_drop_scale=d3.scale, **W, **lnp, **bufs)
    lib = L.load(fmt)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.vault_lm_layer_fwd(C.byref(a), st), "vault_lm_layer_fwd")
    valid = km_d.bool()
    dy = torch.zeros(Mp, H); dy[:M] = torch.randn(M, H, generator=g) * keymask.view(M, 1)
    gw = dict(g_wqkv=z(3 * H, H), g_bqkv=z(3 * H), g_wo=z(H, H), g_bo=z(H), g_wi=z(FF, H), g_bi=z(FF), g_wf=z(H, FF), g_bf=z(H),
              g_ln1w=z(H), g_ln1b=z(H), g_ln2w=z(H), g_ln2b=z(H))
    sc = dict(dx_f32=z(Mp, H), dx_bf16=z(Mp, H, d=dt), dU=z(Mp, FF, d=dt), dN=z(Mp, H, d=dt), dctx=z(Mp, H, d=dt),
              dqkv=z(Mp, 3 * H, d=dt), dmid_bf16=z(Mp, H, d=dt), dh1_bf16=z(Mp, H, d=dt), dmid_f32=z(Mp, H))
    dy_d = dy.to(dev)
    gb = ops.layer_bwd_args(a, dy_f32=dy_d, do_wgrad=1, **gw, **sc)
    L.check(lib.vault_lm_layer_bwd(C.byref(gb), st), "vault_lm_layer_bwd")
    torch.cuda.synchronize()
    # ---- float64 reference: one post-LN layer on the weights the kernels hold, under the restated masks
    Pm = {k: v.double().clone().requires_grad_(True) for k, v in {**W, **lnp}.items()}
    xr = x_d[:M].double().view(B, S, H).clone().requires_grad_(True)
    k_att = D.keep_attn(d_att, B, heads, S).to(dev).double()
    k3 = D.keep_rows(d3, Mp, H)[:M].view(B, S, H).to(dev).double()
    k4 = D.keep_rows(d4, Mp, H)[:M].view(B, S, H).to(dev).double()
    sa, sh = _scale(d_att), _scale(d3)
    lin = torch.nn.functional.linear
    q, k, v = lin(xr, Pm["wqkv"], Pm["bqkv"]).view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~valid[:, None, None, :], float("-inf"))
    c = ((torch.softmax(s, dim=-1) * k_att * sa) @ v).permute(0, 2, 1, 3).reshape(B, S, H)
    y1 = _ln64(lin(c, Pm["wo"], Pm["bo"]) * k3 * sh + xr, Pm["ln1w"], Pm["ln1b"], lm.layer_norm_eps)
    hmid = torch.nn.functional.gelu(lin(y1, Pm["wi"], Pm["bi"]))
    y = _ln64(lin(hmid, Pm["wf"], Pm["bf"]) * k4 * sh + y1, Pm["ln2w"], Pm["ln2b"], lm.layer_norm_eps)
    y.backward(dy_d[:M].double().view(B, S, H))
    out = bufs["x_out"][:M].view(B, S, H).double()
    e_out = float((out[valid] - y.detach()[valid]).abs().max() / y.detach().abs().max())
    assert torch.equal(bufs["x_out_bf16"][:M], bufs["x_out"][:M].to(dt))
    dxm = (sc["dx_f32"][:M].double() + sc["dx_bf16"][:M].double()).view(B, S, H)[valid]
    dxr = xr.grad[valid]
    e_dx = float((dxm - dxr).norm() / dxr.norm())
    errs = {n: float((gw[f"g_{n}"].double() - Pm[n].grad).norm() / Pm[n].grad.norm())
            for n in ("wqkv", "wo", "wi", "wf", "bf", "bo", "ln2w", "ln1b")}
    print(f"LM layer with dropout {fmt}: output {e_out:.2e} of max |y| (bound 2e-2), dx {e_dx:.2e} (2e-2), weight gradients "
          + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()) + " (3e-2)")
    assert e_out < 2e-2 and e_dx < 2e-2
    assert all(e < 3e-2 for e in errs.values()), errs
