"""The last ViLT layer computed for the pooler alone (VaultEngine.PRUNE_LAST_LAYER): the attention kernels' one-live-query form
(vault_attn_args.q_rows = 1) against the full kernels, bit for bit, and the engine's pruned plan against the unpruned one -
logits bit for bit, gradients (and the loss, itself an atomic sum) up to the summation order of float atomics (1e-5 relative L2, the bound of
test_gpu_model.py::test_per_kernel_layer_path_equals_the_stage_calls)."""
import pytest
import torch

from vault_amd import ops
from vault_amd.engine import VaultEngine
from vault_amd.spec import LMSpec, VaultSpec, ViltSpec, build_state, synthetic_batch, synthetic_ragged_batch
from vault_amd.train import TrainStep

pytestmark = pytest.mark.gpu

SHAPES = [(3, 185, 12), (2, 40, 4), (3, 17, 1), (2, 192, 2)]       # (B, S, heads): both resident kernels, one tile, no padding rows


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _to_head_major(x, R):
    M, N = x.shape
    out = torch.zeros(N // 64, R, 64, dtype=x.dtype, device=x.device)
    out[:, :M] = x.view(M, N // 64, 64).permute(1, 0, 2)
    return out


def _from_head_major(y, M):
    P, R, _ = y.shape
    return y[:, :M].permute(1, 0, 2).reshape(M, P * 64)


def _attn_inputs(B, S, heads, hm):
    H, M = heads * 64, B * S
    R = ((M + 255) // 256) * 256 + 256
    qkv = (_rand(M, 3 * H, seed=10) * 1.5).bfloat16()
    keymask = torch.ones(B, S, device="cuda")                      # masked keys, as in test_attention_fwd_bwd
    keymask[1, 5:min(17, S - 1)] = 0
    keymask[B - 1, S - min(9, S - 2):] = 0
    return H, M, R, (_to_head_major(qkv, R) if hm else qkv), keymask, (dict(qkv_hm=R) if hm else {})


@pytest.mark.parametrize("hm", [False, True])
@pytest.mark.parametrize("B,S,heads", SHAPES)
def test_attention_forward_with_one_live_query_equals_row_0_of_the_full_kernel(B, S, heads, hm):
    H, M, R, q_in, keymask, kw = _attn_inputs(B, S, heads, hm)
    Bp = 256
    ctx = torch.zeros(M, H, dtype=torch.bfloat16, device="cuda"); lse = torch.zeros(B, heads, S, device="cuda")
    ops.attention_fwd(q_in, keymask, ctx, lse, B, S, H, heads, **kw)
    ctx_c = torch.full((Bp, H), 7.0, dtype=torch.bfloat16, device="cuda"); lse_c = torch.full((B, heads, S), 5.0, device="cuda")
    ops.attention_fwd(q_in, keymask, ctx_c, lse_c, B, S, H, heads, q_rows=1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(ctx_c[:B], ctx.view(B, S, H)[:, 0])
    assert torch.equal(lse_c[:, :, 0], lse[:, :, 0])
    assert float((ctx_c[B:].float() - 7.0).abs().max()) == 0.0          # the compact buffer's padding rows are untouched
    assert float((lse_c[:, :, 1:] - 5.0).abs().max()) == 0.0            # ... and so is the rest of lse


@pytest.mark.parametrize("hm", [False, True])
@pytest.mark.parametrize("B,S,heads", SHAPES)
def test_attention_backward_with_one_live_query_equals_the_full_kernel_on_zero_rows(B, S, heads, hm):
    H, M, R, q_in, keymask, kw = _attn_inputs(B, S, heads, hm)
    Bp = 256
    ctx = torch.zeros(M, H, dtype=torch.bfloat16, device="cuda"); lse = torch.zeros(B, heads, S, device="cuda")
    ops.attention_fwd(q_in, keymask, ctx, lse, B, S, H, heads, **kw)
    ctx_c = torch.zeros(Bp, H, dtype=torch.bfloat16, device="cuda"); lse_c = torch.full((B, heads, S), 5.0, device="cuda")
    ops.attention_fwd(q_in, keymask, ctx_c, lse_c, B, S, H, heads, q_rows=1, **kw)
    dctx_c = _rand(Bp, H, seed=11).bfloat16()                       # (rows >= B: never read)
    dctx = torch.zeros(M, H, dtype=torch.bfloat16, device="cuda")
    dctx.view(B, S, H)[:, 0] = dctx_c[:B]
    shape = (3 * heads, R, 64) if hm else (M, 3 * H)
    d_full = torch.zeros(shape, dtype=torch.bfloat16, device="cuda")
    ops.attention_bwd(q_in, keymask, ctx, lse, dctx, d_full, B, S, H, heads, **kw)
    d_one = torch.full(shape, 7.0, dtype=torch.bfloat16, device="cuda")
    ops.attention_bwd(q_in, keymask, ctx_c, lse_c, dctx_c, d_one, B, S, H, heads, q_rows=1, **kw)
    torch.cuda.synchronize()
    if hm:
        assert torch.equal(_from_head_major(d_one, M), _from_head_major(d_full, M))
        assert float((d_one[:, M:].float() - 7.0).abs().max()) == 0.0   # rows beyond the tokens are never written
    else:
        assert torch.equal(d_one, d_full)                              # all of dqkv, the zero dQ rows included
    dq = (_from_head_major(d_one, M) if hm else d_one).float()
    assert float(dq.view(B, S, 3 * H)[:, 1:, :H].abs().max()) == 0.0
    # bias partials: every row of the matrix is written, and the rows add up to the column sums of dq
    n = ops.attention_bwd_partials(B, S, H, heads, 1)
    assert n == min(B * heads, 768 if S <= 64 else 256)
    part = torch.full((n, H), 3.0, device="cuda")
    d_two = torch.full(shape, 7.0, dtype=torch.bfloat16, device="cuda")
    ops.attention_bwd(q_in, keymask, ctx_c, lse_c, dctx_c, d_two, B, S, H, heads, q_rows=1, bias_partials=part, bias_thirds=1, **kw)
    out = torch.full((H + 64,), 0.25, device="cuda")
    ops.colsum_partials(part, n, H, out)
    torch.cuda.synchronize()
    assert torch.equal(d_two, d_one)
    ref, got = dq[:, :H].sum(0), out[:H] - 0.25
    tol = 2.0 ** -8 * float(dq.abs().max()) * M ** 0.5 + 1e-4           # (the formula of test_attention_backward_leaves_the_qkv_bias_gradient_as_partial_sums)
    assert float((got - ref).abs().max()) <= tol, (float((got - ref).abs().max()), tol)
    assert float((out[H:] - 0.25).abs().max()) == 0.0


def test_attention_refuses_live_query_counts_it_has_no_form_for():
    B, S, heads = 2, 40, 2
    H, M, R, qkv, keymask, _ = _attn_inputs(B, S, heads, False)
    ctx = torch.zeros(256, H, dtype=torch.bfloat16, device="cuda"); lse = torch.zeros(B, heads, S, device="cuda")
    with pytest.raises(RuntimeError):
        ops.attention_fwd(qkv, keymask, ctx, lse, B, S, H, heads, q_rows=2)
    with pytest.raises(RuntimeError):
        ops.attention_bwd(qkv, keymask, ctx, lse, ctx, torch.zeros_like(qkv), B, S, H, heads, q_rows=16)
    S = 193                                                           # beyond the resident kernels
    big = torch.zeros(B * S, 3 * H, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.attention_fwd(big, None, ctx, torch.zeros(B, heads, S, device="cuda"), B, S, H, heads, q_rows=1)
    with pytest.raises(RuntimeError):
        ops.attention_fwd(qkv, keymask, None, lse, B, 40, H, heads, q_rows=1, ctx_split3=torch.zeros(M, 3 * H, dtype=torch.bfloat16, device="cuda"))


# ---- engine -------------------------------------------------------------------------------------------------------------
def _dev(bn):
    return {k: torch.from_numpy(v).cuda() for k, v in bn.items()}


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _assert_same_loss(l1, l0, B):
    """The loss is a float-atomic sum of B positive per-sample terms (csrc/head.hip, one wave each): its last bits depend on the
    order the waves arrive in, from run to run, pruned or not - two unpruned runs differ the same way.  The terms themselves
    are functions of the logits, which the callers compare bit for bit; what is left is the order: two f32 sums of the same B
    positive terms differ by at most 2 (B - 1) 2^-24 of the sum."""
    l1, l0 = float(l1), float(l0)
    assert abs(l1 - l0) <= 2 * (B - 1) * 2.0 ** -24 * abs(l0), (l1, l0)


def _tiny_engine(spec, state, prune, batched, half="bf16"):
    eng = VaultEngine(spec, "cuda:0", state=state, seed=0, classifier_dropout=0.0, half=half)
    eng.STAGE_MAX_ROWS, eng.PRUNE_MIN_ROWS = 0, 0
    eng.PRUNE_LAST_LAYER, eng.LM_WGRAD_BATCHED = prune, batched
    return eng


@pytest.mark.parametrize("B,batched,half", [(5, True, "bf16"), (9, True, "bf16"), (5, False, "bf16"), (9, False, "bf16"),
                                            (5, True, "fp16")])      # (fp16: the engine's default operand build)
def test_pruned_last_layer_equals_the_unpruned_engine(B, batched, half):
    """VaultSpec.tiny, LM dropout on: eval logits and train logits bit for bit, the loss up to the order of its own atomic sum
    (_assert_same_loss); gradients, and the first moment after one fused train step, up to float-atomic summation order."""
    spec = VaultSpec.tiny(3, "roberta")
    state = build_state(spec, 0)
    b = _dev(synthetic_batch(spec, B, seed=31, n_classes=3))
    res = []
    for prune in (False, True):
        eng = _tiny_engine(spec, state, prune, batched, half)
        ev = eng.forward(b, train=False, need_hidden=False)["logits"].clone()
        assert eng.last["pruned_last"] is prune
        out = eng.forward(b, train=True, labels=b["labels"], need_hidden=False)
        assert eng.last["pruned_last"] is prune and eng.last["vilt_stage"] is False
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        grads = eng.params.g[: eng.params.n_train].clone()
        eng2 = _tiny_engine(spec, state, prune, batched, half)
        step = TrainStep(eng2, learning_rate=5e-5, warmup_ratio=0.0, total_steps=10)
        step({k: v for k, v in b.items() if k != "labels"}, b["labels"])
        torch.cuda.synchronize()
        assert eng2.last["pruned_last"] is prune
        res.append((ev, out["logits"].clone(), out["loss"].clone(), grads, eng2.params.m[: eng2.params.n_train].clone()))
    (ev0, lg0, ls0, g0, m0), (ev1, lg1, ls1, g1, m1) = res
    assert torch.equal(ev1, ev0)
    assert torch.equal(lg1, lg0)
    _assert_same_loss(ls1, ls0, B)
    print(f"B = {B}, batched = {batched}, {half}: gradient rel L2 {_rel(g1, g0):.3e}, exp_avg rel L2 {_rel(m1, m0):.3e}")
    assert _rel(g1, g0) < 1e-5
    assert _rel(m1, m0) < 1e-5


def _full_width_spec():
    spec = VaultSpec(vilt=ViltSpec(num_hidden_layers=2), lm=LMSpec.bertweet_base(), n_classes=3)
    spec.lm.num_hidden_layers = 2
    return spec


def test_pruned_last_layer_at_full_width_with_default_attributes():
    """Hidden 768, 2 + 2 layers, B = 96 (17,760 token rows: above PRUNE_MIN_ROWS, head-major qkv, the grouped ring weight
    gradients with per-kind layer counts, the 8-bit gelu' image): one engine, pruning off and on over the same workspace."""
    spec = _full_width_spec()
    eng = VaultEngine(spec, "cuda:0", seed=0, classifier_dropout=0.0, half="bf16")
    b = _dev(synthetic_batch(spec, 96, seed=33, n_classes=3))
    res = []
    for prune in (False, True, False):          # (and back: the unpruned pass must not see what the pruned one left)
        eng.PRUNE_LAST_LAYER, eng.drop_seed = prune, 0
        out = eng.forward(b, train=True, labels=b["labels"], need_hidden=False)
        assert eng.last["pruned_last"] is prune
        eng.zero_grad()
        eng.backward()
        torch.cuda.synchronize()
        res.append((out["logits"].clone(), out["loss"].clone(), eng.params.g[: eng.params.n_train].clone()))
    assert torch.equal(res[1][0], res[0][0]) and torch.equal(res[2][0], res[0][0])
    _assert_same_loss(res[1][1], res[0][1], 96)
    print(f"full width, B = 96: gradient rel L2 pruned {_rel(res[1][2], res[0][2]):.3e}, unpruned again {_rel(res[2][2], res[0][2]):.3e}")
    assert _rel(res[1][2], res[0][2]) < 1e-5
    assert _rel(res[2][2], res[0][2]) < 1e-5


def test_pruning_guards(monkeypatch):
    spec = VaultSpec.tiny(3, "roberta")
    state = build_state(spec, 0)
    b = _dev(synthetic_batch(spec, 5, seed=31, n_classes=3))
    hid = []
    for prune in (False, True):
        eng = _tiny_engine(spec, state, prune, True)
        out = eng.forward(b, train=True, labels=b["labels"], need_hidden=True)
        assert eng.last["pruned_last"] is False                        # somebody reads the other rows
        hid.append(out["last_hidden_state"].clone())
        eng.zero_grad()
        eng.backward(dhidden=torch.ones_like(hid[-1]))                  # ... and may hand their gradient back
    torch.cuda.synchronize()
    assert torch.equal(hid[1], hid[0])
    eng.forward(b, train=True, labels=b["labels"], need_hidden=False)
    assert eng.last["pruned_last"] is True
    with pytest.raises(ValueError):
        eng.backward(dhidden=torch.ones_like(hid[0]))
    # the off switch is read at construction
    monkeypatch.setenv("VAULT_PRUNE_LAST_LAYER", "0")
    off = VaultEngine(spec, "cuda:0", state=state, seed=0, classifier_dropout=0.0, half="bf16")
    monkeypatch.delenv("VAULT_PRUNE_LAST_LAYER")
    assert off.PRUNE_LAST_LAYER is False and VaultEngine.PRUNE_LAST_LAYER is True
    off.STAGE_MAX_ROWS, off.PRUNE_MIN_ROWS = 0, 0
    off.forward(b, train=False, need_hidden=False)
    assert off.last["pruned_last"] is False
    # small shapes keep today's path by default
    eng = VaultEngine(spec, "cuda:0", state=state, seed=0, classifier_dropout=0.0, half="bf16")
    eng.STAGE_MAX_ROWS = 0
    eng.forward(b, train=False, need_hidden=False)
    assert eng.last["pruned_last"] is False


def test_sequences_beyond_the_resident_attention_kernels_do_not_prune():
    """A padded batch on the 384 x 640 canvas: S = 281 has no one-query attention form."""
    spec = _full_width_spec()
    eng = VaultEngine(spec, "cuda:0", seed=0, classifier_dropout=0.0, half="bf16")
    eng.STAGE_MAX_ROWS, eng.PRUNE_MIN_ROWS = 0, 0
    b = _dev(synthetic_ragged_batch(spec, [(384, 640), (352, 608)], (384, 640), seed=5, n_classes=3))
    out = eng.forward(b, train=False, need_hidden=False)
    torch.cuda.synchronize()
    assert eng.last["S"] == 281 and eng.last["pruned_last"] is False
    assert bool(torch.isfinite(out["logits"]).all())
