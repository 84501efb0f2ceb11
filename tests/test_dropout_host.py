"""The host restatement of the dropout decision (tests/dropout_common.py) and ``ops.Drop``, without a GPU: the threshold and
the scale a probability turns into, the keep rate, the independence of streams and seeds, and the 32-bit wrap of the element
index.  The GPU tests (tests/test_gpu_dropout.py) compare every kernel's mask with this restatement element by element."""
import math

import numpy as np
import pytest

from tests import dropout_common as D
from vault_amd import ops

KEYS = [(7, 3), (12345, 18), (0, 1)]                       # (seed, stream)
N = 1 << 16


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0 - 2.0 ** -33])
def test_drop_threshold_and_scale(p):
    d = ops.Drop(p, seed=-1, stream=(1 << 32) + 5)
    assert d.thresh == D.expected_thresh(p) and d.scale == D.expected_scale(p)
    assert 0 <= d.thresh <= 0xFFFFFFFF and d.seed == 0xFFFFFFFF and d.stream == 5      # 32-bit members of the argument structs
    if p == 0.0:
        assert d.thresh == 0 and d.scale == 1.0                                         # thresh 0 switches the kernels' test off
    if p > 0.9:
        assert d.thresh == 0xFFFFFFFF                                                   # p * 2^32 rounds to 2^32: clamped


def test_mix32_is_the_32_bit_function():
    """Two hand-computed values and the 2^32 period: everything is taken modulo 2^32."""
    assert int(D.mix32(0)) == 0
    x = 1
    x ^= x >> 16; x = (x * 0x7FEB352D) & D.M32; x ^= x >> 15; x = (x * 0x846CA68B) & D.M32; x ^= x >> 16
    assert int(D.mix32(1)) == x
    v = np.array([3, 0xFFFFFFFF, 0x12345678], dtype=np.uint64)
    assert np.array_equal(D.mix32(v), D.mix32(v + np.uint64(1 << 32)))
    assert int(D.mix32(v).max()) <= D.M32


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed,stream", KEYS)
def test_keep_rate(p, seed, stream):
    d = ops.Drop(p, seed=seed, stream=stream)
    rate = float(D.keep(d.seed, d.stream, np.arange(N), d.thresh).mean())
    sd = math.sqrt(p * (1.0 - p) / N)
    print(f"p = {p} key {(seed, stream)}: keep rate {rate:.5f}, {(rate - (1 - p)) / sd:+.2f} standard deviations")
    assert abs(rate - (1.0 - p)) <= 5.0 * sd


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_streams_and_seeds_give_independent_masks(p):
    """Two independent masks differ where exactly one of them keeps: a share 2 p (1 - p) of the positions."""
    idx = np.arange(N)
    q = 2.0 * p * (1.0 - p)
    sd = math.sqrt(q * (1.0 - q) / N)
    t = ops.Drop(p).thresh
    base = D.keep(7, 3, idx, t)
    for what, other in (("stream", D.keep(7, 4, idx, t)), ("seed", D.keep(8, 3, idx, t)), ("both", D.keep(12345, 18, idx, t))):
        share = float((base != other).mean())
        print(f"p = {p}, other {what}: masks differ on {share:.5f} (expected {q:.5f}, {(share - q) / sd:+.2f} standard deviations)")
        assert abs(share - q) <= 5.0 * sd


def test_transposed_mask_is_another_mask_at_p_half():
    """Why the exact mask checks run at p = 0.5: a [S, S] mask equals its own transpose on about half of the off-diagonal
    positions only, so a transposed (or mis-strided) index cannot pass for the right one."""
    d = ops.Drop(0.5, seed=7, stream=3)
    m = D.keep_attn(d, 3, 1, 70)[:, 0].numpy()
    same = float((m == m.transpose(0, 2, 1)).mean())
    assert 0.45 < same < 0.57, same
    r = D.keep_rows(d, 70, 256).numpy()
    r2 = D.keep_rows(d, 70, 256, row_index=np.arange(70) + 1).numpy()           # one row off
    assert 0.45 < float((r == r2).mean()) < 0.55


def test_index_wraps_at_2_to_32():
    """The kernels cast the element index to 32 bits: index i and i + 2^32 share a decision (a tensor of more than 2^32
    elements repeats its mask; no tensor of the model is that large)."""
    i = np.array([0, 1, 12345, (1 << 32) - 1], dtype=np.uint64)
    for seed, stream in KEYS:
        for t in (ops.Drop(0.1).thresh, ops.Drop(0.5).thresh):
            assert np.array_equal(D.keep(seed, stream, i, t), D.keep(seed, stream, i + np.uint64(1 << 32), t))
    lo = D.keep(7, 3, np.arange(N), ops.Drop(0.5).thresh)
    hi = D.keep(7, 3, np.arange(N, dtype=np.uint64) + np.uint64(1 << 32), ops.Drop(0.5).thresh)
    assert np.array_equal(lo, hi)


def test_row_and_attention_indices():
    """keep_rows keys by row * H + col of the PHYSICAL row, keep_attn by ((b * heads + h) * S + q) * S + k."""
    d = ops.Drop(0.5, seed=12345, stream=18)
    H = 256
    rows = D.mapped_rows(7, (3, 5, 2))
    assert rows.tolist() == [2, 3, 4, 7, 8, 9, 12]
    m = D.keep_rows(d, 7, H, row_index=rows).numpy()
    for r, pr in enumerate(rows):
        assert np.array_equal(m[r], D.keep(d.seed, d.stream, pr * H + np.arange(H), d.thresh))
    B, heads, S = 2, 3, 17
    a = D.keep_attn(d, B, heads, S).numpy()
    for (b, h, q, k) in ((0, 0, 0, 0), (1, 2, 16, 3), (1, 0, 5, 16), (0, 2, 9, 9)):
        assert bool(a[b, h, q, k]) == bool(D.keep(d.seed, d.stream, ((b * heads + h) * S + q) * S + k, d.thresh))
    assert bool(D.keep_rows(ops.NO_DROP, 3, H).all())                            # thresh 0: everything is kept
