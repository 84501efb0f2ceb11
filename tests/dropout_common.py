"""What the dropout tests share (tests/test_dropout_host.py, tests/test_gpu_dropout.py): a host restatement, in plain integer
arithmetic, of the keep / drop decision the kernels regenerate in forward and backward (csrc/common.h ``dropout_keep``), and the
element index of each site that draws one.  A plain module: no fixtures, no hooks, no GPU.

    mix32(x)                     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (mod 2^32)
    keep(seed, stream, idx, t)   mix32(idx * 0x9E3779B9 + mix32(seed ^ (stream * 0x85EBCA6B))) >= t,  idx taken mod 2^32

    LayerNorm, residual GEMM (ldo == H), head (row = sample)      idx = row * H + col            keep_rows
    attention probabilities                                       idx = ((b * heads + h) * S + q) * S + k        keep_attn

``thresh`` and ``scale`` are READ from an ``ops.Drop`` (what the launch hands the kernel); ``expected_thresh`` /
``expected_scale`` say what a probability must turn into, for the host test of ``ops.Drop`` itself."""
from fractions import Fraction
from functools import lru_cache

import numpy as np
import torch

M32 = 0xFFFFFFFF


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)        # (both factors < 2^32: the product fits 64 bits)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x


def keep(seed: int, stream: int, idx, thresh: int):
    """bool array of the shape of ``idx`` (non-negative integers of any size below 2^64; only their low 32 bits count)."""
    key = int(mix32((seed & M32) ^ ((stream * 0x85EBCA6B) & M32)))
    idx = np.asarray(idx, dtype=np.uint64) & np.uint64(M32)
    h = mix32(idx * np.uint64(0x9E3779B9) + np.uint64(key))
    return h >= np.uint64(thresh)


def expected_thresh(p: float) -> int:
    """floor(p * 2^32) in exact arithmetic, at most 2^32 - 1; 0 (dropout off) for p <= 0."""
    return 0 if p <= 0.0 else min(int(Fraction(p) * (1 << 32)), M32)


def expected_scale(p: float) -> float:
    return 1.0 if p <= 0.0 else 1.0 / (1.0 - p)


def mapped_rows(rows: int, rowmap=(0, 0, 0)) -> np.ndarray:
    """Physical row of every logical row under a kernel row map (rpg, gstride, goff): (r // rpg) * gstride + goff + r % rpg;
    rpg == 0 is the identity."""
    r = np.arange(rows, dtype=np.int64)
    rpg, gstride, goff = rowmap
    return r if rpg == 0 else (r // rpg) * gstride + goff + r % rpg


@lru_cache(maxsize=16)
def _rows_mask(thresh, seed, stream, H, row_key):
    rows = np.frombuffer(row_key, dtype=np.int64)
    idx = rows[:, None].astype(np.uint64) * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :]
    return keep(seed, stream, idx, thresh)


def keep_rows(drop, rows: int, H: int, row_index=None) -> torch.Tensor:
    """[rows, H] bool: element (r, c) is kept; its index is row_index[r] * H + c (row_index: the PHYSICAL row the kernel keys
    by; default r)."""
    ri = np.arange(rows, dtype=np.int64) if row_index is None else np.ascontiguousarray(np.asarray(row_index, dtype=np.int64))
    assert ri.shape == (rows,)
    return torch.from_numpy(_rows_mask(drop.thresh, drop.seed, drop.stream, H, ri.tobytes()).copy())


@lru_cache(maxsize=16)
def _attn_mask(thresh, seed, stream, B, heads, S):
    idx = np.arange(B * heads * S * S, dtype=np.uint64)        # ((b * heads + h) * S + q) * S + k, in that order
    return keep(seed, stream, idx, thresh).reshape(B, heads, S, S)


def keep_attn(drop, B: int, heads: int, S: int) -> torch.Tensor:
    """[B, heads, S, S] bool: probability (b, h, q, k) is kept."""
    return torch.from_numpy(_attn_mask(drop.thresh, drop.seed, drop.stream, B, heads, S).copy())
