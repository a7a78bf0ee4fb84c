"""Shared by the rank tests (tests/test_rank_segments_*.py, test_live_ranked_*.py):
the reference order in numpy and the score buffers the kernel is checked on.

Reference order (csrc/kernels/sort.hip's total order, written independently of
it): u32 key = the IEEE bits with both zeros as 0, ``~u`` when the sign bit is
set else ``u | 0x80000000``, inverted again for descending, 0xfffffffe for NaN
in both directions; ties by ascending candidate index.
"""
import numpy as np
import torch

# straddle the wave (64), what one thread / one wave of each size class holds,
# the size classes (1024, 4096, 16384) and the cross-wave (LDS) thresholds
GPU_LENGTHS = (0, 1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025, 1500, 4096, 4097, 8192, 8193, 16384)
CPU_LENGTHS = (0, 1, 2, 63, 64, 65, 511, 512, 513)
GAP = 3  # scores in front of the first and behind the last segment that belong to none


def ref_order(v: np.ndarray, descending: bool = False) -> np.ndarray:
    """Permutation that ranks fp32 scores v."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32).copy()
    u[v == 0] = 0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    if descending:
        key = ~key
    key[np.isnan(v)] = np.uint32(0xFFFFFFFE)
    return np.lexsort((np.arange(v.size), key)).astype(np.int64)


def segment_scores(n: int, rng: np.random.Generator) -> np.ndarray:
    """n scores drawn from 8 values (ties everywhere); from 8 scores on with
    NaN, -0.0, +0.0, +inf and -inf planted."""
    v = (rng.integers(0, 8, n).astype(np.float32) - 3) / 4
    if n >= 8:
        pos = rng.choice(n, 5, replace=False)
        v[pos] = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf], dtype=np.float32)
    return v


def make_buffer(lengths, seed: int = 0):
    """(scores [N] fp32, offsets [S + 1] int64, segments [(a, b)]): the
    segments back to back in the given order (offsets[S + 1] describes nothing
    else), with GAP scores in front of the first and behind the last."""
    rng = np.random.default_rng(seed)
    parts, segs, pos = [rng.random(GAP, dtype=np.float32)], [], GAP
    for n in lengths:
        parts.append(segment_scores(n, rng))
        segs.append((pos, pos + n))
        pos += n
    parts.append(rng.random(GAP, dtype=np.float32))
    offsets = np.array([GAP] + [b for _, b in segs], dtype=np.int64)
    return np.concatenate(parts), offsets, segs


def expected(scores: np.ndarray, segs, descending: bool, k: int, sentinel_val: float, sentinel_idx: int):
    """What rank_segments must leave in outputs pre-filled with the sentinels."""
    vals = np.full(scores.size, sentinel_val, dtype=np.float32)
    idx = np.full(scores.size, sentinel_idx, dtype=np.int64)
    for a, b in segs:
        p = ref_order(scores[a:b], descending)
        kk = b - a if k < 0 or k > b - a else k
        vals[a:a + kk] = scores[a:b][p[:kk]]
        idx[a:a + kk] = p[:kk]
        vals[a + kk:b] = 0
        idx[a + kk:b] = -1
    return vals, idx


def bits(t) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
