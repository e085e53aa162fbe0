"""Systematic resampling in integer form restated in numpy and Python integers: the offset of a seeded draw (one 64-bit word of
the Philox stream of tests/host_sampler.py), the integer points t_k = floor((s + k W) / M), the ancestors through a search
of the running sum of the weights, and the exact weight statistics.  Everything is integer arithmetic without rounding, so
these predict rscm_ens_resample, rscm_gpu_resample_offset and rscm_ens_weights_stats (rscm_amd/csrc/resample.hip,
resample_host.cpp) bit for bit, on one handle and on any split of the members into handles or ranks."""
from fractions import Fraction

import numpy as np

from tests.host_sampler import philox4x32_10

STREAM_TAG = 0x52534D50   # RSCM_RESAMPLE_STREAM_TAG of include/rscm_gpu.h


def offset(seed: int, W: int) -> int:
    """s = floor(R W / 2^64), R = (x1 << 32) | x0 of the Philox block with counter (0, 0, 0, STREAM_TAG) and key
    (seed & 0xFFFFFFFF, seed >> 32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x0, x1, _, _ = philox4x32_10(0, 0, 0, STREAM_TAG, seed & 0xFFFFFFFF, seed >> 32)
    R = (int(x1) << 32) | int(x0)
    return (R * int(W)) >> 64


def points(M: int, s: int, W: int, k_first: int = 0, count=None) -> list:
    """t_k = floor((s + k W) / M) for k = k_first .. k_first + count - 1, as Python ints (no 64-bit limit to trip over)."""
    M, s, W = int(M), int(s), int(W)
    count = M - k_first if count is None else count
    return [(s + k * W) // M for k in range(k_first, k_first + count)]


def draw_range(M: int, s: int, W: int, lo: int, hi: int):
    """(k_first, count): the contiguous run of draws whose points fall in [lo, hi) -- t_k is non-decreasing in k, and
    t_k >= x  <=>  k >= ceil((x M - s) / W)."""
    M, s, W = int(M), int(s), int(W)

    def first_at(x):
        return min(M, max(0, -((s - x * M) // W)))
    k0, k1 = first_at(int(lo)), first_at(int(hi))
    return k0, k1 - k0


def ancestors(w, M: int, s: int, w_before: int = 0, w_total=None):
    """(k_first, count, local ancestors as int64) of the handle that owns the weight range [w_before, w_before + sum(w)) of a
    global total w_total (default: alone): np.searchsorted(np.cumsum(w), t, side="right") of its draws' local points."""
    w = np.asarray(w, dtype=np.int64)
    W_local = int(w.sum(dtype=np.int64)) if w.size else 0
    w_total = W_local + int(w_before) if w_total is None else int(w_total)
    k_first, count = draw_range(M, s, w_total, w_before, int(w_before) + W_local)
    t = np.array([p - int(w_before) for p in points(M, s, w_total, k_first, count)], dtype=np.int64)
    anc = np.searchsorted(np.cumsum(w, dtype=np.int64), t, side="right").astype(np.int64)
    return k_first, count, anc


def ancestors_fast(w, M: int, s: int, w_before: int = 0, w_total=None):
    """ancestors() for large M without a Python loop over the draws: the points in uint64 numpy arithmetic as the device forms
    them, t_k = k q + (s + k r) // M (valid for M <= 2^31, s < W < 2^63)."""
    w = np.asarray(w, dtype=np.int64)
    W_local = int(w.sum(dtype=np.int64)) if w.size else 0
    w_total = W_local + int(w_before) if w_total is None else int(w_total)
    k_first, count = draw_range(M, s, w_total, w_before, int(w_before) + W_local)
    q, r = divmod(w_total, int(M))
    k = np.arange(k_first, k_first + count, dtype=np.uint64)
    t = k * np.uint64(q) + (np.uint64(s) + k * np.uint64(r)) // np.uint64(M) - np.uint64(w_before)
    anc = np.searchsorted(np.cumsum(w, dtype=np.int64), t.astype(np.int64), side="right").astype(np.int64)
    return k_first, count, anc


def stats(w) -> dict:
    """Exact total, non-zero count, maximum and sum of squares as Python ints, and ess = total^2 / sum_sq rounded once."""
    x = [int(v) for v in np.asarray(w, dtype=np.int64)]
    total, sq = sum(x), sum(v * v for v in x)
    return {"total": total, "n_nonzero": sum(1 for v in x if v), "w_max": max(x) if x else 0, "sum_sq": sq,
            "ess": float(Fraction(total * total, sq)) if sq else 0.0}
