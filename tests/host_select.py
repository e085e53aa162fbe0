"""The staged radix select of rscm_amd/csrc/select.hip restated in numpy: the same key map, digit width, passes, commit rule
and interpolation.  tests/test_host_select.py pins it against numpy.nanquantile on sharded data; the CPU rehearsal of
rscm_amd.distributed.quantile_rows_global (tests/_dist_quantile_worker.py) uses it as the stand-in ensemble's select."""
import math

import numpy as np

BINS = 256
PASSES = 8
_TOP = np.uint64(1) << np.uint64(63)


def order_keys(x: np.ndarray):
    """(keys, not_nan): the order-preserving uint64 image of float64 ``x`` (-0.0 before +0.0)."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    keys = np.where((u >> np.uint64(63)) != 0, ~u, u | _TOP)
    return keys, ~np.isnan(x)


def key_value(k: int) -> float:
    k = int(k)
    u = (k & 0x7FFFFFFFFFFFFFFF) if k >> 63 else (~k & 0xFFFFFFFFFFFFFFFF)
    return float(np.array([u], dtype=np.uint64).view(np.float64)[0])


class HostSelect:
    """One handle's select over ``rows`` ([n_rows][n_local] float64, this shard's members)."""

    def __init__(self, rows, q):
        self.keys, self.ok = order_keys(np.atleast_2d(np.asarray(rows, dtype=np.float64)))
        self.q = [float(v) for v in np.atleast_1d(q)]
        if not all(0.0 <= v <= 1.0 for v in self.q):
            raise ValueError("Quantiles must be in the range [0, 1]")
        self.n_rows, self.n_t = self.keys.shape[0], 2 * len(self.q)
        self.pass_ = 0
        self.count = [0] * self.n_rows
        self.prefix = [[0] * self.n_t for _ in range(self.n_rows)]
        self.rank = [[-1] * self.n_t for _ in range(self.n_rows)]
        self.hist = None

    def next_pass(self):
        """This shard's int64 histograms of the next pass (flat), or None when no pass is left."""
        if self.n_rows == 0 or self.pass_ == PASSES:
            return None
        p = self.pass_
        shift = np.uint64(56 - 8 * p)
        if p == 0:
            h = np.zeros((self.n_rows, BINS), dtype=np.int64)
            for r in range(self.n_rows):
                d = (self.keys[r][self.ok[r]] >> shift).astype(np.int64)
                h[r] = np.bincount(d, minlength=BINS)
        else:
            h = np.zeros((self.n_rows, self.n_t, BINS), dtype=np.int64)
            for r in range(self.n_rows):
                k = self.keys[r][self.ok[r]]
                top = k >> np.uint64(64 - 8 * p)
                d = ((k >> shift) & np.uint64(BINS - 1)).astype(np.int64)
                for t in range(self.n_t):
                    h[r, t] = np.bincount(d[top == np.uint64(self.prefix[r][t])], minlength=BINS)
        self.hist = h.reshape(-1)
        return self.hist

    def commit(self, reduced=None):
        h = np.asarray(self.hist if reduced is None else reduced, dtype=np.int64)
        p = self.pass_
        for r in range(self.n_rows):
            for t in range(self.n_t):
                if p == 0:
                    bins = h.reshape(self.n_rows, BINS)[r]
                    n = int(bins.sum())
                    self.count[r] = n
                    if n == 0:
                        self.rank[r][t] = -1
                        continue
                    vi = float(n - 1) * self.q[t // 2]
                    prev = min(max(float(math.floor(vi)), 0.0), float(n - 1))
                    ip = int(prev)
                    want = (ip + 1 if ip + 1 < n else n - 1) if t & 1 else ip
                else:
                    want = self.rank[r][t]
                    if want < 0:
                        continue
                    bins = h.reshape(self.n_rows, self.n_t, BINS)[r, t]
                below, b = 0, 0
                while b < BINS - 1 and want >= below + int(bins[b]):
                    below += int(bins[b])
                    b += 1
                self.prefix[r][t] = b if p == 0 else (self.prefix[r][t] << 8) | b
                self.rank[r][t] = want - below
        self.pass_ += 1

    def result(self):
        nq = len(self.q)
        out = np.full((self.n_rows, nq), np.nan)
        for r in range(self.n_rows):
            n = self.count[r]
            if n == 0:
                continue
            for k, qk in enumerate(self.q):
                vi = float(n - 1) * qk
                prev = min(max(float(math.floor(vi)), 0.0), float(n - 1))
                g = vi - prev
                a, b = key_value(self.prefix[r][2 * k]), key_value(self.prefix[r][2 * k + 1])
                d = b - a
                v = a + d * g
                if g >= 0.5:
                    v = b - d * (1.0 - g)
                if d == 0.0:
                    v = a
                out[r, k] = v
        return {"count": np.asarray(self.count, dtype=np.int64), "quantiles": out}


def sharded_quantiles(shards, q):
    """The whole select over several shards ([n_rows][n_i] each), their histograms summed between the passes."""
    sel = [HostSelect(s, q) for s in shards]
    while True:
        bufs = [s.next_pass() for s in sel]
        if bufs[0] is None:
            break
        total = np.sum(bufs, axis=0)
        for s in sel:
            s.commit(total)
    res = [s.result() for s in sel]
    return res
