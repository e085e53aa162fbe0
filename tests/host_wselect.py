"""The weighted radix select of rscm_amd/csrc/wselect.hip restated in numpy: the key map and 8-bit digits of tests/host_select.py,
int64 weight sums in place of counts, one target per quantile found by the C* rule, and the key of the selected member as the
result.  tests/test_host_weighted_select.py pins it against numpy.nanquantile(..., weights=w, method="inverted_cdf"); the CPU
rehearsal of the weighted rscm_amd.distributed.quantile_rows_global (tests/_dist_wquantile_worker.py) uses it as the stand-in
ensemble's select."""
import math

import numpy as np

from tests.host_select import BINS, PASSES, key_value, order_keys

W_MAX = 1 << 53


def weight_target(q: float, W: int) -> int:
    """The smallest integer C >= 1 with float(C) / float(W) >= q (IEEE division), 1 <= W <= 2^53, searched from ceil(q W) as
    the commit kernel does."""
    dw = float(W)
    c = min(max(math.ceil(q * dw), 1.0), dw)
    C = int(c)
    while C > 1 and float(C - 1) / dw >= q:
        C -= 1
    while C < W and float(C) / dw < q:
        C += 1
    return C


class HostWSelect:
    """One handle's weighted select over ``rows`` ([n_rows][n_local] float64) with member weights ``w`` ([n_local] int64)."""

    def __init__(self, rows, w, q):
        self.keys, self.ok = order_keys(np.atleast_2d(np.asarray(rows, dtype=np.float64)))
        self.w = np.ascontiguousarray(w, dtype=np.int64)
        if self.w.shape != (self.keys.shape[1],):
            raise ValueError("one weight per member")
        if (self.w < 0).any():
            raise ValueError("negative weight")
        if sum(int(x) for x in self.w) > W_MAX:   # the library's check when a handle takes its weights: no bin can wrap
            raise ValueError("the weights of this handle sum to more than 2^53")
        self.q = [float(v) for v in np.atleast_1d(q)]
        if not all(0.0 <= v <= 1.0 for v in self.q):
            raise ValueError("Quantiles must be in the range [0, 1]")
        self.n_rows, self.n_t = self.keys.shape[0], len(self.q)
        self.pass_ = 0
        self.weight = [0] * self.n_rows
        self.prefix = [[0] * self.n_t for _ in range(self.n_rows)]
        self.rank = [[-1] * self.n_t for _ in range(self.n_rows)]
        self.hist = None

    def _bins(self, d, w):
        h = np.zeros(BINS, dtype=np.int64)
        np.add.at(h, d, w)
        return h

    def next_pass(self):
        """This shard's int64 weight histograms of the next pass (flat), or None when no pass is left."""
        if self.n_rows == 0 or self.pass_ == PASSES:
            return None
        p = self.pass_
        shift = np.uint64(56 - 8 * p)
        if p == 0:
            h = np.zeros((self.n_rows, BINS), dtype=np.int64)
            for r in range(self.n_rows):
                m = self.ok[r]
                h[r] = self._bins((self.keys[r][m] >> shift).astype(np.int64), self.w[m])
        else:
            h = np.zeros((self.n_rows, self.n_t, BINS), dtype=np.int64)
            for r in range(self.n_rows):
                m = self.ok[r]
                k, w = self.keys[r][m], self.w[m]
                top = k >> np.uint64(64 - 8 * p)
                d = ((k >> shift) & np.uint64(BINS - 1)).astype(np.int64)
                for t in range(self.n_t):
                    sel = top == np.uint64(self.prefix[r][t])
                    h[r, t] = self._bins(d[sel], w[sel])
        self.hist = h.reshape(-1)
        return self.hist

    def commit(self, reduced=None):
        """Raises ValueError (after moving on, as the library returns RSCM_ERR_INVALID) if a row's W exceeds 2^53."""
        h = np.asarray(self.hist if reduced is None else reduced, dtype=np.int64)
        p = self.pass_
        over = False
        for r in range(self.n_rows):
            for t in range(self.n_t):
                if p == 0:
                    bins = h.reshape(self.n_rows, BINS)[r]
                    W = int(sum(int(b) for b in bins))
                    big = W > W_MAX or (bins < 0).any()
                    over = over or big
                    self.weight[r] = 0 if big else W
                    if big or W == 0:
                        self.rank[r][t] = -1
                        continue
                    want = weight_target(self.q[t], W)
                else:
                    want = self.rank[r][t]
                    if want < 0:
                        continue
                    bins = h.reshape(self.n_rows, self.n_t, BINS)[r, t]
                below, b = 0, 0
                while b < BINS - 1 and want > below + int(bins[b]):
                    below += int(bins[b])
                    b += 1
                self.prefix[r][t] = b if p == 0 else (self.prefix[r][t] << 8) | b
                self.rank[r][t] = want - below
        self.pass_ += 1
        if over:
            raise ValueError("a row's weights sum to more than 2^53")

    def result(self):
        out = np.full((self.n_rows, self.n_t), np.nan)
        for r in range(self.n_rows):
            if self.weight[r] == 0:
                continue
            for k in range(self.n_t):
                out[r, k] = key_value(self.prefix[r][k])
        return {"weight": np.asarray(self.weight, dtype=np.int64), "quantiles": out}


def sharded_wquantiles(shards, weights, q):
    """The whole weighted select over several shards ([n_rows][n_i] rows, [n_i] weights each), histograms summed between passes."""
    sel = [HostWSelect(s, w, q) for s, w in zip(shards, weights)]
    while True:
        bufs = [s.next_pass() for s in sel]
        if bufs[0] is None:
            break
        total = np.sum(bufs, axis=0)
        for s in sel:
            s.commit(total)
    return [s.result() for s in sel]
