"""The grouped staged select of rscm_amd/csrc/select.hip (RSCM_SELECT_GROUPED) restated in numpy on top of tests/host_select.py and
tests/host_wselect.py: one HostSelect / HostWSelect per group over the members with ``group[i] == g`` (in member order; -1: in no
group), run through the same passes, their histograms laid out as the library lays them out -- ``[rows][G][256]`` int64 in pass 0,
``[rows][G][n_t][256]`` later -- so that shards sum them as the handles of a sharded select do.  Results are group-major, as
``Ensemble.quantile_rows(..., grouped=True)`` returns them.  tests/test_host_grouped_select.py pins it against numpy on the group
subsets; the CPU rehearsal of the grouped rscm_amd.distributed.quantile_rows_global (tests/_dist_grouped_worker.py) uses it as the
stand-in ensemble's select."""
import numpy as np

from tests.host_select import BINS, PASSES, HostSelect
from tests.host_wselect import HostWSelect

MAX_GROUPS = 64


class HostGSelect:
    """One handle's grouped select over ``rows`` ([n_rows][n_local]) with ``group`` ([n_local] int, -1 or 0 <= id < n_groups) and,
    for the weighted form, member weights ``w`` ([n_local] int64)."""

    def __init__(self, rows, group, n_groups, q, w=None):
        rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
        group = np.asarray(group, dtype=np.int64)
        if not 1 <= n_groups <= MAX_GROUPS:
            raise ValueError("n_groups must be in [1, 64]")
        if group.shape != (rows.shape[1],) or (group < -1).any() or (group >= n_groups).any():
            raise ValueError("one group id in [-1, n_groups) per member")
        self.n_rows, self.G, self.weighted = rows.shape[0], int(n_groups), w is not None
        if self.weighted:
            w = np.asarray(w, dtype=np.int64)
            self.sub = [HostWSelect(rows[:, group == g], w[group == g], q) for g in range(self.G)]
        else:
            self.sub = [HostSelect(rows[:, group == g], q) for g in range(self.G)]
        self.n_t = self.sub[0].n_t
        self.pass_ = 0
        self.hist = None

    def _shape(self):
        return (self.n_rows, self.G, BINS) if self.pass_ == 0 else (self.n_rows, self.G, self.n_t, BINS)

    def next_pass(self):
        """This shard's int64 histograms of the next pass in the library's layout (flat), or None when no pass is left."""
        if self.n_rows == 0 or self.pass_ == PASSES:
            return None
        h = np.zeros(self._shape(), dtype=np.int64)
        for g, s in enumerate(self.sub):
            h[:, g] = s.next_pass().reshape(h[:, g].shape)
        self.hist = h.reshape(-1)
        return self.hist

    def commit(self, reduced=None):
        """Raises ValueError (after moving every group on) if a (row, group) weight exceeds 2^53."""
        h = np.asarray(self.hist if reduced is None else reduced, dtype=np.int64).reshape(self._shape())
        over = None
        for g, s in enumerate(self.sub):
            try:
                s.commit(np.ascontiguousarray(h[:, g]).reshape(-1))
            except ValueError as e:
                over = e
        self.pass_ += 1
        if over is not None:
            raise over

    def result(self):
        res = [s.result() for s in self.sub]
        key = "weight" if self.weighted else "count"
        return {key: np.stack([r[key] for r in res]), "quantiles": np.stack([r["quantiles"] for r in res])}


def sharded_gquantiles(shards, groups, n_groups, q, weights=None):
    """The whole grouped select over several shards ([n_rows][n_i] rows, [n_i] groups and, weighted, [n_i] weights each), their
    histograms summed between the passes; every shard's result."""
    ws = [None] * len(shards) if weights is None else weights
    sel = [HostGSelect(s, g, n_groups, q, w) for s, g, w in zip(shards, groups, ws)]
    while True:
        bufs = [s.next_pass() for s in sel]
        if bufs[0] is None:
            break
        total = np.sum(bufs, axis=0)
        for s in sel:
            s.commit(total)
    return [s.result() for s in sel]


def exceedance_grouped(v, group, n_groups, thresholds, w=None):
    """(hits[G][k], total[G]) as Python-integer sums: rscm_ens_exceedance_grouped."""
    v, group = np.asarray(v, dtype=np.float64), np.asarray(group)
    w = np.ones(v.size, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    hits = [[sum(int(x) for x in w[(group == g) & (v >= t)]) for t in thresholds] for g in range(n_groups)]
    total = [sum(int(x) for x in w[(group == g) & ~np.isnan(v)]) for g in range(n_groups)]
    return np.array(hits, dtype=np.int64).reshape(n_groups, len(thresholds)), np.array(total, dtype=np.int64)
