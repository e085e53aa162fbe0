"""Worker for tests/test_distributed_indicators_cpu.py: one rank of a gloo group running rscm_amd.distributed's
quantile_rows_global(anomaly=True), quantile_vectors_global and exceedance_global.  The compute needs a GPU, so the rank's
ensemble is a stand-in: rows, weights and the indicator vector are known functions of the GLOBAL member id, each member's
baseline and anomalies come from tests/host_indicators.py, and the staged selects are the numpy restatements of select.hip's
two modes.  What is under test is the product's loops and reductions."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from rscm_amd.ensemble import exceedance_result  # noqa: E402
from tests._dist_quantile_worker import _Select, global_rows  # noqa: E402
from tests._dist_wquantile_worker import _Select as _WSelect  # noqa: E402
from tests.host_indicators import anomaly, baseline, exceedance_counts, indicators  # noqa: E402

Q = [0.0, 0.05, 0.5, 0.95, 1.0, 1e-12]
THR = [1.5, 2.0, 3.0]
REF = (0, 3)   # the baseline rows


def global_weights(n_total):
    g = np.arange(n_total)
    return ((g * 2654435761) % 1000).astype(np.int64)   # zeros among them


def global_series(n_total):
    """[8][n_total] warming-like rows: ramps per member with NaN members and a member that never warms."""
    g = np.arange(n_total)
    t = np.arange(8.0)[:, None]
    x = 0.1 * ((g % 17) + 1)[None, :] * t + 0.01 * (g % 3)[None, :]
    x[:, g % 29 == 7] = np.nan
    x[5, g % 31 == 4] = np.nan
    x[:, g % 23 == 1] = -1.0
    return x


class StandInEnsemble:
    def __init__(self, count, offset, n_total):
        sl = slice(offset, offset + count)
        self.rows = global_rows(n_total)[:, sl]
        self.series = global_series(n_total)[:, sl]
        self.w = global_weights(n_total)[sl]
        self.base = None

    def set_baseline(self, var, t_begin, t_end, t_stride=1):
        self.base = baseline(self.series[t_begin:t_end:t_stride])

    def indicators(self, var, t_begin, t_end, t_stride=1, thresholds=(), anomaly=False, slot=0):
        r = self.series[t_begin:t_end:t_stride]
        return indicators(r, 2000.0 + np.arange(t_begin, t_end, t_stride), thresholds, self.base if anomaly else None)

    def select(self, var, q, t_begin=0, t_end=None, t_stride=1, weighted=False, anomaly=False):
        src = self.series if var == 2 else self.rows
        r = src[t_begin:t_end:t_stride]
        if anomaly:
            r = globals()["anomaly"](r, self.base)
        return _WSelect(r, self.w, q) if weighted else _Select(r, q)

    def select_vectors(self, vectors, q, weighted=False):
        r = np.stack(vectors)
        return _WSelect(r, self.w, q) if weighted else _Select(r, q)

    def exceedance(self, vector, thresholds, weighted=False):
        return exceedance_result(*exceedance_counts(vector, thresholds, self.w if weighted else None))


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).astype(str).tolist()


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, n_total)
    se.ensemble.set_baseline(2, *REF)
    out = {"rank": rank, "world": dist.get_world_size()}
    for w in (False, True):
        tag = "w" if w else "u"
        a = se.quantile_rows_global(2, Q, 0, None, 1, weighted=w, anomaly=True)
        ind = se.ensemble.indicators(2, 2, 8, 1, THR, anomaly=True)
        vecs = [ind["mean"], ind["peak"], ind["peak_time"]] + ind["crossing"]
        v = se.quantile_vectors_global(vecs, Q, weighted=w)
        e = se.exceedance_global(ind["peak"], THR, weighted=w)
        out[tag] = {"anomaly": _bits(a["quantiles"]), "vectors": _bits(v["quantiles"]),
                    "n": (a["weight"] if w else a["count"]).tolist(), "vn": (v["weight"] if w else v["count"]).tolist(),
                    "hits": e["hits"].tolist(), "total": e["total"], "prob": _bits(e["probability"])}
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
