"""CPU tier of the exceedance and observation rank of stored rows (rscm_ens_exceedance_rows; the definition is stated in
include/rscm_gpu.h).

* tests/host_exceedance_rows.py, the restatement in numpy and Python integers, against a brute-force Python loop over members on
  tied, NaN, +-Inf and +-0 values.
* The finishers ``rscm_amd.ensemble.exceedance_rows_result`` / ``rank_rows_result`` and ``rank_histogram`` against
  ``fractions.Fraction``; two halves of an ensemble add up to the whole; shape errors are raised before the library is touched.
* ``rscm_amd.distributed.exceedance_rows_global`` / ``rank_rows_global`` on stand-in ensembles
  (tests/_dist_exceedance_rows_worker.py): alone in one process, and over a real 2-rank gloo group on 127.0.0.1."""
import json
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import host_exceedance_rows as he
from tests._dist_exceedance_rows_worker import CALLS, N_GROUPS, N_ROWS, THRESHOLDS, StandInEnsemble, bits, global_data, results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=131, rows=5, seed=4):
    """Rows rounded to one decimal (ties), with NaN, both infinities and both zeros among them; weights with zeros and one of 2^40;
    groups with members of none; a baseline with a NaN."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.standard_normal((rows, n)), 1)
    X[2:, 11] = np.nan
    X[1, 20], X[1, 21] = np.inf, -np.inf
    X[0, 30], X[0, 31] = 0.0, -0.0
    w = rng.integers(0, 9, n)
    w[40] = 1 << 40
    groups = rng.integers(-1, 3, n).astype(np.int32)
    b = np.round(X[:2].mean(axis=0), 1)
    b[50] = np.nan
    return X, w, groups, b


def _brute(X, thr, w=None, groups=None, G=1, baseline=None):
    """The definition member by member in Python floats and integers."""
    R, n = X.shape
    thr = np.asarray(thr, dtype=np.float64)
    K = thr.shape[-1]
    hits = [[[0] * K for _ in range(G)] for _ in range(R)]
    equal = [[[0] * K for _ in range(G)] for _ in range(R)]
    total = [[0] * G for _ in range(R)]
    for r in range(R):
        for i in range(n):
            x = float(X[r, i]) - float(baseline[i]) if baseline is not None else float(X[r, i])
            g = 0 if groups is None else int(groups[i])
            if math.isnan(x) or g < 0:
                continue
            wi = 1 if w is None else int(w[i])
            total[r][g] += wi
            for k in range(K):
                t = float(thr[r, k] if thr.ndim == 2 else thr[k])
                hits[r][g][k] += wi if x >= t else 0
                equal[r][g][k] += wi if x == t else 0
    return hits, equal, total


def test_the_restatement_against_a_loop_over_members():
    X, w, groups, b = _data()
    fixed = [0.0, 0.1, -np.inf, np.inf, np.nan, -0.0, 1.0, -2.5]
    per_row = np.round(np.random.default_rng(1).standard_normal((X.shape[0], 3)), 1)
    per_row[1, 0], per_row[3] = np.nan, [np.inf, -np.inf, 0.0]
    for thr in (fixed, per_row):
        for weights, grp, baseline in ((None, None, None), (w, None, None), (None, groups, None), (w, groups, b), (None, None, b)):
            G = 3 if grp is not None else 1
            got = he.sums(X, thr, weights, grp, G if grp is not None else None, baseline)
            want = _brute(X, thr, weights, grp, G, baseline)
            for a, c in zip(got, want):
                assert a.dtype == np.int64 and a.tolist() == c
    hits, equal, total = he.sums(X, fixed)
    n = X.shape[1]
    assert total[:, 0].tolist() == [n, n, n - 1, n - 1, n - 1]
    assert (hits[:, 0, 2] == total[:, 0]).all() and hits[:, 0, 3].tolist() == [0, 1, 0, 0, 0] and equal[1, 0, 2] == 1   # -Inf, +Inf
    assert not hits[:, 0, 4].any() and not equal[:, 0, 4].any()                                                      # a NaN threshold
    assert (hits[:, :, 0] == hits[:, :, 5]).all() and (equal[:, :, 0] == equal[:, :, 5]).all() and equal[0, 0, 0] >= 2   # -0 equals +0
    assert he.sums(X, fixed, w)[2].max() > 1 << 40


def _fraction_dicts(hits, equal, total, record):
    prob = [[[float(Fraction(int(h), int(t))) if t else math.nan for h in hk] for hk, t in zip(hr, tr)] for hr, tr in zip(hits, total)]
    pit = [[float(Fraction(2 * (int(t) - int(h[0])) + int(e[0]), 2 * int(t))) if t and not math.isnan(rec) else math.nan
            for h, e, t in zip(hr, er, tr)] for hr, er, tr, rec in zip(hits, equal, total, record)]
    return np.array(prob), np.array(pit)


def test_the_finishers_against_fractions():
    """total == 0 (a row of NaN, and a group nobody is in), no record, a record at or above every member; weights that take the sums
    past 2^53, where a conversion to double before the division would round twice."""
    from rscm_amd.ensemble import exceedance_rows_result, rank_rows_result
    X, w, groups, b = _data()
    X[4] = np.nan
    record = np.array([0.1, np.nan, 99.0, -99.0, 0.0])
    big = w.astype(np.int64) * 3 + (1 << 47)                       # every sum of a few members is beyond 2^53 and odd at places
    for weights, grp in ((None, None), (w, None), (big, None), (w, groups), (big, groups)):
        G = 4 if grp is not None else 1                            # group 3 has no member
        kw = dict(weights=weights, groups=grp, n_groups=G if grp is not None else None)
        hits, equal, total = he.sums(X, record[:, None], **kw)
        prob, pit = _fraction_dicts(hits, equal, total, record)
        got = exceedance_rows_result(hits, total, grouped=grp is not None)
        want = {"hits": hits, "total": total, "probability": prob}
        assert he.same(got, want if grp is not None else {k: v[:, 0] for k, v in want.items()})
        assert he.same(got, he.exceedance_rows(X, record[:, None], **kw))
        got = rank_rows_result(hits[..., 0], equal[..., 0], total, record, grouped=grp is not None)
        want = {"below": total - hits[..., 0], "equal": equal[..., 0], "total": total, "pit": pit}
        assert he.same(got, want if grp is not None else {k: v[:, 0] for k, v in want.items()})
        assert he.same(got, he.rank_rows(X, record, **kw))
        p = np.asarray(got["pit"]).reshape(5, -1)
        assert np.isnan(p[1]).all() and np.isnan(p[4]).all()       # no record; no weight
        assert (p[2, :3] == 1.0).all() and (p[3, :3] == 0.0).all()  # above every member, below every member
        if grp is not None:
            assert np.isnan(p[:, 3]).all() and not np.asarray(got["total"])[:, 3].any()
        # the finishers take the arrays with the group axis dropped as well
        if grp is None:
            assert he.same(exceedance_rows_result(hits[:, 0], total[:, 0], grouped=False), he.exceedance_rows(X, record[:, None], **kw))
            assert he.same(rank_rows_result(hits[:, 0, 0], equal[:, 0, 0], total[:, 0], record, grouped=False), got)
    assert int(he.sums(X, record[:, None], big)[2].max()) > 1 << 53


def test_rank_histogram_bins_in_integers():
    from rscm_amd.ensemble import rank_histogram
    X, w, groups, _ = _data(n=200, rows=40, seed=9)
    rng = np.random.default_rng(10)
    record = np.round(rng.standard_normal(40), 1)
    record[3], record[7], record[8], record[9] = np.nan, 99.0, -99.0, np.nanmax(X[9])     # a gap, above all, below all, at the largest
    X[12] = np.nan                                                                   # a row without weight
    for weights, grp in ((None, None), (w, None), (w, groups)):
        G = 3 if grp is not None else 1
        r = he.rank_rows(X, record, weights, grp, G if grp is not None else None)
        for n_bins in (1, 4, 10, 7):
            got = rank_histogram(r["below"], r["equal"], r["total"], n_bins, record)
            assert got.dtype == np.int64 and got.shape == ((G, n_bins) if grp is not None else (n_bins,))
            assert (got == he.rank_histogram(r["below"], r["equal"], r["total"], n_bins, record)).all()
            want = np.zeros((G, n_bins), dtype=np.int64)
            b2, e2, t2 = (np.asarray(r[k]).reshape(40, G) for k in ("below", "equal", "total"))
            for t in range(40):
                for g in range(G):
                    if math.isnan(record[t]) or t2[t, g] == 0:
                        continue
                    f = n_bins * Fraction(2 * int(b2[t, g]) + int(e2[t, g]), 2 * int(t2[t, g]))
                    want[g, min(math.floor(f), n_bins - 1)] += 1
            assert (got.reshape(G, n_bins) == want).all()
            assert got.sum() == 38 * G                                               # the gap and the row without weight are left out
        top = rank_histogram(np.asarray(r["below"])[7:8], np.asarray(r["equal"])[7:8], np.asarray(r["total"])[7:8], 10)
        assert (top.reshape(G, 10)[:, 9] == 1).all() and top.sum() == G              # a record above every member: the last bin
        at_max = rank_histogram(np.asarray(r["below"])[9:10], np.asarray(r["equal"])[9:10], np.asarray(r["total"])[9:10], 10)
        assert at_max.sum() == G
        low = rank_histogram(np.asarray(r["below"])[8:9], np.asarray(r["equal"])[8:9], np.asarray(r["total"])[8:9], 10)
        assert (low.reshape(G, 10)[:, 0] == 1).all()
        # without the record a row that has none reads as one above every member
        assert rank_histogram(r["below"], r["equal"], r["total"], 10).sum() == 39 * G
    with pytest.raises(ValueError):
        rank_histogram([1], [0], [2], 0)
    with pytest.raises(ValueError):
        rank_histogram([1, 2], [0], [2, 2], 4)


def test_two_halves_add_up():
    from rscm_amd.ensemble import exceedance_rows_result, rank_rows_result
    X, w, groups, b = _data()
    thr = [0.0, 0.5, -1.0]
    record = np.array([0.1, np.nan, 0.3, -0.2, 0.0])
    h = X.shape[1] // 3
    parts = (slice(0, h), slice(h, None))
    whole = he.sums(X, thr, w, groups, 3, b)
    halves = [he.sums(X[:, s], thr, w[s], groups[s], 3, b[s]) for s in parts]
    for k in range(3):
        assert (halves[0][k] + halves[1][k] == whole[k]).all()
    got = exceedance_rows_result(halves[0][0] + halves[1][0], halves[0][2] + halves[1][2])
    assert he.same(got, he.exceedance_rows(X, thr, w, groups, 3, b))
    r = [he.sums(X[:, s], record[:, None], w[s]) for s in parts]
    got = rank_rows_result((r[0][0] + r[1][0])[..., 0], (r[0][1] + r[1][1])[..., 0], r[0][2] + r[1][2], record, grouped=False)
    assert he.same(got, he.rank_rows(X, record, w))


def test_shape_errors_come_before_the_library(monkeypatch):
    """exceedance_rows and rank_rows check their thresholds and record first: with a handle that cannot make any call (no library,
    no device) the shape errors are still ValueErrors, and a good shape reaches the missing library."""
    from rscm_amd.ensemble import Ensemble, exceedance_rows_thresholds, rank_rows_record
    e = object.__new__(Ensemble)
    e.n_times = 6

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was touched: {name}")

    e._lib, e._h = NoLibrary(), None
    for bad in (1.5, [], np.zeros(9), np.zeros((5, 2)), np.zeros((6, 0)), np.zeros((6, 9)), np.zeros((6, 2, 1))):
        with pytest.raises(ValueError, match="thresholds must be"):
            e.exceedance_rows(1, bad)
        with pytest.raises(ValueError):
            exceedance_rows_thresholds(bad, 6)
    with pytest.raises(ValueError, match="thresholds must be"):
        e.exceedance_rows(1, np.zeros((6, 2)), 0, 6, 2)              # three rows, six sets of thresholds
    for bad in (0.5, np.zeros(5), np.zeros((6, 1)), []):
        with pytest.raises(ValueError, match="record must be"):
            e.rank_rows(1, bad)
        with pytest.raises(ValueError):
            rank_rows_record(bad, 6)
    with pytest.raises(ValueError, match="record must be"):
        e.rank_rows(1, np.zeros(6), 0, 6, 2)
    thr, per_row = exceedance_rows_thresholds([1.5, 2, 3], 6)
    assert thr.dtype == np.float64 and thr.shape == (3,) and not per_row
    thr, per_row = exceedance_rows_thresholds(np.zeros((3, 8)), 3)
    assert thr.shape == (3, 8) and per_row
    assert rank_rows_record([1, np.nan, 3], 3).dtype == np.float64
    with pytest.raises(AssertionError, match="the library was touched"):
        e.exceedance_rows(1, [1.5])


def test_abi_minor_26_declares_and_binds_the_entry_point():
    from rscm_amd import _lib
    header = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", header).group(1)) >= 26
    assert "rscm_ens_exceedance_rows" in re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 26
    assert "rscm_ens_exceedance_rows" in _lib.SIGNATURES and hasattr(lib, "rscm_ens_exceedance_rows")
    assert int(re.search(r"#define\s+RSCM_EXCEEDANCE_ROWS_MAX_THRESHOLDS\s+(\d+)", header).group(1)) == 8 == _lib.EXCEEDANCE_ROWS_MAX_THRESHOLDS
    device = open(os.path.join(ROOT, "rscm_amd", "csrc", "rscm_device.hpp")).read()
    blocks = int(re.search(r"constexpr int kExcRowsBlocks = (\d+);", device).group(1))
    assert int(re.search(r"constexpr int64_t kExceedanceRowsMembersPerPass = (\d+);", device).group(1)) == 256 * blocks


def _want(n_total):
    rows, record, w, groups, b = global_data(n_total)
    full = dict(weights=w, groups=groups, n_groups=N_GROUPS, baseline=b)
    return {"exc_plain": bits(he.exceedance_rows(rows, THRESHOLDS)), "exc_full": bits(he.exceedance_rows(rows[1:N_ROWS:2], THRESHOLDS, **full)),
            "rank_plain": bits(he.rank_rows(rows, record)), "rank_full": bits(he.rank_rows(rows[1:N_ROWS:2], record[1:N_ROWS:2], **full))}


def test_one_process_global():
    from rscm_amd.distributed import ShardedEnsemble
    n_total = 301
    data = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: StandInEnsemble(c, 0, *data), rank=0, world=1)
    got = results(se, data[1])
    assert got == _want(n_total)
    assert [list(c) for c in se.ensemble.calls] == CALLS
    plain = se.exceedance_rows_global("T", THRESHOLDS)
    assert plain["hits"].shape == (N_ROWS, 3) and plain["total"].tolist() == [301, 301, 300, 300, 300, 300]
    assert (plain["hits"][:, 2] == [0, 0, 0, 1, 0, 0]).all()
    full = se.rank_rows_global("T", data[1][1:N_ROWS:2], 1, N_ROWS, 2, weighted=True, anomaly=True, grouped=True)
    assert full["pit"].shape == (3, N_GROUPS) and np.isnan(full["pit"][0]).all() and int(full["total"].max()) > 1 << 40


def test_two_rank_gloo_global(tmp_path):
    n_total = 301
    port = "29881"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_exceedance_rows_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    want = _want(n_total)
    assert sum(x["count"] for x in res) == n_total and all(0 < x["count"] < n_total for x in res)
    for x in res:
        assert x["world"] == 2 and x["calls"] == CALLS
        for key, value in want.items():
            assert x[key] == value, key
