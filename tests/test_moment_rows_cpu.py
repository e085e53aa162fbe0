"""CPU tier of the moments of stored rows (rscm_ens_moment_rows_sums; the definition is stated in include/rscm_gpu.h).

* tests/host_moment_rows.py, the restatement in Python integers, against plain ``fractions.Fraction`` means and variances on 5 rows
  of 257 members: per-row counting, anomaly, weights.
* ``rscm_amd.ensemble.moment_rows_result`` against the restatement, through the built library's rscm_gpu_moment_finish, which needs
  no device: the sums are formed here by the limb scheme.
* ``rscm_amd.distributed.moment_rows_global`` / ``ShardedEnsemble.moment_rows_global`` on stand-in ensembles
  (tests/_dist_moment_rows_worker.py): alone in one process, and over a real 2-rank gloo group on 127.0.0.1."""
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np

from tests import host_moment_rows as hr
from tests import host_moments as hm
from tests._dist_moment_rows_worker import N_GROUPS, N_ROWS, StandInEnsemble, bits, global_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=257, rows=5, seed=3):
    rng = np.random.default_rng(seed)
    V = np.stack([rng.uniform(0.5, 1.5, n), rng.normal(0.0, 2.0, n)])
    X = np.stack([0.2 * (t + 1) * V[0] + 0.05 * rng.normal(0.0, 1.0, n) for t in range(rows)])
    X[2:, 11] = np.nan          # drops out of rows 2 .. only
    X[1, 200] = -np.inf
    w = rng.integers(0, 9, n)   # zero weights among them
    b = X[:2].mean(axis=0)
    b[40] = np.nan
    return X, V, w, b


def _fraction_mean_var(x, w):
    """(RN(sum w x / W), RN(sum w RN(x - mean)^2 / W)) over the finite x, in Fractions."""
    ok = np.isfinite(x)
    xs, ws = x[ok].tolist(), [int(v) for v in w[ok].tolist()]
    W = sum(ws)
    mean = float(sum(Fraction(v) * k for v, k in zip(xs, ws)) / W)
    d = (x[ok] - np.float64(mean))
    p = (d * d).tolist()
    return int(ok.sum()), W, mean, float(sum(Fraction(v) * k for v, k in zip(p, ws)) / W)


def test_the_restatement_against_fractions():
    X, V, w, b = _data()
    for weights, baseline in ((None, None), (w, None), (None, b), (w, b)):
        got = hr.ungrouped(hr.moment_rows(X, (), weights, baseline=baseline))
        x = hr.row_values(X, baseline)
        ww = np.ones(X.shape[1], dtype=np.int64) if weights is None else weights
        for r in range(X.shape[0]):
            n, W, mean, var = _fraction_mean_var(x[r], ww)
            assert (got["count"][r], got["weight"][r]) == (n, W)
            assert hm.same_bits(got["mean"][r], mean) and hm.same_bits(got["var"][r], var), (r, got["mean"][r], mean)
            assert hm.same_bits(got["sd"][r], math.sqrt(var))
        # the counts differ by row: member 11 is gone from row 2 on, member 200 from row 1 alone; a baseline that is not finite
        # (members 40 and 200: it is a mean over rows 0 and 1) drops its member from every row
        n = X.shape[1]
        assert got["count"].tolist() == ([n, n - 1, n - 1, n - 1, n - 1] if baseline is None else [n - 2, n - 2, n - 3, n - 3, n - 3])


def test_the_restatement_of_the_covariances():
    """cov and the vectors' moments against Fractions over the row's own counted members (a NaN in a vector drops the member
    from every row); blocks in the definition's order."""
    X, V, w, _ = _data()
    V = V.copy()
    V[1, 30] = np.nan
    got, s1, s2 = hr.moment_rows(X, V, w, with_sums=True)
    got = hr.ungrouped(got)
    assert got["cov"].shape == (5, 2) and len(s1[0][0][2]) == 3 and len(s2[0][0][2]) == 5
    for r in range(X.shape[0]):
        ok = np.isfinite(X[r]) & np.isfinite(V).all(axis=0)
        ws = [int(v) for v in w[ok].tolist()]
        W = sum(ws)
        assert got["count"][r] == ok.sum() and not ok[30]
        mx = float(sum(Fraction(v) * k for v, k in zip(X[r, ok].tolist(), ws)) / W)
        assert hm.same_bits(got["mean"][r], mx)
        for k in range(2):
            mv = float(sum(Fraction(v) * q for v, q in zip(V[k, ok].tolist(), ws)) / W)
            assert hm.same_bits(got["vec_mean"][r, k], mv)
            p = ((X[r, ok] - np.float64(mx)) * (V[k, ok] - np.float64(mv))).tolist()
            cov = float(sum(Fraction(v) * q for v, q in zip(p, ws)) / W)
            pv = ((V[k, ok] - np.float64(mv)) * (V[k, ok] - np.float64(mv))).tolist()
            vv = float(sum(Fraction(v) * q for v, q in zip(pv, ws)) / W)
            assert hm.same_bits(got["cov"][r, k], cov) and hm.same_bits(got["vec_var"][r, k], vv)
            assert hm.same_bits(got["slope"][r, k], np.float64(cov) / np.float64(vv))
            assert hm.same_bits(got["corr"][r, k], np.float64(cov) / (np.sqrt(got["var"][r]) * np.sqrt(np.float64(vv))))
    assert (got["slope"][1:, 0] > 0).all()   # the rows were built to warm with the first vector


def test_moment_rows_result_finishes_the_limb_sums():
    from rscm_amd.ensemble import moment_rows_means, moment_rows_result
    X, V, w, b = _data()
    groups = (np.arange(X.shape[1]) % 4 - 1).astype(np.int32)   # -1: in no group; three groups interleaved
    for K, weights, grp, baseline in ((0, None, None, None), (2, w, None, b), (1, w, groups, None), (2, None, groups, b)):
        G = 3 if grp is not None else 1
        kw = dict(weights=weights, groups=grp, n_groups=G if grp is not None else None, baseline=baseline)
        want = hr.moment_rows(X, V[:K], **kw)
        a1 = hr.sums_array(X, 1, V[:K], None, **kw)
        mean = moment_rows_means(a1, K, G)
        assert mean.shape == (5, G, 1 + K) and hm.same_bits(mean[..., 0], want["mean"])
        a2 = hr.sums_array(X, 2, V[:K], mean, **kw)
        got = moment_rows_result(a1, a2, K, G, grouped=grp is not None)
        want = want if grp is not None else hr.ungrouped(want)
        assert set(got) == set(want)
        for key in want:
            assert got[key].shape == want[key].shape, key
            assert hm.same_bits(got[key], want[key]) if got[key].dtype == np.float64 else (got[key] == want[key]).all(), key
        # two shards add up element by element
        h = X.shape[1] // 3
        parts = [dict(kw, weights=None if weights is None else weights[s], groups=None if grp is None else grp[s],
                      baseline=None if baseline is None else baseline[s]) for s in (slice(0, h), slice(h, None))]
        sl = (slice(0, h), slice(h, None))
        b1 = sum(hr.sums_array(X[:, s], 1, V[:K, s], None, **p) for s, p in zip(sl, parts))
        b2 = sum(hr.sums_array(X[:, s], 2, V[:K, s], mean, **p) for s, p in zip(sl, parts))
        assert hr.array_sums(b1, K, 1) == hr.array_sums(a1, K, 1) and hr.array_sums(b2, K, 2) == hr.array_sums(a2, K, 2)
        again = moment_rows_result(b1, b2, K, G, grouped=grp is not None)
        assert all(hm.same_bits(again[key], got[key]) for key in got if got[key].dtype == np.float64)


def test_a_row_without_weight_and_a_non_finite_centre():
    from rscm_amd.ensemble import moment_rows_result
    X = np.array([[1.0, 2.0, 4.0], [np.nan, np.nan, np.nan], [1e308, -1e308, 1e308]])
    a1 = hr.sums_array(X, 1)
    a2 = hr.sums_array(X, 2, (), hr.means(hr.sums(X, 1)))
    got = moment_rows_result(a1, a2, 0, 1, grouped=False)
    assert got["count"].tolist() == [3, 0, 3]
    assert got["mean"][0] == 7.0 / 3.0 and np.isnan(got["mean"][1]) and np.isnan(got["var"][1])
    assert np.isfinite(got["mean"][2]) and np.isnan(got["var"][2])   # the products overflow: NaN in that row's var only
    assert np.isfinite(got["var"][0])


def _want(n_total):
    rows, V, w, groups, baseline = global_data(n_total)
    plain = hr.ungrouped(hr.moment_rows(rows))
    full = hr.moment_rows(rows[1:N_ROWS:2], V[[1, 0]], w, groups, N_GROUPS, baseline)
    return bits(plain), bits(full)


def test_one_process_moment_rows_global():
    from rscm_amd.distributed import ShardedEnsemble
    n_total = 301
    data = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: StandInEnsemble(c, 0, *data), rank=0, world=1)
    plain, full = _want(n_total)
    got = se.moment_rows_global("T")
    assert got["mean"].shape == (N_ROWS,) and "cov" not in got and got["count"][0] - got["count"][2] == 1
    assert bits(got) == plain
    got = se.moment_rows_global("T", 1, N_ROWS, 2, vectors=[1, 0], weighted=True, anomaly=True, grouped=True)
    assert got["mean"].shape == (3, N_GROUPS) and got["slope"].shape == (3, N_GROUPS, 2)
    assert bits(got) == full
    assert se.ensemble.calls == [(1, False, False, False), (2, False, False, False), (1, True, True, True), (2, True, True, True)]


def test_two_rank_gloo_moment_rows_global(tmp_path):
    n_total = 301
    port = "29879"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_moment_rows_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    plain, full = _want(n_total)
    assert sum(x["count"] for x in res) == n_total and all(0 < x["count"] < n_total for x in res)
    for x in res:
        assert x["world"] == 2
        assert x["plain"] == plain and x["full"] == full
        assert x["calls"] == [[1, False, False, False], [2, False, False, False], [1, True, True, True], [2, True, True, True]]
    assert np.isfinite(np.array(plain["mean"], dtype=np.uint64).view(np.float64)).all()
