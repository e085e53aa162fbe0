"""GPU tier of the exceedance and observation rank of a stored variable at every row (csrc/exceedance_rows.hip, ABI minor 26) against
the numpy and Python integers of tests/host_exceedance_rows.py.  Every comparison is of integers, or of doubles that are one exact
quotient of those integers rounded once, so equality is the only tolerance.

The rows are those of a small two-layer ensemble, overwritten with set_state so that they take any bits."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import host_exceedance_rows as he
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import f_syn, magicc_chain, two_layer_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_AXIS = np.arange(1750.0, 1758.0)          # 8 rows


def _members_per_pass() -> int:
    """Members one pass of the kernel's capped grid takes, read from the code: kExcRowsBlocks blocks of four waves of 64."""
    text = open(os.path.join(ROOT, "rscm_amd", "csrc", "rscm_device.hpp")).read()
    blocks = int(re.search(r"constexpr int kExcRowsBlocks = (\d+);", text).group(1))
    per_pass = int(re.search(r"constexpr int64_t kExceedanceRowsMembersPerPass = (\d+);", text).group(1))
    hip = open(os.path.join(ROOT, "rscm_amd", "csrc", "exceedance_rows.hip")).read()
    threads = int(re.search(r"constexpr int kExcRowsThreads = (\d+);", hip).group(1))
    assert per_pass == blocks * threads
    return per_pass


def _rows_ens(ra, n, X=None, steps=None, t=T_AXIS, **kw):
    """A two-layer ensemble run to `steps` (None: the end, 0: not at all); X[R][n] then overwrites rows 0 .. R-1 of variable 1."""
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0), **kw)
    e.set_params(two_layer_params(n))
    e.set_forcing(f_syn(t))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    if steps != 0:
        e.run(steps)
    if X is not None:
        _fill(e, X)
    return e


def _fill(e, X, var=1):
    for t, row in enumerate(np.asarray(X, dtype=np.float64)):
        e.set_state(var, t, row)
    got = e.get_series(var, 0, len(X))
    assert np.array_equal(got.view(np.uint64), np.asarray(X, dtype=np.float64).view(np.uint64))


def _tied(rng, rows, n):
    """Rows of standard normals rounded to one decimal: a few dozen distinct values, so full of ties."""
    return np.round(rng.standard_normal((rows, n)), 1)


def _weights(rng, n):
    """Weights of 0, values below 2^20 and one of 2^40: a sum truncated to 32 bits anywhere fails."""
    w = rng.integers(0, 1 << 20, n)
    w[rng.random(n) < 0.1] = 0
    w[n // 2] = 1 << 40
    return w


def _check(e, X, thr, w=None, groups=None, G=None, baseline=None, rows=None, what="", var=1):
    """exceedance_rows over the rows `rows` = (t_begin, t_end, t_stride) of X (default: all of X) against the restatement."""
    X = np.asarray(X, dtype=np.float64)
    tb, te, ts = rows if rows is not None else (0, X.shape[0], 1)
    want = he.exceedance_rows(X[tb:te:ts], thr, w, groups, G, baseline)
    got = e.exceedance_rows(var, thr, tb, te, ts, weighted=w is not None, grouped=groups is not None, anomaly=baseline is not None)
    assert he.same(got, want), (what, got, want)
    return got


def _check_rank(e, X, record, w=None, groups=None, G=None, baseline=None, rows=None, what="", var=1):
    X = np.asarray(X, dtype=np.float64)
    tb, te, ts = rows if rows is not None else (0, X.shape[0], 1)
    want = he.rank_rows(X[tb:te:ts], record, w, groups, G, baseline)
    got = e.rank_rows(var, record, tb, te, ts, weighted=w is not None, grouped=groups is not None, anomaly=baseline is not None)
    assert he.same(got, want), (what, got, want)
    return got


# ---- sizes and shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_rows_and_threshold_counts(ra, n):
    """One member, the edges of a wave and of a block, several blocks; 1, 2 and 5 rows and a stride of 2 whose end is off the
    stride; K = 1, 3, 8, fixed and per row -- against the restatement, and every row against ``exceedance`` of that row (a
    DeviceVector into the fully stored series), plain and weighted."""
    rng = np.random.default_rng(n)
    X = _tied(rng, 8, n)
    w = _weights(rng, n)
    fixed = np.array([0.0, -0.5, 1.2, 0.3, -1.7, 2.0, 0.1, -0.1])
    table = np.round(rng.standard_normal((8, 8)), 1)
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        base = e.series_devptr(1)
        for rows in ((0, 1, 1), (0, 2, 1), (0, 5, 1), (1, 8, 2)):
            sel = slice(*rows)
            for K in (1, 3, 8):
                for weights in (None, w):
                    got = _check(e, X, fixed[:K], weights, rows=rows, what=(n, rows, K, "fixed"))
                    _check(e, X, table[sel, :K], weights, rows=rows, what=(n, rows, K, "per row"))
                    for r, t in enumerate(range(*rows)):
                        row_t = ra.ensemble.DeviceVector(base + 8 * n * t, n, np.float64, e)
                        one = e.exceedance(row_t, fixed[:K], weighted=weights is not None)
                        assert (one["hits"] == got["hits"][r]).all() and one["total"] == got["total"][r], (n, rows, K, t)
        assert (_check(e, X, fixed)["total"] == n).all()


def test_past_the_grid_cap(ra):
    """One tile and three members past what one pass of the capped grid takes, two rows: the grid-stride second pass and its ragged
    tile, with a NaN and the heaviest member in that tail, weighted, in two contiguous groups that meet inside the tail."""
    n = _members_per_pass() + 64 + 3
    rng = np.random.default_rng(11)
    X = _tied(rng, 2, n)
    X[0, n - 2] = np.nan
    w = rng.integers(0, 1 << 20, n)
    w[n - 1] = 1 << 40
    X[:, n - 1] = [0.3, -5.0]                 # the heaviest member: at a threshold in row 0, below every one in row 1
    groups = (np.arange(n) >= n - 30).astype(np.int32)
    thr = [0.3, -1.0, 1.5]
    record = np.array([0.3, -0.2])
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        e.set_member_groups(groups, 2)
        got = _check(e, X, thr, w, groups, 2, what="past the cap")
        assert got["total"][0, 1] > 1 << 40 and got["hits"][0, 1, 0] > 1 << 40 and got["hits"][1, 1, 1] < 1 << 40
        plain = _check(e, X, thr, groups=groups, G=2, what="past the cap, counts")
        assert plain["total"].tolist() == [[n - 30, 29], [n - 30, 30]]
        _check(e, X, thr, w, what="past the cap, one group")
        _check(e, X, thr, what="past the cap, plain")
        r = _check_rank(e, X, record, w, groups, 2, what="past the cap, rank")
        assert r["equal"][0, 1] >= 1 << 40


# ---- values -----------------------------------------------------------------------------------------------------------------------

def test_special_values_and_thresholds(ra):
    """NaN, +Inf and -Inf among the members; -0.0 against a threshold of +0.0, which counts in both hits and equal; values equal to
    the threshold bit for bit; a NaN threshold in some rows of a per-row table; thresholds of +-Inf."""
    n = 300
    rng = np.random.default_rng(2)
    X = _tied(rng, 5, n)
    X[0, :40] = -0.0
    X[0, 40:60] = 0.0
    X[1, 5], X[1, 70], X[1, 299] = np.nan, np.inf, -np.inf
    X[2, 64:128] = np.nan                       # a whole wave of one row
    X[3, :] = np.nan                            # a row nobody takes part in
    X[4, 100:110] = 0.1 + 0.2                   # 0.30000000000000004: not the 0.3 of the rounded members
    fixed = [0.0, np.inf, -np.inf, 0.3, 0.1 + 0.2, np.nan, -0.0, 1e308]
    table = np.array([[0.0, np.nan], [np.inf, -np.inf], [np.nan, np.nan], [0.0, 1.0], [0.1 + 0.2, 0.3]])
    record = np.array([0.0, np.inf, np.nan, 0.0, 0.1 + 0.2])
    with _rows_ens(ra, n, X) as e:
        got = _check(e, X, fixed, what="special, fixed")
        assert got["total"].tolist() == [n, n - 1, n - 64, 0, n]
        assert (got["hits"][:, 0] == got["hits"][:, 6]).all() and got["hits"][0, 0] >= 60      # -0 is at or above +0
        assert got["hits"][:, 1].tolist() == [0, 1, 0, 0, 0] and (got["hits"][:, 2] == got["total"]).all()
        assert not got["hits"][:, 5].any() and np.isnan(got["probability"][3]).all()
        assert (got["probability"][[0, 1, 2, 4], 5] == 0.0).all()                              # a NaN threshold: 0 of total
        _check(e, X, table, what="special, per row")
        r = _check_rank(e, X, record, what="special, rank")
        assert r["equal"][0] >= 60 and r["equal"][1] == 1 and r["equal"][4] == 10              # both zeros; +Inf; bit for bit
        assert r["below"][2] == r["total"][2] == n - 64 and np.isnan(r["pit"][2]) and np.isnan(r["pit"][3])
        assert r["below"][1] == n - 2


def test_weights(ra):
    """Weights of 0, values below 2^20 and one of 2^40; total and hits above 2^32; weights that are set but not asked for."""
    n = 777
    rng = np.random.default_rng(7)
    X = _tied(rng, 3, n)
    w = _weights(rng, n)
    w[64:128] = 0                               # a wave without weight
    X[:, n // 2] = 9.0                          # the heaviest member is at or above every threshold
    thr = [0.0, 9.0, -0.4]
    with _rows_ens(ra, n, X) as e:
        plain = _check(e, X, thr, what="no weights set")
        e.set_member_weights(w)
        got = _check(e, X, thr, w, what="weighted")
        assert (got["total"] > 1 << 32).all() and (got["hits"] > 1 << 32).all() and (got["total"] == int(w.sum())).all()
        assert he.same(e.exceedance_rows(1, thr, 0, 3), plain)
        r = _check_rank(e, X, np.array([9.0, 0.1, np.nan]), w, what="weighted rank")
        assert r["equal"][0] >= 1 << 40 and r["below"][1] < 1 << 40
        e.set_member_weights(np.zeros(n, dtype=np.int64))
        none = _check(e, X, thr, np.zeros(n, dtype=np.int64), what="no weight at all")
        assert not none["total"].any() and np.isnan(none["probability"]).all()


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
@pytest.mark.parametrize("G", [1, 3, 64])
def test_grouped(ra, G, layout):
    """1, 3 and 64 groups, contiguous blocks and posterior()'s i % G, with members of group -1 and (3 and 64 groups) one group that
    no member has; plain and weighted, fixed and per-row thresholds, exceedance and rank; every group against ``exceedance`` of
    row 0."""
    n = 1000
    rng = np.random.default_rng(8 + G)
    groups = (np.arange(n) * G // n if layout == "contiguous" else np.arange(n) % G).astype(np.int32)
    groups[rng.random(n) < 0.05] = -1
    empty = G - 2
    if G > 1:
        groups[groups == empty] = -1
    X = _tied(rng, 3, n) + 0.5 * (groups % 3)
    X[1, groups == 0] = np.nan                  # a group that is empty in row 1
    w = _weights(rng, n)
    thr = [0.5, 0.0, 1.5]
    table = np.round(rng.standard_normal((3, 2)), 1)
    record = np.array([0.5, 0.7, np.nan])
    with _rows_ens(ra, n, X) as e:
        e.set_member_groups(groups, G)
        e.set_member_weights(w)
        for weights in (None, w):
            got = _check(e, X, thr, weights, groups, G, what=(G, layout, "fixed"))
            assert got["hits"].shape == (3, G, 3) and got["total"].shape == (3, G)
            assert got["total"][1, 0] == 0 and np.isnan(got["probability"][1, 0]).all()
            if G > 1:
                assert not got["total"][:, empty].any()
            _check(e, X, table, weights, groups, G, what=(G, layout, "per row"))
            r = _check_rank(e, X, record, weights, groups, G, what=(G, layout, "rank"))
            assert r["pit"].shape == (3, G) and np.isnan(r["pit"][2]).all()
            one = e.exceedance(ra.ensemble.DeviceVector(e.series_devptr(1), n, np.float64, e), thr, weighted=weights is not None, grouped=True)
            assert (one["hits"] == got["hits"][0]).all() and (one["total"] == got["total"][0]).all()
        assert _check(e, X, thr, what="groups set, not asked for")["total"].shape == (3,)


def test_anomaly(ra):
    """The baseline is each member's mean over rows 0 .. 2 (set_baseline); then one with a NaN for one member, who takes no part."""
    n = 513
    rng = np.random.default_rng(10)
    X = np.round(np.cumsum(0.1 + 0.05 * rng.standard_normal((6, n)), axis=0) + 13.0, 2)
    thr = [0.0, 0.1, 0.25]
    record = np.array([-0.1, 0.0, np.nan, 0.2, 0.3, 0.35])
    with _rows_ens(ra, n, X) as e:
        assert refusal_code(e.exceedance_rows, 1, thr, 0, 3, anomaly=True) == 2
        e.set_baseline(1, 0, 3)
        b = e.baseline()
        got = _check(e, X, thr, baseline=b, what="anomaly")
        assert (got["total"] == n).all() and got["hits"][5, 2] > got["hits"][0, 2]
        _check(e, X, thr, baseline=b, rows=(1, 6, 2), what="anomaly, strided")
        _check_rank(e, X, record, baseline=b, what="anomaly rank")
        b = b.copy()
        b[40] = np.nan
        e.set_baseline_values(b)
        got = _check(e, X, thr, baseline=b, what="NaN baseline")
        assert (got["total"] == n - 1).all()
        _check_rank(e, X, record, baseline=b, what="NaN baseline, rank")
        e.clear_baseline()
        assert refusal_code(e.rank_rows, 1, record, 0, 6, anomaly=True) == 2


# ---- storage layouts --------------------------------------------------------------------------------------------------------------

def test_windowed_handle(ra):
    """A window of 8 rows and every 5th row in the output store: the resident rows give a fully stored twin's integers; a row that
    has slid out and is not kept is RSCM_ERR_STATE."""
    n = 321
    t = np.arange(1750, 1791, dtype=np.float64)
    with _rows_ens(ra, n, t=t) as full, _rows_ens(ra, n, steps=0, t=t, window_rows=8, output_stride=5) as w:
        while w.time_index < len(t) - 1:
            w.run(min(w.time_index + 4, len(t) - 1))
        S = full.get_series(1)
        thr = [float(np.median(S[20])), float(np.median(S[40])), 0.0]
        table = np.median(S, axis=1)[:, None] * [1.0, 0.9]
        record = S[:, 7].copy()                                                        # member 7's own series as the record
        want = full.exceedance_rows(1, thr)
        assert he.same(want, he.exceedance_rows(S, thr)) and 0 < want["hits"][40, 1] < n
        kept = w.exceedance_rows(1, thr, 0, 41, 5)                                     # the output store
        assert he.same(kept, {k: v[0:41:5] for k, v in want.items()})
        last = w.exceedance_rows(1, table[36:41], 36, 41)                              # the window's last rows, per-row thresholds
        assert he.same(last, he.exceedance_rows(S[36:41], table[36:41]))
        r = w.rank_rows(1, record[0:41:5], 0, 41, 5)
        assert he.same(r, full.rank_rows(1, record[0:41:5], 0, 41, 5)) and (r["equal"] >= 1).all()
        assert refusal_code(w.exceedance_rows, 1, thr, 0, 3) == 2                      # row 1 is neither in the window nor kept
        assert refusal_code(w.rank_rows, 1, record[31:34], 31, 34) == 2


def test_rows_past_the_time_index(ra):
    n = 100
    with _rows_ens(ra, n, steps=3) as e:
        S = e.get_series(1, 0, 4)
        thr = [float(np.median(S[3])), 0.0]
        got = e.exceedance_rows(1, thr)
        assert got["total"].tolist() == [n] * 4 + [0] * 4 and not got["hits"][4:].any() and np.isnan(got["probability"][4:]).all()
        assert he.same({k: v[:4] for k, v in got.items()}, he.exceedance_rows(S, thr))
        table = np.tile(thr, (8, 1))
        assert he.same(e.exceedance_rows(1, table), got)
        r = e.rank_rows(1, np.full(8, thr[0]))
        assert r["total"].tolist() == [n] * 4 + [0] * 4 and not r["below"][4:].any() and np.isnan(r["pit"][4:]).all()
        assert he.same({k: v[:4] for k, v in r.items()}, he.rank_rows(S, np.full(4, thr[0])))
        past = e.exceedance_rows(1, thr, 4, 8)
        assert not past["total"].any() and not past["hits"].any()
        assert e.exceedance_rows(1, thr, 5, 5)["hits"].shape == (0, 2)


def test_a_diagnostic_by_name(ra):
    """The heat content works once computed -- the restatement over its rows -- and is refused while it is stale."""
    n = 129
    with _rows_ens(ra, n) as e:
        vid = e.define_heat_content()
        assert refusal_code(e.exceedance_rows, "Ocean Heat Content", [0.0]) == 2
        e.compute_diagnostic(vid)
        S = e.get_series(vid)
        thr = [float(np.median(S[5])), 0.0]
        got = e.exceedance_rows("Ocean Heat Content", thr)
        assert he.same(got, he.exceedance_rows(S, thr)) and (got["total"] == n).all() and 0 < got["hits"][5, 0] < n
        assert he.same(e.rank_rows(vid, S[:, 3].copy()), he.rank_rows(S, S[:, 3]))
        e.set_state(1, 0, 0.25)
        assert refusal_code(e.exceedance_rows, "Ocean Heat Content", thr) == 2
        from rscm_amd._lib import RscmGpuError
        with pytest.raises(RscmGpuError, match="is stale: compute it again"):
            e.rank_rows(vid, S[:, 3].copy())


# ---- the rank of a record ---------------------------------------------------------------------------------------------------------

def test_rank_rows_against_the_restatement(ra):
    """A record with NaN gaps, a value below every member and one above every member; the rank histogram of the device's integers."""
    n = 1000
    rng = np.random.default_rng(3)
    X = _tied(rng, 8, n)
    X[5, 17] = np.nan
    w = _weights(rng, n)
    record = np.array([0.1, np.nan, -9.0, 9.0, -0.3, 0.0, np.nan, 1.1])
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        for weights in (None, w):
            r = _check_rank(e, X, record, weights, what="rank")
            W = n if weights is None else int(w.sum())
            assert r["below"][2] == 0 and r["equal"][2] == 0 and r["pit"][2] == 0.0
            assert r["below"][3] == W and r["pit"][3] == 1.0 and np.isnan(r["pit"][[1, 6]]).all()
            hist = ra.ensemble.rank_histogram(r["below"], r["equal"], r["total"], 5, record)
            assert (hist == he.rank_histogram(r["below"], r["equal"], r["total"], 5, record)).all() and hist.sum() == 6
            assert hist[0] >= 1 and hist[4] >= 1
        _check_rank(e, X, record[1:8:3], w, rows=(1, 8, 3), what="rank, strided")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_rank_rows_brackets_the_quantiles(ra, n):
    """With record[t] = the q-quantile of row t it must hold that below / total < q <= (below + equal) / total, in Fractions,
    weighted and unweighted, at q = 0.05, 0.17, 0.5, 0.83, 0.95.  Rows of np.round(rng.standard_normal(n), 1), full of ties, from
    default_rng(n); weights rng.integers(0, 1 << 20, n) with one entry 1 << 40.  The quantile is the one for which the bracket is
    the definition, numpy's "inverted_cdf", which satisfies it on all 60 of these cases on the CPU: weighted it is
    ``quantile_rows(weighted=True)`` under those weights, unweighted the same call under unit weights.  (The library's unweighted
    ``quantile_rows`` is numpy's "linear", which interpolates between members; numpy's own misses the bracket in 10 of the 30
    unweighted cases, e.g. n = 64 at every q.)"""
    rng = np.random.default_rng(n)
    x = np.round(rng.standard_normal(n), 1)
    w = rng.integers(0, 1 << 20, n)
    w[n // 2] = 1 << 40
    X = x[None, :]
    with _rows_ens(ra, n, X) as e:
        for weights in (np.ones(n, dtype=np.int64), w):
            e.set_member_weights(weights)
            weighted = weights is w
            for q in (0.05, 0.17, 0.5, 0.83, 0.95):
                record = np.ascontiguousarray(e.quantile_rows(1, [q], 0, 1, weighted=True)["quantiles"][:, 0])
                assert np.isin(record, x).all()
                r = e.rank_rows(1, record, 0, 1, weighted=weighted)
                assert he.same(r, he.rank_rows(X, record, w if weighted else None))
                for t in range(1):
                    below, equal, total = int(r["below"][t]), int(r["equal"][t]), int(r["total"][t])
                    print(f"n={n} weighted={weighted} q={q} row={t}: below={below} equal={equal} total={total}")
                    assert total == (int(w.sum()) if weighted else n) and equal >= 1
                    assert Fraction(below, total) < Fraction(q) <= Fraction(below + equal, total), (n, weighted, q, t)


# ---- graphs, shards, refusals -----------------------------------------------------------------------------------------------------

def test_graph_model(ra):
    """By variable name on a small linked graph: the home ensemble's rows."""
    mod = magicc_chain()
    n = 257
    model = mod.build_chain(n, 12, "topological")
    try:
        model.run()
        name = "Surface Temperature"
        S = model.get_series(name)
        last = S.shape[0] - 1
        thr = [float(np.median(S[last // 2])), float(np.median(S[last]))]
        got = model.exceedance_rows(name, thr)
        assert he.same(got, he.exceedance_rows(S, thr)) and 0 < got["hits"][last, 1] < n
        assert he.same(model.exceedance_rows(name, thr, 2, 10, 3), {k: v[2:10:3] for k, v in got.items()})
        record = np.median(S, axis=1)
        record[4] = np.nan
        r = model.rank_rows(name, record)
        assert he.same(r, he.rank_rows(S, record)) and np.isnan(r["pit"][4])
        assert he.same(model.rank_rows(name, record[2:10:3], 2, 10, 3), he.rank_rows(S[2:10:3], record[2:10:3]))
    finally:
        model.close()


def test_two_handles_add_up(ra):
    """The integers of two handles over the two parts of a member set add up to those of one handle over the whole set."""
    n, h = 901, 333
    rng = np.random.default_rng(12)
    X = _tied(rng, 3, n)
    w = _weights(rng, n)
    groups = (np.arange(n) % 3).astype(np.int32)
    thr = [0.0, 0.7]
    record = np.array([0.2, np.nan, -0.4])
    with _rows_ens(ra, n, X) as e, _rows_ens(ra, h, X[:, :h]) as e1, _rows_ens(ra, n - h, X[:, h:]) as e2:
        for x, s in ((e, slice(None)), (e1, slice(0, h)), (e2, slice(h, None))):
            x.set_member_weights(w[s])
            x.set_member_groups(groups[s], 3)
        a, b, c = (x.exceedance_rows(1, thr, 0, 3, weighted=True, grouped=True) for x in (e, e1, e2))
        assert (b["hits"] + c["hits"] == a["hits"]).all() and (b["total"] + c["total"] == a["total"]).all()
        assert he.same(ra.ensemble.exceedance_rows_result(b["hits"] + c["hits"], b["total"] + c["total"]), a)
        a, b, c = (x.rank_rows(1, record, 0, 3, weighted=True) for x in (e, e1, e2))
        total = b["total"] + c["total"]
        got = ra.ensemble.rank_rows_result(total - (b["below"] + c["below"]), b["equal"] + c["equal"], total, record, grouped=False)
        assert he.same(got, a) and he.same(a, he.rank_rows(X, record, w))


def test_refusals(ra):
    from rscm_amd import _lib
    n = 70
    with _rows_ens(ra, n) as e:
        lib, h = e._lib, e._h
        thr = np.zeros(8 * 8)
        hits, equal, total = np.zeros(8 * 8, dtype=np.int64), np.zeros(8 * 8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        pt, ph, pe, po = thr.ctypes.data_as(f64), hits.ctypes.data_as(i64), equal.ctypes.data_as(i64), total.ctypes.data_as(i64)

        def call(var=1, tb=0, te=8, ts=1, n_thr=2, t=pt, per_row=0, flags=0, hi=ph, eq=pe, to=po):
            return lib.rscm_ens_exceedance_rows(h, var, tb, te, ts, n_thr, t, per_row, flags, hi, eq, to)

        assert call() == _lib.OK and (total == n).all()
        assert call(eq=None) == _lib.OK and call(n_thr=8, per_row=1) == _lib.OK and call(n_thr=1) == _lib.OK and call(tb=5, te=5) == _lib.OK
        for kw in (dict(n_thr=0), dict(n_thr=9), dict(n_thr=-1), dict(tb=-1), dict(te=9), dict(tb=5, te=4), dict(ts=0), dict(ts=-1),
                   dict(flags=8), dict(flags=_lib.SELECT_WEIGHTED | 16), dict(t=None), dict(hi=None), dict(to=None), dict(var=99)):
            assert call(**kw) == _lib.ERR_INVALID, kw
        for flags in (_lib.SELECT_WEIGHTED, _lib.SELECT_GROUPED, _lib.SELECT_ANOMALY):
            assert call(flags=flags) == _lib.ERR_STATE, flags
        assert refusal_code(e.exceedance_rows, 1, [0.0], weighted=True) == 2
        assert refusal_code(e.exceedance_rows, 1, [0.0], grouped=True) == 2
        assert refusal_code(e.rank_rows, 1, np.zeros(8), anomaly=True) == 2
        assert refusal_code(e.exceedance_rows, 1, [0.0], 0, 9) == 1 and refusal_code(e.exceedance_rows, 1, [0.0], 0, 8, 0) == 1
        with pytest.raises(ValueError):
            e.exceedance_rows(1, np.zeros(9))
        with pytest.raises(ValueError):
            e.exceedance_rows(1, np.zeros((7, 2)))
        with pytest.raises(ValueError):
            e.rank_rows(1, np.zeros(7))
        with e.select(1, [0.5], 0, 8):
            assert refusal_code(e.exceedance_rows, 1, [0.0]) == 2
        e.exceedance_rows(1, [0.0])
