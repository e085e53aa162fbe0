"""GPU tier: anomaly plumes, per-member indicators, quantiles of per-member vectors and exceedance (csrc/indicators.hip, the
anomaly flag of the select in select.hip; rscm_ens_set_baseline, rscm_ens_quantile_rows_ex,
rscm_ens_member_indicators, rscm_ens_quantile_vectors, rscm_ens_exceedance).  The oracle is the numpy restatement in
tests/host_indicators.py on rows copied to the host, compared bit for bit: zeros without their sign (the select's key order puts
-0.0 first, numpy keeps member order) and any NaN equal to any NaN."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import axis_values, f_syn, magicc_chain, same_values, two_layer_params
from tests.host_indicators import anomaly, baseline, exceedance_counts, indicators

pytestmark = pytest.mark.gpu

Q = [0.0, 0.05, 0.17, 0.5, 0.83, 0.95, 1.0]
THR = [0.5, 1.0, 1.5, 2.0, 3.0]


def _np_q(rows):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(np.asarray(rows), Q, axis=1).T


def _np_wq(rows, w):
    rows = np.asarray(rows)
    W = ((~np.isnan(rows)) * w[None, :]).sum(axis=1)
    out = np.full((rows.shape[0], len(Q)), np.nan)
    live = W > 0
    if live.any():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            sub = rows[live]
            out[live] = np.nanquantile(sub, Q, axis=1, weights=np.broadcast_to(w, sub.shape), method="inverted_cdf").T
    return out, W


def _two_layer(ra, n, P=None, steps=None, **kw):
    t = axis_values()
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0), **kw)
    e.set_params(two_layer_params(n) if P is None else P)
    e.set_forcing(f_syn(t))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run(steps)
    return e


def _adversarial(e, rng, rows=(120, 400, 700)):
    n = e.n_members
    for k, r in enumerate(rows):
        x = e.get_series(1, r, r + 1)[0]
        x[rng.random(n) < 0.05 * (k + 1)] = np.nan if k != 1 else -np.float64(np.nan)
        x[rng.random(n) < 0.01] = rng.choice([np.inf, -np.inf, 0.0, -0.0, 1.5])
        e.set_state(1, r, x)


def _weights(rng, n):
    w = rng.integers(1, 1 << 30, n, dtype=np.int64)
    w[rng.random(n) < 0.2] = 0
    w[:3] = 0
    return w


def _ind_host(d):
    return {"mean": d["mean"].to_host(), "peak": d["peak"].to_host(), "peak_time": d["peak_time"].to_host(),
            "crossing": [c.to_host() for c in d["crossing"]]}


def _ind_same(got, want):
    return all(same_values(got[k], want[k]) for k in ("mean", "peak", "peak_time")) and len(got["crossing"]) == len(want["crossing"]) and \
        all(same_values(a, b) for a, b in zip(got["crossing"], want["crossing"]))


@pytest.mark.parametrize("n", [30_001, 30_000])
def test_anomaly_plume_full_storage(ra, n):
    """Odd N (rows alternate between 16- and 8-byte alignment, the baseline is 16-byte aligned) and even N: the baseline equals
    the host's left-to-right mean bit for bit, and the anomaly plume, plain, strided and weighted, numpy on x - b."""
    rng = np.random.default_rng(n)
    P = two_layer_params(n)
    P[0, rng.random(n) < 0.002] = np.nan
    with _two_layer(ra, n, P) as e:
        _adversarial(e, rng, rows=(105, 400, 700))
        e.set_baseline(1, 100, 151)
        ser = e.get_series(1)
        b = baseline(ser[100:151])
        assert same_values(e.baseline(), b)
        assert np.isnan(b).any()                          # members with a NaN reference row
        a = anomaly(ser, b)
        got = e.quantile_rows(1, Q, anomaly=True)
        assert same_values(got["quantiles"], _np_q(a)) and np.array_equal(got["count"], (~np.isnan(a)).sum(axis=1))
        mid = e.quantile_rows(1, Q, 3, 700, 7, anomaly=True)
        assert same_values(mid["quantiles"], got["quantiles"][3:700:7])
        plain = e.quantile_rows(1, Q)                     # the plain select is untouched by the baseline
        assert same_values(plain["quantiles"], _np_q(ser))
        w = _weights(rng, n)
        e.set_member_weights(w)
        wq = e.quantile_rows(1, Q, weighted=True, anomaly=True)
        want, W = _np_wq(a, w)
        assert same_values(wq["quantiles"], want) and np.array_equal(wq["weight"], W)
        e.set_baseline_values(b[::-1].copy())             # host values, then a device vector, then kept across rewind / run
        assert same_values(e.baseline(), b[::-1])
        e.set_baseline_values(e.indicators(1, 100, 151)["mean"])
        assert same_values(e.baseline(), b)
        e.rewind()
        e.run()
        assert same_values(e.baseline(), b)
        e.clear_baseline()
        assert refusal_code(e.baseline) == 2


def test_two_handles_summing_anomaly_histograms(ra):
    """Two handles holding the halves of one ensemble, each with its members' baselines, sum their staged buffers: both end with
    the single handle's anomaly plume, plain and weighted."""
    n, k = 20_011, 7_003
    P = two_layer_params(n)
    rng = np.random.default_rng(5)
    w = _weights(rng, n)
    with _two_layer(ra, n, P, steps=80) as whole, _two_layer(ra, k, np.ascontiguousarray(P[:, :k]), steps=80) as a, \
            _two_layer(ra, n - k, np.ascontiguousarray(P[:, k:]), steps=80) as b:
        x = rng.choice([-np.inf, np.inf, 0.0, -0.0, np.nan, 1.0, 2.0], n)
        for h, sl in ((whole, slice(0, n)), (a, slice(0, k)), (b, slice(k, n))):
            h.set_state(1, 7, np.ascontiguousarray(x[sl]))
            h.set_member_weights(np.ascontiguousarray(w[sl]))
            h.set_baseline(1, 10, 31, 2)
        for weighted in (False, True):
            want = whole.quantile_rows(1, Q, 0, 81, weighted=weighted, anomaly=True)
            sels = [h.select(1, Q, 0, 81, weighted=weighted, anomaly=True) for h in (a, b)]
            try:
                passes = 0
                while True:
                    bufs = [s.next_pass() for s in sels]
                    if bufs[0] is None:
                        break
                    total = np.sum([buf.to_host() for buf in bufs], axis=0)
                    for s in sels:
                        s.commit(total)
                    passes += 1
                assert passes == 8
                for s in sels:
                    res = s.result()
                    assert np.array_equal(res["quantiles"].view(np.uint64), want["quantiles"].view(np.uint64))
            finally:
                for s in sels:
                    s.close()


def test_indicators_two_layer(ra):
    """Indicators over full storage, anomaly off and on, strided, with NaN members, +-inf, ties at the peak and thresholds never
    crossed: bit for bit the host restatement; two slots live side by side."""
    n = 40_001
    rng = np.random.default_rng(21)
    P = two_layer_params(n)
    P[0, rng.random(n) < 0.002] = np.nan
    with _two_layer(ra, n, P) as e:
        _adversarial(e, rng, rows=(260, 400, 520))
        x = e.get_series(1, 300, 301)[0]
        x[:50] = 1e3                                      # a tie at the peak with row 330
        e.set_state(1, 300, x)
        x = e.get_series(1, 330, 331)[0]
        x[:50] = 1e3
        e.set_state(1, 330, x)
        ser, times = e.get_series(1), e.bounds[:e.n_times]
        e.set_baseline(1, 100, 151)
        b = baseline(ser[100:151])
        for anom, slot, (t0, t1, s) in ((False, 0, (250, 751, 1)), (True, 1, (250, 751, 1)), (True, 2, (251, 700, 3))):
            d = e.indicators(1, t0, t1, s, THR, anomaly=anom, slot=slot)
            want = indicators(ser[t0:t1:s], times[t0:t1:s], THR, b if anom else None)
            assert _ind_same(_ind_host(d), want), (anom, slot)
        d0 = e.indicators(1, 250, 751, 1, (), slot=3)     # no thresholds; the mean over the reference rows is the baseline
        assert d0["crossing"] == []
        ref = e.indicators(1, 100, 151, slot=3)
        assert same_values(ref["mean"].to_host(), b)


def test_windowed_graph(ra):
    """The windowed MAGICC chain (a 16-row window, every 12th row kept): the anomaly plume of the annual rows, plain and weighted,
    the indicators with anomaly on and off, their quantiles and exceedance -- all equal to the host on rows fetched from the
    output store."""
    mod = magicc_chain()
    n = 3001
    model = mod.build_chain(n, 30, "topological", steps_per_year=12, series_window=16, output_stride=12)
    try:
        model.run()
        name = "Surface Temperature"
        ens, vid = model.variable_home(name)
        ser = model.get_series(name, t_stride=12)
        times = ens.bounds[:ens.n_times][::12]
        model.set_baseline(name, 0, 61, 12)
        b = baseline(ser[:6])
        assert same_values(model.baseline(name), b)
        a = anomaly(ser, b)
        got = model.quantile_rows(name, Q, t_stride=12, anomaly=True)
        assert same_values(got["quantiles"], _np_q(a))
        rng = np.random.default_rng(2)
        w = _weights(rng, n)
        model.set_member_weights(w)
        wq = model.quantile_rows(name, Q, t_stride=12, weighted=True, anomaly=True)
        want, W = _np_wq(a, w)
        assert same_values(wq["quantiles"], want) and np.array_equal(wq["weight"], W)
        for anom in (False, True):
            d = model.indicators(name, 120, ens.n_times, 12, [0.2, 0.5, 10.0], anomaly=anom, slot=int(anom))
            want = indicators(ser[10:], times[10:], [0.2, 0.5, 10.0], b if anom else None)
            assert _ind_same(_ind_host(d), want), anom
            vecs = [d["mean"], d["peak"], d["peak_time"]] + d["crossing"]
            host = np.stack([v.to_host() for v in vecs])
            q = model.quantile_vectors(vecs, Q)
            assert same_values(q["quantiles"], _np_q(host))
            wq = model.quantile_vectors(vecs, Q, weighted=True)
            assert same_values(wq["quantiles"], _np_wq(host, w)[0])
            ex = model.exceedance(d["peak"], [0.2, 0.5, 10.0], weighted=True)
            hits, total = exceedance_counts(host[1], [0.2, 0.5, 10.0], w)
            assert ex["hits"].tolist() == hits and ex["total"] == total
    finally:
        model.close()


def test_quantile_vectors_and_exceedance(ra):
    """quantile_vectors of indicator rows (crossing times with +inf and NaN) and of a parameter row, plain and weighted, equals
    numpy; exceedance gives the exact integer counts and weight sums, and probabilities hits / total."""
    n = 50_001
    rng = np.random.default_rng(4)
    P = two_layer_params(n)
    P[0, rng.random(n) < 0.003] = np.nan
    with _two_layer(ra, n, P) as e:
        e.set_baseline(1, 100, 151)
        d = e.indicators(1, 300, 751, 1, THR, anomaly=True)
        vecs = [d["mean"], d["peak"], d["peak_time"]] + d["crossing"] + [e.params_vector(1)]
        host = np.stack([v.to_host() for v in vecs])
        assert np.isinf(host[3:3 + len(THR)]).any() and np.isnan(host).any()
        got = e.quantile_vectors(vecs, Q)
        assert same_values(got["quantiles"], _np_q(host)) and np.array_equal(got["count"], (~np.isnan(host)).sum(axis=1))
        w = _weights(rng, n)
        e.set_member_weights(w)
        wq = e.quantile_vectors(vecs, Q, weighted=True)
        want, W = _np_wq(host, w)
        assert same_values(wq["quantiles"], want) and np.array_equal(wq["weight"], W)
        with e.select_vectors(vecs, Q) as s:              # the staged form, on one handle
            while s.next_pass() is not None:
                s.commit()
            assert same_values(s.result()["quantiles"], got["quantiles"])
        for weighted in (False, True):
            ex = e.exceedance(d["peak"], THR, weighted=weighted)
            hits, total = exceedance_counts(host[1], THR, w if weighted else None)
            assert ex["hits"].tolist() == hits and ex["total"] == total
            assert np.array_equal(ex["probability"], np.array(hits, dtype=np.float64) / total)
        big = np.zeros(n, dtype=np.int64)
        big[:2] = 1 << 52                                  # W = 2^53: exact
        e.set_member_weights(big)
        ex = e.exceedance(e.params_vector(1), [-np.inf], weighted=True)
        assert ex["total"] == 1 << 53 and ex["hits"].tolist() == [1 << 53]
        none = e.exceedance(d["peak"], [], weighted=False)
        assert none["hits"].size == 0 and none["total"] == int((~np.isnan(host[1])).sum())


def test_errors(ra):
    """No baseline: RSCM_ERR_STATE; baseline rows not resident or not computed: RSCM_ERR_STATE; anomaly on vectors, a bad slot,
    too many thresholds, a host address as a vector: RSCM_ERR_INVALID; changing the baseline or an indicator slot while a staged
    select is in flight: RSCM_ERR_STATE."""
    from rscm_amd import _lib
    n = 1001
    with _two_layer(ra, n, steps=40) as e:
        assert refusal_code(e.quantile_rows, 1, Q, anomaly=True) == 2
        assert refusal_code(e.select, 1, Q, anomaly=True) == 2
        assert refusal_code(e.indicators, 1, 0, 30, anomaly=True) == 2
        assert refusal_code(e.baseline) == 2
        assert refusal_code(e.set_baseline, 1, 30, 60) == 2              # rows beyond the time index
        assert refusal_code(e.set_baseline, 1, 5, 5) == 1                # no row
        e.set_baseline(1, 0, 11)
        d = e.indicators(1, 0, 30)
        assert refusal_code(e.indicators, 1, 0, 30, slot=4) == 1
        assert refusal_code(e.indicators, 1, 0, 30, slot=-1) == 1
        assert refusal_code(e.indicators, 1, 0, 30, thresholds=list(range(9))) == 1
        lib = _lib.load()
        arr = (C.POINTER(C.c_double) * 1)(C.cast(C.c_void_p(d["peak"].ptr), C.POINTER(C.c_double)))
        q = np.array(Q)
        out, cnt = np.empty((1, len(Q))), np.empty(1)
        assert lib.rscm_ens_quantile_vectors(e._h, 1, arr, len(Q), _lib.dptr(q), _lib.SELECT_ANOMALY, _lib.dptr(out), _lib.dptr(cnt)) == 1
        assert lib.rscm_ens_select_begin_vectors(e._h, 1, arr, len(Q), _lib.dptr(q), _lib.SELECT_ANOMALY) == 1
        host = np.zeros(n)
        harr = (C.POINTER(C.c_double) * 1)(_lib.dptr(host))
        assert lib.rscm_ens_quantile_vectors(e._h, 1, harr, len(Q), _lib.dptr(q), 0, _lib.dptr(out), _lib.dptr(cnt)) == 1
        assert refusal_code(e.exceedance, d["peak"], [1.0], weighted=True) == 2   # no weights
        b = e.baseline()
        with e.select(1, Q, 0, 30, anomaly=True) as s:
            assert refusal_code(e.set_baseline, 1, 0, 5) == 2
            assert refusal_code(e.set_baseline_values, np.zeros(n)) == 2
            assert refusal_code(e.clear_baseline) == 2
            assert refusal_code(e.indicators, 1, 0, 30) == 2
            while s.next_pass() is not None:
                s.commit()
            res = s.result()
        assert same_values(e.baseline(), b)
        assert same_values(res["quantiles"], _np_q(anomaly(e.get_series(1, 0, 30), b)))
    t = np.arange(1750, 1901, dtype=np.float64)
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0), window_rows=8, output_stride=5) as w:
        w.set_params(two_layer_params(n))
        w.set_forcing(f_syn(t))
        w.set_initial(1, 0.0)
        w.set_initial(2, 0.0)
        while w.time_index < len(t) - 1:
            w.run(min(w.time_index + 4, len(t) - 1))
        assert refusal_code(w.set_baseline, 1, 0, 3) == 2                # row 1 is neither in the window nor in the output store
        assert refusal_code(w.indicators, 1, 0, 3) == 2
        w.set_baseline(1, 0, 51, 5)                              # output-store rows are resident
        assert same_values(w.baseline(), baseline(w.get_series(1, 0, 51, 5)))
