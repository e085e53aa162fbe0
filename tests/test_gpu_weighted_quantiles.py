"""GPU tier: likelihood-weighted ensemble quantiles (the weighted select of csrc/select.hip, rscm_ens_weighted_quantile_rows, the
weighted staged select, the member weights and their quantisation from a log-likelihood, csrc/weights.hip).  The oracle is
numpy.nanquantile(row, q, weights=w, method="inverted_cdf"), compared bit for bit with zeros taken without their sign (the key
order puts -0.0 first, numpy keeps member order)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import axis_values, f_syn, magicc_chain, two_layer_params

pytestmark = pytest.mark.gpu

Q = [0.0, 0.05, 0.17, 0.5, 0.83, 0.95, 1.0]


def _unsign(x):
    return np.where(np.asarray(x) == 0, 0.0, x)


def _same_nan_bits(a, b):
    """Bit equality with zeros compared without sign (NaN == NaN when their bits agree)."""
    return np.array_equal(_unsign(a).view(np.uint64), _unsign(b).view(np.uint64))


def _np_weighted(rows, w, q=Q):
    """[rows][len(q)] numpy weighted quantiles (rows with W == 0 left NaN), and [rows] W."""
    rows = np.asarray(rows)
    ok = ~np.isnan(rows)
    W = (ok * w[None, :]).sum(axis=1)
    out = np.full((rows.shape[0], len(q)), np.nan)
    live = W > 0
    if live.any():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            sub = rows[live]
            out[live] = np.nanquantile(sub, q, axis=1, weights=np.broadcast_to(w, sub.shape), method="inverted_cdf").T
    return out, W


def _two_layer(ra, n, P=None, t=None, steps=None):
    t = axis_values() if t is None else t
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0))
    e.set_params(two_layer_params(n) if P is None else P)
    e.set_forcing(f_syn(t))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run(steps)
    return e


def _weights(rng, n):
    w = rng.integers(1, 1 << 30, n, dtype=np.int64)
    w[rng.random(n) < 0.2] = 0
    w[:3] = 0                                    # leading zero weights (the unpaired head member among them)
    return w


def _legacy_entry_points_match_ex(e, rows):
    """The four entry points older than the flags (rscm_ens_quantile_rows, rscm_ens_weighted_quantile_rows,
    rscm_ens_select_begin, rscm_ens_select_begin_weighted) give the bits of their _ex form with the matching flags."""
    from rscm_amd import _lib as L
    lib, q = L.load(), np.asarray(Q, dtype=np.float64)

    def staged(begin, *flags):
        L.check(begin(e._h, 1, 0, rows, 1, q.size, L.dptr(q), *flags))
        try:
            done, p, n = C.c_int32(0), C.POINTER(C.c_int64)(), C.c_int64(0)
            while True:
                L.check(lib.rscm_ens_select_pass(e._h, C.byref(done), C.byref(p), C.byref(n)))
                if done.value:
                    break
                L.check(lib.rscm_ens_select_commit(e._h))
            out, cnt = np.empty((rows, q.size)), np.empty(rows)
            L.check(lib.rscm_ens_select_result(e._h, L.dptr(out), L.dptr(cnt)))
        finally:
            L.check(lib.rscm_ens_select_end(e._h))
        return out, cnt

    def direct(fn, *flags):
        out, cnt = np.empty((rows, q.size)), np.empty(rows)
        L.check(fn(e._h, 1, 0, rows, 1, q.size, L.dptr(q), *flags, L.dptr(out), L.dptr(cnt)))
        return out, cnt

    for flags, legacy_rows, legacy_begin in ((0, lib.rscm_ens_quantile_rows, lib.rscm_ens_select_begin),
                                             (L.SELECT_WEIGHTED, lib.rscm_ens_weighted_quantile_rows, lib.rscm_ens_select_begin_weighted)):
        want = direct(lib.rscm_ens_quantile_rows_ex, flags)
        for got in (direct(legacy_rows), staged(legacy_begin), staged(lib.rscm_ens_select_begin_ex, flags)):
            assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, want))


def test_weighted_rows_equal_numpy_bit_for_bit(ra):
    """1e5 members x 751 rows, random int64 weights with zeros, NaN members in some rows and failed members: every row at
    seven quantiles equals numpy's weighted nanquantile, and ``weight`` is numpy's per-row sum over non-NaN members."""
    n = 100_001
    rng = np.random.default_rng(17)
    P = two_layer_params(n)
    P[0, rng.random(n) < 0.001] = np.nan          # members whose run goes NaN from the start
    with _two_layer(ra, n, P) as e:
        assert e.n_times == 751
        for k, r in enumerate((5, 300, 750)):      # rows with NaN members of both signs, +-inf, ties and zeros
            x = e.get_series(1, r, r + 1)[0]
            x[rng.random(n) < 0.1 * (k + 1)] = np.nan if k != 1 else -np.float64(np.nan)
            x[rng.random(n) < 0.01] = rng.choice([np.inf, -np.inf, 0.0, -0.0, 1.5])
            e.set_state(1, r, x)
        w = _weights(rng, n)
        e.set_member_weights(w)
        assert np.array_equal(e.member_weights(), w)
        got = e.quantile_rows(1, Q, weighted=True)
        want, W = _np_weighted(e.get_series(1), w)
        assert np.array_equal(got["weight"], W)
        assert _same_nan_bits(got["quantiles"], want)
        mid = e.quantile_rows("Surface Temperature", Q, 3, 700, 7, weighted=True)    # strided
        assert _same_nan_bits(mid["quantiles"], got["quantiles"][3:700:7]) and np.array_equal(mid["weight"], W[3:700:7])
        _legacy_entry_points_match_ex(e, 40)
        e.rewind()
        e.run(40)                                                                  # weights survive rewind and run
        part = e.quantile_rows(1, Q, 0, 60, weighted=True)
        assert np.array_equal(e.member_weights(), w)
        assert (part["weight"][41:] == 0).all() and np.isnan(part["quantiles"][41:]).all()
        want, W = _np_weighted(e.get_series(1, 0, 41), w)
        assert _same_nan_bits(part["quantiles"][:41], want) and np.array_equal(part["weight"][:41], W)


def test_unit_and_constant_weights(ra):
    """Weights all 1 give np.nanquantile(method="inverted_cdf"); a constant weight k gives the same numbers."""
    n = 30_011
    with _two_layer(ra, n, steps=120) as e:
        x = e.get_series(1, 50, 51)[0]
        x[::9] = np.nan
        e.set_state(1, 50, x)
        ser = e.get_series(1, 0, 121)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            want = np.nanquantile(ser, Q, axis=1, method="inverted_cdf").T
        for k in (1, 3, 1 << 35):
            e.set_member_weights(np.full(n, k, dtype=np.int64))
            got = e.quantile_rows(1, Q, 0, 121, weighted=True)
            assert _same_nan_bits(got["quantiles"], want), k
            assert np.array_equal(got["weight"], k * (~np.isnan(ser)).sum(axis=1))


def test_two_handles_summing_their_weight_histograms(ra):
    """Two handles holding the two halves of one ensemble (and of its weights) sum their pass buffers on the host: both end
    with the single handle's bits."""
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
        want = whole.quantile_rows(1, Q, 0, 81, weighted=True)
        sels = [h.select(1, Q, 0, 81, weighted=True) for h in (a, b)]
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
                assert np.array_equal(res["weight"], want["weight"])
        finally:
            for s in sels:
                s.close()


def test_weights_from_loglik(ra):
    """set_weights_from_loglik: within 1 of rint(exp(ll - max) * 2^bits) for ok members, 0 for failed members and -inf, the
    clamp when ll_max is below some ll, and the max that loglik_max reports."""
    n = 50_003
    rng = np.random.default_rng(9)
    P = two_layer_params(n)
    bad = rng.random(n) < 0.01
    P[0, bad] = np.nan
    with _two_layer(ra, n, P, steps=30) as e:
        status = e.status()
        assert (status[bad] != 0).all()
        ll = -np.abs(rng.standard_normal(n)) * 20.0
        ll[rng.random(n) < 0.01] = -np.inf
        ll[np.flatnonzero(status != 0)[0]] = 5.0  # a failed member's ll never sets the max
        ok = (status == 0) & np.isfinite(ll)
        want_max = float(ll[ok].max())
        assert e.loglik_max(ll) == want_max
        got_max, bits = e.set_weights_from_loglik(ll)
        assert got_max == want_max and bits == 53 - int(np.ceil(np.log2(n)))
        w = e.member_weights()
        ref = np.rint(np.exp(np.where(ok, ll - want_max, 0.0)) * 2.0 ** bits)
        assert (w[~ok] == 0).all()
        assert np.abs(w[ok] - ref[ok]).max() <= 1 and w[ok].max() == 2 ** bits
        low = want_max - 3.0                        # ll_max below some ll: those members clamp to 2^bits
        e.set_weights_from_loglik(ll, bits=20, ll_max=low)
        w2 = e.member_weights()
        assert (w2[ok & (ll >= low)] == 2 ** 20).all() and (w2[~ok] == 0).all()
        # a device log-likelihood, as rscm_ens_loglik_device leaves it
        dv = e.loglik(["Surface Temperature"] * 2, [10, 20], [0.1, 0.2], [0.1, 0.1], on_device=True)
        host = dv.to_host()
        okd = (status == 0) & np.isfinite(host)
        assert e.loglik_max(dv) == float(host[okd].max())
        e.set_weights_from_loglik(dv, bits=30)
        ref = np.rint(np.exp(np.where(okd, host - host[okd].max(), 0.0)) * 2.0 ** 30)
        wd = e.member_weights()
        assert (wd[~okd] == 0).all() and np.abs(wd[okd] - ref[okd]).max() <= 1
        assert 1.0 <= e.weights_ess() <= n


def test_errors(ra):
    """No weights set: RSCM_ERR_STATE; a negative weight (host or device), W > 2^53, bits outside [0, 52]: RSCM_ERR_INVALID; a
    wrong length: ValueError before the library is called."""
    n = 1001
    with _two_layer(ra, n, steps=5) as e:
        assert refusal_code(e.quantile_rows, 1, Q, weighted=True) == 2
        assert refusal_code(e.select, 1, Q, weighted=True) == 2
        assert refusal_code(e.member_weights) == 2
        w = np.ones(n, dtype=np.int64)
        e.set_member_weights(w)
        bad = w.copy()
        bad[500] = -1
        assert refusal_code(e.set_member_weights, bad) == 1
        assert np.array_equal(e.member_weights(), w)           # the weights set before stay
        with _two_layer(ra, n, steps=1) as other:                # device input: another handle's weight buffer, written raw
            import ctypes as C
            from rscm_amd import _lib
            other.set_member_weights(w)
            dv = other.member_weights_device()
            _lib.check(_lib.load().rscm_gpu_copy_to_device(other.device, C.c_void_p(dv.ptr), bad.ctypes.data_as(C.c_void_p), bad.nbytes))
            assert refusal_code(e.set_member_weights, dv) == 1
            other.set_member_weights(2 * w)
            e.set_member_weights(other.member_weights_device())
            assert np.array_equal(e.member_weights(), 2 * w)
        with pytest.raises(ValueError):
            e.set_member_weights(w[:-1])
        big = np.zeros(n, dtype=np.int64)
        big[:2] = (1 << 52) + 1                                  # the handle's weights sum to 2^53 + 2: refused when set
        assert refusal_code(e.set_member_weights, big) == 1
        wrap = np.zeros(n, dtype=np.int64)                       # sums that wrap 64 bits: refused, not a small wrong W
        wrap[:3] = [2**63 - 1, 2**63 - 1, 3]
        assert refusal_code(e.set_member_weights, wrap) == 1
        assert refusal_code(e.set_member_weights, np.full(n, 1 << 53, dtype=np.int64)) == 1
        assert np.array_equal(e.member_weights(), 2 * w)         # the weights set before stay
        big[1] = (1 << 52) - 1                                   # W = 2^53: accepted
        e.set_member_weights(big)
        assert (e.quantile_rows(1, [0.5], 0, 6, weighted=True)["weight"] == 1 << 53).all()
        assert refusal_code(e.set_weights_from_loglik, np.zeros(n), bits=52) == 1  # quantising 1001 weights of 2^52 can pass 2^53: refused
        assert (e.member_weights() == big).all()
        for b in (-1, 53):
            assert refusal_code(e.set_weights_from_loglik, np.zeros(n), bits=b) == 1
        e.set_member_weights(np.zeros(n, dtype=np.int64))        # W == 0: weight 0, NaN
        res = e.quantile_rows(1, Q, 0, 6, weighted=True)
        assert (res["weight"] == 0).all() and np.isnan(res["quantiles"]).all()


def test_handles_summing_past_2_53(ra):
    """Two handles whose weights each sum to less than 2^53 but together to more: the first commit of the staged select returns
    RSCM_ERR_INVALID on both."""
    with _two_layer(ra, 101, steps=5) as a, _two_layer(ra, 101, steps=5) as b:
        for h in (a, b):
            w = np.zeros(101, dtype=np.int64)
            w[50] = (1 << 52) + 1
            h.set_member_weights(w)
        sels = [h.select(1, Q, 0, 6, weighted=True) for h in (a, b)]
        try:
            total = np.sum([s.next_pass().to_host() for s in sels], axis=0)
            for s in sels:
                assert refusal_code(s.commit, total) == 1
        finally:
            for s in sels:
                s.close()


def test_windowed_graph_weighted_quantile_rows(ra):
    """The windowed MAGICC chain (a 16-row window, every 12th row kept): weighted GraphModel.quantile_rows over the annual rows
    equals numpy on the rows fetched to the host, with weights set directly and from a log-likelihood."""
    mod = magicc_chain()
    names = ["Surface Temperature", "Atmospheric Concentration|CO2", "Effective Radiative Forcing"]
    n = 3001
    model = mod.build_chain(n, 30, "topological", steps_per_year=12, series_window=16, output_stride=12)
    try:
        model.run()
        rng = np.random.default_rng(2)
        w = _weights(rng, n)
        model.set_member_weights(w)
        for name in names:
            got = model.quantile_rows(name, Q, t_stride=12, weighted=True)
            want, W = _np_weighted(model.get_series(name, t_stride=12), w)
            assert _same_nan_bits(got["quantiles"], want), name
            assert np.array_equal(got["weight"], W), name
        ll = -0.5 * rng.standard_normal(n) ** 2
        ll_max, bits = model.set_weights_from_loglik(ll)
        alive = np.logical_and.reduce([x.status() == 0 for x in model.ensembles.values()])
        assert ll_max == float(ll[alive].max()) and bits == 53 - int(np.ceil(np.log2(n)))
        ws = [e.member_weights() for e in model.ensembles.values()]
        assert all(np.array_equal(x, ws[0]) for x in ws)
        got = model.quantile_rows("Surface Temperature", Q, t_stride=12, weighted=True)
        want, W = _np_weighted(model.get_series("Surface Temperature", t_stride=12), ws[0])
        assert _same_nan_bits(got["quantiles"], want) and np.array_equal(got["weight"], W)
    finally:
        model.close()
