"""GPU tier: rscm_ens_quantile_rows and the staged select (csrc/select.hip) -- exact ensemble quantiles over any storage layout
and over shards of one member set.  The oracle is numpy.nanquantile; rscm_ens_quantile_series runs the same select on full
storage and must carry the same bits, signed zeros included, for any number of quantiles."""
import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.helpers import axis_values, f_syn, magicc_chain, same_values, two_layer_params

pytestmark = pytest.mark.gpu

Q = [0.0, 1.0, 0.5, 1e-12, 0.05, 0.17, 0.83, 0.95]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _nanq(rows, q):
    with np.errstate(all="ignore"), _quiet():
        return np.nanquantile(rows, q, axis=1).T


class _quiet:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *a):
        return self._w.__exit__(*a)


def _adversarial(rng, n):
    neg_nan = -np.float64(np.nan)
    return [
        np.where(rng.random(n) < 0.3, np.nan, np.where(rng.random(n) < 0.5, neg_nan, rng.standard_normal(n))),
        rng.choice([-np.inf, np.inf, -0.0, 0.0, 5e-324, -5e-324, 1e-310, np.nan, neg_nan, 1.0], n),
        rng.choice([-1.0, 0.0, 2.5, 2.5, 7.0], n),                      # ties
        np.full(n, np.nan),                                             # every member NaN
        np.where(np.arange(n) == n - 1, -3.0, neg_nan),                 # n = 1, the last member (the unpaired tail)
        np.where(np.arange(n) == 0, 2.0, np.nan),                       # n = 1, the first member
        rng.choice([-0.0, 0.0], n),
        1.2 + 1e-9 * rng.standard_normal(n),                            # clustered: the top digits of every key agree
        rng.standard_normal(n) * 1e300,
    ]


def _two_layer(ra, n, P=None, t=None, steps=None):
    t = axis_values(1750, 1830) if t is None else t
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0))
    e.set_params(two_layer_params(n) if P is None else P)
    e.set_forcing(f_syn(t))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run(steps)
    return e


@pytest.mark.parametrize("n", [70_001, 4099, 3, 1])
def test_quantile_rows_equals_quantile_series_and_numpy(ra, n):
    """Full storage: quantile_series' bits (signed zeros included) and numpy's numbers, on adversarial rows written with set_state;
    N odd (every other row starts 8-byte aligned), not a multiple of 64 or of the block; rows past the time index empty."""
    rng = np.random.default_rng(n)
    with _two_layer(ra, n, steps=60) as e:
        for k, row in enumerate(_adversarial(rng, n)):
            e.set_state(1, 2 + k, row)
        got = e.quantile_rows(1, Q)
        ref = e.quantile_series(1, Q)
        assert _bits_equal(got["quantiles"], ref["quantiles"]) and np.array_equal(got["count"], ref["count"])
        ts = e.get_series(1)
        assert same_values(got["quantiles"][:61], _nanq(ts[:61], Q))
        assert np.array_equal(got["count"][:61], (~np.isnan(ts[:61])).sum(axis=1))
        assert (got["count"][61:] == 0).all() and np.isnan(got["quantiles"][61:]).all()
        sub = e.quantile_rows("Surface Temperature", Q, 1, 75, 3)          # stride > 1, across the time index
        assert _bits_equal(sub["quantiles"], got["quantiles"][1:75:3]) and np.array_equal(sub["count"], ref["count"][1:75:3])
        one = e.quantile_rows(2, 0.5, 10, 11)
        assert _bits_equal(one["quantiles"][:, 0], np.nanmedian(e.get_series(2)[10:11], axis=1))
        assert e.quantile_rows(1, Q, 5, 5)["quantiles"].shape == (0, len(Q))
        if n >= 3:                                                          # the select's order of zeros: -0.0 before +0.0
            e.set_state(1, 20, np.where(np.arange(n) % 2 == 0, 0.0, -0.0))
            for z in (e.quantile_rows(1, [0.0, 1.0], 20, 21)["quantiles"][0], e.quantile_series(1, [0.0, 1.0], 20, 21)["quantiles"][0]):
                assert np.signbit(z[0]) and not np.signbit(z[1])
        with pytest.raises(Exception, match="Quantiles must be in the range"):
            e.quantile_rows(1, [1.5])
        with pytest.raises(Exception, match="bad time range"):
            e.quantile_rows(1, Q, 0, 10, 0)


@pytest.mark.parametrize("n_q", [129, 300])
def test_quantile_series_takes_more_quantiles_than_one_select(ra, n_q):
    """quantile_series over a list longer than the select's 128 quantiles: numpy's numbers, the bits of quantile_rows called on
    the same list in pieces of at most 128, and the non-NaN count, on adversarial rows (N odd, no multiple of 64 or the block)."""
    n = 4099
    rng = np.random.default_rng(n_q)
    q = np.concatenate([[0.0, 1.0, 0.5, 0.5, 1.0, 0.0, 1e-12], rng.random(n_q - 7)])
    q[127] = q[128] = 0.0                                                   # repeated across the first block boundary
    q[-1] = 1.0
    with _two_layer(ra, n, steps=12) as e:
        for k, row in enumerate(_adversarial(rng, n)[:8]):
            e.set_state(1, 2 + k, row)
        rows = e.get_series(1)[2:10]
        got = e.quantile_series(1, q, 2, 10)
        assert got["quantiles"].shape == (8, n_q)
        assert same_values(got["quantiles"], _nanq(rows, q))
        pieces = [e.quantile_rows(1, q[k:k + 128], 2, 10) for k in range(0, n_q, 128)]
        assert _bits_equal(got["quantiles"], np.concatenate([p["quantiles"] for p in pieces], axis=1))
        assert np.array_equal(got["count"], (~np.isnan(rows)).sum(axis=1))
        assert all(np.array_equal(p["count"], got["count"]) for p in pieces)


def test_quantile_series_leaves_a_staged_select_alone(ra):
    """A staged select three passes in, quantile_series on another variable and range, then the staged select's other five
    passes: both carry the bits they have when computed alone."""
    n = 4099
    rng = np.random.default_rng(11)
    with _two_layer(ra, n, steps=60) as e:
        for k, row in enumerate(_adversarial(rng, n)):
            e.set_state(1, 2 + k, row)
        alone_rows, alone_series = e.quantile_rows(1, Q, 0, 20), e.quantile_series(2, Q, 30, 70)
        with e.select(1, Q, 0, 20) as s:
            for _ in range(3):
                assert s.next_pass() is not None
                s.commit()
            series = e.quantile_series(2, Q, 30, 70)
            while s.next_pass() is not None:
                s.commit()
            staged = s.result()
        for got, want in ((staged, alone_rows), (series, alone_series)):
            assert _bits_equal(got["quantiles"], want["quantiles"]) and np.array_equal(got["count"], want["count"])


def test_quantile_series_refusals_keep_code_and_text(ra):
    """What quantile_series refuses, with the code and text it always had: handles without whole series are RSCM_ERR_STATE,
    a bad range or an empty quantile list RSCM_ERR_INVALID; an empty range is a success of no rows."""
    from rscm_amd import RscmGpuError
    t = axis_values(1750, 1830)
    b = np.append(t, t[-1] + 1.0)
    for kw in (dict(window_rows=8), dict(store_series=False)):
        with ra.Ensemble(ra.KIND_TWO_LAYER, 3, b, **kw) as e:
            with pytest.raises(RscmGpuError, match="does not store whole series") as err:
                e.quantile_series(1, Q)
            assert err.value.code == 2                    # RSCM_ERR_STATE
    with _two_layer(ra, 3, steps=10) as e:
        for bad in (lambda: e.quantile_series(1, Q, 7, 5), lambda: e.quantile_series(1, [])):
            with pytest.raises(RscmGpuError, match="bad variable / time range / quantile list") as err:
                bad()
            assert err.value.code == 1                    # RSCM_ERR_INVALID
        empty = e.quantile_series(1, Q, 5, 5)
        assert empty["quantiles"].shape == (0, len(Q)) and empty["count"].shape == (0,)


def _staged_sum(parts, q, t_begin=0, t_end=None, t_stride=1):
    """The select of several handles, their int64 buffers summed on the host between the passes."""
    sels = [p.select(1, q, t_begin, t_end, t_stride) for p in parts]
    try:
        passes = 0
        while True:
            bufs = [s.next_pass() for s in sels]
            if bufs[0] is None:
                assert all(b is None for b in bufs)
                break
            total = np.sum([b.to_host() for b in bufs], axis=0)
            for s in sels:
                s.commit(total)
            passes += 1
        assert passes == 8
        return [s.result() for s in sels]
    finally:
        for s in sels:
            s.close()


@pytest.mark.parametrize("split", [0.5, 0.137])
def test_two_handles_summing_their_histograms_equal_the_whole(ra, split):
    """Two ensembles on one GPU hold the two halves of one member set; the host sums their pass buffers.  Both end with the
    bits of quantile_rows of the whole ensemble -- the reduction contract of the staged select, without ranks."""
    n = 20_011
    k = int(n * split)
    P = two_layer_params(n)
    rng = np.random.default_rng(3)
    rows = _adversarial(rng, n)
    with _two_layer(ra, n, P, steps=50) as whole, _two_layer(ra, k, np.ascontiguousarray(P[:, :k]), steps=50) as a, \
            _two_layer(ra, n - k, np.ascontiguousarray(P[:, k:]), steps=50) as b:
        for j, row in enumerate(rows):
            whole.set_state(1, 3 + j, row)
            a.set_state(1, 3 + j, np.ascontiguousarray(row[:k]))
            b.set_state(1, 3 + j, np.ascontiguousarray(row[k:]))
        want = whole.quantile_rows(1, Q)
        for res in _staged_sum([a, b], Q):
            assert _bits_equal(res["quantiles"], want["quantiles"]) and np.array_equal(res["count"], want["count"])
        want = whole.quantile_rows(1, Q, 2, 70, 4)
        for res in _staged_sum([a, b], Q, 2, 70, 4):
            assert _bits_equal(res["quantiles"], want["quantiles"])
        # the staged API refuses calls out of order
        with a.select(1, Q) as s:
            with pytest.raises(Exception, match="no pass to commit"):
                s.commit()
            with pytest.raises(Exception, match="already in flight"):
                a.select(1, Q)
            s.next_pass()
            with pytest.raises(Exception, match="commit the previous pass"):
                s.next_pass()
            with pytest.raises(Exception, match="still to run"):
                s.result()
            assert _bits_equal(a.quantile_rows(1, Q)["quantiles"], a.quantile_series(1, Q)["quantiles"])   # untouched by it


def test_windowed_graph_quantile_rows(ra):
    """The MAGICC chain, monthly steps, a 16-row window and every 12th row kept (configs[3]'s storage at a few thousand members):
    GraphModel.quantile_rows over the annual rows is numpy.nanquantile of get_series(t_stride=12), mid-run and at the end, for
    five variables; rows still in the window are read there; a row that is in neither is RSCM_ERR_STATE."""
    from rscm_amd import RscmGpuError
    mod = magicc_chain()
    names = ["Surface Temperature", "Atmospheric Concentration|CO2", "Effective Radiative Forcing", "Sea Surface Temperature",
             "Atmospheric Concentration|CH4"]
    model = mod.build_chain(3001, 30, "topological", steps_per_year=12, series_window=16, output_stride=12)
    try:
        for stop in (200, None):
            if stop is None:
                model.run()
            else:
                for _ in range(stop):
                    model.step()
            ti = model.time_index
            for name in names:
                got = model.quantile_rows(name, Q, t_stride=12)
                ser = model.get_series(name, t_stride=12)
                assert same_values(got["quantiles"], _nanq(ser, Q)), (stop, name)
                assert np.array_equal(got["count"], (~np.isnan(ser)).sum(axis=1)), (stop, name)
                assert np.isfinite(got["quantiles"][1: ti // 12 + 1]).all(), (stop, name)
                w0 = ti - 2                               # rows of the window, at every index
                win = model.quantile_rows(name, Q, w0, ti + 1)
                assert same_values(win["quantiles"], _nanq(model.get_series(name, t_begin=w0, t_end=ti + 1), Q))
            with pytest.raises(RscmGpuError, match="not resident") as err:
                model.quantile_rows("Surface Temperature", Q, 13, 14)
            assert err.value.code == 2                    # RSCM_ERR_STATE
    finally:
        model.close()
