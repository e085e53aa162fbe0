"""GPU tier of the per-member covariability of two variables (csrc/covariability.hip; rscm_ens_member_covariability;
Ensemble.covariability, GraphModel.covariability).  The oracle is the numpy restatement of tests/host_covariability.py on rows
copied to the host, compared by value (+0 equal to -0, any NaN equal to any NaN).

The data are those of tests/test_gpu_variability.py: two-layer ensembles with per-member forcing noise on a 48-point annual axis,
half the members under zero forcing and half under a ramp, with the ocean heat content as a diagnostic variable.  From 63 members
on, three members are special -- a silent one under zero forcing (constant series), one with a NaN parameter and one with an
amplitude that overflows -- and two more have +Inf written into one row of the surface temperature alone and -Inf into one row of
the deep temperature alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import host_covariability as hc
from tests import host_likelihood as hl
from tests import host_variability as hv
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import built_once, noise_ensemble, plant, refusal_code
from tests.helpers import annual_bounds, magicc_chain, same_values

pytestmark = pytest.mark.gpu

T = 48
YEARS, BOUNDS = annual_bounds(T)
SEED = 20260327
DETREND = ("mean", "linear", "difference")
PAIRS = list(itertools.product(DETREND, DETREND))
LAGS = (0, 1, 2, 3)
SIZES = [1, 63, 64, 257, 1000]       # a single member; below, at and past a wave; a ragged last block; more than one block
# 3 .. 7: the limits n >= 3 + n_lags of every lag count with and without a differenced variable; 3, 4, 5, 8 and 9: one below, at, one
# past and twice the kernel's load batch of 4 rows, and one past that (a differenced pair's terms straddle the batches); 40: ten batches
ROWS = [3, 4, 5, 6, 7, 8, 9, 40]
TS, TD, HEAT = 1, 2, "heat"


def _ensemble(ra, n, offset=0, n_total=None, steps=None, **kw):
    return noise_ensemble(ra, n, BOUNDS, SEED, offset, n_total, steps, **kw)


@pytest.fixture(scope="module")
def cases(ra):
    """{N: (ensemble, {variable: its series [T][N] on the host})}, each built and run once and left unchanged."""
    def build(n):
        e = _ensemble(ra, n)
        if n >= 63:
            for var, member, row, value in ((TS, 5, 1, np.inf), (TD, 7, 2, -np.inf)):
                plant(e, var, member, row, value)
        e.define_heat_content(HEAT)
        e.compute_diagnostic(HEAT)
        ser = {v: e.get_series(v) for v in (TS, TD, HEAT)}
        for s in ser.values():
            s.setflags(write=False)
        return e, ser

    yield from built_once(build)


def _host(d):
    return [v.to_host() for v in hc.flat(d)]


def _check(got, want, what):
    want = hc.flat(want)
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert same_values(g, w), (what, j, np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])


def _terms(R, dx, dy):
    return R - (1 if "difference" in (dx, dy) else 0)


@pytest.mark.parametrize("n", SIZES)
def test_statistics_equal_the_restatement(ra, cases, n):
    """Surface against deep temperature: every mode pair, lag count and row count, the refused shapes just below the limits."""
    e, ser = cases(n)
    x, y = ser[TS], ser[TD]
    if n >= 63:
        assert (x[:, n - 3] == 0.0).all() and (y[:, n - 3] == 0.0).all() and np.isnan(x[1:, n - 1]).all() and not np.isfinite(x[:, n - 2]).all()
        assert np.isposinf(x[1, 5]) and np.isfinite(y[:, 5]).all() and np.isneginf(y[2, 7]) and np.isfinite(x[:, 7]).all()
    for (dx, dy), lags, R in itertools.product(PAIRS, LAGS, ROWS):
        kw = dict(detrend_x=dx, detrend_y=dy, lags=lags)
        if _terms(R, dx, dy) < 3 + lags:
            assert refusal_code(e.covariability, TS, TD, 0, R, **kw) == 1
            continue
        res = e.covariability(TS, TD, 0, R, **kw)
        assert set(res) == set(hc.NAMES) | {"lead", "lag"} and len(res["lead"]) == len(res["lag"]) == lags
        got = _host(res)
        _check(got, hc.covariability(x[:R], y[:R], dx, dy, lags), (dx, dy, lags, R))
        if n >= 63:
            assert got[0][n - 3] == 0.0 and got[1][n - 3] == 0.0 and all(np.isnan(g[n - 3]) for g in got[3:])     # constant: 0 / 0
            bad = ~(np.isfinite(x[:R]).all(axis=0) & np.isfinite(y[:R]).all(axis=0))
            assert bad[[n - 1, 5, 7]].all() and not bad[:5].any() and (R < 40 or bad[n - 2])
            for g in got:
                assert np.isnan(g[bad]).all() and np.isfinite(g[:5]).all(), (dx, dy, lags, R)
    for dx, dy in PAIRS:
        _check(_host(e.covariability(TS, TD, 2, T, 3, dx, dy, 3)), hc.covariability(x[2:T:3], y[2:T:3], dx, dy, 3), (dx, dy, "strided"))
        _check(_host(e.covariability(TS, TD, T - 7, T, 1, dx, dy, 3, slot=3)), hc.covariability(x[T - 7:], y[T - 7:], dx, dy, 3), (dx, dy, "last rows"))


@pytest.mark.parametrize("vx,vy", [(TS, HEAT), (HEAT, TS), (TS, TS), (HEAT, HEAT)])
def test_pairs_with_a_diagnostic_and_a_variable_with_itself(cases, vx, vy):
    for n in (64, 257):
        e, ser = cases(n)
        for (dx, dy), (R, lags) in itertools.product(PAIRS, ((T, 3), (9, 1), (4, 0))):
            got = _host(e.covariability(vx, vy, 0, R, 1, dx, dy, lags, slot=2))
            _check(got, hc.covariability(ser[vx][:R], ser[vy][:R], dx, dy, lags), (vx, vy, dx, dy, R))
    assert np.isfinite(got[3][:5]).all()


@pytest.mark.parametrize("n", [257, 1000])
def test_exchange_and_variance_equalities_on_the_device(cases, n):
    """Exchanging (x, mode_x) with (y, mode_y) exchanges var_x with var_y and r_{+l} with r_{-l} and keeps cov and corr; with no
    mode mixed var_x and var_y are the variances of variability() -- all value for value (+0 equal to -0), on device results alone."""
    e, ser = cases(n)
    for vx, vy in ((TS, TD), (TS, HEAT)):
        for dx, dy in PAIRS:
            s = e.covariability(vx, vy, 3, T, 1, dx, dy, 3, slot=0)
            s = {k: [w.to_host() for w in v] if isinstance(v, list) else v.to_host() for k, v in s.items()}
            t = e.covariability(vy, vx, 3, T, 1, dy, dx, 3, slot=1)
            t = {k: [w.to_host() for w in v] if isinstance(v, list) else v.to_host() for k, v in t.items()}
            assert same_values(s["var_x"], t["var_y"]) and same_values(s["var_y"], t["var_x"]) and same_values(s["cov"], t["cov"]) and same_values(s["corr"], t["corr"])
            for l in range(3):
                assert same_values(s["lead"][l], t["lag"][l]) and same_values(s["lag"][l], t["lead"][l])
            assert np.isfinite(s["corr"][:5]).all() and not same_values(s["lead"][0], s["lag"][0])
            if (dx == "difference") == (dy == "difference"):
                assert same_values(s["var_x"], e.variability(vx, 3, T, detrend=dx, slot=2)["variance"].to_host())
                assert same_values(s["var_y"], e.variability(vy, 3, T, detrend=dy, slot=2)["variance"].to_host())
            live = np.isfinite(s["corr"])
            for g in [s["corr"]] + s["lead"] + s["lag"]:
                assert np.abs(g[live]).max() <= 1.0 + 8 * T * 2.0 ** -53


def test_windowed_graph(ra):
    """Two outputs of one home ensemble of a windowed graph, from the output store, give the bits of the full-storage build; rows
    that are not resident are refused; two variables with different homes raise."""
    mod = magicc_chain()
    plant_pool, soil, co2 = "Carbon Pool|Plant", "Carbon Pool|Soil", "Atmospheric Concentration|CO2"
    got = {}
    for key, kw in (("windowed", dict(series_window=16, output_stride=12)), ("full", {})):
        model = mod.build_chain(65, 30, "topological", steps_per_year=12, **kw)
        try:
            model.run()
            ens, _ = model.variable_home(plant_pool)
            assert model.variable_home(soil)[0] is ens and model.variable_home(co2)[0] is not ens
            n_times = ens.n_times
            got[key] = {p: _host(model.covariability(plant_pool, soil, 0, n_times, 12, p[0], p[1], 3, slot=1)) for p in PAIRS}
            if key == "full":
                x, y = model.get_series(plant_pool, t_stride=12), model.get_series(soil, t_stride=12)
                for p in PAIRS:
                    _check(got[key][p], hc.covariability(x, y, p[0], p[1], 3), ("chain", p))
            else:
                assert refusal_code(model.covariability, plant_pool, soil, 0, 9, 3) == 2       # rows 3 and 6: outside the window and the output stride
            with pytest.raises(ValueError, match="share one home"):
                model.covariability(plant_pool, co2, 0, n_times, 12)
        finally:
            model.close()
    for p in PAIRS:
        assert all(same_values(a, b) for a, b in zip(got["windowed"][p], got["full"][p])), p


def test_slots_and_refusals(ra, cases):
    e, ser = cases(257)
    ind = e.indicators(TS, 0, 30, thresholds=[0.2, 0.5], slot=0)
    keep = [ind["mean"].to_host(), ind["peak"].to_host()] + [c.to_host() for c in ind["crossing"]]
    cov = e.covariability(TS, TD, 0, 30, lags=3, slot=1)
    assert all(same_values(a, b) for a, b in zip(keep, [ind["mean"].to_host(), ind["peak"].to_host()] + [c.to_host() for c in ind["crossing"]]))
    assert cov["var_x"].ptr != ind["mean"].ptr
    want = hc.covariability(ser[TS][:30], ser[TD][:30], "linear", "linear", 3)
    _check(_host(cov), want, "slot 1")
    # a slot keeps the vectors of the last call of any kind: the last of eleven vectors survives a call on another slot, not one on its own
    last = cov["lag"][2]
    e.spectrum(TS, 0, 30, slot=2)
    assert same_values(last.to_host(), want["lag"][2])
    var = e.variability(TS, 0, 30, slot=1)
    assert var["mean"].ptr == cov["var_x"].ptr and same_values(var["variance"].to_host(), hv.variability(ser[TS][:30], "linear")["variance"])
    assert e.covariability(TS, TD, 0, 30, slot=0)["var_x"].ptr == ind["mean"].ptr
    assert refusal_code(e.covariability, TS, TD, 0, 30, slot=4) == 1 and refusal_code(e.covariability, TS, TD, 0, 30, slot=-1) == 1
    assert refusal_code(e.covariability, TS, TD, 0, 30, lags=4) == 1 and refusal_code(e.covariability, TS, TD, 0, 30, lags=-1) == 1
    with pytest.raises(ValueError):
        e.covariability(TS, TD, 0, 30, detrend_x="quadratic")
    with pytest.raises(ValueError):
        e.covariability(TS, TD, 0, 30, detrend_y="quadratic")
    p = C.c_void_p()
    call = e._lib.rscm_ens_member_covariability
    for mx, my in ((-1, 0), (3, 0), (0, -1), (0, 3)):
        assert call(e._h, 1, 2, 0, 30, 1, mx, my, 0, 0, C.byref(p)) == 1 and p.value is None
    assert call(e._h, 0, 1, 0, 30, 1, 0, 0, 0, 0, C.byref(p)) == 1 and call(e._h, 1, 0, 0, 30, 1, 0, 0, 0, 0, C.byref(p)) == 1     # no stored series
    assert call(e._h, 1, 7, 0, 30, 1, 0, 0, 0, 0, C.byref(p)) == 1                  # neither a stored variable nor a diagnostic
    assert call(e._h, 1, 2, 0, 30, 1, 0, 0, 0, 0, None) == 1
    assert refusal_code(e.covariability, TS, TD, 0, 2) == 1 and refusal_code(e.covariability, TS, TD, 5, 5) == 1 and refusal_code(e.covariability, TS, TD, 0, 30, 0) == 1
    with e.select(1, [0.5], 0, 30) as s:
        assert refusal_code(e.covariability, TS, TD, 0, 30) == 2
        while s.next_pass() is not None:
            s.commit()
    with _ensemble(ra, 64, steps=10) as h:
        assert h.time_index == 10
        assert refusal_code(h.covariability, TS, TD, 0, 20) == 2                           # rows beyond the time index
        vid = h.define_heat_content()
        assert refusal_code(h.covariability, TS, vid, 0, 11) == 2                          # no rows computed yet
        h.compute_diagnostic(vid, 0, 8)
        assert refusal_code(h.covariability, vid, TS, 0, 11) == 2                          # rows 8 .. 10 are not held
        h.covariability(vid, TS, 0, 8)
        h.run(20)
        assert refusal_code(h.covariability, TS, vid, 0, 8) == 2 and refusal_code(h.covariability, vid, TS, 0, 8) == 2      # stale
        h.covariability(TS, TD, 0, 21)
        h.compute_diagnostic(vid)
        h.covariability(TS, vid, 0, 21, lags=3)


def test_loglik_vectors_onto_a_point_likelihood(cases):
    e, ser = cases(1000)
    c = e.covariability(TS, HEAT, 0, T, 1, "linear", "difference", 1, slot=1)
    want = hc.covariability(ser[TS], ser[HEAT], "linear", "difference", 1)
    dev, host = [c["corr"], c["slope"], c["lead"][0]], [want["corr"], want["slope"], want["lead"][0]]
    tidx = list(range(4, T, 4))
    obs, sig = [0.02 * t for t in tidx], [0.5] * len(tidx)
    point = hl.loglik({1: ser[TS]}, [1] * len(tidx), tidx, obs, sig)
    ll = e.loglik([1] * len(tidx), tidx, obs, sig, on_device=True)
    assert np.array_equal(ll.to_host(), point) and np.isneginf(point).any()
    values = [float(np.nanmedian(h)) for h in host]
    sigmas = [0.2, 2.0, 0.2]
    out = e.loglik_vectors(dev, values, sigmas, add_to=ll)
    assert out.ptr == ll.ptr
    got, ref = out.to_host(), hv.loglik_vectors(host, values, sigmas, add=point)
    assert np.array_equal(got, ref)
    n = e.n_members
    assert np.isneginf(got[[n - 1, n - 2, n - 3, 5, 7]]).all() and np.isfinite(got[:5]).all()
    # the vectors are indicator-slot vectors like any other: exceedance counts them in integers
    ex = e.exceedance(c["corr"], [0.0, 0.5])
    live = ~np.isnan(want["corr"])
    assert ex["total"] == live.sum() and list(ex["hits"]) == [(want["corr"][live] >= thr).sum() for thr in (0.0, 0.5)]


def test_two_shards_give_the_halves(ra, cases):
    """Two handles over the halves of the 257 members (member_offset) hold the halves of the one handle's vectors."""
    n, k = 257, 129
    e, ser = cases(n)
    pairs = (("linear", "difference"), ("difference", "mean"), ("linear", "linear"))
    whole = {p: _host(e.covariability(TS, HEAT, 4, T, 1, p[0], p[1], 3, slot=2)) for p in pairs}     # (the rows from 4 on: none was overwritten)
    for offset, count in ((0, k), (k, n - k)):
        with _ensemble(ra, count, offset, n) as h:
            vid = h.define_heat_content(HEAT)
            h.compute_diagnostic(vid, 4, T)
            for p in pairs:
                got = _host(h.covariability(TS, HEAT, 4, T, 1, p[0], p[1], 3))
                for j, g in enumerate(got):
                    assert same_values(g, whole[p][j][offset:offset + count]), (p, j, offset)
