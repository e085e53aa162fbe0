"""GPU tier of the per-member co-spectra of two variables in frequency bands (csrc/cross_spectrum.hip;
rscm_ens_member_cross_spectrum; Ensemble.cross_spectrum, GraphModel.cross_spectrum).  The oracle is the numpy restatement of
tests/host_cross_spectrum.py on rows copied to the host, compared by value (+0 equal to -0, any NaN equal to any NaN).

The data are those of tests/test_gpu_covariability.py on an axis of 4 F + 8 = 40 annual points (F = 8, the kernel's tile of
frequencies): two-layer ensembles with per-member forcing noise, half the members under zero forcing and half under a ramp, with the
ocean heat content as a diagnostic variable.  From 63 members on, three members are special -- a silent one under zero forcing
(constant series), one with a NaN parameter and one with an amplitude that overflows -- and two more have +Inf written into one row
of the surface temperature alone and -Inf into one row of the deep temperature alone.  Every refusal below is a host-side check
before any launch."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import host_cross_spectrum as hx
from tests import host_likelihood as hl
from tests import host_variability as hv
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import built_once, noise_ensemble, plant, refusal_code
from tests.helpers import annual_bounds, magicc_chain, same_values, two_layer_params

pytestmark = pytest.mark.gpu

F = 8                                # kXSpecF of csrc/cross_spectrum.hip: the frequencies a lane carries per pass over the rows
T = 4 * F + 8
YEARS, BOUNDS = annual_bounds(T)
SEED = 20260327
DETREND = ("mean", "linear", "difference")
PAIRS = list(itertools.product(DETREND, DETREND))
SUBSET = [("linear", "linear"), ("mean", "difference"), ("difference", "linear"), ("difference", "difference")]
SIZES = [1, 63, 64, 257, 1000]       # a single member; below, at and past a wave; a ragged last block; more than one block
# terms of the working series.  3, 4, 5, 8, 9: the lower limit; one below, at, one past and twice the load batch of 4 rows, and one past
# that.  2 F - 1 .. 2 F + 4 (J = F - 1, F, F, F + 1, F + 1, F + 2): a partial tile, a full one, one and two frequencies into the second,
# odd and even.  4 F + 3, 4 F + 4 (J = 2 F + 1): one frequency into the third tile.
TERMS = [3, 4, 5, 8, 9] + list(range(2 * F - 1, 2 * F + 5)) + [4 * F + 3, 4 * F + 4]
MID = 2 * F + 3                      # the mid-size at which all nine mode pairs run
TS, TD, HEAT, TWICE = 1, 2, "heat", "twice"


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
        e.define_diagnostic(TWICE, [(TS, None, 2.0)])
        e.compute_diagnostic(HEAT)
        e.compute_diagnostic(TWICE)
        ser = {v: e.get_series(v) for v in (TS, TD, HEAT, TWICE)}
        for s in ser.values():
            s.setflags(write=False)
        return e, ser

    yield from built_once(build)


def _host(d):
    return [v.to_host() for v in hx.flat(d)]


def _check(got, want, what):
    want = hx.flat(want)
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert same_values(g, w), (what, j, np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])


def _rows(n, dx, dy):
    return n + (1 if "difference" in (dx, dy) else 0)


def _band_lists(n):
    """bands = 1, 2, 3 (fewer where the series has fewer frequencies) and explicit edge lists that start above 1 and end below J + 1,
    inside one tile and across two."""
    J = (n - 1) // 2
    out = [1, 2, 3]
    if J >= 3:
        out += [[2, J], [2, 3, J + 1]]
    if J >= F + 2:
        out += [[F - 1, F + 2], [3, F, F + 1, J], [F + 1, J + 1]]
    return out


@pytest.mark.parametrize("n", SIZES)
def test_statistics_equal_the_restatement(ra, cases, n):
    """Surface against deep temperature: every length of the list, band count and edge list; all nine mode pairs at the mid-size, a
    covering subset elsewhere; strides, the last rows, slot 3."""
    e, ser = cases(n)
    x, y = ser[TS], ser[TD]
    if n >= 63:
        assert (x[:, n - 3] == 0.0).all() and (y[:, n - 3] == 0.0).all() and np.isnan(x[1:, n - 1]).all() and not np.isfinite(x[:, n - 2]).all()
        assert np.isposinf(x[1, 5]) and np.isfinite(y[:, 5]).all() and np.isneginf(y[2, 7]) and np.isfinite(x[:, 7]).all()
    for terms in TERMS:
        for dx, dy in (PAIRS if terms == MID else SUBSET):
            R = _rows(terms, dx, dy)
            for bands in _band_lists(terms):
                res = e.cross_spectrum(TS, TD, 0, R, 1, dx, dy, bands)
                B = len(res["edges"]) - 1
                assert set(res) == {"var_x", "var_y", "coherence2", "gain", "gain_quad", "edges", "counts"}
                assert len(res["coherence2"]) == len(res["gain"]) == len(res["gain_quad"]) == B == len(res["counts"])
                if isinstance(bands, int):
                    assert B == min(bands, (terms - 1) // 2) and res["edges"][0] == 1 and res["edges"][-1] == (terms - 1) // 2 + 1
                got = _host(res)
                _check(got, hx.cross_spectrum(x[:R], y[:R], dx, dy, res["edges"]), (dx, dy, terms, bands))
                if n >= 63:
                    assert got[0][n - 3] == 0.0 and got[1][n - 3] == 0.0 and all(np.isnan(g[n - 3]) for g in got[2:])     # constant: 0 / 0
                    bad = ~(np.isfinite(x[:R]).all(axis=0) & np.isfinite(y[:R]).all(axis=0))
                    assert bad[[n - 1, 5, 7]].all() and not bad[:5].any()
                    for g in got:
                        assert np.isnan(g[bad]).all() and np.isfinite(g[:5]).all(), (dx, dy, terms, bands)
    for dx, dy in PAIRS:
        s = e.cross_spectrum(TS, TD, 1, T, 2, dx, dy, 3)
        _check(_host(s), hx.cross_spectrum(x[1:T:2], y[1:T:2], dx, dy, s["edges"]), (dx, dy, "strided"))
        s = e.cross_spectrum(TS, TD, T - 11, T, 1, dx, dy, [2, 4, 5], slot=3)
        _check(_host(s), hx.cross_spectrum(x[T - 11:], y[T - 11:], dx, dy, [2, 4, 5]), (dx, dy, "last rows"))
        s = e.cross_spectrum(TS, TD, 0, T, 1, dx, dy, 3)
        _check(_host(s), hx.cross_spectrum(x, y, dx, dy, s["edges"]), (dx, dy, "all rows"))


@pytest.mark.parametrize("vx,vy", [(TS, HEAT), (HEAT, TS), (TS, TS), (HEAT, HEAT), (TS, TWICE)])
def test_pairs_with_a_diagnostic_and_a_variable_with_itself(cases, vx, vy):
    for n in (64, 257):
        e, ser = cases(n)
        for (dx, dy), (R, bands) in itertools.product(PAIRS, ((T, 3), (2 * F + 2, [2, F, F + 1]), (4, 1))):
            s = e.cross_spectrum(vx, vy, 0, R, 1, dx, dy, bands, slot=2)
            got = _host(s)
            _check(got, hx.cross_spectrum(ser[vx][:R], ser[vy][:R], dx, dy, s["edges"]), (vx, vy, dx, dy, R))
    assert np.isfinite(got[2][:5]).all()


@pytest.mark.parametrize("n", [257, 1000])
def test_equalities_on_the_device(cases, n):
    """var_x, var_y are covariability()'s for the same arguments; the exchange keeps every coh2 and exchanges the variances; a variable
    against itself and against twice itself: quadrature +-0.0, the same coherence, twice the gain -- value for value, on device results."""
    e, ser = cases(n)
    host = lambda d: {k: [w.to_host() for w in v] if isinstance(v, list) else v.to_host() for k, v in d.items() if k not in ("edges", "counts")}
    for dx, dy in PAIRS:
        for vx, vy in ((TS, TD), (TS, HEAT)):
            s, t = host(e.cross_spectrum(vx, vy, 3, T, 1, dx, dy, 3, slot=0)), host(e.cross_spectrum(vy, vx, 3, T, 1, dy, dx, 3, slot=1))
            cov = e.covariability(vx, vy, 3, T, 1, dx, dy, 0, slot=2)
            assert same_values(s["var_x"], cov["var_x"].to_host()) and same_values(s["var_y"], cov["var_y"].to_host())
            assert same_values(s["var_x"], t["var_y"]) and same_values(s["var_y"], t["var_x"])
            live = np.isfinite(s["var_x"]) & (s["var_x"] > 0.0)
            assert live[:5].all()
            for b in range(3):
                assert same_values(s["coherence2"][b], t["coherence2"][b]) and np.isfinite(s["coherence2"][b][live]).all()
                # coh2 <= 1 up to the rounding bound tests/test_cross_spectrum_cpu.py derives (6 x 1e-8)
                assert s["coherence2"][b][live].max() <= 1.0 + 6e-8 and s["coherence2"][b][live].min() >= 0.0
        same = host(e.cross_spectrum(TS, TS, 3, T, 1, dx, dx, 3, slot=0))
        twice = host(e.cross_spectrum(TS, TWICE, 3, T, 1, dx, dx, 3, slot=1))
        live = np.isfinite(same["var_x"]) & (same["var_x"] > 0.0)
        for b in range(3):
            assert (same["gain_quad"][b][live] == 0.0).all() and (twice["gain_quad"][b][live] == 0.0).all()
            assert same_values(twice["coherence2"][b], same["coherence2"][b])
            assert same_values(twice["gain"][b], 2.0 * same["gain"][b])
            assert np.abs(same["gain"][b][live] - 1.0).max() <= 6e-8


def test_windowed_graph(ra):
    """Two outputs of one home ensemble of a windowed graph, from the output store, give the bits of the full-storage build; rows
    that are not resident are refused; two variables with different homes raise."""
    mod = magicc_chain()
    plant_pool, soil, co2 = "Carbon Pool|Plant", "Carbon Pool|Soil", "Atmospheric Concentration|CO2"
    pairs = SUBSET + [("mean", "mean")]
    got = {}
    for key, kw in (("windowed", dict(series_window=16, output_stride=12)), ("full", {})):
        model = mod.build_chain(65, 30, "topological", steps_per_year=12, **kw)
        try:
            model.run()
            ens, _ = model.variable_home(plant_pool)
            assert model.variable_home(soil)[0] is ens and model.variable_home(co2)[0] is not ens
            n_times = ens.n_times
            got[key] = {p: _host(model.cross_spectrum(plant_pool, soil, 0, n_times, 12, p[0], p[1], 3, slot=1)) for p in pairs}
            if key == "full":
                x, y = model.get_series(plant_pool, t_stride=12), model.get_series(soil, t_stride=12)
                for p in pairs:
                    terms = len(x) - (1 if "difference" in p else 0)
                    from rscm_amd.variability import band_edges
                    _check(got[key][p], hx.cross_spectrum(x, y, p[0], p[1], band_edges(terms, 3)), ("chain", p))
            else:
                assert refusal_code(model.cross_spectrum, plant_pool, soil, 0, 9, 3) == 2       # rows 3 and 6: outside the window and the output stride
            with pytest.raises(ValueError, match="share one home"):
                model.cross_spectrum(plant_pool, co2, 0, n_times, 12)
        finally:
            model.close()
    for p in pairs:
        assert all(same_values(a, b) for a, b in zip(got["windowed"][p], got["full"][p])), p


def test_slots_and_refusals(ra, cases):
    e, ser = cases(257)
    ind = e.indicators(TS, 0, 30, thresholds=[0.2, 0.5], slot=0)
    keep = [ind["mean"].to_host(), ind["peak"].to_host()] + [c.to_host() for c in ind["crossing"]]
    xs = e.cross_spectrum(TS, TD, 0, 30, bands=3, slot=1)
    assert all(same_values(a, b) for a, b in zip(keep, [ind["mean"].to_host(), ind["peak"].to_host()] + [c.to_host() for c in ind["crossing"]]))
    assert xs["var_x"].ptr != ind["mean"].ptr
    want = hx.cross_spectrum(ser[TS][:30], ser[TD][:30], "linear", "linear", xs["edges"])
    _check(_host(xs), want, "slot 1")
    # a slot keeps the vectors of the last call of any kind: the last of eleven vectors survives a call on another slot, not one on its own
    last = xs["gain_quad"][2]
    e.spectrum(TS, 0, 30, slot=2)
    e.covariability(TS, TD, 0, 30, lags=3, slot=0)
    assert same_values(last.to_host(), want["gain_quad"][2])
    var = e.variability(TS, 0, 30, slot=1)
    assert var["mean"].ptr == xs["var_x"].ptr and same_values(var["variance"].to_host(), hv.variability(ser[TS][:30], "linear")["variance"])
    assert e.cross_spectrum(TS, TD, 0, 30, slot=0)["var_x"].ptr == ind["mean"].ptr
    assert refusal_code(e.cross_spectrum, TS, TD, 0, 30, slot=4) == 1 and refusal_code(e.cross_spectrum, TS, TD, 0, 30, slot=-1) == 1
    with pytest.raises(ValueError):
        e.cross_spectrum(TS, TD, 0, 30, bands=0)
    with pytest.raises(ValueError):
        e.cross_spectrum(TS, TD, 0, 30, bands=4)
    with pytest.raises(ValueError):
        e.cross_spectrum(TS, TD, 0, 30, detrend_x="quadratic")
    with pytest.raises(ValueError):
        e.cross_spectrum(TS, TD, 0, 30, detrend_y="quadratic")
    # J = 14 of 30 terms: five edges (four bands), edges out of order, equal, below 1, past J + 1
    for bad in ([1, 2, 3, 4, 5], [3, 2], [1, 4, 4], [0, 3], [1, 16], [1, 5, 3, 9]):
        assert refusal_code(e.cross_spectrum, TS, TD, 0, 30, bands=bad) == 1
    e.cross_spectrum(TS, TD, 0, 30, 1, "mean", "difference", [1, 15])                          # 29 terms: J + 1 = 15 is the last edge allowed
    assert refusal_code(e.cross_spectrum, TS, TD, 0, 30, 1, "mean", "difference", [1, 16]) == 1
    p = C.c_void_p()
    call = e._lib.rscm_ens_member_cross_spectrum
    edges = (C.c_int32 * 5)(1, 2, 3, 4, 5)
    for nb in (0, 4, -1):
        assert call(e._h, 1, 2, 0, 30, 1, 0, 0, nb, edges, 0, C.byref(p)) == 1 and p.value is None
    assert call(e._h, 1, 2, 0, 30, 1, 0, 0, 2, None, 0, C.byref(p)) == 1
    for mx, my in ((-1, 0), (3, 0), (0, -1), (0, 3)):
        assert call(e._h, 1, 2, 0, 30, 1, mx, my, 2, edges, 0, C.byref(p)) == 1 and p.value is None
    assert call(e._h, 0, 1, 0, 30, 1, 0, 0, 2, edges, 0, C.byref(p)) == 1 and call(e._h, 1, 0, 0, 30, 1, 0, 0, 2, edges, 0, C.byref(p)) == 1     # no stored series
    assert call(e._h, 1, 9, 0, 30, 1, 0, 0, 2, edges, 0, C.byref(p)) == 1           # neither a stored variable nor a diagnostic
    assert call(e._h, 1, 2, 0, 30, 1, 0, 0, 2, edges, 0, None) == 1
    assert call(e._h, 1, 2, 0, 30, 1, 0, 0, 3, edges, 0, C.byref(p)) == 0 and p.value is not None
    # n of 2, an empty range, a zero stride
    assert refusal_code(e.cross_spectrum, TS, TD, 0, 2) == 1 and refusal_code(e.cross_spectrum, TS, TD, 0, 3, 1, "difference", "mean") == 1
    assert refusal_code(e.cross_spectrum, TS, TD, 5, 5) == 1 and refusal_code(e.cross_spectrum, TS, TD, 0, 30, 0) == 1
    with e.select(1, [0.5], 0, 30) as s:
        assert refusal_code(e.cross_spectrum, TS, TD, 0, 30) == 2
        while s.next_pass() is not None:
            s.commit()
    with _ensemble(ra, 64, steps=10) as h:
        assert h.time_index == 10
        assert refusal_code(h.cross_spectrum, TS, TD, 0, 20) == 2                          # rows beyond the time index
        vid = h.define_heat_content()
        assert refusal_code(h.cross_spectrum, TS, vid, 0, 11) == 2                         # no rows computed yet
        h.compute_diagnostic(vid, 0, 8)
        assert refusal_code(h.cross_spectrum, vid, TS, 0, 11) == 2                         # rows 8 .. 10 are not held
        h.cross_spectrum(vid, TS, 0, 8)
        h.run(20)
        assert refusal_code(h.cross_spectrum, TS, vid, 0, 8) == 2 and refusal_code(h.cross_spectrum, vid, TS, 0, 8) == 2      # stale
        h.cross_spectrum(TS, TD, 0, 21)
        h.compute_diagnostic(vid)
        h.cross_spectrum(TS, vid, 0, 21)


def test_more_than_4096_terms_are_refused(ra):
    """A long axis with few members: n = 4096 is served (against the restatement, a band list inside the last tile), n = 4097 is
    refused -- the spectrum's cap, for the same reason."""
    steps = 4099
    bounds = np.arange(1000.0, 1000.0 + steps + 1)
    with ra.Ensemble(ra.KIND_TWO_LAYER, 8, bounds, noise_params=True) as e:
        P = np.vstack([two_layer_params(8), np.full(8, 0.3), np.linspace(0.0, 0.9, 8)])
        e.set_params(P)
        e.set_forcing(np.zeros(steps))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.set_forcing_noise_members(SEED, 0)
        e.run()
        assert refusal_code(e.cross_spectrum, TS, TD, 0, 4097, 1, "mean", "linear") == 1
        assert refusal_code(e.cross_spectrum, TS, TD, 0, 4098, 1, "difference", "linear") == 1
        edges = [2040, 2044, 2048]
        d = e.cross_spectrum(TS, TD, 0, 4097, 1, "linear", "difference", edges)
        _check(_host(d), hx.cross_spectrum(e.get_series(TS, 0, 4097), e.get_series(TD, 0, 4097), "linear", "difference", edges), "4096 terms")


def test_loglik_vectors_onto_a_point_likelihood(cases):
    e, ser = cases(1000)
    c = e.cross_spectrum(TS, HEAT, 0, T, 1, "linear", "difference", 3, slot=1)
    want = hx.cross_spectrum(ser[TS], ser[HEAT], "linear", "difference", c["edges"])
    dev, host = [c["coherence2"][0], c["gain"][0]], [want["coherence2"][0], want["gain"][0]]
    tidx = list(range(4, T, 4))
    obs, sig = [0.02 * t for t in tidx], [0.5] * len(tidx)
    point = hl.loglik({1: ser[TS]}, [1] * len(tidx), tidx, obs, sig)
    ll = e.loglik([1] * len(tidx), tidx, obs, sig, on_device=True)
    assert np.array_equal(ll.to_host(), point) and np.isneginf(point).any()
    values = [float(np.nanmedian(h)) for h in host]
    sigmas = [0.2, 2.0]
    out = e.loglik_vectors(dev, values, sigmas, add_to=ll)
    assert out.ptr == ll.ptr
    got, ref = out.to_host(), hv.loglik_vectors(host, values, sigmas, add=point)
    assert np.array_equal(got, ref)
    n = e.n_members
    assert np.isneginf(got[[n - 1, n - 2, n - 3, 5, 7]]).all() and np.isfinite(got[:5]).all()
    # the vectors are indicator-slot vectors like any other: exceedance counts them in integers
    ex = e.exceedance(c["coherence2"][1], [0.5, 0.9])
    live = ~np.isnan(want["coherence2"][1])
    assert ex["total"] == live.sum() and list(ex["hits"]) == [(want["coherence2"][1][live] >= thr).sum() for thr in (0.5, 0.9)]


def test_two_shards_give_the_halves(ra, cases):
    """Two handles over the halves of the 257 members (member_offset) hold the halves of the one handle's vectors."""
    n, k = 257, 129
    e, ser = cases(n)
    pairs = (("linear", "difference"), ("difference", "mean"), ("linear", "linear"))
    whole = {p: _host(e.cross_spectrum(TS, HEAT, 4, T, 1, p[0], p[1], 3, slot=2)) for p in pairs}     # (the rows from 4 on: none was overwritten)
    for offset, count in ((0, k), (k, n - k)):
        with _ensemble(ra, count, offset, n) as h:
            vid = h.define_heat_content(HEAT)
            h.compute_diagnostic(vid, 4, T)
            for p in pairs:
                got = _host(h.cross_spectrum(TS, HEAT, 4, T, 1, p[0], p[1], 3))
                for j, g in enumerate(got):
                    assert same_values(g, whole[p][j][offset:offset + count]), (p, j, offset)
