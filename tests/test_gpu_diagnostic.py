"""GPU tier of the diagnostic variables (csrc/diagnostic.hip, csrc/diagnostic_host.cpp; rscm_ens_define_diagnostic,
rscm_ens_compute_diagnostic, rscm_ens_diagnostic, rscm_ens_clear_diagnostics; Ensemble.define_diagnostic, define_heat_content,
compute_diagnostic, GraphModel.define_diagnostic).  The oracle is the numpy restatement of tests/host_diagnostic.py applied to rows
fetched with get_series and parameters fetched with get_params, compared bit for bit (any NaN equal to any NaN).

The data: two-layer ensembles with per-member forcing noise on a 72-point annual axis, as in tests/test_gpu_variability.py: from
63 members on a silent one (its noise amplitude is 0.0, so the weight -2.5 * sigma_i is -0.0), one whose amplitude overflows and
one with a NaN parameter; +Inf and -Inf written into one row each, a denormal into another, and three rows of random doubles with
full mantissas (tests/test_diagnostic_cpu.py shows that they tell a fused multiply-add from the definition).  A coupled ensemble
(8 variables, 10 parameters) carries the three- and four-term cases."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

from tests import host_diagnostic as hd
from tests import host_indicators as hi
from tests import host_likelihood as hl
from tests import host_spectrum as hs
from tests import host_variability as hv
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import built_once, noise_ensemble, plant, refusal_code
from tests.helpers import annual_bounds, coupled_params, magicc_chain, same_bits, same_values, two_layer_params

pytestmark = pytest.mark.gpu

T = 72
YEARS, BOUNDS = annual_bounds(T)
SEED = 20260418
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
TILE, BATCH = 32, 4                  # kDiagTile and kDiagBatch of csrc/diagnostic.hpp
# (t_begin, t_end, t_stride): row counts around the tile and around the load batch, strides 1 and 3, a range that ends at the time index
RANGES = ([(0, R, 1) for R in (1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]
          + [(0, T, 1), (2, T, 3), (T - 5, T, 1), (1, T, 2)])
Q = [0.05, 0.5, 0.95]
# name -> terms (variable id, parameter row or None, scale); "heat" is defined through define_heat_content
TL_DIAGS = {"copy": [(1, None, 1.0)], "deep": [(2, 5, -2.5)], "heat": hd.HEAT_CONTENT, "twice": [(1, 6, -2.5), (1, None, 16.1)]}
CP_DIAGS = {"three": [(1, 0, 1.0), (3, None, -2.5), (5, 7, 16.1)], "four": [(1, 4, 1.0), (2, 5, 1.0), (3, None, 0.3), (4, 9, -2.5)]}


def _ensemble(ra, n, offset=0, n_total=None, steps=None, special_rows=True):
    e = noise_ensemble(ra, n, BOUNDS, SEED, offset, n_total, steps)
    if special_rows and e.time_index >= max(hd.RANDOM_ROWS):
        x = hd.random_rows(n, offset, n_total)
        for v in (1, 2):
            for k, row in enumerate(hd.RANDOM_ROWS):
                e.set_state(v, row, x[v - 1, k])
    return e


def _define_two_layer(e):
    ids = {}
    for name, terms in TL_DIAGS.items():
        ids[name] = e.define_heat_content(name) if name == "heat" else e.define_diagnostic(name, terms)
    return ids


def _series(e, n_vars):
    ser = {v: e.get_series(v) for v in range(1, n_vars)}
    for x in ser.values():
        x.setflags(write=False)
    return ser


def _restate(terms, ser, P, tb, te, ts):
    return hd.diagnostic(terms, [ser[v][tb:te:ts] for v, _, _ in terms], P)


@pytest.fixture(scope="module")
def cases(ra):
    """{N: (ensemble with the four diagnostics defined, {variable id: [T][N] on the host}, its parameters)}, built once."""
    def build(n):
        e = _ensemble(ra, n)
        if n >= 63:
            for member, row, value in ((5, 1, np.inf), (7, 2, -np.inf), (9, 3, 5e-324)):
                plant(e, 1, member, row, value)
        ids = _define_two_layer(e)
        assert list(ids.values()) == [3, 4, 5, 6]                      # V, V + 1, ... in order of definition
        return e, _series(e, 3), e.get_params()

    yield from built_once(build)


@pytest.mark.parametrize("n", SIZES)
def test_two_layer_diagnostics_equal_the_restatement(ra, cases, n):
    e, ser, P = cases(n)
    if n >= 63:
        assert np.isposinf(ser[1][1, 5]) and np.isneginf(ser[1][2, 7]) and ser[1][3, 9] == 5e-324
        assert np.isnan(ser[1][13:, n - 1]).all() and (ser[1][:10, n - 3] == 0.0).all() and not np.isfinite(ser[1][:, n - 2]).all()
        w = hd.weights(TL_DIAGS["twice"], P)[0]
        assert w[n - 3] == 0.0 and np.signbit(w[n - 3])                    # a weight of -0.0
    assert np.array_equal(ser[1][list(hd.RANDOM_ROWS)], hd.random_rows(n)[0]) and same_values(P, hd.two_layer_case(n)[0])
    got_def = e.diagnostics
    assert got_def["heat"]["terms"] == [(1, 4, 1.0), (2, 5, 1.0)]          # define_heat_content is the explicit definition
    for name, terms in TL_DIAGS.items():
        assert got_def[name]["terms"] == [tuple(t) for t in terms]
        for tb, te, ts in RANGES:
            e.compute_diagnostic(name, tb, te, ts)
            got = e.get_series(name, tb, te, ts)
            want = _restate(terms, ser, P, tb, te, ts)
            assert same_bits(got, want), (name, tb, te, ts, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])
            held = e.diagnostics[name]
            assert (held["rows_held"], held["t_begin"], held["t_stride"]) == (len(range(tb, te, ts)), tb, ts)
        e.compute_diagnostic(name)                                         # t_end=None: up to and including the time index
        assert e.diagnostics[name]["rows_held"] == T and same_bits(e.get_series(name), _restate(terms, ser, P, 0, T, 1))
    assert same_bits(e.get_series("copy"), ser[1])                         # 1.0 * x is x
    if n >= 63:
        heat = e.get_series("heat")
        assert np.isposinf(heat[1, 5]) and np.isneginf(heat[2, 7]) and np.isnan(heat[13:, n - 1]).all() and np.isfinite(heat[:, :5]).all()
        assert heat[3, 9] == P[4, 9] * 5e-324 + P[5, 9] * ser[2][3, 9]


def _coupled(ra, n):
    P = coupled_params(n)
    E = np.interp(np.arange(T, dtype=np.float64), [0, 30, 71], [0.0, 4.0, 9.0])
    e = ra.Ensemble(ra.KIND_COUPLED, n, BOUNDS)
    e.set_params(P)
    e.set_forcing(E)
    for v, x in ((1, 0.0), (2, 0.0), (3, 278.0), (4, 0.0), (5, 0.0)):
        e.set_initial(v, x)
    e.run()
    return e


@pytest.mark.parametrize("n", SIZES)
def test_coupled_diagnostics_of_three_and_four_terms(ra, n):
    with _coupled(ra, n) as e:
        x = hd.random_case(4, n)[1]                                        # random rows in four variables: an fma or another order would show
        for v in (1, 2, 3, 4):
            for k, row in enumerate(hd.RANDOM_ROWS):
                e.set_state(v, row, x[v - 1, k])
        ser, P = _series(e, 8), e.get_params()
        assert P.shape == (10, n)
        for name, terms in CP_DIAGS.items():
            assert e.define_diagnostic(name, terms) == 8 + list(CP_DIAGS).index(name)
            assert len({v for v, _, _ in terms}) == len(terms)             # distinct variables
            for tb, te, ts in RANGES:
                e.compute_diagnostic(name, tb, te, ts)
                got, want = e.get_series(name, tb, te, ts), _restate(terms, ser, P, tb, te, ts)
                assert same_bits(got, want), (name, tb, te, ts)
        four = [(v, r, s) for v, r, s in CP_DIAGS["four"]]
        rows = list(hd.RANDOM_ROWS)
        if n >= 64:                                                        # the order matters on this data
            assert not same_bits(hd.diagnostic_right_to_left(four, [ser[v][rows] for v, _, _ in four], P),
                                  hd.diagnostic(four, [ser[v][rows] for v, _, _ in four], P))


# ---------------------------------------------------------------------------------------------- every consumer reads it
def _np_q(rows):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(np.asarray(rows), Q, axis=1).T


def _np_wq(rows, w):
    rows = np.asarray(rows)
    W = ((~np.isnan(rows)) * w[None, :]).sum(axis=1)
    out = np.full((rows.shape[0], len(Q)), np.nan)
    live = W > 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sub = rows[live]
        out[live] = np.nanquantile(sub, Q, axis=1, weights=np.broadcast_to(w, sub.shape), method="inverted_cdf").T
    return out, W


def test_every_consumer_reads_the_diagnostic(ra, cases):
    n, R = 257, 48
    e, ser, P = cases(n)
    vid = e.var_ids["heat"]
    e.compute_diagnostic("heat", 0, R)
    H = _restate(hd.HEAT_CONTENT, ser, P, 0, R, 1)
    assert same_bits(e.get_series("heat", 0, R), H) and same_bits(e.get_series(vid, 4, R, 5, 3, 200), H[4:R:5, 3:200])
    assert np.isnan(H).any() and np.isinf(H).any()
    # the selects: plain, weighted, anomaly, grouped
    got = e.quantile_rows("heat", Q, 0, R)
    assert same_values(got["quantiles"], _np_q(H)) and np.array_equal(got["count"], (~np.isnan(H)).sum(axis=1))
    strided = e.quantile_rows(vid, Q, 1, R, 3)
    assert same_values(strided["quantiles"], _np_q(H[1:R:3]))
    rng = np.random.default_rng(n)
    w = rng.integers(1, 1 << 30, n, dtype=np.int64)
    w[rng.random(n) < 0.2] = 0
    e.set_member_weights(w)
    wq = e.quantile_rows("heat", Q, 0, R, weighted=True)
    want, W = _np_wq(H, w)
    assert same_values(wq["quantiles"], want) and np.array_equal(wq["weight"], W)
    e.set_baseline("heat", 5, 15)
    b = hi.baseline(H[5:15])
    assert same_values(e.baseline(), b)
    a = hi.anomaly(H, b)
    aq = e.quantile_rows("heat", Q, 0, R, anomaly=True)
    assert same_values(aq["quantiles"], _np_q(a)) and np.array_equal(aq["count"], (~np.isnan(a)).sum(axis=1))
    group = (np.arange(n) % 3).astype(np.int32)
    e.set_member_groups(group, 3)
    gq = e.quantile_rows("heat", Q, 0, R, grouped=True)
    assert gq["quantiles"].shape == (3, R, len(Q))
    for g in range(3):
        assert same_values(gq["quantiles"][g], _np_q(H[:, group == g])), g
    with e.select("heat", Q, 0, R) as s:                                   # the staged form
        while s.next_pass() is not None:
            s.commit()
        assert same_values(s.result()["quantiles"], _np_q(H))
    e.clear_member_groups()
    e.clear_baseline()
    # the per-member statistics
    thr = [float(np.nanmedian(H[R - 1]))]
    ind = e.indicators("heat", 0, R, thresholds=thr)
    want = hi.indicators(H, YEARS[:R], thr)
    assert all(same_values(ind[k].to_host(), want[k]) for k in ("mean", "peak", "peak_time")) and same_values(ind["crossing"][0].to_host(), want["crossing"][0])
    for d in ("mean", "linear", "difference"):
        got, want = e.variability("heat", 0, R, detrend=d), hv.variability(H, d)
        for k in hv.NAMES:
            assert same_values(got[k].to_host(), want[k]), (d, k)
    sp = e.spectrum("heat", 0, R, detrend="difference", bands=3)
    want = hs.spectrum(H, "difference", sp["edges"])
    for k in hs.FIRST:
        assert same_values(sp[k].to_host(), want[k]), k
    assert all(same_values(p.to_host(), q) for p, q in zip(sp["power"], want["power"]))
    # the stored likelihoods: bit for bit without the normalisation's logarithm, within its bound (rtol 1e-13, as the stored
    # likelihood's own tests) with it
    tidx = list(range(4, R, 4))
    obs = [float(np.nanmedian(H[t])) for t in tidx]
    sig = [float(0.3 * np.nanstd(np.where(np.isfinite(H[t]), H[t], np.nan))) + 1e-3 for t in tidx]
    for reference in (None, {"heat": (5, 15)}):
        href = None if reference is None else {vid: (5, 15)}
        for normalize in (False, True):
            got = e.loglik(["heat"] * len(tidx), tidx, obs, sig, normalize, reference=reference)
            want = hl.loglik({vid: H}, [vid] * len(tidx), tidx, obs, sig, normalize, href)
            assert (np.isneginf(got) == np.isneginf(want)).all() and np.isneginf(want).any() and np.isfinite(want).sum() > n // 2
            fin = np.isfinite(want)
            if normalize:
                assert np.allclose(got[fin], want[fin], rtol=1e-13, atol=0)
            else:
                assert np.array_equal(got, want)
        dev = e.loglik(["heat"] * len(tidx), tidx, obs, sig, on_device=True, reference=reference)
        assert np.array_equal(dev.to_host(), hl.loglik({vid: H}, [vid] * len(tidx), tidx, obs, sig, False, href))
    # a diagnostic and a stored variable in one observation list
    both = e.loglik(["Surface Temperature", "Surface Temperature", "heat"], [8, 20, 20], [0.1, 0.2, obs[4]], [0.5, 0.5, sig[4]])
    assert np.array_equal(both, hl.loglik({1: ser[1], vid: H}, [1, 1, vid], [8, 20, 20], [0.1, 0.2, obs[4]], [0.5, 0.5, sig[4]]))
    # the summary: the finite members' count, min and max exactly; the mean within the error of a sum of n terms in any order,
    # n 2^-53 sum|x| (the device adds by a tree, the reference exactly), and two more roundings for the two divisions
    row = H[20]
    fin = np.isfinite(row)
    s = e.summary("heat", 20)
    assert s["count"] == fin.sum() and s["min"] == row[fin].min() and s["max"] == row[fin].max()
    assert abs(s["mean"] - math.fsum(row[fin]) / fin.sum()) <= (n + 2) * 2.0 ** -53 * np.abs(row[fin]).sum() / fin.sum()


# ---------------------------------------------------------------------------------------------- storage layouts
def test_windowed_graph_with_an_output_store(ra):
    """A windowed graph that keeps every 12th row: a diagnostic over two carbon pools of one ensemble, by names, from rows in the
    output store and rows in the window; a range with a row that is no longer resident is refused and the rows held stay."""
    model = magicc_chain().build_chain(65, 30, "topological", steps_per_year=12, series_window=16, output_stride=12)
    try:
        model.run()
        plant_pool, soil = "Carbon Pool|Plant", "Carbon Pool|Soil"
        ens, v_plant = model.variable_home(plant_pool)
        assert model.variable_home(soil)[0] is ens
        with pytest.raises(ValueError, match="share one home"):
            model.define_diagnostic("mixed", [(plant_pool, None), ("Atmospheric Concentration|CO2", None)])
        with pytest.raises(ValueError, match="no parameter of"):
            model.define_diagnostic("wrong", [(plant_pool, "CO2Budget.gtc_per_ppm")])
        vid = model.define_diagnostic("pools", [(plant_pool, "TerrestrialCarbon.beta", 2.0), (soil, None)])
        assert model.variable_home("pools") == (ens, vid) and vid == ens.n_vars
        beta = ens.get_params()[model.param_home["TerrestrialCarbon.beta"][1]]
        terms = [(0, 0, 2.0), (1, None, 1.0)]
        n_times = ens.n_times
        model.compute_diagnostic("pools", 0, n_times, 12)                  # the output store, and the last row from the window
        want = hd.diagnostic(terms, [model.get_series(plant_pool, t_stride=12), model.get_series(soil, t_stride=12)], beta[None, :])
        assert same_bits(model.get_series("pools", t_stride=12), want) and np.isfinite(want).any()
        got = model.variability("pools", 0, n_times, 12, detrend="difference")
        ref = hv.variability(want, "difference")
        assert all(same_values(got[k].to_host(), ref[k]) for k in hv.NAMES)
        q = model.quantile_rows("pools", Q, t_stride=12)
        assert same_values(q["quantiles"], _np_q(want))
        assert refusal_code(model.compute_diagnostic, "pools", 0, 9, 3) == 2      # rows 3 and 6 of the sources are not resident any more
        assert ens.diagnostics["pools"]["rows_held"] == len(want) and same_bits(model.get_series("pools", t_stride=12), want)
        k = model.time_index
        w0 = k - 1
        model.compute_diagnostic("pools", w0)                              # the window's last rows, up to the current step
        win = hd.diagnostic(terms, [model.get_series(plant_pool, t_begin=w0, t_end=k + 1), model.get_series(soil, t_begin=w0, t_end=k + 1)], beta[None, :])
        assert same_bits(model.get_series("pools", t_begin=w0, t_end=k + 1), win)
        assert refusal_code(model.get_series, "pools", t_stride=12) == 2          # the strided range is held no longer
    finally:
        model.close()


# ---------------------------------------------------------------------------------------------- staleness
def test_rows_go_stale_with_every_writer_and_come_back_with_a_compute(ra):
    n = 65
    with _ensemble(ra, n, steps=40) as e, _ensemble(ra, n, steps=40) as src:
        vid = e.define_heat_content()
        definition = e.diagnostics["Ocean Heat Content"]["terms"]
        ck = e.checkpoint()

        def fresh(what):
            k = e.time_index
            e.compute_diagnostic(vid)
            H = hd.diagnostic(hd.HEAT_CONTENT, [e.get_series(1, 0, k + 1), e.get_series(2, 0, k + 1)], e.get_params())
            assert same_bits(e.get_series(vid, 0, k + 1), H), what
            assert e.diagnostics["Ocean Heat Content"]["rows_held"] == k + 1
            return H

        def stale(what):
            assert refusal_code(e.summary, vid, 0) == 2, what
            assert refusal_code(e.get_series, vid, 0, 1) == 2 and refusal_code(e.quantile_rows, vid, Q, 0, 1) == 2, what
            assert refusal_code(e.loglik, [vid], [0], [0.0], [1.0]) == 2 and refusal_code(e.indicators, vid, 0, 1) == 2, what
            from rscm_amd._lib import RscmGpuError
            with pytest.raises(RscmGpuError, match="is stale: compute it again"):
                e.set_baseline(vid, 0, 1)
            d = e.diagnostics["Ocean Heat Content"]
            assert d["terms"] == definition and d["rows_held"] == 0, what  # the definition survives, the rows do not

        first = fresh("first")
        # what hands out pointers does not move the epoch
        e.params_vector(4)
        e.series_devptr(1)
        assert same_bits(e.get_series(vid, 0, 41), first) and e.summary(vid, 40)["count"] > 0
        writers = {
            "run": lambda: e.run(50),
            "rewind": lambda: e.rewind(),
            "set_params": lambda: e.set_params(e.get_params() * 1.0),
            "set_state": lambda: e.set_state(1, 0, 0.25),
            "sample_lhs": lambda: e.sample_lhs(3, [0.8, 0.0, 1.0, 0.5, 5.0, 50.0, 0.1, 0.0], [1.5, 0.1, 1.8, 1.0, 15.0, 200.0, 0.6, 0.9]),
            "restore": lambda: e.restore(ck),
            "branch": lambda: src.branch(e, np.arange(n, dtype=np.int64)),
            "set_forcing_noise_members": lambda: e.set_forcing_noise_members(SEED + 1),
        }
        for what, write in writers.items():
            write()
            stale(what)
            fresh(what)
        e.run()                                                            # and a run with the new noise, to the end
        stale("run to the end")
        assert fresh("the end").shape == (T, n)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(ra):
    n = 64
    lib_q = [0.5]
    with _ensemble(ra, n) as e:
        # definitions
        assert refusal_code(e.define_diagnostic, "none", []) == 1
        assert refusal_code(e.define_diagnostic, "five", [(1, None)] * 5) == 1
        for var in (0, 3, -1):
            assert refusal_code(e.define_diagnostic, "var", [(var, None)]) == 1
        for row in (-2, 8):
            assert refusal_code(e.define_diagnostic, "row", [(1, row)]) == 1
        for scale in (np.nan, np.inf, -np.inf):
            assert refusal_code(e.define_diagnostic, "scale", [(1, None, scale)]) == 1
        assert e.diagnostics == {} and set(e.var_ids) == {"Effective Radiative Forcing", "Surface Temperature", "Deep Ocean Temperature"}
        ids = [e.define_diagnostic(f"d{k}", [(1, k, 1.0)]) for k in range(4)]
        assert ids == [3, 4, 5, 6]
        n_diag = C.c_int32()
        assert e._lib.rscm_ens_n_diagnostics(e._h, C.byref(n_diag)) == 0 and n_diag.value == 4
        n_vars = C.c_int32()
        assert e._lib.rscm_ens_n_vars(e._h, C.byref(n_vars)) == 0 and n_vars.value == 3
        assert refusal_code(e.define_diagnostic, "fifth", [(1, None)]) == 1 and "fifth" not in e.var_ids
        assert refusal_code(e.define_diagnostic, "of a diagnostic", [(3, None)]) == 1
        with pytest.raises(ValueError):
            e.define_diagnostic("d0", [(1, None)])                         # the name is taken
        with pytest.raises(ValueError):
            e.define_diagnostic("by name", [("d0", None)])
        # ranges and ids
        for tb, te, ts in ((5, 3, 1), (0, T + 1, 1), (4, 4, 1), (0, 10, 0), (-1, 4, 1)):
            assert refusal_code(e.compute_diagnostic, "d0", tb, te, ts) == 1, (tb, te, ts)
        for var in (1, 0, 7, 99, -1):
            assert refusal_code(e.compute_diagnostic, var, 0, 4) == 1
            assert e._lib.rscm_ens_diagnostic(e._h, var, None, None, None, None, None, None, None) == 1
        # a consumer on rows outside the held range; a diagnostic never computed
        assert refusal_code(e.get_series, "d1", 0, 4) == 2 and refusal_code(e.variability, "d1", 0, 10) == 2
        e.compute_diagnostic("d0", 0, 20)
        e.variability("d0", 0, 20)
        assert refusal_code(e.variability, "d0", 0, 30) == 2 and refusal_code(e.get_series, "d0", 0, 30) == 2 and refusal_code(e.summary, "d0", 25) == 2
        assert refusal_code(e.quantile_rows, "d0", lib_q, 0, 30) == 2 and refusal_code(e.loglik, ["d0"], [25], [0.0], [1.0]) == 2
        assert refusal_code(e.loglik, ["d0"], [5], [0.0], [1.0], reference={"d0": (15, 25)}) == 2
        assert refusal_code(e.set_baseline, "d0", 18, 22) == 2 and refusal_code(e.spectrum, "d0", 10, 40) == 2
        e.compute_diagnostic("d0", 0, 30, 3)
        assert refusal_code(e.indicators, "d0", 0, 30) == 2                        # row 1 is not one of the strided rows
        e.indicators("d0", 0, 30, 3)
        # who keeps refusing the id
        assert refusal_code(e.series_devptr, "d0") == 1 and refusal_code(e.summary_series, "d0") == 1 and refusal_code(e.quantile_series, "d0", lib_q) == 1
        assert refusal_code(e.set_state, "d0", 3, 0.0) == 1 and refusal_code(e.set_initial, "d0", 0.0) == 1
        # a select in flight: define, compute and clear all refuse
        with e.select("d0", lib_q, 0, 30, 3) as s:
            assert refusal_code(e.compute_diagnostic, "d0", 0, 10) == 2 and refusal_code(e.clear_diagnostics) == 2
            while s.next_pass() is not None:
                s.commit()
        e.clear_diagnostics()
        assert e.diagnostics == {} and "d0" not in e.var_ids and refusal_code(e.compute_diagnostic, 3, 0, 4) == 1
        with e.select(1, lib_q, 0, 30) as s:
            assert refusal_code(e.define_diagnostic, "late", [(1, None)]) == 2 and "late" not in e.var_ids
            while s.next_pass() is not None:
                s.commit()
        assert e.define_diagnostic("again", [(2, None)]) == 3               # the id is free again
        with pytest.raises(ValueError):
            ra.Ensemble.define_heat_content(e, "again")
    # rows beyond the time index; a handle that stores only its initial row
    with _ensemble(ra, n, steps=10) as e:
        vid = e.define_heat_content()
        assert refusal_code(e.compute_diagnostic, vid, 0, 20) == 2
        e.compute_diagnostic(vid)
        assert e.diagnostics["Ocean Heat Content"]["rows_held"] == 11
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS, store_series=False) as e:
        e.set_params(two_layer_params(n))
        e.set_forcing(0.05 * np.arange(T))
        e.set_initial(1, 0.5)
        e.set_initial(2, 0.25)
        vid = e.define_heat_content()
        assert refusal_code(e.compute_diagnostic, vid, 0, 2) == 2
        e.compute_diagnostic(vid, 0, 1)
        P = e.get_params()
        assert same_bits(e.get_series(vid, 0, 1)[0], P[4] * 0.5 + P[5] * 0.25)
    with ra.Ensemble(ra.KIND_UDEB, 4, BOUNDS) as e:
        with pytest.raises(ValueError):
            e.define_heat_content()


def test_linked_inputs_fused_runs_and_samplers_refuse_a_diagnostic(ra):
    n = 64
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS) as e, ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS) as consumer:
        e.set_params(two_layer_params(n))
        e.set_forcing(0.05 * np.arange(T))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.run()
        vid = e.define_heat_content()
        e.compute_diagnostic(vid)
        assert refusal_code(consumer.link_input, 0, e, vid) == 1
        assert refusal_code(e.run_loglik, [vid], [5], [0.0], [1.0]) == 1
        assert e.diagnostics["Ocean Heat Content"]["rows_held"] == T        # (neither call ran anything)
        e.rewind()                                                         # (the fused run starts from index 0)
        e.compute_diagnostic(vid, 0, 1)
        assert e.summary(vid, 0)["count"] == n
        e.run_loglik([1], [5], [0.0], [1.0])                               # the fused run leaves the time index alone, but it is a run
        assert refusal_code(e.summary, vid, 0) == 2
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    axis = core.TimeAxis.from_values(YEARS)
    b = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
         .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(0.05 * np.arange(T), axis, "W/m^2", core.InterpolationStrategy.Linear))
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0})
         .with_diagnostic("Ocean Heat Content", {"Surface Temperature": "heat_capacity_surface", "Deep Ocean Temperature": "heat_capacity_deep"}))
    model = b.build(n_members=8)
    try:
        model.run()
        ens = model.ensemble
        assert ens.diagnostics["Ocean Heat Content"]["terms"] == [(1, 4, 1.0), (2, 5, 1.0)]
        ens.compute_diagnostic("Ocean Heat Content")
        want = 8.0 * ens.get_series(1) + 100.0 * ens.get_series(2)
        assert same_bits(ens.get_series("Ocean Heat Content"), want)
        assert "Ocean Heat Content" not in model.timeseries().names()
    finally:
        model.close()
    with pytest.raises(ValueError, match="diagnostic"):
        cal.ModelRunner(b, ["lambda0"], ["Ocean Heat Content"])
    runner = cal.ModelRunner(b, ["lambda0"], ["Surface Temperature"])
    target = cal.Target()
    target.add_observation("Ocean Heat Content", 1860.0, 1.0, 0.5)
    params = cal.ParameterSet().add("lambda0", cal.Uniform(0.8, 1.6))
    for sampler in (cal.DeviceEnsembleSampler, cal.EnsembleSampler):
        with pytest.raises(ValueError, match="compute_diagnostic"):
            sampler(params, runner, cal.GaussianLikelihood(), target)
    with pytest.raises(ValueError, match="compute_diagnostic"):
        runner.log_likelihood_batch(np.array([[1.1]]), target, cal.GaussianLikelihood())


# ---------------------------------------------------------------------------------------------- shards and posteriors
def test_two_shards_give_the_halves(ra, cases):
    n, k = 257, 129
    e, ser, P = cases(n)
    e.compute_diagnostic("heat", 13, T)                                    # (the rows from 13 on: none was overwritten)
    whole = e.get_series("heat", 13, T)
    for offset, count in ((0, k), (k, n - k)):
        with _ensemble(ra, count, offset, n, special_rows=False) as h:
            vid = h.define_heat_content("heat")
            h.compute_diagnostic(vid, 13, T)
            assert same_bits(h.get_series(vid, 13, T), whole[:, offset:offset + count]), offset
    # ShardedEnsemble forwards define and compute to its block; the global select and constrain() then take the name
    from rscm_amd.distributed import ShardedEnsemble
    sh = ShardedEnsemble(n, lambda count, device: _ensemble(ra, count, special_rows=False), rank=0, world=1)
    try:
        vid = sh.define_diagnostic("heat", [("Surface Temperature", 4), ("Deep Ocean Temperature", 5)])
        sh.compute_diagnostic("heat", 13, T)
        assert same_bits(sh.ensemble.get_series(vid, 13, T), whole)
        got = sh.quantile_rows_global("heat", Q, 13, T)
        assert same_values(got["quantiles"], _np_q(whole)) and np.array_equal(got["count"], (~np.isnan(whole)).sum(axis=1))
        tidx, obs = [20, 40], [float(np.nanmedian(whole[20 - 13])), float(np.nanmedian(whole[40 - 13]))]
        ll_max, bits = sh.constrain(["heat"] * 2, tidx, obs, [5.0, 5.0])
        want = hl.loglik({vid: np.vstack([np.full((13, n), np.nan), whole])}, [vid] * 2, tidx, obs, [5.0, 5.0])
        assert ll_max == want[np.isfinite(want) & (sh.ensemble.status() == 0)].max() and sh.ensemble.member_weights().max() == 2 ** bits
        wq = sh.quantile_rows_global("heat", Q, 13, T, weighted=True)
        assert same_values(wq["quantiles"], _np_wq(whole, sh.ensemble.member_weights())[0])
    finally:
        sh.ensemble.close()


def test_a_posterior_defines_what_its_source_defines(ra, cases):
    e, ser, P = cases(257)
    e.set_member_weights(np.where(np.isfinite(ser[1]).all(axis=0), 1, 0).astype(np.int64))

    def factory(count):
        d = ra.Ensemble(ra.KIND_TWO_LAYER, count, BOUNDS, noise_params=True)
        d.set_forcing(np.stack([np.zeros(T), 0.05 * np.arange(T)]), np.ones(count, dtype=np.int32))
        return d

    dst, _ = e.posterior(factory, 40, seed=1)
    try:
        assert {k: v["terms"] for k, v in dst.diagnostics.items()} == {k: [tuple(t) for t in v] for k, v in TL_DIAGS.items()}
        assert all(v["rows_held"] == 0 for v in dst.diagnostics.values()) and dst.time_index == T - 1
        dst.compute_diagnostic("heat", T - 1, T)
        want = hd.diagnostic(hd.HEAT_CONTENT, [dst.get_series(1, T - 1, T), dst.get_series(2, T - 1, T)], dst.get_params())
        assert same_bits(dst.get_series("heat", T - 1, T), want)
    finally:
        dst.close()
