"""GPU tier of the energy-budget diagnostics (csrc/energy_budget.hip, csrc/energy_budget_host.cpp; rscm_ens_define_energy_budget,
rscm_ens_diagnostic_quantity, rscm_ens_compute_diagnostic; Ensemble.define_energy_budget, define_toa_imbalance).  The oracle is the
numpy restatement of tests/host_energy_budget.py applied to rows fetched with get_series, parameters fetched with get_params and
the member forcing of the existing restatements (host_forcing_mix, host_forcing_noise, _red, _members), compared bit for bit (any
NaN equal to any NaN).

The data: two-layer ensembles on a 72-point annual axis with the parameters of host_diagnostic.two_layer_case -- from 63 members
on a silent one, one whose noise amplitude (on a mix handle: first coefficient) overflows and one with a NaN parameter -- and three
rows of random doubles with full mantissas written into both stored variables (tests/test_energy_budget_cpu.py shows that they tell
another association of the imbalance from the definition)."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from tests import host_covariability as hc
from tests import host_cross_spectrum as hx
from tests import host_diagnostic as hd
from tests import host_energy_budget as hb
from tests import host_indicators as hi
from tests import host_likelihood as hl
from tests import host_spectrum as hs
from tests import host_variability as hv
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import annual_bounds, same_bits, same_values, two_layer_params

pytestmark = pytest.mark.gpu

T = 72
YEARS, BOUNDS = annual_bounds(T)
SEED = 20260422
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
_HPP = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rscm_amd", "csrc", "diagnostic.hpp")).read()
TILE = int(re.search(r"kDiagTile\s*=\s*(\d+)", _HPP).group(1))      # rows a block walks
BATCH = int(re.search(r"kDiagBatch\s*=\s*(\d+)", _HPP).group(1))    # rows whose loads are issued before use
# (t_begin, t_end, t_stride): row counts around the load batch and the tile, the whole axis, one strided range, the last rows
RANGES = ([(0, R, 1) for R in (1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]
          + [(0, T, 1), (2, T, 3), (T - 5, T, 1)])
Q = [0.05, 0.5, 0.95]
TS, TD = 1, 2


def _table(K):
    """[2][T] of a plain handle, [2][K][T] of a mix handle: scenario 0 is zero forcing on a plain handle (the silent member's)."""
    if not K:
        return np.stack([np.zeros(T), 0.05 * np.arange(T)])
    rng = np.random.default_rng(100 + K)
    return rng.uniform(-1.0, 2.0, (2, K, T))                                # full mantissas: the order of the mix sum shows


def _params(n, K, members, offset=0, n_total=None):
    """([6 + K (+ 2)][n], scenario [n]): two_layer_case's six parameters, K coefficient rows -- the first is the case's amplitude row
    with its 0.0 and its 1.7e308 -- and, for the per-member noise, its two noise rows."""
    n_total = n if n_total is None else n_total
    P8, scen = hd.two_layer_case(n, offset, n_total)
    rows = [P8[:6]]
    if K:
        rng = np.random.default_rng(9000 + n_total + K)
        rows += [P8[6:7], rng.uniform(-1.0, 1.5, (K - 1, n_total))[:, offset:offset + n]]
    if members:
        rows.append(P8[6:8])
    return np.ascontiguousarray(np.vstack(rows)), scen


class Case:
    """One ensemble run to `steps` with its host copy of rows, parameters and member forcing."""

    def __init__(self, ra, n, K=0, noise=None, offset=0, n_total=None, source=None, fast=False, steps=None, random_rows=True):
        members = noise is not None and noise[0] == "members"
        self.n, self.K, self.noise, self.offset = n, K, noise, offset
        self.off = 1 if source == ra.SRC_UPSTREAM else 0
        P, self.scen = _params(n, K, members, offset, n_total)
        self.table = _table(K)
        e = self.e = ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS, forcing_components=K or None, noise_params=members)
        if fast:
            e.set_mode(ra.MODE_FAST)
        e.set_params(P)
        e.set_forcing(self.table, self.scen, source=ra.SRC_EXOGENOUS if source is None else source)
        e.set_initial(TS, 0.0)
        e.set_initial(TD, 0.0)
        if noise is not None:
            if noise[0] == "members":
                e.set_forcing_noise_members(noise[1], offset)
            else:
                e.set_forcing_noise(noise[2], noise[1], offset, phi=noise[3] if noise[0] == "red" else 0.0)
        e.run(steps)
        if random_rows and e.time_index >= max(hd.RANDOM_ROWS):
            x = hd.random_rows(n, offset, n_total)
            for v in (TS, TD):
                for k, row in enumerate(hd.RANDOM_ROWS):
                    e.set_state(v, row, x[v - 1, k])
        self.refresh()

    def refresh(self):
        e = self.e
        k = e.time_index
        self.P = e.get_params()
        self.ts = np.full((T, self.n), np.nan)
        self.td = np.full((T, self.n), np.nan)
        self.ts[:k + 1], self.td[:k + 1] = e.get_series(TS, 0, k + 1), e.get_series(TD, 0, k + 1)
        self.F = hb.member_forcing(self.table, self.P, self.scen, self.K, self.noise, self.offset)     # [N][T]
        for x in (self.ts, self.td, self.F):
            x.setflags(write=False)

    def want(self, quantity, tb, te, ts, scale=1.0):
        idx = np.arange(tb, te, ts)
        F = np.full((len(idx), self.n), np.nan)
        ok = idx + self.off < T
        F[ok] = self.F[:, idx[ok] + self.off].T
        return hb.budget(quantity, self.ts[tb:te:ts], self.td[tb:te:ts], self.P, F, scale)

    def check(self, ids, ranges=RANGES, scale=1.0):
        e = self.e
        for quantity, vid in ids.items():
            for tb, te, ts in ranges:
                e.compute_diagnostic(vid, tb, te, ts)
                got, want = e.get_series(vid, tb, te, ts), self.want(quantity, tb, te, ts, scale)
                assert same_bits(got, want), (quantity, tb, te, ts, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])
                held = e.diagnostics[e_name(e, vid)]
                assert (held["rows_held"], held["t_begin"], held["t_stride"]) == (len(range(tb, te, ts)), tb, ts)

    def close(self):
        self.e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def e_name(e, vid):
    return next(k for k, v in e._diagnostic_names.items() if v == vid)


def _define_all(e, scale=1.0):
    return {q: e.define_energy_budget(q, scale=scale) for q in hb.QUANTITIES}


def _special_members(c):
    """What two_layer_case promises from 63 members on, seen in the budget's own rows."""
    n = c.n
    if n < 63:
        return
    assert np.isnan(c.P[0, n - 1]) and np.isnan(c.want("imbalance", 0, T, 1)[:, n - 1]).all()
    assert np.isnan(c.want("response", 0, T, 1)[1:, n - 1]).all()
    if c.K:
        assert not np.isfinite(c.want("forcing", 0, T, 1)[:, n - 2]).all()      # the coefficient 1.7e308 overflows the mix sum


# ---------------------------------------------------------------------------------------------- bit-exact against the restatement
@pytest.mark.parametrize("n", SIZES)
def test_plain_handle_with_two_scenarios(ra, n):
    with Case(ra, n) as c:
        ids = _define_all(c.e)
        assert list(ids.values()) == [3, 4, 5, 6]
        d = c.e.diagnostics
        assert [d[k]["quantity"] for k in ("Member Forcing", "Radiative Response", "Deep Ocean Heat Uptake", "Top of Atmosphere Imbalance")] \
            == list(hb.QUANTITIES)
        assert all(v["terms"] == [] and v["scale"] == 1.0 for v in d.values())
        c.check(ids)
        _special_members(c)
        # on a plain handle the forcing is the member's scenario's table value, exactly; the last row is served (index T - 1 exists)
        c.e.compute_diagnostic("Member Forcing", 0, T)
        assert same_bits(c.e.get_series("Member Forcing"), c.table[c.scen].T)
        if n >= 64:
            rows = list(hd.RANDOM_ROWS)
            wrong = hb.imbalance_wrong_association(c.ts[rows], c.td[rows], c.P, c.F[:, rows].T)
            assert not same_bits(wrong, c.want("imbalance", 10, 13, 1))        # the association matters on this data


@pytest.mark.parametrize("n", SIZES)
def test_mix_handle_with_three_components(ra, n):
    with Case(ra, n, K=3) as c:
        assert c.P.shape == (9, n)
        c.check(_define_all(c.e))
        _special_members(c)


def test_mix_handle_with_eight_components(ra):
    with Case(ra, 65, K=8) as c:
        c.check(_define_all(c.e))
        _special_members(c)


NOISES = {"white": ("white", SEED, 0.3), "red": ("red", SEED + 1, 0.3, 0.6), "members": ("members", SEED + 2)}


@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("kind", list(NOISES))
def test_noise_kinds_on_a_plain_and_on_a_mix_handle(ra, kind, K):
    n = 257
    offset, n_total = (1000, 1000 + n) if (kind, K) == ("red", 3) else (0, None)     # a non-zero member_offset once
    with Case(ra, n, K=K, noise=NOISES[kind], offset=offset, n_total=n_total) as c:
        ids = _define_all(c.e)
        c.check(ids)
        _special_members(c)
        # against existing device code: the forcing rows are the shared forcing plus forcing_noise_rows(), bit for bit
        base = hb.member_forcing(c.table, c.P, c.scen, K)                   # [N][T] without the noise
        c.e.compute_diagnostic(ids["forcing"], 0, T)
        with np.errstate(all="ignore"):
            assert same_bits(c.e.get_series(ids["forcing"]), base.T + c.e.forcing_noise_rows(0, T))
        assert not same_bits(c.e.get_series(ids["forcing"])[:, :5], base.T[:, :5])


def test_upstream_source_reads_the_next_index(ra):
    with Case(ra, 65, source=ra.SRC_UPSTREAM) as c:
        assert c.off == 1
        ids = _define_all(c.e)
        ranges = [(tb, min(te, T - 1), ts) for tb, te, ts in RANGES if tb < T - 1]      # no step leaves the last row
        c.check({q: ids[q] for q in ("forcing", "imbalance")}, ranges)
        c.check({q: ids[q] for q in ("response", "deep_uptake")})
        c.e.compute_diagnostic(ids["forcing"], 0, T - 1)
        assert same_bits(c.e.get_series(ids["forcing"], 0, T - 1), c.table[c.scen].T[1:])
        for q in ("forcing", "imbalance"):
            c.e.compute_diagnostic(ids[q], 0, T - 1)
            assert refusal_code(c.e.compute_diagnostic, ids[q], 0, T) == 1 and refusal_code(c.e.compute_diagnostic, ids[q], T - 1, T) == 1
            assert c.e.diagnostics[e_name(c.e, ids[q])]["rows_held"] == T - 1           # a refused compute leaves the rows held
        c.e.compute_diagnostic(ids["response"], T - 1, T)


def test_fast_mode_gives_the_same_bits_from_the_same_stored_rows(ra):
    with Case(ra, 65, fast=True) as c:
        c.check(_define_all(c.e))                                           # the statements do not depend on the arithmetic mode


def test_a_scale_is_one_more_rounding(ra):
    with Case(ra, 257, K=3, noise=NOISES["white"]) as c:
        c.check(_define_all(c.e, scale=-2.5), scale=-2.5)
        assert c.e.diagnostics["Member Forcing"]["scale"] == -2.5


def test_the_response_without_curvature_is_the_linear_diagnostic(ra):
    n = 257
    with Case(ra, n, random_rows=False) as c:
        e = c.e
        P = c.P.copy()
        P[1] = 0.0
        e.set_params(P)
        e.rewind()
        e.run()
        x = hd.random_rows(n)
        for k, row in enumerate(hd.RANDOM_ROWS):
            e.set_state(TS, row, x[0, k])
        r, lin = e.define_energy_budget("response"), e.define_diagnostic("lambda0 Ts", [(TS, 0, 1.0)])
        e.compute_diagnostic(r, 0, T)
        e.compute_diagnostic(lin, 0, T)
        assert same_bits(e.get_series(r), e.get_series(lin)) and np.isfinite(e.get_series(r)[:, :5]).all()
        assert e.diagnostics["lambda0 Ts"]["quantity"] is None and e.diagnostics["lambda0 Ts"]["scale"] is None
        q, s = C.c_int32(-1), C.c_double(-1.0)
        assert e._lib.rscm_ens_diagnostic_quantity(e._h, lin, C.byref(q), C.byref(s)) == 0 and (q.value, s.value) == (0, 0.0)
        n_terms = C.c_int32(-1)
        tv, tr, tsc = np.full(4, 9, dtype=np.int32), np.full(4, 9, dtype=np.int32), np.full(4, 9.0)
        from rscm_amd import _lib as L
        assert e._lib.rscm_ens_diagnostic(e._h, r, C.byref(n_terms), L.iptr(tv), L.iptr(tr), L.dptr(tsc), None, None, None) == 0
        assert n_terms.value == 0 and list(tv) == [0] * 4 and list(tr) == [-1] * 4 and list(tsc) == [0.0] * 4


# ---------------------------------------------------------------------------------------------- every consumer reads it
def _np_q(rows):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(np.asarray(rows), Q, axis=1).T


@pytest.fixture(scope="module")
def noisy(ra):
    """257 members under per-member noise with the imbalance defined and computed over 48 rows; its host copy beside it."""
    c = Case(ra, 257, noise=NOISES["members"])
    vid = c.e.define_toa_imbalance()
    c.e.compute_diagnostic(vid, 0, 48)
    N = c.want("imbalance", 0, 48, 1)
    N.setflags(write=False)
    yield c, vid, N
    c.close()


def test_the_selects_read_the_imbalance(noisy):
    c, vid, N = noisy
    e, n, R, name = c.e, c.n, 48, "Top of Atmosphere Imbalance"
    assert e.var_ids[name] == vid and same_bits(e.get_series(name, 0, R), N) and same_bits(e.get_series(vid, 4, R, 5, 3, 200), N[4:R:5, 3:200])
    assert np.isnan(N).any() and np.isfinite(N[:, :5]).all()
    got = e.quantile_rows(name, Q, 0, R)
    assert same_values(got["quantiles"], _np_q(N)) and np.array_equal(got["count"], (~np.isnan(N)).sum(axis=1))
    group = (np.arange(n) % 3).astype(np.int32)
    e.set_member_groups(group, 3)
    gq = e.quantile_rows(name, Q, 0, R, grouped=True)
    assert gq["quantiles"].shape == (3, R, len(Q))
    for g in range(3):
        assert same_values(gq["quantiles"][g], _np_q(N[:, group == g])), g
    e.clear_member_groups()
    e.set_baseline(name, 5, 15)
    b = hi.baseline(N[5:15])
    assert same_values(e.baseline(), b)
    a = hi.anomaly(N, b)
    aq = e.quantile_rows(name, Q, 0, R, anomaly=True)
    assert same_values(aq["quantiles"], _np_q(a)) and np.array_equal(aq["count"], (~np.isnan(a)).sum(axis=1))
    e.clear_baseline()


def test_the_member_statistics_read_the_imbalance(noisy):
    c, vid, N = noisy
    e, R, name = c.e, 48, "Top of Atmosphere Imbalance"
    thr = [float(np.nanmedian(N[R - 1]))]
    ind = e.indicators(name, 0, R, thresholds=thr)
    want = hi.indicators(N, YEARS[:R], thr)
    assert all(same_values(ind[k].to_host(), want[k]) for k in ("mean", "peak", "peak_time")) and same_values(ind["crossing"][0].to_host(), want["crossing"][0])
    for d in ("mean", "linear", "difference"):
        got, want = e.variability(name, 0, R, detrend=d), hv.variability(N, d)
        for k in hv.NAMES:
            assert same_values(got[k].to_host(), want[k]), (d, k)
    sp = e.spectrum(name, 0, R, detrend="linear", bands=3)
    want = hs.spectrum(N, "linear", sp["edges"])
    for k in hs.FIRST:
        assert same_values(sp[k].to_host(), want[k]), k
    assert all(same_values(p.to_host(), q) for p, q in zip(sp["power"], want["power"]))
    ts = c.ts[:R]
    for dx, dy, lags in (("linear", "linear", 0), ("mean", "difference", 2)):
        got = [v.to_host() for v in hc.flat(e.covariability("Surface Temperature", name, 0, R, 1, dx, dy, lags))]
        for j, (g, w) in enumerate(zip(got, hc.flat(hc.covariability(ts, N, dx, dy, lags)))):
            assert same_values(g, w), (dx, dy, lags, j)
    xs = e.cross_spectrum("Surface Temperature", name, 0, R, 1, "linear", "linear", bands=3)
    got = [v.to_host() for v in hx.flat(xs)]
    for j, (g, w) in enumerate(zip(got, hx.flat(hx.cross_spectrum(ts, N, "linear", "linear", xs["edges"])))):
        assert same_values(g, w), j


def test_the_likelihood_and_the_summary_read_the_imbalance(noisy):
    import math
    c, vid, N = noisy
    e, n, R, name = c.e, c.n, 48, "Top of Atmosphere Imbalance"
    tidx = list(range(4, R, 4))
    obs = [float(np.nanmedian(N[t])) for t in tidx]
    sig = [float(0.3 * np.nanstd(np.where(np.isfinite(N[t]), N[t], np.nan))) + 1e-3 for t in tidx]
    for reference in (None, {name: (5, 15)}):
        href = None if reference is None else {vid: (5, 15)}
        got = e.loglik([name] * len(tidx), tidx, obs, sig, False, reference=reference)
        want = hl.loglik({vid: N}, [vid] * len(tidx), tidx, obs, sig, False, href)
        assert np.array_equal(got, want) and np.isneginf(want).any() and np.isfinite(want).sum() > n // 2
    row = N[20]
    fin = np.isfinite(row)
    s = e.summary(name, 20)
    assert s["count"] == fin.sum() and s["min"] == row[fin].min() and s["max"] == row[fin].max()
    # the mean within the error of a sum of n terms in any order (the device adds by a tree) and two divisions
    assert abs(s["mean"] - math.fsum(row[fin]) / fin.sum()) <= (n + 2) * 2.0 ** -53 * np.abs(row[fin]).sum() / fin.sum()


# ---------------------------------------------------------------------------------------------- Gregory
def test_the_gregory_slope_is_minus_the_feedback(ra):
    """64 members under a constant 4 W m^-2 from a zero state, a = 0 and efficacy = 1: N = F - lambda0 Ts exactly in real arithmetic,
    so the regression slope of N on Ts is -lambda0.  N is rounded at about 1e-16 x 4 against a spread of Ts of order 1 K: 1e-9
    relative leaves six orders of margin."""
    n = 64
    rng = np.random.default_rng(64)
    P = two_layer_params(n)
    P[0], P[1], P[2] = rng.uniform(0.8, 1.5, n), 0.0, 1.0
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS) as e:
        e.set_params(P)
        e.set_forcing(np.full(T, 4.0))
        e.set_initial(TS, 0.0)
        e.set_initial(TD, 0.0)
        e.run()
        N = e.define_toa_imbalance()
        e.compute_diagnostic(N)
        slope = e.covariability("Surface Temperature", N, 0, T, 1, "mean", "mean", 0)["slope"].to_host()
        assert np.ptp(e.get_series(TS), axis=0).min() > 0.5
    assert np.isfinite(slope).all() and (np.abs(slope + P[0]) <= 1e-9 * P[0]).all(), np.abs(slope / P[0] + 1.0).max()


# ---------------------------------------------------------------------------------------------- staleness
def test_staleness_follows_the_write_epoch_and_the_forcing_epoch(ra):
    n = 65
    with Case(ra, n, noise=NOISES["members"], steps=40) as c, Case(ra, n, noise=NOISES["members"], steps=40) as src:
        e = c.e
        ids = {q: e.define_energy_budget(q) for q in ("forcing", "response", "imbalance")}
        ids["heat"] = e.define_heat_content()
        ck = e.checkpoint()

        def fresh(what, names=tuple(ids)):
            c.refresh()
            k = e.time_index
            for q in names:
                e.compute_diagnostic(ids[q])
                want = (hd.diagnostic(hd.HEAT_CONTENT, [c.ts[:k + 1], c.td[:k + 1]], c.P) if q == "heat" else c.want(q, 0, k + 1, 1))
                assert same_bits(e.get_series(ids[q], 0, k + 1), want), (what, q)
                assert e.diagnostics[e_name(e, ids[q])]["rows_held"] == k + 1

        def stale(what, names=tuple(ids)):
            from rscm_amd._lib import RscmGpuError
            for q in names:
                vid = ids[q]
                assert refusal_code(e.summary, vid, 0) == 2 and refusal_code(e.get_series, vid, 0, 1) == 2 and refusal_code(e.quantile_rows, vid, Q, 0, 1) == 2, (what, q)
                with pytest.raises(RscmGpuError, match="is stale: compute it again"):
                    e.set_baseline(vid, 0, 1)
                assert e.diagnostics[e_name(e, vid)]["rows_held"] == 0, (what, q)

        def current(what, names):
            k = e.time_index
            for q in names:
                assert e.summary(ids[q], 0)["count"] >= 0 and e.diagnostics[e_name(e, ids[q])]["rows_held"] == k + 1, (what, q)

        fresh("first")
        e.params_vector(4)                                                  # what hands out pointers does not move an epoch
        e.series_devptr(1)
        current("pointers", tuple(ids))
        writers = {
            "run": lambda: e.run(50),
            "rewind": lambda: e.rewind(),
            "set_params": lambda: e.set_params(e.get_params() * 1.0),
            "set_state": lambda: e.set_state(1, 0, 0.25),
            "sample_lhs": lambda: e.sample_lhs(3, [0.8, 0.0, 1.0, 0.5, 5.0, 50.0, 0.1, 0.0], [1.5, 0.1, 1.8, 1.0, 15.0, 200.0, 0.6, 0.9]),
            "restore": lambda: e.restore(ck),
            "branch": lambda: src.e.branch(e, np.arange(n, dtype=np.int64)),
            "set_forcing_noise_members": lambda: e.set_forcing_noise_members(SEED + 7),
        }
        for what, write in writers.items():
            write()
            if what == "set_forcing_noise_members":
                c.noise = ("members", SEED + 7)
            stale(what)
            fresh(what)
        # the forcing epoch: a new table, a new scenario assignment or a new source make the two that read the forcing stale, only them
        c.table = c.table * 1.5
        e.set_forcing(c.table, c.scen)
        stale("set_forcing", ("forcing", "imbalance"))
        current("set_forcing", ("response", "heat"))
        fresh("set_forcing", ("forcing", "imbalance"))
        c.scen = np.ascontiguousarray(1 - c.scen)
        e.set_forcing(c.table, c.scen)
        stale("scenarios", ("forcing", "imbalance"))
        current("scenarios", ("response", "heat"))
        fresh("scenarios", ("forcing", "imbalance"))
        e.run()
        stale("run to the end")
        fresh("the end")
        # ... and the deep-ocean heat uptake reads no forcing either
        e.clear_diagnostics()
        ids = {q: e.define_energy_budget(q) for q in ("deep_uptake", "imbalance")}
        fresh("again", tuple(ids))
        e.set_forcing(c.table, c.scen)
        stale("set_forcing", ("imbalance",))
        current("set_forcing", ("deep_uptake",))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(ra):
    n = 64
    with Case(ra, n) as c:
        e = c.e
        vid = C.c_int32(-1)
        for quantity in (0, 5, -1):
            assert e._lib.rscm_ens_define_energy_budget(e._h, quantity, 1.0, C.byref(vid)) == 1
        for scale in (np.nan, np.inf, -np.inf):
            assert refusal_code(e.define_energy_budget, "imbalance", "scaled", scale) == 1
        assert e._lib.rscm_ens_define_energy_budget(e._h, 4, 1.0, None) == 1
        assert e.diagnostics == {} and "scaled" not in e.var_ids
        ids = _define_all(e)
        n_diag = C.c_int32()
        assert e._lib.rscm_ens_n_diagnostics(e._h, C.byref(n_diag)) == 0 and n_diag.value == 4
        assert refusal_code(e.define_energy_budget, "imbalance", "fifth") == 1 and "fifth" not in e.var_ids
        assert refusal_code(e.define_heat_content) == 1                            # the slots are the linear diagnostics' too
        with pytest.raises(ValueError):
            e.define_energy_budget("imbalance")                             # the default name is taken
        with pytest.raises(ValueError):
            e.define_energy_budget("albedo")
        assert e._lib.rscm_ens_diagnostic_quantity(e._h, 2, None, None) == 1 and e._lib.rscm_ens_diagnostic_quantity(e._h, 7, None, None) == 1
        # ranges, as for any diagnostic
        for tb, te, ts in ((5, 3, 1), (0, T + 1, 1), (4, 4, 1), (0, 10, 0), (-1, 4, 1)):
            assert refusal_code(e.compute_diagnostic, ids["imbalance"], tb, te, ts) == 1, (tb, te, ts)
        # a select in flight: define and compute refuse
        e.compute_diagnostic(ids["imbalance"], 0, 30)
        with e.select(ids["imbalance"], [0.5], 0, 30) as s:
            assert refusal_code(e.compute_diagnostic, ids["imbalance"], 0, 10) == 2 and refusal_code(e.clear_diagnostics) == 2
            while s.next_pass() is not None:
                s.commit()
        e.clear_diagnostics()
        assert e.diagnostics == {} and "Member Forcing" not in e.var_ids and refusal_code(e.compute_diagnostic, 3, 0, 4) == 1
        with e.select(TS, [0.5], 0, 30) as s:
            assert refusal_code(e.define_energy_budget, "response") == 2 and "Radiative Response" not in e.var_ids
            while s.next_pass() is not None:
                s.commit()
        assert e.define_toa_imbalance() == 3                                # the id is free again
        # the fused run + likelihood refuses the id as it refuses any diagnostic
        assert refusal_code(e.run_loglik, [3], [5], [0.0], [1.0]) == 1
    # rows beyond the time index
    with Case(ra, n, steps=10) as c:
        vid = c.e.define_toa_imbalance()
        assert refusal_code(c.e.compute_diagnostic, vid, 0, 20) == 2
        c.e.compute_diagnostic(vid)
        assert c.e.diagnostics["Top of Atmosphere Imbalance"]["rows_held"] == 11
    # another kind
    with ra.Ensemble(ra.KIND_UDEB, 4, BOUNDS) as e:
        assert refusal_code(e.define_energy_budget, "response") == 1 and refusal_code(e.define_toa_imbalance) == 1
    with ra.Ensemble(ra.KIND_COUPLED, 4, BOUNDS) as e:
        assert refusal_code(e.define_energy_budget, "forcing") == 1
    # forcing never set, parameters never set
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS) as e:
        ids = {q: e.define_energy_budget(q) for q in ("forcing", "response", "imbalance")}
        e.set_initial(TS, 0.5)
        e.set_initial(TD, 0.25)
        assert all(refusal_code(e.compute_diagnostic, v, 0, 1) == 2 for v in ids.values())     # no parameters
        P = two_layer_params(n)
        e.set_params(P)
        assert refusal_code(e.compute_diagnostic, ids["forcing"], 0, 1) == 2 and refusal_code(e.compute_diagnostic, ids["imbalance"], 0, 1) == 2
        e.compute_diagnostic(ids["response"], 0, 1)
        assert same_bits(e.get_series(ids["response"], 0, 1)[0], (P[0] - P[1] * 0.5) * 0.5)
        e.set_forcing(0.05 * np.arange(T))
        e.compute_diagnostic(ids["forcing"], 0, 1)


def test_a_linked_handle_in_both_directions(ra):
    n = 64
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS) as src, ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS) as e:
        for h in (src, e):
            h.set_params(two_layer_params(n))
            h.set_forcing(0.05 * np.arange(T))
            h.set_initial(TS, 0.0)
            h.set_initial(TD, 0.0)
        src.run()
        e.run(20)
        # defined first, linked afterwards: the compute refuses, the forcing-free quantities go on
        ids = {q: e.define_energy_budget(q) for q in ("forcing", "response", "imbalance")}
        for v in ids.values():
            e.compute_diagnostic(v)
        e.link_input(0, src, TS)
        try:
            assert refusal_code(e.get_series, ids["imbalance"], 0, 1) == 2        # the link replaced the forcing: stale
            assert refusal_code(e.compute_diagnostic, ids["forcing"]) == 1 and refusal_code(e.compute_diagnostic, ids["imbalance"]) == 1
            assert e.summary(ids["response"], 0)["count"] == n             # current still
            e.compute_diagnostic(ids["response"])
            # linked first: the two that read the forcing are refused at define time, the other two are defined
            e.clear_diagnostics()
            assert refusal_code(e.define_energy_budget, "forcing") == 1 and refusal_code(e.define_toa_imbalance) == 1
            assert "Member Forcing" not in e.var_ids and e.diagnostics == {}
            up = e.define_energy_budget("deep_uptake")
            e.compute_diagnostic(up)
            P = e.get_params()
            want = hb.budget("deep_uptake", e.get_series(TS, 0, 21), e.get_series(TD, 0, 21), P, np.zeros((21, n)))
            assert same_bits(e.get_series(up, 0, 21), want)
        finally:
            e.unlink_input(0)
        vid = e.define_toa_imbalance()                                      # unlinked again: available again
        e.compute_diagnostic(vid)


def test_the_samplers_and_the_builder_refuse_the_names(ra):
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    axis = core.TimeAxis.from_values(YEARS)
    F = 0.05 * np.arange(T)
    b = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
         .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(F, axis, "W/m^2", core.InterpolationStrategy.Linear))
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0})
         .with_energy_budget("imbalance").with_energy_budget("response", "R", -1.0))
    model = b.build(n_members=8)
    try:
        model.run()
        ens = model.ensemble
        d = ens.diagnostics
        assert (d["Top of Atmosphere Imbalance"]["quantity"], d["R"]["quantity"], d["R"]["scale"]) == ("imbalance", "response", -1.0)
        ens.compute_diagnostic("Top of Atmosphere Imbalance")
        P = ens.get_params()
        Fm = np.repeat(F[:, None], 8, axis=1)
        assert same_bits(ens.get_series("Top of Atmosphere Imbalance"), hb.budget("imbalance", ens.get_series(TS), ens.get_series(TD), P, Fm))
        assert "Top of Atmosphere Imbalance" not in model.timeseries().names()
    finally:
        model.close()
    with pytest.raises(ValueError, match="diagnostic"):
        cal.ModelRunner(b, ["lambda0"], ["Top of Atmosphere Imbalance"])
    runner = cal.ModelRunner(b, ["lambda0"], ["Surface Temperature"])
    target = cal.Target()
    target.add_observation("Top of Atmosphere Imbalance", 1860.0, 1.0, 0.5)
    params = cal.ParameterSet().add("lambda0", cal.Uniform(0.8, 1.6))
    for sampler in (cal.DeviceEnsembleSampler, cal.EnsembleSampler):
        with pytest.raises(ValueError, match="compute_diagnostic"):
            sampler(params, runner, cal.GaussianLikelihood(), target)
    with pytest.raises(ValueError, match="compute_diagnostic"):
        runner.log_likelihood_batch(np.array([[1.1]]), target, cal.GaussianLikelihood())


# ---------------------------------------------------------------------------------------------- around a run
def test_a_windowed_handle_with_an_output_store(ra):
    n = 65
    P = two_layer_params(n)
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS, window_rows=8, output_stride=4) as e:
        e.set_params(P)
        e.set_forcing(0.05 * np.arange(T))
        e.set_initial(TS, 0.0)
        e.set_initial(TD, 0.0)
        for k in list(range(6, T - 1, 6)) + [T - 1]:                        # (a window of 8 rows keeps 2: six steps at a time)
            e.run(k)
        assert e.time_index == T - 1
        vid = e.define_energy_budget("response")
        e.compute_diagnostic(vid, 0, T - 3, 4)                              # the output store
        ts, td = e.get_series(TS, 0, T - 3, 4), e.get_series(TD, 0, T - 3, 4)
        want = hb.budget("response", ts, td, P, np.zeros_like(ts))
        assert same_bits(e.get_series(vid, 0, T - 3, 4), want) and np.isfinite(want).all() and len(want) == 18
        assert refusal_code(e.compute_diagnostic, vid, 0, 9, 3) == 2              # rows 3 and 6 are not resident any more
        assert e.diagnostics["Radiative Response"]["rows_held"] == 18
        k = e.time_index
        e.compute_diagnostic(vid, k - 2)                                    # the window's last rows
        ts, td = e.get_series(TS, k - 2, k + 1), e.get_series(TD, k - 2, k + 1)
        assert same_bits(e.get_series(vid, k - 2, k + 1), hb.budget("response", ts, td, P, np.zeros_like(ts)))


def test_two_shards_give_the_halves(ra):
    n, k = 257, 129
    with Case(ra, n, noise=NOISES["members"], random_rows=False) as whole:
        ids = _define_all(whole.e)
        rows = {}
        for q, vid in ids.items():
            whole.e.compute_diagnostic(vid, 0, T)
            rows[q] = whole.e.get_series(vid)
            assert same_bits(rows[q], whole.want(q, 0, T, 1))
        for offset, count in ((0, k), (k, n - k)):
            with Case(ra, count, noise=NOISES["members"], offset=offset, n_total=n, random_rows=False) as h:
                for q, vid in _define_all(h.e).items():
                    h.e.compute_diagnostic(vid, 0, T)
                    assert same_bits(h.e.get_series(vid), rows[q][:, offset:offset + count]), (q, offset)
        from rscm_amd.distributed import ShardedEnsemble
        made = []

        def factory(count, device):
            made.append(Case(ra, count, noise=NOISES["members"], random_rows=False))
            return made[-1].e

        sh = ShardedEnsemble(n, factory, rank=0, world=1)
        try:
            vid = sh.define_energy_budget("imbalance")
            sh.compute_diagnostic("Top of Atmosphere Imbalance", 0, T)
            assert same_bits(sh.ensemble.get_series(vid), rows["imbalance"])
            got = sh.quantile_rows_global("Top of Atmosphere Imbalance", Q, 0, T)
            assert same_values(got["quantiles"], _np_q(rows["imbalance"]))
        finally:
            sh.ensemble.close()


def test_a_posterior_defines_what_its_source_defines(ra):
    n, k0 = 257, 40
    with Case(ra, n, noise=NOISES["members"], steps=k0, random_rows=False) as c:
        e = c.e
        e.define_toa_imbalance(scale=-2.5)
        e.define_energy_budget("forcing")
        e.define_heat_content()
        e.set_member_weights(np.where(np.isfinite(c.ts[:k0 + 1]).all(axis=0), 1, 0).astype(np.int64))
        table = np.stack([np.zeros(T), 0.07 * np.arange(T)])

        def factory(count):
            d = ra.Ensemble(ra.KIND_TWO_LAYER, count, BOUNDS, noise_params=True)
            d.set_forcing(table, np.ones(count, dtype=np.int32))
            d.set_forcing_noise_members(SEED + 11)
            return d

        dst, _ = e.posterior(factory, 40, seed=1)
        try:
            d = dst.diagnostics
            assert {name: (v["quantity"], v["scale"], v["terms"]) for name, v in d.items()} == {
                "Top of Atmosphere Imbalance": ("imbalance", -2.5, []), "Member Forcing": ("forcing", 1.0, []),
                "Ocean Heat Content": (None, None, [(1, 4, 1.0), (2, 5, 1.0)])}
            assert all(v["rows_held"] == 0 for v in d.values()) and dst.time_index == k0
            dst.run()
            dst.compute_diagnostic("Top of Atmosphere Imbalance", k0, T)
            P = dst.get_params()
            F = hb.member_forcing(table, P, np.ones(40, dtype=np.int32), 0, ("members", SEED + 11))
            want = hb.budget("imbalance", dst.get_series(TS, k0, T), dst.get_series(TD, k0, T), P, F[:, k0:].T, -2.5)
            assert same_bits(dst.get_series("Top of Atmosphere Imbalance", k0, T), want) and np.isfinite(want).all()
        finally:
            dst.close()
