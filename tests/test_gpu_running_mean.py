"""GPU tier of the running-mean diagnostics (csrc/running_mean.hip, csrc/running_mean_host.cpp; rscm_ens_define_running_mean,
rscm_ens_diagnostic_running_mean, rscm_ens_compute_diagnostic; Ensemble.define_running_mean, compute_diagnostic,
GraphModel.define_running_mean).  The oracle is the numpy restatement of tests/host_running_mean.py applied to the source's rows
fetched with get_series, compared bit for bit (any NaN equal to any NaN).

The data: two-layer ensembles with per-member forcing noise on a 72-point annual axis (tests/gpu_support.py, noise_ensemble), every
row of the surface temperature overwritten with +-uniform(0.01, 5) -- full mantissas of mixed sign, on which the reversed order and
a sliding update differ from the definition in most elements (tests/test_running_mean_cpu.py) -- so the order matters in every
window.  The deep-ocean temperature keeps the run's values, its non-finite members included: the heat content and the shards use it."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

from tests import host_exceedance_rows as he
from tests import host_indicators as hi
from tests import host_likelihood as hl
from tests import host_moment_rows as hm
from tests import host_running_mean as hr
from tests import host_variability as hv
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import built_once, noise_ensemble, plant, refusal_code
from tests.helpers import annual_bounds, magicc_chain, same_bits, same_values

pytestmark = pytest.mark.gpu

T = 72
YEARS, BOUNDS = annual_bounds(T)
SEED = 20261021
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
WINDOWS = (2, 3, 11, 20, 64)
ALIGNS = ("trailing", "centre")
STEPS = ((1, 1), (1, 3), (2, 2), (2, 4), (3, 12))            # (step, t_stride)
DISJOINT = ((3, 1, 5), (12, 1, 12))                           # (window, step, t_stride) with t_stride >= window * step
Q = [0.05, 0.5, 0.95]
# kRunMeanThreads, kRunMeanBatch, kRunMeanMinBlocks and kRunMeanMaxOverlap of csrc/running_mean.hpp
THREADS, BATCH, MIN_BLOCKS, MAX_OVERLAP = 256, 8, 2048, 4


def tile_rows(n_rows, window, m, n):
    """running_mean_tile of csrc/running_mean.hip: the outputs a block forms, for n_rows outputs m source rows apart of n members."""
    blocks_x = -(-n // THREADS)
    tiles = -(-MIN_BLOCKS // blocks_x)
    rows = -(-n_rows // tiles)
    if m < window:
        rows = max(rows, -(-MAX_OVERLAP * (window - m) // m))
    return -(-max(rows, 1) // BATCH) * BATCH


def _random_surface(e, n):
    X = hr.mixed_sign_rows(T, n, SEED + n)
    for t in range(T):
        e.set_state(1, t, X[t])
    return X


@pytest.fixture(scope="module")
def cases(ra):
    """{N: (the ensemble, its surface temperature [T][N] on the host -- the random rows --, its deep-ocean temperature)}, built once."""
    def build(n):
        e = noise_ensemble(ra, n, BOUNDS, SEED)
        X = _random_surface(e, n)
        ts, td = e.get_series(1), e.get_series(2)
        assert same_bits(ts, X)
        for x in (ts, td):
            x.setflags(write=False)
        return e, ts, td

    yield from built_once(build)


def _ranges(window, align, step, t_stride, n):
    """(t_begin, t_end) of the ranges to compute at t_stride: from the first valid row, row counts around the load batch and the
    tile, two tiles plus one, all the valid rows; and one that ends at the last valid row without starting at the first."""
    first, last = hr.valid_rows(T, window, align, step)
    if last < first:
        return []
    r_max = (last - first) // t_stride + 1
    tile = tile_rows(r_max, window, t_stride // step, n)
    counts = {1, BATCH - 1, BATCH, BATCH + 1, tile - 1, tile, tile + 1, 2 * tile + 1, r_max}
    out = [(first, first + (r - 1) * t_stride + 1) for r in sorted(counts) if 1 <= r <= r_max]
    k = min(5, r_max)
    out.append((last - (k - 1) * t_stride, last + 1))
    return out


def _check_definition(e, X, n, window, align, step, t_stride):
    first, last = hr.valid_rows(T, window, align, step)
    if last < first:
        return 0
    name = f"m{window}{align}{step}"
    if name not in e.var_ids:
        if len(e.diagnostics) == 4:
            e.clear_diagnostics()
        e.define_running_mean(name, 1, window, align, step)
        assert e.diagnostics[name]["running_mean"] == {"source": 1, "window": window, "align": align, "step": step}
        assert e.diagnostics[name]["terms"] == [] and e.diagnostics[name]["quantity"] is None
    full = hr.running_mean(X, window, align, step, first, last + 1, 1)             # every valid row, once
    done = 0
    for tb, te in _ranges(window, align, step, t_stride, n):
        e.compute_diagnostic(name, tb, te, t_stride)
        got = e.get_series(name, tb, te, t_stride)
        want = full[tb - first:te - first:t_stride]
        assert same_bits(got, want), (name, tb, te, t_stride, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])
        held = e.diagnostics[name]
        assert (held["rows_held"], held["t_begin"], held["t_stride"]) == (len(range(tb, te, t_stride)), tb, t_stride)
        done += 1
    e.compute_diagnostic(name, t_stride=t_stride)                                    # the None defaults: every row with a full window
    held = e.diagnostics[name]
    assert (held["rows_held"], held["t_begin"], held["t_stride"]) == (len(range(first, last + 1, t_stride)), first, t_stride)
    assert same_bits(e.get_series(name, first, last + 1, t_stride), full[::t_stride])
    return done + 1


@pytest.mark.parametrize("n", SIZES)
def test_running_means_equal_the_restatement(ra, cases, n):
    e, X, _ = cases(n)
    done = 0
    for window in WINDOWS:
        for align in ALIGNS:
            for step, t_stride in STEPS:
                done += _check_definition(e, X, n, window, align, step, t_stride)
    for window, step, t_stride in DISJOINT:
        assert t_stride >= window * step
        done += _check_definition(e, X, n, window, "centre", step, t_stride)
    assert done > 200
    e.clear_diagnostics()
    # the ranges above do cross tiles and batches: a short window has a short tile
    assert tile_rows(70, 2, 1, n) == 8 and tile_rows(14, 3, 5, n) == 8 and tile_rows(62, 11, 1, n) == 40


def test_special_values_stay_in_their_windows(ra):
    n, window = 257, 11
    planted = ((5, 20, np.inf), (7, 21, -np.inf), (9, 30, np.nan), (11, 31, 5e-324), (5, 60, np.nan))   # (member, row, value)
    with noise_ensemble(ra, n, BOUNDS, SEED) as e:
        clean = _random_surface(e, n)
        for member, row, value in planted:
            plant(e, 1, member, row, value)
        X = e.get_series(1)
        assert np.isposinf(X[20, 5]) and np.isneginf(X[21, 7]) and np.isnan(X[30, 9]) and X[31, 11] == 5e-324
        for align in ALIGNS:
            name = "special " + align
            e.define_running_mean(name, 1, window, align)
            e.compute_diagnostic(name)
            first, last = hr.valid_rows(T, window, align)
            got = e.get_series(name, first, last + 1)
            assert same_bits(got, hr.running_mean(X, window, align, 1, first, last + 1, 1))
            # outside the windows that hold a planted value, the rows after them included, nothing has changed
            b = hr.back(window, align)
            touched = np.zeros_like(got, dtype=bool)
            for member, row, value in planted:
                lo, hi_ = row - (window - 1 - b), row + b                       # the rows whose window holds `row`
                touched[max(lo, first) - first:min(hi_, last) - first + 1, member] = True
            want_clean = hr.running_mean(clean, window, align, 1, first, last + 1, 1)
            assert np.isfinite(got[~touched]).all() and same_bits(got[~touched], want_clean[~touched])
            for member, row, value in planted:
                if not np.isfinite(value):
                    assert not np.isfinite(got[touched[:, member], member]).any()
            after = slice(31 + b + 1 - first, 60 - (window - 1 - b) - first)        # between the two groups of planted rows
            assert after.stop - after.start >= 5 and np.isfinite(got[after]).all() and same_bits(got[after], want_clean[after])


# ---------------------------------------------------------------------------------------------- diagnostic sources
def test_the_source_may_be_a_diagnostic(ra, cases):
    n = 257
    e, _, _ = cases(n)
    e.clear_diagnostics()
    heat = e.define_heat_content("heat")
    imb = e.define_toa_imbalance("imb")
    e.compute_diagnostic("heat")
    e.compute_diagnostic("imb")
    H, I = e.get_series("heat"), e.get_series("imb")
    assert np.isnan(H).any() and np.isfinite(H).sum() > H.size // 2 and np.isfinite(I).sum() > I.size // 2
    hid = e.define_running_mean("heat20", "heat", 20, "centre")
    iid = e.define_running_mean("imb5", imb, 5, "trailing")
    assert (hid, iid) == (imb + 1, imb + 2) and e.diagnostics["heat20"]["running_mean"]["source"] == heat
    for name, S, window, align in (("heat20", H, 20, "centre"), ("imb5", I, 5, "trailing")):
        e.compute_diagnostic(name)
        first, last = hr.valid_rows(T, window, align)
        want = hr.running_mean(S, window, align, 1, first, last + 1, 1)
        assert same_bits(e.get_series(name, first, last + 1), want), name
        assert e.diagnostics[name]["rows_held"] == last - first + 1
    # the source held over too short a range: refused, and the rows held before stay
    first, last = hr.valid_rows(T, 20, "centre")
    before = e.get_series("heat20", first, last + 1)
    e.compute_diagnostic("heat", 0, 30)
    assert refusal_code(e.compute_diagnostic, "heat20") == 2 and refusal_code(e.compute_diagnostic, "heat20", first, first + 15) == 2
    assert e.diagnostics["heat20"]["rows_held"] == last - first + 1
    e.compute_diagnostic("heat20", first, 30 - 10)                                   # what the 30 rows do serve
    assert e.diagnostics["heat20"]["rows_held"] == 30 - 10 - first
    assert same_bits(e.get_series("heat20", first, 20), before[:20 - first])
    # the source computed over another range: the running mean does not depend on its store
    e.compute_diagnostic("heat")
    e.compute_diagnostic("heat20")
    e.compute_diagnostic("heat", 40, 50)
    assert e.diagnostics["heat20"]["rows_held"] == last - first + 1 and same_bits(e.get_series("heat20", first, last + 1), before)
    e.compute_diagnostic("heat", 0, T, 2)                                            # held, but not at exactly the window's indices
    assert refusal_code(e.compute_diagnostic, "heat20") == 2
    e.clear_diagnostics()


# ---------------------------------------------------------------------------------------------- every reader takes it
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


def test_every_reader_takes_the_running_mean(ra, cases):
    n = 257
    e, X, _ = cases(n)
    e.clear_diagnostics()
    vid = e.define_running_mean("ts20", "Surface Temperature", 20, "centre")
    e.compute_diagnostic("ts20")
    first, last = hr.valid_rows(T, 20, "centre")
    tb, te = first, last + 1
    M = hr.running_mean(X, 20, "centre", 1, tb, te, 1)
    assert same_bits(e.get_series("ts20", tb, te), M) and same_bits(e.get_series(vid, tb + 4, te, 5, 3, 200), M[4::5, 3:200])
    # the selects: plain, weighted, anomaly against a baseline on the running mean itself, grouped
    got = e.quantile_rows("ts20", Q, tb, te)
    assert same_values(got["quantiles"], _np_q(M)) and np.array_equal(got["count"], (~np.isnan(M)).sum(axis=1))
    rng = np.random.default_rng(n)
    w = rng.integers(1, 1 << 30, n, dtype=np.int64)
    w[rng.random(n) < 0.2] = 0
    e.set_member_weights(w)
    wq = e.quantile_rows("ts20", Q, tb, te, weighted=True)
    want, W = _np_wq(M, w)
    assert same_values(wq["quantiles"], want) and np.array_equal(wq["weight"], W)
    e.set_baseline("ts20", tb + 2, tb + 12)
    b = hi.baseline(M[2:12])
    assert same_values(e.baseline(), b)
    a = hi.anomaly(M, b)
    aq = e.quantile_rows("ts20", Q, tb, te, anomaly=True)
    assert same_values(aq["quantiles"], _np_q(a))
    group = (np.arange(n) % 3).astype(np.int32)
    e.set_member_groups(group, 3)
    gq = e.quantile_rows("ts20", Q, tb, te, grouped=True)
    for g in range(3):
        assert same_values(gq["quantiles"][g], _np_q(M[:, group == g])), g
    e.clear_member_groups()
    e.clear_baseline()
    # the crossing of the smoothed series, and the other per-member statistics
    thr = [float(np.median(M[-1])), 0.25]
    ind = e.indicators("ts20", tb, te, thresholds=thr)
    want = hi.indicators(M, YEARS[tb:te], thr)
    assert all(same_values(ind[k].to_host(), want[k]) for k in ("mean", "peak", "peak_time"))
    for k in range(len(thr)):
        assert same_values(ind["crossing"][k].to_host(), want["crossing"][k]), k
    assert np.isfinite(want["crossing"][1]).any()
    for d in ("mean", "linear", "difference"):
        got, want = e.variability("ts20", tb, te, detrend=d), hv.variability(M, d)
        for k in hv.NAMES:
            assert same_values(got[k].to_host(), want[k]), (d, k)
    # exceedance and moments at every row
    thr2 = np.array([0.0, 0.3])
    assert he.same(e.exceedance_rows("ts20", thr2, tb, te), he.exceedance_rows(M, thr2))
    assert he.same(e.exceedance_rows("ts20", thr2, tb, te, weighted=True), he.exceedance_rows(M, thr2, w))
    got, want = e.moment_rows("ts20", tb, te), hm.ungrouped(hm.moment_rows(M))
    assert set(got) == set(want)
    for k in want:
        assert same_bits(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)), k
    # the stored likelihood against decadal means: bit for bit without the normalisation's logarithm, rtol 1e-13 with it
    full = np.full((T, n), np.nan)
    full[tb:te] = M
    tidx = list(range(tb + 1, te, 10))
    obs = [float(np.median(M[t - tb])) for t in tidx]
    sig = [float(0.3 * np.std(M[t - tb])) + 1e-3 for t in tidx]
    for reference in (None, {"ts20": (tb, tb + 10)}):
        href = None if reference is None else {vid: (tb, tb + 10)}
        got = e.loglik(["ts20"] * len(tidx), tidx, obs, sig, reference=reference)
        assert np.array_equal(got, hl.loglik({vid: full}, [vid] * len(tidx), tidx, obs, sig, False, href)) and np.isfinite(got).all()
        norm = e.loglik(["ts20"] * len(tidx), tidx, obs, sig, True, reference=reference)
        assert np.allclose(norm, hl.loglik({vid: full}, [vid] * len(tidx), tidx, obs, sig, True, href), rtol=1e-13, atol=0)
    assert refusal_code(e.loglik, ["ts20"], [tb - 1], [0.0], [1.0]) == 2                # a row without a full window is not held
    # the summary: count, min and max exactly; the mean within the error of a sum of n terms in any order and two divisions
    row = M[20]
    s = e.summary("ts20", tb + 20)
    assert s["count"] == n and s["min"] == row.min() and s["max"] == row.max()
    assert abs(s["mean"] - math.fsum(row) / n) <= (n + 2) * 2.0 ** -53 * np.abs(row).sum() / n
    e.clear_diagnostics()


# ---------------------------------------------------------------------------------------------- staleness
def test_rows_go_stale_with_every_writer_and_the_forcing_where_the_source_reads_it(ra):
    n, window = 65, 5
    with noise_ensemble(ra, n, BOUNDS, SEED, steps=40) as e:
        ts = e.define_running_mean("ts5", 1, window, "trailing")
        imb = e.define_toa_imbalance("imb")
        im = e.define_running_mean("imb5", imb, window, "trailing")

        def fresh(what):
            k = e.time_index
            e.compute_diagnostic("imb")
            for name, src in (("ts5", 1), ("imb5", imb)):
                e.compute_diagnostic(name)
                want = hr.running_mean(e.get_series(src, 0, k + 1), window, "trailing", 1, window - 1, k + 1, 1)
                assert same_bits(e.get_series(name, window - 1, k + 1), want), (what, name)
                assert e.diagnostics[name]["rows_held"] == k + 2 - window, (what, name)

        def stale(what, names=("ts5", "imb5")):
            for name in names:
                assert refusal_code(e.get_series, name, window - 1, window) == 2, (what, name)
                assert refusal_code(e.quantile_rows, name, Q, window - 1, window) == 2, (what, name)
                d = e.diagnostics[name]
                assert d["rows_held"] == 0 and d["running_mean"]["window"] == window, (what, name)   # the definition survives

        fresh("first")
        writers = {
            "run": lambda: e.run(50),
            "set_params": lambda: e.set_params(e.get_params() * 1.0),
            "set_state": lambda: e.set_state(1, 0, 0.25),
        }
        for what, write in writers.items():
            write()
            stale(what)
            fresh(what)
        e.rewind()
        stale("rewind")
        e.run(30)
        stale("run after rewind")
        fresh("run after rewind")
        # the forcing: the mean of the imbalance is a snapshot of it, the mean of the temperature is not
        before = e.get_series(ts, window - 1, 31)
        e.set_forcing(np.stack([np.zeros(T), 0.07 * np.arange(T)]), (np.arange(n) % 2).astype(np.int32))
        stale("set_forcing", names=("imb5",))
        assert refusal_code(e.compute_diagnostic, im) == 2                          # its source is stale as well
        assert e.diagnostics["ts5"]["rows_held"] == 31 - (window - 1) and same_bits(e.get_series(ts, window - 1, 31), before)
        fresh("set_forcing")


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(ra):
    n = 64
    with noise_ensemble(ra, n, BOUNDS, SEED, steps=40) as e:
        lib, out = e._lib, C.c_int32(-7)

        def define(source, window=20, align=1, step=1):
            return lib.rscm_ens_define_running_mean(e._h, source, window, align, step, C.byref(out))

        for window in (1, 65, 0, -3):
            assert define(1, window=window) == 1
        assert define(1, align=2) == 1 and define(1, align=-1) == 1 and define(1, step=0) == 1 and define(1, step=-2) == 1
        for source in (0, 3, 99, -1):                                               # the input, and ids that are not defined
            assert define(source) == 1
        assert lib.rscm_ens_define_running_mean(e._h, 1, 20, 1, 1, None) == 1
        assert out.value == -7 and e.diagnostics == {}
        assert refusal_code(e.define_running_mean, "w", 1, 65) == 1 and "w" not in e.var_ids
        with pytest.raises(ValueError):
            e.define_running_mean("a", 1, align="leading")
        lin = e.define_diagnostic("lin", [(1, None, 1.0)])
        m3 = e.define_running_mean("m3", "Surface Temperature", 3, "centre", 2)
        assert (lin, m3) == (3, 4)
        assert define(m3) == 1                                                      # a running mean as source
        assert refusal_code(e.define_running_mean, "of a mean", "m3") == 1 and define(5) == 1
        e.define_running_mean("m4", lin, 4, "trailing")
        e.define_running_mean("m5", 2, 5)
        assert define(1) == 1 and refusal_code(e.define_running_mean, "fifth", 1) == 1 and "fifth" not in e.var_ids
        n_diag = C.c_int32()
        assert lib.rscm_ens_n_diagnostics(e._h, C.byref(n_diag)) == 0 and n_diag.value == 4
        # read-back
        src, win, al, st, nt, q = (C.c_int32(-1) for _ in range(6))
        qs = C.c_double(-1.0)
        assert lib.rscm_ens_diagnostic_running_mean(e._h, m3, C.byref(src), C.byref(win), C.byref(al), C.byref(st)) == 0
        assert (src.value, win.value, al.value, st.value) == (1, 3, 1, 2)
        assert lib.rscm_ens_diagnostic_running_mean(e._h, lin, C.byref(src), C.byref(win), C.byref(al), C.byref(st)) == 0 and src.value == 0
        assert lib.rscm_ens_diagnostic_running_mean(e._h, m3, None, None, None, None) == 0
        for var in (1, 0, 7, -1):
            assert lib.rscm_ens_diagnostic_running_mean(e._h, var, C.byref(src), None, None, None) == 1
        assert lib.rscm_ens_diagnostic(e._h, m3, C.byref(nt), None, None, None, None, None, None) == 0 and nt.value == 0
        assert lib.rscm_ens_diagnostic_quantity(e._h, m3, C.byref(q), C.byref(qs)) == 0 and (q.value, qs.value) == (0, 0.0)
        assert e.diagnostics["lin"]["running_mean"] is None and e.diagnostics["m4"]["running_mean"]["source"] == lin
        # ranges: m3 is centred over t - 2, t, t + 2; the ensemble stands at index 40
        assert e.time_index == 40
        for t_stride in (1, 3, 5):
            assert refusal_code(e.compute_diagnostic, "m3", 2, 30, t_stride) == 1   # no multiple of the step
        assert refusal_code(e.compute_diagnostic, "m3", 1, 30, 2) == 1              # the window reaches before row 0
        assert refusal_code(e.compute_diagnostic, "m3", 0, 30, 2) == 1
        assert refusal_code(e.compute_diagnostic, "m3", 2, T, 2) == 1               # ... and past the end of the axis
        for tb, te, ts in ((10, 5, 2), (4, 4, 2), (2, 10, 0), (-2, 10, 2), (2, T + 1, 2)):
            assert refusal_code(e.compute_diagnostic, "m3", tb, te, ts) == 1, (tb, te, ts)
        assert refusal_code(e.compute_diagnostic, "m3", 2, 41, 2) == 2              # row 40 reads row 42: past the time index
        assert refusal_code(e.compute_diagnostic, "m3", 3, 42, 2) == 2
        assert e.diagnostics["m3"]["rows_held"] == 0
        assert refusal_code(e.compute_diagnostic, "m4") == 2                        # its source was never computed
        e.compute_diagnostic("m3", 2, 39, 2)
        assert e.diagnostics["m3"]["rows_held"] == 19
        assert refusal_code(e.compute_diagnostic, "m3") == 1                        # None: rows 2 .. 38, but one apart
        e.compute_diagnostic("m3", 2, 11, 2)
        e.compute_diagnostic("m3", t_stride=2)                                      # None: rows 2, 4, .. 38 (38 reads 36, 38, 40)
        assert (e.diagnostics["m3"]["rows_held"], e.diagnostics["m3"]["t_begin"]) == (19, 2)
        X = e.get_series(1, 0, 41)
        assert same_bits(e.get_series("m3", 2, 39, 2), hr.running_mean(X, 3, "centre", 2, 2, 39, 2))
        assert refusal_code(e.get_series, "m3", 1, 3) == 2 and refusal_code(e.get_series, "m3", 38, 40) == 2
        # a select in flight: define and compute refuse
        with e.select("m3", [0.5], 2, 39, 2) as s:
            assert refusal_code(e.compute_diagnostic, "m3") == 2
            while s.next_pass() is not None:
                s.commit()
        e.clear_diagnostics()
        with e.select(1, [0.5], 0, 30) as s:
            assert define(1) == 2 and refusal_code(e.define_running_mean, "late", 1) == 2 and "late" not in e.var_ids
            while s.next_pass() is not None:
                s.commit()
        assert e.define_running_mean("again", 1) == 3                               # the id is free again


# ---------------------------------------------------------------------------------------------- storage layouts
def test_windowed_graph_with_an_output_store(ra):
    """A windowed monthly graph that keeps every 12th row: the three-year mean of a carbon pool from the output store."""
    model = magicc_chain().build_chain(65, 30, "topological", steps_per_year=12, series_window=16, output_stride=12)
    try:
        model.run()
        pool = "Carbon Pool|Plant"
        ens, v_pool = model.variable_home(pool)
        vid = model.define_running_mean("pool3", pool, window=3, step=12)
        assert model.variable_home("pool3") == (ens, vid) and vid == ens.n_vars
        assert ens.diagnostics["pool3"]["running_mean"] == {"source": v_pool, "window": 3, "align": "centre", "step": 12}
        model.compute_diagnostic("pool3", t_stride=12)
        S = model.get_series(pool, t_stride=12)
        lo, hi_ = ens.running_mean_range(vid, time_index=model.time_index)
        rows = len(range(lo, hi_, 12))
        assert lo == 12 and rows >= 20 and ens.diagnostics["pool3"]["rows_held"] == rows
        want = hr.running_mean(S, 3, "centre", 1, 1, 1 + rows, 1)
        assert same_bits(model.get_series("pool3", t_begin=lo, t_end=hi_, t_stride=12), want) and np.isfinite(want).any()
        assert refusal_code(model.compute_diagnostic, "pool3", 12, 48, 6) == 1    # no multiple of the step
        assert refusal_code(model.compute_diagnostic, "pool3", 13, 48, 12) == 2   # rows 1, 13, 25, ... are not resident any more
        assert ens.diagnostics["pool3"]["rows_held"] == rows
        with pytest.raises(ValueError):
            model.define_running_mean("pool3", pool)
    finally:
        model.close()


# ---------------------------------------------------------------------------------------------- shards and posteriors
def test_two_shards_give_the_halves(ra, cases):
    n, k = 257, 129
    e, _, td = cases(n)
    e.clear_diagnostics()
    e.define_running_mean("td20", "Deep Ocean Temperature", 20)
    e.compute_diagnostic("td20")
    first, last = hr.valid_rows(T, 20, "centre")
    whole = e.get_series("td20", first, last + 1)
    assert same_bits(whole, hr.running_mean(td, 20, "centre", 1, first, last + 1, 1)) and np.isnan(whole).any()
    e.clear_diagnostics()
    for offset, count in ((0, k), (k, n - k)):
        with noise_ensemble(ra, count, BOUNDS, SEED, offset, n) as h:
            vid = h.define_running_mean("td20", 2, 20)
            h.compute_diagnostic(vid)
            assert same_bits(h.get_series(vid, first, last + 1), whole[:, offset:offset + count]), offset
    from rscm_amd.distributed import ShardedEnsemble
    sh = ShardedEnsemble(n, lambda count, device: noise_ensemble(ra, count, BOUNDS, SEED), rank=0, world=1)
    try:
        vid = sh.define_running_mean("td20", "Deep Ocean Temperature")
        sh.compute_diagnostic("td20")
        assert same_bits(sh.ensemble.get_series(vid, first, last + 1), whole)
    finally:
        sh.ensemble.close()


def test_a_posterior_carries_the_running_mean_after_its_source(ra):
    n = 257
    with noise_ensemble(ra, n, BOUNDS, SEED) as e:
        heat = e.define_heat_content()
        e.define_running_mean("heat20", "Ocean Heat Content", 20)
        e.define_running_mean("ts11", 1, 11, "trailing", 2)
        e.set_member_weights(np.where(np.isfinite(e.get_series(1)).all(axis=0), 1, 0).astype(np.int64))

        def factory(count):
            d = ra.Ensemble(ra.KIND_TWO_LAYER, count, BOUNDS, noise_params=True)
            d.set_forcing(np.stack([np.zeros(T), 0.05 * np.arange(T)]), np.ones(count, dtype=np.int32))
            d.define_diagnostic("its own", [(2, None, 1.0)])                        # so that dst's ids are not the source's
            return d

        dst, _ = e.posterior(factory, 40, seed=1)
        try:
            got = dst.diagnostics
            assert list(got) == ["its own", "Ocean Heat Content", "heat20", "ts11"]
            assert got["Ocean Heat Content"]["id"] == heat + 1 and all(v["rows_held"] == 0 for v in got.values())
            assert got["heat20"]["running_mean"] == {"source": heat + 1, "window": 20, "align": "centre", "step": 1}
            assert got["ts11"]["running_mean"] == {"source": 1, "window": 11, "align": "trailing", "step": 2}
            assert dst.time_index == T - 1                                          # (only that row was gathered: the rows are dst's to run)
            assert refusal_code(dst.get_series, "heat20", 9, 10) == 2
        finally:
            dst.close()
