"""GPU tier of the per-member variability statistics and of the Gaussian likelihood over per-member vectors
(csrc/variability.hip; rscm_ens_member_variability, rscm_ens_loglik_vectors_device; Ensemble.variability, Ensemble.loglik_vectors,
GraphModel.variability).  The oracle is the numpy restatement of tests/host_variability.py on rows copied to the host, compared
by value (+0 equal to -0, any NaN equal to any NaN).

The data: two-layer ensembles with per-member forcing noise (noise_params=True, set_forcing_noise_members) on a 48-point annual
axis, half the members under zero forcing and half under a ramp.  From 63 members on, three members are special -- a silent one
under zero forcing (a constant series), one with a NaN parameter (NaN rows) and one with an amplitude that overflows -- and two
more have +Inf / -Inf written into one row."""
import ctypes as C

import numpy as np
import pytest

from tests import host_likelihood as hl
from tests import host_variability as hv
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import built_once, noise_ensemble, plant, refusal_code
from tests.helpers import annual_bounds, magicc_chain, same_values, two_layer_params

pytestmark = pytest.mark.gpu

T = 48
YEARS, BOUNDS = annual_bounds(T)
SEED = 20260327
DETREND = ("mean", "linear", "difference")
SIZES = [1, 63, 64, 257, 1000]       # a single member; below, at and past a wave; a ragged last block; more than one block
# the least; below, at and one past the load batch of 8; a batch, a pair and a single term (11 terms: plain from 11 rows, differenced
# from 12); two batches and one past; five
ROWS = [3, 4, 7, 8, 9, 10, 11, 12, 16, 17, 40]


def _ensemble(ra, n, offset=0, n_total=None, steps=None, **kw):
    return noise_ensemble(ra, n, BOUNDS, SEED, offset, n_total, steps, **kw)


@pytest.fixture(scope="module")
def cases(ra):
    """{N: (ensemble, its Surface Temperature series [T][N] on the host)}, each built and run once and left unchanged."""
    def build(n):
        e = _ensemble(ra, n)
        if n >= 63:
            for member, row, value in ((5, 1, np.inf), (7, 2, -np.inf)):
                plant(e, 1, member, row, value)
        ser = e.get_series(1)
        ser.setflags(write=False)
        return e, ser

    yield from built_once(build)


def _host(d):
    return {k: d[k].to_host() for k in hv.NAMES}


def _check(got, want, what):
    assert set(got) == set(hv.NAMES)
    for k in hv.NAMES:
        assert same_values(got[k], want[k]), (what, k, np.flatnonzero(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))[:5])


@pytest.mark.parametrize("n", SIZES)
def test_statistics_equal_the_restatement(ra, cases, n):
    e, ser = cases(n)
    if n >= 63:
        assert (ser[:, n - 3] == 0.0).all() and np.isnan(ser[1:, n - 1]).all() and not np.isfinite(ser[:, n - 2]).all()
        assert np.isposinf(ser[1, 5]) and np.isneginf(ser[2, 7])
    for detrend in DETREND:
        for R in ROWS:
            if detrend == "difference" and R == 3:
                assert refusal_code(e.variability, 1, 0, R, detrend=detrend) == 1       # two differences
                continue
            got, want = _host(e.variability(1, 0, R, detrend=detrend)), hv.variability(ser[:R], detrend)
            _check(got, want, (detrend, R))
            if n >= 63:
                assert got["variance"][n - 3] == 0.0 and got["sd"][n - 3] == 0.0 and np.isnan(got["r1"][n - 3])
                bad = ~np.isfinite(ser[:R]).all(axis=0)
                assert bad[[n - 1, 5, 7]].all() and not bad[:5].any() and (R < 40 or bad[n - 2])
                for k in hv.NAMES:
                    assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][:5]).all(), (detrend, R, k)
        _check(_host(e.variability(1, 2, T, 3, detrend=detrend)), hv.variability(ser[2:T:3], detrend), (detrend, "strided"))
        _check(_host(e.variability(1, T - 5, T, detrend=detrend, slot=3)), hv.variability(ser[T - 5:], detrend), (detrend, "last rows"))


def test_storage_layouts(ra):
    """A windowed graph's output-store rows give the statistics of the full-storage build of the same graph; rows that are not
    resident, or not yet computed, are refused."""
    mod = magicc_chain()
    name, n = "Surface Temperature", 301
    got = {}
    for key, kw in (("windowed", dict(series_window=16, output_stride=12)), ("full", {})):
        model = mod.build_chain(n, 30, "topological", steps_per_year=12, **kw)
        try:
            model.run()
            ens, vid = model.variable_home(name)
            n_times = ens.n_times
            got[key] = {d: _host(model.variability(name, 0, n_times, 12, detrend=d, slot=1)) for d in DETREND}
            if key == "full":
                ser = model.get_series(name, t_stride=12)
                for d in DETREND:
                    _check(got[key][d], hv.variability(ser, d), ("chain", d))
            else:
                assert refusal_code(model.variability, name, 0, 9, 3) == 2          # rows 3 and 6: outside the window and the output stride
        finally:
            model.close()
    for d in DETREND:
        _check(got["windowed"][d], got["full"][d], ("windowed against full", d))
    with _ensemble(ra, 64, steps=10) as e:
        assert e.time_index == 10
        assert refusal_code(e.variability, 1, 0, 20) == 2                           # rows beyond the time index
        e.variability(1, 0, 11)
    with ra.Ensemble(ra.KIND_TWO_LAYER, 64, BOUNDS, window_rows=8, output_stride=5) as w:    # (a windowed handle takes no noise rows)
        w.set_params(two_layer_params(64))
        w.set_forcing(0.05 * np.arange(T) + 0.3 * np.sin(YEARS))
        w.set_initial(1, 0.0)
        w.set_initial(2, 0.0)
        while w.time_index < T - 1:
            w.run(min(w.time_index + 4, T - 1))
        assert refusal_code(w.variability, 1, 0, 3) == 2                            # row 1 is neither in the window nor in the output store
        _check(_host(w.variability(1, 0, T, 5, detrend="difference")), hv.variability(w.get_series(1, 0, T, 5), "difference"), "output store")


def test_slots_and_refusals(ra, cases):
    e, ser = cases(257)
    ind = e.indicators(1, 0, 30, thresholds=[0.2, 0.5], slot=0)
    keep = [ind["mean"].to_host(), ind["peak"].to_host(), ind["peak_time"].to_host()] + [c.to_host() for c in ind["crossing"]]
    var = e.variability(1, 0, 30, slot=1)
    again = [ind["mean"].to_host(), ind["peak"].to_host(), ind["peak_time"].to_host()] + [c.to_host() for c in ind["crossing"]]
    assert all(same_values(a, b) for a, b in zip(keep, again))
    assert var["mean"].ptr != ind["mean"].ptr
    _check(_host(var), hv.variability(ser[:30], "linear"), "slot 1")
    assert e.variability(1, 0, 30, slot=0)["mean"].ptr == ind["mean"].ptr         # the slots are the indicators'
    assert refusal_code(e.variability, 1, 0, 30, slot=4) == 1
    assert refusal_code(e.variability, 1, 0, 30, slot=-1) == 1
    with pytest.raises(ValueError):
        e.variability(1, 0, 30, detrend="quadratic")
    p = C.c_void_p()
    for mode in (-1, 3):
        assert e._lib.rscm_ens_member_variability(e._h, 1, 0, 30, 1, mode, 0, C.byref(p)) == 1 and p.value is None
    assert e._lib.rscm_ens_member_variability(e._h, 0, 0, 30, 1, 0, 0, C.byref(p)) == 1       # no stored series
    assert refusal_code(e.variability, 1, 0, 2) == 1 and refusal_code(e.variability, 1, 5, 5) == 1
    with e.select(1, [0.5], 0, 30) as s:
        assert refusal_code(e.variability, 1, 0, 30) == 2
        while s.next_pass() is not None:
            s.commit()


@pytest.fixture(scope="module")
def scored(cases):
    """The 1000-member case with its statistics, an indicator and a parameter row, on the device and restated (computed once)."""
    e, ser = cases(1000)
    diff = e.variability(1, 0, T, detrend="difference", slot=1)
    lin = e.variability(1, 0, T, detrend="linear", slot=2)
    ind = e.indicators(1, T - 10, T, slot=3)
    want_diff, want_lin = hv.variability(ser, "difference"), hv.variability(ser, "linear")
    with np.errstate(all="ignore"):
        acc = ser[T - 10].copy()
        for r in ser[T - 9:T]:
            acc = acc + r
        mean10 = np.where(np.isnan(ser[T - 10:T]).any(axis=0), np.nan, acc / 10.0)
    sig_row = e.noise_param_rows[0]
    dev = [diff["sd"], diff["r1"], lin["slope"], lin["sd"], ind["mean"], e.params_vector(sig_row)]
    host = [want_diff["sd"], want_diff["r1"], want_lin["slope"], want_lin["sd"], mean10, e.get_params()[sig_row]]
    for d, h in zip(dev, host):
        assert same_values(d.to_host(), h)
    return e, ser, dev, host


@pytest.mark.parametrize("n_vec", [1, 2, 16])
def test_loglik_vectors_equal_the_restatement(scored, n_vec):
    e, ser, dev, host = scored
    pick = [(k + 1) % len(dev) for k in range(n_vec)]          # begins with r1: the NaN, Inf and constant members score -inf
    rng = np.random.default_rng(n_vec)
    values = [float(np.nanmedian(np.where(np.isfinite(host[k]), host[k], np.nan))) * rng.uniform(0.9, 1.1) for k in pick]
    sigmas = [float(rng.uniform(0.01, 0.3)) for _ in pick]
    got = e.loglik_vectors([dev[k] for k in pick], values, sigmas).to_host()
    want = hv.loglik_vectors([host[k] for k in pick], values, sigmas)
    assert np.array_equal(got, want)
    n = e.n_members
    assert np.isneginf(got[[n - 1, n - 2, n - 3, 5, 7]]).all() and np.isfinite(got[:5]).all()


def test_loglik_vectors_onto_a_point_likelihood(scored):
    e, ser, dev, host = scored
    tidx = list(range(4, T, 4))
    obs = [0.02 * t for t in tidx]
    sig = [0.5] * len(tidx)
    point = hl.loglik({1: ser}, [1] * len(tidx), tidx, obs, sig)
    ll = e.loglik([1] * len(tidx), tidx, obs, sig, on_device=True)
    assert np.array_equal(ll.to_host(), point) and np.isneginf(point).any()
    values, sigmas = [float(np.nanmedian(host[0])), float(np.nanmedian(host[1]))], [0.05, 0.2]
    out = e.loglik_vectors(dev[:2], values, sigmas, add_to=ll)                      # in place: the handle's likelihood vector
    assert out.ptr == ll.ptr
    want = hv.loglik_vectors(host[:2], values, sigmas, add=point)
    with np.errstate(all="ignore"):
        plain = point + hv.loglik_vectors(host[:2], values, sigmas)
    assert np.array_equal(want, np.where(np.isfinite(point) & np.isfinite(plain), plain, -np.inf))
    got = out.to_host()
    assert np.array_equal(got, want)
    assert np.isneginf(got[np.isneginf(point)]).all()
    # the weights and the weighted quantiles of the statistics, from the combined likelihood
    ll_max, bits = e.set_weights_from_loglik(out)
    ok = np.isfinite(want) & (e.status() == 0)
    assert ll_max == want[ok].max()
    ref = np.rint(np.exp(np.where(ok, want - ll_max, 0.0)) * 2.0 ** bits)
    w = e.member_weights()
    # (the device's exp and numpy's may differ in the last bit: one unit of the quantised weight, as for every set_weights_from_loglik)
    assert (w[~ok] == 0).all() and np.abs(w[ok] - ref[ok]).max() <= 1 and w.max() == 2 ** bits and (w > 0).sum() > 1
    q = [0.05, 0.5, 0.95]
    res = e.quantile_vectors(dev[:2], q, weighted=True)
    for k in range(2):
        live = ~np.isnan(host[k])
        assert res["weight"][k] == w[live].sum()
        assert np.array_equal(res["quantiles"][k], np.quantile(host[k][live], q, weights=w[live], method="inverted_cdf"))


def test_loglik_vectors_refusals(scored):
    e, ser, dev, host = scored
    assert refusal_code(e.loglik_vectors, dev[:1], [0.1], [0.0]) == 1
    assert refusal_code(e.loglik_vectors, dev[:1], [0.1], [-1.0]) == 1
    assert refusal_code(e.loglik_vectors, dev[:1], [0.1], [np.inf]) == 1
    assert refusal_code(e.loglik_vectors, dev[:1], [np.nan], [1.0]) == 1
    assert refusal_code(e.loglik_vectors, [], [], []) == 1
    assert refusal_code(e.loglik_vectors, [dev[0]] * 17, [0.1] * 17, [1.0] * 17) == 1
    with pytest.raises(ValueError):
        e.loglik_vectors(dev[:2], [0.1], [1.0])
    from rscm_amd import _lib
    one = np.array([1.0])
    host = np.zeros(e.n_members)
    harr = (C.POINTER(C.c_double) * 1)(_lib.dptr(host))
    p = C.c_void_p()
    assert e._lib.rscm_ens_loglik_vectors_device(e._h, 1, harr, _lib.dptr(one), _lib.dptr(one), None, C.byref(p)) == 1 and p.value is None
    darr = (C.POINTER(C.c_double) * 1)(C.cast(C.c_void_p(dev[0].ptr), C.POINTER(C.c_double)))
    assert e._lib.rscm_ens_loglik_vectors_device(e._h, 1, darr, _lib.dptr(one), _lib.dptr(one), _lib.dptr(host), C.byref(p)) == 1


def test_two_shards_give_the_halves(ra, cases):
    """Two handles over the halves of the 257 members (member_offset) hold the halves of the one handle's vectors."""
    n, k = 257, 129
    e, ser = cases(n)
    whole = {d: _host(e.variability(1, 4, T, detrend=d, slot=2)) for d in DETREND}     # (the rows from 4 on: none was overwritten)
    for offset, count in ((0, k), (k, n - k)):
        with _ensemble(ra, count, offset, n) as h:
            for d in DETREND:
                got = _host(h.variability(1, 4, T, detrend=d))
                for name in hv.NAMES:
                    assert same_values(got[name], whole[d][name][offset:offset + count]), (d, name, offset)
