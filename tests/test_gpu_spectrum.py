"""GPU tier of the per-member band powers and of the spectral likelihood over them (csrc/spectrum.hip; rscm_ens_member_spectrum,
rscm_ens_loglik_spectrum_device; Ensemble.spectrum, Ensemble.loglik_spectrum, GraphModel.spectrum).  The oracle of the statistic is
the numpy restatement of tests/host_spectrum.py on rows copied to the host, compared by value (+0 equal to -0, any NaN equal to
any NaN); the likelihood takes logarithms and is held to a derived bound against the restatement in np.longdouble.

The data are those of tests/test_gpu_variability.py on a longer axis: two-layer ensembles with per-member forcing noise
(noise_params=True, set_forcing_noise_members) on a 72-point annual axis (4 F + 8 with the kernel's tile of F = 16 frequencies), half
the members under zero forcing and half under a ramp.  From 63 members on, three members are special -- a silent one under zero
forcing (a constant series), one with a NaN parameter (NaN rows) and one with an amplitude that overflows -- and two more have
+Inf / -Inf written into one row."""
import ctypes as C

import numpy as np
import pytest

from tests import host_likelihood as hl
from tests import host_spectrum as hs
from tests import host_variability as hv
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import built_once, noise_ensemble, plant, refusal_code
from tests.helpers import annual_bounds, magicc_chain, same_values, two_layer_params

pytestmark = pytest.mark.gpu

F = 16                               # kSpecF of csrc/spectrum.hip: the frequencies a lane carries per pass over the rows
T = 4 * F + 8
YEARS, BOUNDS = annual_bounds(T)
SEED = 20260327
DETREND = ("mean", "linear", "difference")
SIZES = [1, 63, 64, 257, 1000]       # a single member; below, at and past a wave; a ragged last block; more than one block
# Working-series lengths n: J = (n - 1) // 2 = 1 (n = 3 and 4); 7, 8, 9 and 10 terms (below, at and past the load batch of 8 rows, in
# every mode: "difference" reads one row more); J = F - 1 (31, 32), F (33, 34), F + 1 (35, 36), 2 F + 1 (67, 68): a partial tile, a
# full one, one frequency into the second, one into the third -- each with an odd and an even n (the recurrence's last term lands in
# either register set)
TERMS = [3, 4, 7, 8, 9, 10, 2 * F - 1, 2 * F, 2 * F + 1, 2 * F + 2, 2 * F + 3, 2 * F + 4, 4 * F + 3, 4 * F + 4]


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
    return {"mean": d["mean"].to_host(), "slope": d["slope"].to_host(), "variance": d["variance"].to_host(),
            "power": [p.to_host() for p in d["power"]]}


def _vectors(d):
    return [d[k] for k in hs.FIRST] + list(d["power"])


def _check(got, want, what):
    gv, wv = _vectors(got), _vectors(want)
    assert len(gv) == len(wv), what
    for k, (g, w) in enumerate(zip(gv, wv)):
        assert same_values(g, w), (what, k, np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])


def _band_choices(n):
    """bands = 1, 3, 8 (fewer where the series has fewer frequencies) and one explicit edge list that leaves frequencies out at both ends."""
    J = (n - 1) // 2
    out = [1, 3, 8]
    if J >= 5:
        out.append([2, 4, J])                       # frequency 1 and frequency J belong to no band
    return out


@pytest.mark.parametrize("n", SIZES)
def test_spectrum_equals_the_restatement(ra, cases, n):
    from rscm_amd.variability import band_edges
    e, ser = cases(n)
    if n >= 63:
        assert (ser[:, n - 3] == 0.0).all() and np.isnan(ser[1:, n - 1]).all() and not np.isfinite(ser[:, n - 2]).all()
        assert np.isposinf(ser[1, 5]) and np.isneginf(ser[2, 7])
    for detrend in DETREND:
        extra = 1 if detrend == "difference" else 0
        for terms in TERMS:
            R = terms + extra
            rows = ser[:R]
            for bands in _band_choices(terms):
                d = e.spectrum(1, 0, R, detrend=detrend, bands=bands)
                edges = band_edges(terms, bands) if isinstance(bands, int) else np.asarray(bands)
                assert np.array_equal(d["edges"], edges) and np.array_equal(d["counts"], np.diff(edges)) and len(d["power"]) == len(edges) - 1
                got, want = _host(d), hs.spectrum(rows, detrend, edges)
                _check(got, want, (detrend, terms, bands))
                if n >= 63:
                    assert got["variance"][n - 3] == 0.0 and all(p[n - 3] == 0.0 for p in got["power"])
                    bad = ~np.isfinite(rows).all(axis=0)
                    assert bad[[n - 1, 5, 7]].all() and not bad[:5].any()
                    for v in _vectors(got):
                        assert np.isnan(v[bad]).all() and np.isfinite(v[:5]).all(), (detrend, terms, bands)
        strided = ser[2:T:3]
        _check(_host(e.spectrum(1, 2, T, 3, detrend=detrend, bands=3)), hs.spectrum(strided, detrend, band_edges(len(strided) - extra, 3)),
               (detrend, "strided"))
        _check(_host(e.spectrum(1, T - 12, T, detrend=detrend, bands=[1, 2, 4], slot=3)), hs.spectrum(ser[T - 12:], detrend, [1, 2, 4]),
               (detrend, "last rows"))


def test_first_three_are_variabilitys_bits(cases):
    e, ser = cases(257)
    for detrend in DETREND:
        for R in (9, 40, T):
            var = e.variability(1, 0, R, detrend=detrend, slot=0)
            want = {k: var[k].to_host() for k in hs.FIRST}
            spec = e.spectrum(1, 0, R, detrend=detrend, slot=1)
            for k in hs.FIRST:
                assert same_values(spec[k].to_host(), want[k]), (detrend, R, k)
            ref = hv.variability(ser[:R], detrend)
            assert all(same_values(want[k], ref[k]) for k in hs.FIRST)


def test_storage_layouts(ra):
    """A windowed graph's output-store rows give the band powers of the full-storage build of the same graph; rows that are not
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
            got[key], edges = {}, {}
            for d in DETREND:                                             # (one slot: each result is copied before the next call)
                res = model.spectrum(name, 0, n_times, 12, detrend=d, slot=1)
                got[key][d], edges[d] = _host(res), res["edges"]
            if key == "full":
                ser = model.get_series(name, t_stride=12)
                for d in DETREND:
                    _check(got[key][d], hs.spectrum(ser, d, edges[d]), ("chain", d))
            else:
                assert refusal_code(model.spectrum, name, 0, 9, 3) == 2          # rows 3 and 6: outside the window and the output stride
        finally:
            model.close()
    for d in DETREND:
        _check(got["windowed"][d], got["full"][d], ("windowed against full", d))
    with _ensemble(ra, 64, steps=10) as e:
        assert e.time_index == 10
        assert refusal_code(e.spectrum, 1, 0, 20) == 2                           # rows beyond the time index
        e.spectrum(1, 0, 11)


def test_slots_and_refusals(ra, cases):
    e, ser = cases(257)
    var = e.variability(1, 0, 30, slot=0)
    keep = {k: var[k].to_host() for k in hv.NAMES}
    spec = e.spectrum(1, 0, 40, detrend="linear", bands=8, slot=1)
    assert all(same_values(var[k].to_host(), keep[k]) for k in hv.NAMES)
    assert spec["mean"].ptr != var["mean"].ptr
    kept = _host(spec)
    _check(kept, hs.spectrum(ser[:40], "linear", spec["edges"]), "slot 1")
    e.variability(1, 0, 30, detrend="mean", slot=0)
    e.indicators(1, 0, 30, thresholds=[0.2], slot=2)
    _check(_host(spec), kept, "slot 1 after calls on slots 0 and 2")
    assert e.spectrum(1, 0, 30, slot=0)["mean"].ptr == var["mean"].ptr          # the slots are the indicators'
    assert refusal_code(e.spectrum, 1, 0, 30, slot=4) == 1
    assert refusal_code(e.spectrum, 1, 0, 30, slot=-1) == 1
    with pytest.raises(ValueError):
        e.spectrum(1, 0, 30, detrend="quadratic")
    p = C.c_void_p()
    two = (C.c_int32 * 2)(1, 2)
    for mode in (-1, 3):
        assert e._lib.rscm_ens_member_spectrum(e._h, 1, 0, 30, 1, mode, 1, two, 0, C.byref(p)) == 1 and p.value is None
    assert e._lib.rscm_ens_member_spectrum(e._h, 0, 0, 30, 1, 0, 1, two, 0, C.byref(p)) == 1       # no stored series
    assert e._lib.rscm_ens_member_spectrum(e._h, 1, 0, 30, 1, 0, 1, None, 0, C.byref(p)) == 1      # no edges
    # too short: two terms, and two differences
    assert refusal_code(e.spectrum, 1, 0, 2, detrend="mean") == 1 and refusal_code(e.spectrum, 1, 0, 3, detrend="difference") == 1
    assert refusal_code(e.spectrum, 1, 5, 5) == 1
    # the edges: 30 rows, "mean": n = 30, J = 14, edges inside [1, 15]
    for edges in ([1, 5, 5], [3, 2], [0, 4], [1, 16], [-1, 3], list(range(1, 11))):
        assert refusal_code(e.spectrum, 1, 0, 30, detrend="mean", bands=edges) == 1, edges
    e.spectrum(1, 0, 30, detrend="mean", bands=[1, 15])
    e.spectrum(1, 0, 30, detrend="mean", bands=list(range(1, 10)))
    assert refusal_code(e.spectrum, 1, 0, 28, detrend="difference", bands=[1, 15]) == 1       # n = 27: J + 1 = 14
    with e.select(1, [0.5], 0, 30) as s:
        assert refusal_code(e.spectrum, 1, 0, 30) == 2
        while s.next_pass() is not None:
            s.commit()


def test_more_than_4096_terms_are_refused(ra):
    """n = 4096 is served (against the restatement), n = 4097 is refused: the cap that bounds the recurrence's error."""
    steps = 4098
    bounds = np.arange(1000.0, 1000.0 + steps + 1)
    with ra.Ensemble(ra.KIND_TWO_LAYER, 64, bounds, noise_params=True) as e:
        P = np.vstack([two_layer_params(64), np.full(64, 0.3), np.linspace(0.0, 0.9, 64)])
        e.set_params(P)
        e.set_forcing(np.zeros(steps))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.set_forcing_noise_members(SEED, 0)
        e.run()
        assert refusal_code(e.spectrum, 1, 0, 4097, detrend="mean") == 1
        assert refusal_code(e.spectrum, 1, 0, 4098, detrend="difference") == 1
        d = e.spectrum(1, 0, 4097, detrend="difference")
        _check(_host(d), hs.spectrum(e.get_series(1, 0, 4097), "difference", d["edges"]), "4096 terms")


# ---- the likelihood --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scored(cases):
    """The 1000-member case with sixteen band powers on the device (two detrenders, eight bands each) and on the host, the bands'
    counts, and a record's band powers to score against (computed once)."""
    from rscm_amd.variability import series_spectrum
    e, ser = cases(1000)
    diff = e.spectrum(1, 0, T, detrend="difference", slot=1)
    lin = e.spectrum(1, 0, T, detrend="linear", slot=2)
    assert len(diff["power"]) == len(lin["power"]) == 8
    dev = list(diff["power"]) + list(lin["power"])
    host = [p.to_host() for p in dev]
    want = hs.spectrum(ser, "difference", diff["edges"])["power"] + hs.spectrum(ser, "linear", lin["edges"])["power"]
    assert all(same_values(h, w) for h, w in zip(host, want))
    counts = [int(c) for c in diff["counts"]] + [int(c) for c in lin["counts"]]
    rec = ser[:, 2]                                                    # one member's series serves as the record
    record = series_spectrum(rec, "difference", diff["edges"])["power"] + series_spectrum(rec, "linear", lin["edges"])["power"]
    assert all(np.isfinite(r) and r > 0.0 for r in record)
    return e, ser, dev, host, counts, record


def _check_loglik(got, power, record, counts, add=None):
    """The bound.  The restatement in np.longdouble (t = P + I_b formed in float64, as the definition forms it; the logarithms and
    all that follows in longdouble) is exact to well below a double's rounding.  On the device, per band: log_f64 is
    pinned to 1 ulp (tests/test_gpu_device_math.py), so ln P and ln t each err by at most 2^-52 of their size; the doubling of ln t
    is exact; the subtraction and the product with m_b round to half an ulp each of values no larger than m_b (|ln P| + 2 |ln t|);
    each of the at most B accumulations of `partial` and the final `add + partial` round to half an ulp of a partial sum no larger
    than the total |add| + sum_b m_b (|ln P_b| + 2 |ln t_b|).  Summed: at most (1 + 1/2 + 1/2) 2^-52 of the band's magnitude from
    the band's own operations and (B + 1) / 2 * 2^-52 of the total from the sums, with second-order terms inside the margin the
    statement below leaves: (4 + B) 2^-52 (|add_i| + sum_b m_b (|ln P_b| + 2 |ln t_b|))."""
    B = len(power)
    want = hs.loglik_spectrum(power, record, counts, add=add, dtype=hs.LD)
    mag = hs.loglik_spectrum_magnitude(power, record, counts, add=add)
    dead = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), dead) and np.isfinite(got[~dead]).all()
    err = np.abs(got[~dead].astype(hs.LD) - want[~dead])
    bound = hs.LD(4 + B) * hs.LD(2.0) ** -52 * mag[~dead]
    print(f"B = {B}: largest error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    return want


@pytest.mark.parametrize("n_vec", [1, 2, 16])
def test_loglik_spectrum_within_its_bound(scored, n_vec):
    e, ser, dev, host, counts, record = scored
    pick = list(range(n_vec))
    got = e.loglik_spectrum([dev[k] for k in pick], [record[k] for k in pick], [counts[k] for k in pick]).to_host()
    _check_loglik(got, [host[k] for k in pick], [record[k] for k in pick], [counts[k] for k in pick])
    n = e.n_members
    assert np.isneginf(got[[n - 1, n - 2, n - 3, 5, 7]]).all() and np.isfinite(got[:5]).all()      # NaN, overflow, constant, +-Inf rows


def test_loglik_spectrum_onto_a_point_likelihood(scored):
    e, ser, dev, host, counts, record = scored
    tidx = list(range(4, T, 4))
    obs = [0.02 * t for t in tidx]
    sig = [0.5] * len(tidx)
    point = hl.loglik({1: ser}, [1] * len(tidx), tidx, obs, sig)
    ll = e.loglik([1] * len(tidx), tidx, obs, sig, on_device=True)
    assert np.array_equal(ll.to_host(), point) and np.isneginf(point).any()
    out = e.loglik_spectrum(dev[:8], record[:8], counts[:8], add_to=ll)                  # in place: the handle's likelihood vector
    assert out.ptr == ll.ptr
    got = out.to_host()
    _check_loglik(got, host[:8], record[:8], counts[:8], add=point)
    assert np.isneginf(got[np.isneginf(point)]).all()
    # the weights take the result as they take any log-likelihood
    ll_max, bits = e.set_weights_from_loglik(e.loglik_spectrum(dev[:8], record[:8], counts[:8]))
    assert np.isfinite(ll_max) and (e.member_weights() > 0).sum() > 1


def test_loglik_spectrum_refusals(scored):
    e, ser, dev, host, counts, record = scored
    assert refusal_code(e.loglik_spectrum, dev[:1], [0.0], [1]) == 1
    assert refusal_code(e.loglik_spectrum, dev[:1], [-1.0], [1]) == 1
    assert refusal_code(e.loglik_spectrum, dev[:1], [np.nan], [1]) == 1
    assert refusal_code(e.loglik_spectrum, dev[:1], [np.inf], [1]) == 1
    assert refusal_code(e.loglik_spectrum, dev[:1], [0.1], [0]) == 1
    assert refusal_code(e.loglik_spectrum, dev[:1], [0.1], [-2]) == 1
    assert refusal_code(e.loglik_spectrum, [], [], []) == 1
    assert refusal_code(e.loglik_spectrum, [dev[0]] * 17, [0.1] * 17, [1] * 17) == 1
    e.loglik_spectrum([dev[0]] * 16, [0.1] * 16, [1] * 16)
    with pytest.raises(ValueError):
        e.loglik_spectrum(dev[:2], [0.1], [1])
    from rscm_amd import _lib
    one, cnt = np.array([1.0]), (C.c_int32 * 1)(1)
    host_vec = np.zeros(e.n_members)
    harr = (C.POINTER(C.c_double) * 1)(_lib.dptr(host_vec))
    p = C.c_void_p()
    assert e._lib.rscm_ens_loglik_spectrum_device(e._h, 1, harr, _lib.dptr(one), cnt, None, C.byref(p)) == 1 and p.value is None
    darr = (C.POINTER(C.c_double) * 1)(C.cast(C.c_void_p(dev[0].ptr), C.POINTER(C.c_double)))
    assert e._lib.rscm_ens_loglik_spectrum_device(e._h, 1, darr, _lib.dptr(one), cnt, _lib.dptr(host_vec), C.byref(p)) == 1


def test_two_shards_give_the_halves(ra, cases):
    """Two handles over the halves of the 257 members (member_offset) hold the halves of the one handle's vectors."""
    n, k = 257, 129
    e, ser = cases(n)
    whole = {d: _host(e.spectrum(1, 4, T, detrend=d, slot=2)) for d in DETREND}     # (the rows from 4 on: none was overwritten)
    for offset, count in ((0, k), (k, n - k)):
        with _ensemble(ra, count, offset, n) as h:
            for d in DETREND:
                got = _host(h.spectrum(1, 4, T, detrend=d))
                for g, w in zip(_vectors(got), _vectors(whole[d])):
                    assert same_values(g, w[offset:offset + count]), (d, offset)
