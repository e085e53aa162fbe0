"""CPU tier: the yardstick of tests/test_gpu_device_math.py measured against itself (tests/host_math.py).  The ulp measure passes what is
accurate (the host's correctly-rounded-or-nearly log and exp), fails what is two steps off, keeps the books on zeros, infinities and
NaN; and the bulk reference (np.longdouble) is pinned to mpmath at 50 digits on a sample of every argument family and every edge."""
import numpy as np
import pytest

from tests import host_math as M

LD = M.LD


@pytest.fixture(scope="module")
def fam():
    return M.log_families()


def test_longdouble_width_is_checked_not_assumed():
    assert M.LONGDOUBLE_OK == (np.finfo(np.longdouble).nmant >= 63)
    x = np.linspace(1.0, 2.0, 50_000)
    idx, true = M.reference("log", x)
    assert idx.size == (x.size if M.LONGDOUBLE_OK else M.MP_FALLBACK) and true.shape == idx.shape and true.dtype == LD
    # the mpmath route gives the same answers whichever one is in use
    i2 = M.sample_indices(x.size, 64)
    assert float(M.ulp_error(np.log(x[i2]), M.mp_reference("log", x[i2])).max()) <= 1.0


def test_the_families_are_seeded_and_reach_what_they_are_for(fam):
    again = M.log_families()
    assert sorted(fam) == ["a", "b", "c", "d", "e"]
    for k, v in fam.items():
        assert v.shape == (M.FAMILY_SIZE,) and np.array_equal(v, again[k])
    e = np.frexp(fam["a"])[1]
    assert e.min() == -1021 and e.max() == 1024                      # every binade of the normals, both ends
    assert fam["b"].min() >= 0.5 and fam["b"].max() < 2.0 and fam["e"].min() >= 1.0 and fam["e"].max() < 4.0
    c = fam["c"]
    assert (c == 1.0).any() and (c == np.nextafter(1.0, 2.0)).any() and (c == np.nextafter(1.0, 0.0)).any() and (c < 0.01).any()
    m = np.frexp(fam["d"])[0]                                        # [0.5, 1): what log_f64 compares with the fold
    assert (m < M.SQRT_HALF).sum() > 1000 and (m >= M.SQRT_HALF).sum() > 1000
    assert (np.abs(m - M.SQRT_HALF) <= 2.0 ** -52).sum() >= 41       # the last step before the fold, in every binade
    assert len(set(np.frexp(fam["d"])[1])) >= 41
    assert (M.log_edges_normal() >= M.DBL_MIN).all() and np.isfinite(M.log_edges_normal()).all()
    o = M.log_edges_other()
    assert not ((o >= M.DBL_MIN) & np.isfinite(o)).any()             # each of them takes the fall-back branch
    ins, out = M.rcp_arguments()
    assert M.in_rcp_window(ins).all() and not M.in_rcp_window(out).any()
    assert (np.abs(ins) == 2.0 ** -128).any() and (np.abs(ins) == np.nextafter(2.0 ** 129, 0.0)).any()
    assert (np.abs(out) == 2.0 ** 129).any() and (np.abs(out) == np.nextafter(2.0 ** -128, 0.0)).any()


def test_the_hosts_log_and_exp_measure_within_one_ulp(fam):
    worst = {}
    for k, x in fam.items():
        idx, true = M.reference("log", x)
        worst["log " + k] = float(M.ulp_error(np.log(x[idx]), true).max())
    for k, x in M.exp_families().items():
        idx, true = M.reference("exp", x)
        worst["exp " + k] = float(M.ulp_error(np.exp(x[idx]), true).max())
    print({k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert min(worst.values()) > 0.25, worst          # a measure that reads 0 everywhere measures nothing


def test_two_steps_off_measures_at_least_one_and_a_half_ulp(fam):
    """The measure can fail: the correctly rounded result moved two doubles away measures 1.5 to 2.5 ulp.  (Results within two
    doubles of a power of two are left out of the count: the doubles change their spacing there, so two steps are 1 to 4 units
    of the true value's binade.  They are a handful.)"""
    for op, x in (("log", fam["b"]), ("log", fam["c"]), ("log", fam["a"]), ("exp", M.exp_families()["unit"])):
        idx, true = M.reference(op, x)
        with np.errstate(over="ignore"):
            rounded = true.astype(np.float64)
        m, _ = np.frexp(np.abs(rounded))
        ok = np.isfinite(rounded) & (np.abs(rounded) > 1e-300) & (m > 0.5 + 2.0 ** -52) & (m < 1.0 - 2.0 ** -52)
        assert ok.sum() > 0.9 * (rounded != 0.0).sum() > 0.5 * idx.size
        assert float(M.ulp_error(rounded[ok], true[ok]).max()) <= 0.5
        for k in (2, -2):
            off = M.ulp_error(M.steps_off(rounded[ok], k), true[ok])
            assert float(off.min()) >= 1.5 and float(off.max()) <= 2.5


def test_zero_rule_and_nonfinite_bookkeeping():
    inf, nan = np.inf, np.nan
    E = lambda got, true: [float(v) for v in np.atleast_1d(M.ulp_error(got, np.asarray(true, dtype=LD)))]   # noqa: E731
    assert E([0.0, -0.0, 5e-324, -5e-324], [0.0, 0.0, 0.0, 0.0]) == [0.0, 0.0, inf, inf]       # a true 0 demands 0
    assert E([nan, 1.0, inf], [nan, nan, nan]) == [0.0, inf, inf]                              # a true NaN demands NaN
    assert E([inf, -inf, 1e308, nan], [inf, inf, inf, inf]) == [0.0, inf, inf, inf]            # an infinity demands itself
    assert E([-inf, inf], [-inf, -inf]) == [0.0, inf]
    assert E([nan, inf, -inf], [1.0, 1.0, 1.0]) == [inf, inf, inf]                             # nothing non-finite for a finite truth
    big = np.ldexp(LD(1.0), 1024)                                                              # beyond the doubles: rounds to inf
    assert E([inf, M.DBL_MAX], [big, big]) == [0.0, inf]
    # units: 2^-52 in [1, 2), 2^-53 in [0.5, 1), 2^-1074 for every denormal and for what rounds to 0
    assert E([1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 0.75 + 2.0 ** -53], [1.0, 1.0, 0.75]) == [1.0, 0.5, 1.0]
    assert E([1e-310 + 5e-324, 0.0, 5e-324], [LD(1e-310), np.ldexp(LD(1.0), -1076), np.ldexp(LD(1.0), -1076)]) == [1.0, 0.25, 0.75]
    # the unit is the binade of the true value ROUNDED to double: just below 2 it rounds to 2
    t = LD(2.0) - np.ldexp(LD(1.0), -60)
    assert E([2.0], [t])[0] == pytest.approx(2.0 ** -60 / 2.0 ** -51)
    assert float(M.ulp_of(t)) == 2.0 ** -51 and float(M.ulp_of(LD(1.5))) == 2.0 ** -52


def test_mpmath_pins_the_longdouble_reference(fam):
    """np.longdouble's log / exp / pow / reciprocal against mpmath at 50 digits on MP_SAMPLE arguments of every family and on every
    edge argument: they agree to 2^-9 ulp of a double, so a bound of 1 or 2 ulp measured against either is the same bound."""
    if not M.LONGDOUBLE_OK:      # np.longdouble is no wider than double here: the bulk reference IS mpmath, nothing is left to pin
        x = fam["b"][:8]
        assert np.array_equal(M.reference("log", x)[1], M.mp_reference("log", x))
        return
    worst = {}

    def pin(name, op, x, y=None):
        i = M.sample_indices(len(x), M.MP_SAMPLE)
        xs, ys = x[i], (None if y is None else y[i])
        mp = M.mp_reference(op, xs, ys)
        ld = M.ld_reference(op, xs, ys)
        fin = np.isfinite(mp)
        assert np.array_equal(np.isnan(mp), np.isnan(ld)) and np.array_equal(mp[~fin & ~np.isnan(mp)], ld[~fin & ~np.isnan(mp)])
        with np.errstate(invalid="ignore"):
            d = np.abs(ld[fin] - mp[fin]) / M.ulp_of(mp[fin])
        worst[name] = float(d.max())

    for k, x in fam.items():
        pin("log " + k, "log", x)
    pin("log edges", "log", np.concatenate([M.log_edges_normal(), M.log_edges_other()]))
    for k, x in M.exp_families().items():
        pin("exp " + k, "exp", x)
    pin("exp edges", "exp", M.exp_edges())
    px, py = M.pow_arguments()
    pin("pow", "pow", px, py)
    ins, out = M.rcp_arguments()
    pin("rcp", "rcp", ins)
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= M.PIN, worst
