"""The hand-written math primitives of csrc/rk4_device.hpp and csrc/chem_body.hpp -- log_f64, chem::pow_ratio, guarded_rcp -- and the device
library's log / exp as this library is compiled, on the GPU through rscm_gpu_selftest_math, against a high-precision reference
(tests/host_math.py: np.longdouble pinned to mpmath at 50 digits; the measure is ulp_error, units in the last place of a double).

The bounds are the code's own claims, not measurements: log_f64's header promises <= 1 ulp and the library's log for everything that
is not a positive normal; the kinds' parity tests (test_gpu_parity.py, test_gpu_chem.py, test_gpu_halocarbon.py, test_gpu_pointwise.py)
rest their tolerances on "device exp / log <= 1-2 ulp".  Each test prints what it measures before it asserts."""
import numpy as np
import pytest

from tests import host_math as M
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import bits

pytestmark = pytest.mark.gpu
LD = M.LD
OP_LOG_F64, OP_LOG, OP_EXP, OP_POW_RATIO, OP_GUARDED_RCP = range(5)


@pytest.fixture(scope="module")
def math(ra):
    from rscm_amd.ensemble import selftest_math
    return selftest_math


@pytest.fixture(scope="module")
def logs():
    """The log arguments of both log tests and their reference, computed once: families a-e back to back, then the normal edges.
    (idx, true) per family as host_math.reference gives them; the edges through mpmath."""
    fam = M.log_families()
    edges = M.log_edges_normal()
    x = np.concatenate([fam[k] for k in "abcde"] + [edges])
    ref, at = {}, 0
    for k in "abcde":
        idx, true = M.reference("log", fam[k])
        ref[k] = (at + idx, true)
        at += fam[k].size
    ref["edges"] = (at + np.arange(edges.size), M.mp_reference("log", edges))
    x.setflags(write=False)
    return fam, x, ref


def _maxima(got, ref):
    return {k: float(M.ulp_error(got[idx], true).max()) for k, (idx, true) in ref.items()}


def test_log_f64_within_its_stated_bound(math, logs):
    """log_f64 <= 1 ulp (its header's claim) on the families a-e and the normal edge arguments (1 and its neighbours, 0.5, 2, the fold
    sqrt(1/2) and its neighbours, DBL_MIN and the double above it, DBL_MAX); log_f64(1) = +0 exactly -- CO2ERF's known answer at the
    pre-industrial concentration rests on it; non-decreasing across the fold m < sqrt(1/2) in every binade of family d.

    Measured on an MI355X (gfx950), maximum ulp_error per family:
        a 0.6909   b 0.7852   c 0.7329   d 0.7910   e 0.7739   edges 0.2500"""
    fam, x, ref = logs
    got = math(OP_LOG_F64, x)
    worst = _maxima(got, ref)
    print("log_f64 max ulp:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    one = x == 1.0
    assert one.sum() > 100 and (got[one] == 0.0).all() and not np.signbit(got[one]).any()
    d = fam["d"]
    out_d = got[3 * M.FAMILY_SIZE:4 * M.FAMILY_SIZE]
    binade = np.frexp(d)[1]
    both_sides = 0
    for k in np.unique(binade):
        sel = binade == k
        order = np.argsort(d[sel], kind="stable")
        xs, ys = d[sel][order], out_d[sel][order]
        assert (np.diff(ys) >= 0.0).all(), f"log_f64 decreases inside binade {k}"
        m = np.frexp(xs)[0]
        both_sides += bool((m < M.SQRT_HALF).any() and (m >= M.SQRT_HALF).any())
    assert both_sides >= 41                                              # the fold was crossed in that many binades


def test_log_f64_fallback_branch_is_the_librarys_log(math):
    """Everything that is not a positive normal takes the library's log: denormals within 1 ulp; +-0 -> -inf; negatives and -inf ->
    NaN; +inf -> +inf; NaN -> NaN; and op 0 equals op 1 bit for bit on all of them -- it is the same call.

    Measured on an MI355X: denormals max 0.5000 ulp."""
    rng = np.random.default_rng(5)
    den = np.concatenate([np.ldexp(rng.random(4096), -1022), np.ldexp(1.0 + rng.random(2048), rng.integers(-1074, -1022, 2048)),
                          [5e-324, 1e-310, np.nextafter(M.DBL_MIN, 0.0)]])
    den = den[(den > 0.0) & (den < M.DBL_MIN)]
    neg = -np.concatenate([np.ldexp(1.0 + rng.random(1024), rng.integers(-1022, 1024, 1024)), den[:64], [1.0, M.DBL_MAX, M.DBL_MIN]])
    other = M.log_edges_other()
    x = np.concatenate([den, neg, other])
    assert not ((x >= M.DBL_MIN) & np.isfinite(x)).any()
    mine, lib = math(OP_LOG_F64, x), math(OP_LOG, x)
    assert np.array_equal(bits(mine), bits(lib))
    err = M.ulp_error(mine[:den.size], M.mp_reference("log", den))
    print("log_f64 on denormals, max ulp:", round(float(err.max()), 4))
    assert float(err.max()) <= 1.0
    assert np.isnan(mine[den.size:den.size + neg.size]).all()
    want = dict(zip(("below DBL_MIN", "5e-324", "1e-310", "+0", "-0", "-1", "-inf", "+inf", "nan"), mine[den.size + neg.size:]))
    assert want["+0"] == -np.inf and want["-0"] == -np.inf and want["+inf"] == np.inf
    assert np.isnan(want["-1"]) and np.isnan(want["-inf"]) and np.isnan(want["nan"])
    assert float(M.ulp_error(list(want.values())[:3], M.mp_reference("log", other[:3])).max()) <= 1.0


def test_library_log_and_exp_within_two_ulp(math, logs):
    """The premise of the kinds' tolerances ("device exp / log <= 1-2 ulp"): the device library's log on the families a-e and its exp
    on 2^18 arguments uniform in [-700, 700], 2^18 in [-1, 1] and the edges 0, +-709.78, -745.2, 710, +-inf, NaN, each <= 2 ulp; the
    overflow, underflow and NaN results exact.

    Measured on an MI355X, maximum ulp_error:
        log   a 0.5498   b 0.6343   c 0.6240   d 0.6299   e 0.6313   edges 0.2500
        exp   wide 0.8379   unit 0.8198   edges 0.4677"""
    _, x, ref = logs
    worst = {"log " + k: v for k, v in _maxima(math(OP_LOG, x), ref).items()}
    fam = M.exp_families()
    edges = M.exp_edges()
    xe = np.concatenate([fam["wide"], fam["unit"], edges])
    got = math(OP_EXP, xe)
    at = 0
    for k in ("wide", "unit"):
        idx, true = M.reference("exp", fam[k])
        worst["exp " + k] = float(M.ulp_error(got[at + idx], true).max())
        at += fam[k].size
    g = got[at:]
    worst["exp edges"] = float(M.ulp_error(g, M.mp_reference("exp", edges)).max())
    print("library log / exp max ulp:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 2.0, worst
    by = dict(zip((0.0, 709.78, -709.78, -745.2, 710.0, "+inf", "-inf", "nan"), g))
    assert by[0.0] == 1.0 and by[710.0] == np.inf and by["+inf"] == np.inf                     # overflow
    assert by[-745.2] == 0.0 and by["-inf"] == 0.0 and not np.signbit([by[-745.2], by["-inf"]]).any()   # underflow (exp(-745.2) < 2^-1075)
    assert np.isnan(by["nan"]) and np.isfinite(by[709.78]) and 0.0 < by[-709.78] < M.DBL_MIN   # the last finite / a denormal result


def test_pow_ratio_over_its_call_sites_ranges_and_beyond(math):
    """chem::pow_ratio(x, y) = exp(y * log_f64(x)) for x in [1, 16) (a block on 1, a block just above it) and y in [-2, 2] (which
    covers ozone's exp(p2 * log_f64(.)) too), against x^y in np.longdouble / mpmath.  Per element the relative error is at most
    2^-52 * (1.5 |y ln x| + 2) * 1.01: log_f64's 1 ulp and the product's half ulp are errors of the exponent, relative
    (1 + 0.5) 2^-52 of |y ln x| in absolute terms, which is what they cost the power in relative terms; 2 is exp's own bound (above);
    1.01 covers the second-order terms.  Exactly 1.0 for x == 1 with any y and for any x with y == 0: what fmax(ratio, 1.0) hands
    the Prather iterations in a pre-industrial year.

    Measured on an MI355X: largest error / bound 0.4848 (0.4172 on the mpmath sample); largest error 4.39 * 2^-52, at |y ln x| = 4.89."""
    x, y = M.pow_arguments()
    got = math(OP_POW_RATIO, x, y)
    idx, true = M.reference("pow", x, y)
    i2 = M.sample_indices(x.size, M.MP_SAMPLE)
    for ii, tt in ((idx, true), (i2, M.mp_reference("pow", x[i2], y[i2]))):
        rel = np.abs(got[ii].astype(LD) - tt) / tt
        expo = np.abs(y[ii].astype(LD) * np.log(x[ii].astype(LD)))
        bound = np.ldexp(LD(1.0), -52) * (LD(1.5) * expo + 2) * LD(1.01)
        worst = int(np.argmax(rel / bound))
        print(f"pow_ratio: max error / bound {float((rel / bound)[worst]):.4f}; max error {float(rel.max() * 2.0 ** 52):.3f} * 2^-52 "
              f"(|y ln x| = {float(expo[int(np.argmax(rel))]):.2f}) over {ii.size}")
        assert (rel <= bound).all(), (x[ii][worst], y[ii][worst], float(rel[worst]), float(bound[worst]))
    flat = (x == 1.0) | (y == 0.0)
    assert (x == 1.0).sum() > 1000 and (y == 0.0).sum() > 1000 and ((x == 1.0) & (y != 0.0)).any() and ((y == 0.0) & (x != 1.0)).any()
    assert (got[flat] == 1.0).all()


def test_guarded_rcp_inside_and_outside_the_divisor_window(math):
    """guarded_rcp(d): inside the divisor window |d| in [2^-128, 2^129) the refined reciprocal, within 1 ulp of 1/d (two Newton steps:
    expect about 0.5); outside it -- zeros, denormals, the normals beyond either edge, DBL_MAX, infinities, NaN -- the IEEE quotient
    1.0 / d, bit for bit the host's.  Both edges are approached from both sides, in both signs.

    Measured on an MI355X: inside the window max 0.5000 ulp; 12 of 262400 results differ from the correctly rounded quotient."""
    inside, outside = M.rcp_arguments()
    assert M.in_rcp_window(inside).all() and not M.in_rcp_window(outside).any()
    got = math(OP_GUARDED_RCP, np.concatenate([inside, outside]))
    gi, go = got[:inside.size], got[inside.size:]
    idx, true = M.reference("rcp", inside)
    err = M.ulp_error(gi[idx], true)
    with np.errstate(divide="ignore", over="ignore"):
        host_in, host_out = 1.0 / inside, 1.0 / outside
    print(f"guarded_rcp inside the window: max {float(err.max()):.4f} ulp, {int((gi != host_in).sum())} of {gi.size} not correctly rounded")
    assert float(err.max()) <= 1.0
    nan = np.isnan(outside)
    assert nan.sum() == 1 and np.isnan(go[nan]).all()
    assert np.array_equal(bits(go[~nan]), bits(host_out[~nan]))        # signed zeros, signed infinities and denormal quotients included
    assert np.isinf(go).sum() > 100 and ((go != 0.0) & (np.abs(go) < M.DBL_MIN)).sum() > 100


@pytest.mark.parametrize("n", [1, 65])
def test_co2_erf_is_relatively_accurate_next_to_preindustrial(ra, n):
    """One call site with a RELATIVE bound (the kinds' own tests hold this row to an absolute 1e-12): RSCM_KIND_CO2_ERF on a table input,
    64 rows, concentrations conc_pi (1 +- 2^-j) for j = 1..50 (and a few between them) and conc_pi itself, every member with its own
    conc_pi and erf_2xco2.  Reference: fl(erf_2xco2 / ln 2) * ln(arg) in mpmath with arg = 1.0 + (c - pi) / pi formed in numpy double
    -- the IEEE operations the kernel performs, so its argument bit for bit.  Relative error at most 2 * 2^-52: 1 ulp of the
    logarithm and half an ulp of the product are 1.5 * 2^-52, the rest is slack for the binade edges.  Exactly 0.0 at c == conc_pi.

    Measured on an MI355X: largest relative error 0.838 * 2^-52 (n = 1), 0.948 * 2^-52 (n = 65)."""
    import mpmath
    mpmath.mp.dps = M.MP_DIGITS
    T = 64
    rng = np.random.default_rng(n)
    erf2x = np.full(n, 3.7) if n == 1 else rng.uniform(3.0, 4.5, n)
    pi = np.full(n, 278.0) if n == 1 else rng.uniform(260.0, 300.0, n)
    scale = erf2x / 0.693147180559945309417
    j = np.arange(1, 51)
    between = np.arange(2, 14)
    worst = 0.0
    for sign in (1.0, -1.0):
        factor = np.concatenate([[1.0], 1.0 + sign * np.ldexp(1.0, -j), 1.0 + sign * np.ldexp(1.5, -between), [1.0]])
        assert factor.size == T
        conc = pi[:, None] * factor[None, :]                                  # [n][T]
        with ra.Ensemble(ra.KIND_CO2_ERF, n, np.arange(T + 1, dtype=float) + 1750.0) as e:
            e.set_params(np.stack([erf2x, pi]))
            e.set_forcing(conc[:, None, :], np.arange(n, dtype=np.int32))
            e.run()
            assert not e.status().any()
            got = e.get_series(1)                                             # [T][n]; row k + 1 from concentration k
        assert np.isnan(got[0]).all()
        arg = 1.0 + (conc - pi[:, None]) / pi[:, None]
        assert (arg[:, 0] == 1.0).all() and (arg[:, 1:T - 1] != 1.0).all()
        for i in range(n):
            for k in range(T - 1):
                g = got[k + 1, i]
                if conc[i, k] == pi[i]:
                    assert g == 0.0 and not np.signbit(g)
                    continue
                true = mpmath.mpf(float(scale[i])) * mpmath.log(mpmath.mpf(float(arg[i, k])))
                rel = float(abs((mpmath.mpf(float(g)) - true) / true))
                worst = max(worst, rel)
                assert rel <= 2.0 * 2.0 ** -52, (i, k, conc[i, k], g, rel * 2.0 ** 52)
    print(f"CO2ERF next to pre-industrial, n = {n}: max relative error {worst * 2.0 ** 52:.3f} * 2^-52")


def test_the_hook_checks_its_arguments(ra, math):
    from rscm_amd import _lib
    lib = _lib.load()
    x = np.array([1.0, 2.0, 4.0])
    out = np.full(3, -1.0)
    p = _lib.dptr
    for op in (-1, 5, 1 << 20):
        assert lib.rscm_gpu_selftest_math(op, 3, p(x), None, p(out)) == _lib.ERR_INVALID
    assert lib.rscm_gpu_selftest_math(0, -1, p(x), None, p(out)) == _lib.ERR_INVALID
    assert lib.rscm_gpu_selftest_math(0, 3, None, None, p(out)) == _lib.ERR_INVALID
    assert lib.rscm_gpu_selftest_math(0, 3, p(x), None, None) == _lib.ERR_INVALID
    assert lib.rscm_gpu_selftest_math(OP_POW_RATIO, 3, p(x), None, p(out)) == _lib.ERR_INVALID    # pow_ratio reads y
    assert (out == -1.0).all()
    for op in range(5):
        assert lib.rscm_gpu_selftest_math(op, 0, p(x), p(x) if op == OP_POW_RATIO else None, p(out)) == _lib.OK   # n == 0: nothing to do
    assert (out == -1.0).all()
    assert np.array_equal(math(OP_GUARDED_RCP, x), [1.0, 0.5, 0.25])                               # y may be absent for a one-argument op
    assert np.array_equal(math(OP_POW_RATIO, [1.0, 3.0], [2.0, 0.0]), [1.0, 1.0])
    with pytest.raises(_lib.RscmGpuError):
        math(7, x)
