"""The yardstick of the device-math tests: an error measure in units in the last place of a double, high-precision references and the
argument families the CPU test (test_host_math.py) and the GPU test (test_gpu_device_math.py) share.

The measure.  ulp_error(got, true) = |got - true| / 2^(e - 52), formed in np.longdouble, where e is the binade of `true` rounded to
double (clamped at -1022: below it the spacing of the doubles is 2^-1074).  A correctly rounded result measures at most 0.5.

The references.  np.log / np.exp / np.power / division on np.longdouble (x87 extended: 64-bit significand, results within ~1 ulp of
THAT format, 2^-11 ulp of a double) for the bulk; mpmath at 50 digits for the edge arguments and for a sample of every family, which
pins the bulk reference too: the two must agree to 2^-9 ulp of a double (test_host_math.py).  Where np.longdouble is not wider than
63 fraction bits (LONGDOUBLE_OK false: checked, not assumed) the bulk is a seeded sample of MP_FALLBACK arguments per family through
mpmath instead."""
import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = np.finfo(LD).nmant >= 63
FAMILY_SIZE = 1 << 18
MP_SAMPLE = 4096         # arguments of every family that mpmath checks the longdouble reference on
MP_FALLBACK = 20_000     # arguments per family through mpmath where longdouble is no wider than double
MP_DIGITS = 50
PIN = 2.0 ** -9          # longdouble vs mpmath, in ulp of a double

DBL_MIN = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308
SQRT_HALF = 0.70710678118654752440   # the fold of log_f64: the double nearest sqrt(1/2)


# ---- the measure -----------------------------------------------------------------------------------------------------------------

def ulp_of(true_ld):
    """2^(e - 52) as longdouble, e the binade of |true| rounded to double, at least -1022."""
    with np.errstate(over="ignore"):
        t64 = np.abs(np.asarray(true_ld, dtype=LD)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        _, ex = np.frexp(np.where(np.isfinite(t64), t64, 1.0))
    e = np.where(t64 == 0.0, -1022, np.maximum(ex.astype(np.int64) - 1, -1022))   # a true value that rounds to 0 sits among the denormals
    return np.ldexp(LD(1.0), (e - 52).astype(np.int64))


def ulp_error(got, true_ld):
    """Error of the doubles `got` against the high-precision `true_ld`, in ulp of a double (longdouble array).  The bookkeeping of
    what has no ulp: a true NaN demands NaN, a true value that is +-inf or rounds to +-inf as a double demands that infinity, a true
    0 demands got == 0 (either sign: the sign of a zero is asserted where it matters); a miss measures inf.  A NaN or an infinity
    returned for a finite true value measures inf too."""
    got = np.asarray(got, dtype=np.float64)
    true_ld = np.asarray(true_ld, dtype=LD)
    got, true_ld = np.broadcast_arrays(got, true_ld)
    with np.errstate(over="ignore"):
        t64 = true_ld.astype(np.float64)
    err = np.full(got.shape, LD(np.inf))
    nan = np.isnan(true_ld)
    inf = ~nan & np.isinf(t64)
    zero = ~nan & (true_ld == 0)
    err[nan & np.isnan(got)] = 0
    err[inf & (got == t64)] = 0
    err[zero & (got == 0.0)] = 0
    num = ~(nan | inf | zero) & np.isfinite(got)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(got.astype(LD) - true_ld) / ulp_of(true_ld)
    err[num] = e[num]
    return err


def steps_off(x, k):
    """x moved k nextafter steps (k > 0 up, k < 0 down)."""
    x = np.asarray(x, dtype=np.float64).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


# ---- mpmath <-> longdouble ---------------------------------------------------------------------------------------------------------

def _mp():
    import mpmath
    mpmath.mp.dps = MP_DIGITS
    return mpmath


def mp_to_ld(v):
    """An mpmath value as longdouble: the two doubles hi + lo carry 106 bits, their longdouble sum is `v` rounded (to 2^-64
    relative, 2^-12 ulp of a double: inside PIN)."""
    mp = _mp()
    if mp.isnan(v):
        return LD(np.nan)
    if mp.isinf(v):
        return LD(np.inf) if v > 0 else LD(-np.inf)
    if v == 0:
        return LD(0.0)
    m, e = mp.frexp(v)               # scaled: results beyond the doubles (exp(710)) or among the denormals keep their bits
    hi = float(m)
    lo = float(m - mp.mpf(hi))
    return np.ldexp(LD(hi) + LD(lo), int(e))


def _mp_fn(op):
    mp = _mp()

    def log(x):
        if mp.isnan(x) or x < 0:
            return mp.nan
        if x == 0:
            return mp.ninf
        return mp.log(x)

    def power(x, y):
        return mp.power(x, y)

    return {"log": log, "exp": mp.exp, "pow": power, "rcp": lambda x: 1 / x}[op]


def mp_reference(op, x, y=None):
    """op in log / exp / pow / rcp of the doubles x (and y) through mpmath at 50 digits, as longdouble."""
    mp = _mp()
    f = _mp_fn(op)
    x = np.asarray(x, dtype=np.float64).ravel()
    out = np.empty(x.size, dtype=LD)
    if y is None:
        for i, a in enumerate(x):
            out[i] = mp_to_ld(f(mp.mpf(float(a))))
    else:
        y = np.asarray(y, dtype=np.float64).ravel()
        for i, (a, b) in enumerate(zip(x, y)):
            out[i] = mp_to_ld(f(mp.mpf(float(a)), mp.mpf(float(b))))
    return out


def ld_reference(op, x, y=None):
    """The same through np.longdouble."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    with np.errstate(all="ignore"):
        if op == "log":
            return np.log(x)
        if op == "exp":
            return np.exp(x)
        if op == "pow":
            return np.power(x, np.asarray(y, dtype=np.float64).astype(LD))
        if op == "rcp":
            return LD(1.0) / x
    raise ValueError(op)


def sample_indices(n, k, seed=7):
    """k of the n indices, seeded, ascending (all of them if k >= n)."""
    if k >= n:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


def reference(op, x, y=None):
    """(idx, true): the bulk reference of op over x[idx].  idx is every index where longdouble carries 64 bits; otherwise a seeded
    sample of MP_FALLBACK indices, and true comes from mpmath."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if LONGDOUBLE_OK:
        return np.arange(x.size), ld_reference(op, x, y)
    idx = sample_indices(x.size, MP_FALLBACK)
    return idx, mp_reference(op, x[idx], None if y is None else np.asarray(y, dtype=np.float64).ravel()[idx])


# ---- the argument families ---------------------------------------------------------------------------------------------------------

def log_families(n=FAMILY_SIZE, seed=20240):
    """name -> n doubles, seeded:
      a  log-uniform over all normals: ldexp(U[1,2), k), k in -1022..1023
      b  uniform on [0.5, 2)
      c  1 +- u 2^-j, j in 0..52: hugging 1, where f - f^2/2 cancels (many are 1 exactly, or one of its neighbours)
      d  sqrt(1/2) (1 +- 2^-j) 2^k, j in 1..52, k in -20..20: both sides of the fold m < sqrt(1/2) in many binades -- every (sign, j, k)
         once, then draws sqrt(1/2) (1 +- u 2^-j) 2^k between them up to n
      e  uniform on [1, 4): the concentration ratios the forcing formulas see"""
    rng = np.random.default_rng(seed)
    fam = {}
    fam["a"] = np.ldexp(1.0 + rng.random(n), rng.integers(-1022, 1024, n))
    fam["b"] = 0.5 + 1.5 * rng.random(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    fam["c"] = 1.0 + sign * np.ldexp(rng.random(n), -rng.integers(0, 53, n))
    s, j, k = np.meshgrid([-1.0, 1.0], np.arange(1, 53), np.arange(-20, 21), indexing="ij")
    grid = np.ldexp(SQRT_HALF * (1.0 + s.ravel() * np.ldexp(1.0, -j.ravel())), k.ravel())
    m = n - grid.size
    assert m > 0
    sign = np.where(rng.random(m) < 0.5, -1.0, 1.0)
    fill = np.ldexp(SQRT_HALF * (1.0 + sign * np.ldexp(1.0 - rng.random(m), -rng.integers(1, 53, m))), rng.integers(-20, 21, m))
    fam["d"] = np.concatenate([grid, fill])
    fam["e"] = 1.0 + 3.0 * rng.random(n)
    for v in fam.values():
        assert v.shape == (n,) and (v >= DBL_MIN).all() and np.isfinite(v).all()
    return fam


def log_edges_normal():
    """The edge arguments log_f64 evaluates itself."""
    return np.array([1.0, np.nextafter(1.0, np.inf), np.nextafter(1.0, -np.inf), 0.5, 2.0,
                     SQRT_HALF, np.nextafter(SQRT_HALF, np.inf), np.nextafter(SQRT_HALF, -np.inf),
                     DBL_MIN, np.nextafter(DBL_MIN, np.inf), DBL_MAX])


def log_edges_other():
    """The arguments that take the library's log: denormals (the neighbour of DBL_MIN below it among them), zeros, negatives,
    infinities, NaN."""
    return np.array([np.nextafter(DBL_MIN, 0.0), 5e-324, 1e-310, 0.0, -0.0, -1.0, -np.inf, np.inf, np.nan])


def exp_families(n=FAMILY_SIZE, seed=20241):
    rng = np.random.default_rng(seed)
    return {"wide": rng.uniform(-700.0, 700.0, n), "unit": rng.uniform(-1.0, 1.0, n)}


def exp_edges():
    return np.array([0.0, 709.78, -709.78, -745.2, 710.0, np.inf, -np.inf, np.nan])


def pow_arguments(n=FAMILY_SIZE, seed=20242):
    """(x, y): x in [1, 16) with a block sitting on 1 and a block just above it (1 + u 2^-j), y in [-2, 2] with a block of zeros."""
    rng = np.random.default_rng(seed)
    x = 1.0 + 15.0 * rng.random(n)
    y = rng.uniform(-2.0, 2.0, n)
    b = n // 16
    x[:b] = 1.0
    x[b:2 * b] = 1.0 + np.ldexp(rng.random(b), -rng.integers(0, 53, b))
    y[3 * b:4 * b] = 0.0
    y[:b // 2] = 0.0          # and both at once
    y[4 * b:5 * b] = rng.uniform(-1.0, 1.0, b)   # the lifetime feedbacks' |y| < 1
    return x, y


def rcp_arguments(n=FAMILY_SIZE, seed=20243):
    """(inside, outside) of guarded_rcp's divisor window, biased exponent in [895, 1151], i.e. |d| in [2^-128, 2^129):
    inside  log-uniform over the window in both signs, then both edges approached from inside;
    outside both edges approached from outside, log-uniform over the normals beyond them, the two top binades (denormal quotients),
            denormals (infinite quotients below 2^-1024), zeros, infinities, NaN, DBL_MIN and DBL_MAX."""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    inside = sign * np.ldexp(1.0 + rng.random(n), rng.integers(-128, 129, n))
    lo, hi = np.ldexp(1.0, -128), np.ldexp(1.0, 129)
    inside = np.concatenate([inside, _walk(lo, np.inf, 64), _walk(np.nextafter(hi, 0.0), 0.0, 64),
                             -_walk(lo, np.inf, 64), -_walk(np.nextafter(hi, 0.0), 0.0, 64)])
    m = 1 << 12
    below = np.ldexp(1.0 + rng.random(m), rng.integers(-1022, -128, m))
    above = np.ldexp(1.0 + rng.random(m), rng.integers(129, 1024, m))
    den = np.ldexp(rng.random(m), -1022)
    huge = np.ldexp(1.0 + rng.random(256), rng.integers(1022, 1024, 256))      # their reciprocals are denormal
    outside = np.concatenate([_walk(np.nextafter(lo, 0.0), 0.0, 64), _walk(hi, np.inf, 64), below, -below, above, -above, den, -den,
                              huge, -huge,
                              [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, DBL_MIN, -DBL_MIN, DBL_MAX, -DBL_MAX,
                               np.nextafter(DBL_MIN, 0.0)]])
    outside = np.concatenate([outside, -_walk(np.nextafter(lo, 0.0), 0.0, 64), -_walk(hi, np.inf, 64)])
    return inside, outside


def _walk(start, toward, count):
    out = np.empty(count)
    x = float(start)
    for i in range(count):
        out[i] = x
        x = np.nextafter(x, toward)
    return out


def in_rcp_window(d):
    e = (np.asarray(d, dtype=np.float64).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)
    return (e >= 895) & (e <= 1151)
