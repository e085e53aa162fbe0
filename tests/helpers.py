"""Shared synthetic inputs: F_syn forcing, the notebook's emissions
scenario, Latin-hypercube two-layer parameter draws.  Pure numpy; no oracle, no product code."""
import numpy as np

TL_RANGES = [(0.8, 1.5), (0.0, 0.1), (1.0, 1.8), (0.5, 1.0), (5.0, 15.0), (50.0, 200.0)]
CC_RANGES = [(15.0, 40.0), (0.0, 0.1)]  # tau, alpha_temperature
SEED = 20260327


def axis_values(start=1750, end=2500):
    """python/rscm/config/builder.py:95: np.arange(start, end + 1) as f64."""
    return np.arange(start, end + 1, dtype=np.float64)


def f_syn(t):
    return 4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)) + 0.3 * np.sin(2.0 * np.pi * (t - 1750.0) / 11.0)


def emissions_syn(t):
    """docs/notebooks/coupled_model.py:397-407 knots, linear between, 1.0 after 2100."""
    years = np.array([1750.0, 1850.0, 1950.0, 2000.0, 2020.0, 2050.0, 2100.0])
    vals = np.array([0.0, 0.5, 3.0, 7.0, 10.0, 5.0, 1.0])
    return np.interp(t, years, vals)


def lhs(n, ranges, seed=SEED):
    """One sample per stratum per dimension, shuffled per dimension -> [P][n] SoA."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((len(ranges), n))
    for j, (lo, hi) in enumerate(ranges):
        u = (np.arange(n) + rng.random(n)) / n
        rng.shuffle(u)
        out[j] = lo + u * (hi - lo)
    return out


def two_layer_params(n, seed=SEED):
    return lhs(n, TL_RANGES, seed)


def coupled_params(n, seed=SEED):
    """[10][n]: two-layer 6, tau, conc_pi, alpha_temperature, erf_2xco2."""
    p = lhs(n, TL_RANGES + CC_RANGES, seed)
    out = np.empty((10, n))
    out[:6] = p[:6]
    out[6] = p[6]
    out[7] = 278.0
    out[8] = p[7]
    out[9] = 3.7
    return out


def two_layer_noise_case(n, offset=0, n_total=None):
    """(P [8][n], scenario [n]) of the noisy two-layer handles of the series, diagnostic and energy-budget files: the block
    [offset, offset + n) of the draw of n_total members seeded by n_total -- the six two-layer rows, then the noise amplitude and
    persistence rows -- with scenarios alternating 0, 1.  From 63 members on the last three of the draw are special: member
    n_total - 3 is silent under zero forcing (sigma_i = 0 in scenario 0: a constant series), member n_total - 2 has the amplitude
    1.7e308 (sigma_i z overflows) and member n_total - 1 has a NaN in parameter row 0."""
    n_total = n if n_total is None else n_total
    rng = np.random.default_rng(n_total)
    P = np.vstack([two_layer_params(n_total), rng.uniform(0.1, 0.6, n_total), rng.uniform(0.0, 0.9, n_total)])
    scen = (np.arange(n_total) % 2).astype(np.int32)
    if n_total >= 63:
        scen[n_total - 3], P[6, n_total - 3] = 0, 0.0
        P[6, n_total - 2] = 1.7e308
        P[0, n_total - 1] = np.nan
    return np.ascontiguousarray(P[:, offset:offset + n]), np.ascontiguousarray(scen[offset:offset + n])


def annual_bounds(T, start=1850):
    """(YEARS [T], BOUNDS [T + 1]): an annual axis of T points from `start` and its time bounds."""
    years = np.arange(start, start + T, dtype=np.float64)
    return years, np.append(years, years[-1] + 1.0)


def load_script(name, folder="scripts"):
    """The module of <repository>/<folder>/<name>.py, executed afresh (folder "": bench.py, at the root)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, folder, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def magicc_chain():
    return load_script("bench_magicc_chain")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_values(a, b):
    """Value equality of two arrays as float64: +0 equals -0 and any NaN equals any NaN; False on a shape mismatch.  Both sides are
    converted to float64, so integers beyond 2^53 are not told apart: compare those with np.array_equal."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _bits_differ(a, b):
    """Where two float64 arrays of one shape differ in their bits; any NaN == any NaN (payload bits are not part of the contract)."""
    return (bits(a) != bits(b)).reshape(a.shape) & ~(np.isnan(a) & np.isnan(b))


def same_bits(a, b):
    """Bit equality of two arrays as float64: the sign of a zero counts and any NaN equals any NaN; False on a shape mismatch."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and not bool(_bits_differ(a, b).any())


def assert_bit_equal(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = _bits_differ(a, b)
    if bad.any():
        idx = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} differ; first at {tuple(idx)}: "
                             f"{a[tuple(idx)]!r} vs {b[tuple(idx)]!r}")
