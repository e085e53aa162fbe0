"""CPU tier of the device Latin hypercube through Normal, LogNormal and truncated priors (include/rscm_gpu.h,
rscm_ens_sample_lhs_priors): the restatement tests/host_lhs_priors.py against the forcing noise's deviate, scipy and the uniform
hypercube, the table builder rscm_amd.calibrate.prior_table, and the properties that make the columns a Latin hypercube -- ranks,
bounds and recovered strata, all exact.  The GPU tier (tests/test_gpu_lhs_priors.py) pins the device to the restatement."""
import math
import os
import re

import numpy as np
import pytest

from rscm_amd import _lib
from rscm_amd.calibrate import Bound, LogNormal, Normal, ParameterSet, Uniform, prior_table
from tests import host_forcing_noise as hn
from tests import host_lhs_priors as hp
from tests.helpers import assert_bit_equal, same_bits
from tests.host_sampler import lhs_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20260117
TOP = (1 << 52) - 1


# ---------------------------------------------------------------------------------------------- 1. the quantile
def test_quantile_on_the_noise_grid_is_the_noise_deviate():
    """normal_from_p((2k + 1) 2^-53) == normal_from_k(k), bit for bit: the integers that put every branch in play and 2e5 random ones."""
    rng = np.random.default_rng(SEED)
    for what, k in (("chosen", hn.chosen_k()), ("random", rng.integers(0, TOP + 1, 200_000, dtype=np.uint64)),
                    ("lower tail", rng.integers(0, 1 << 30, 50_000, dtype=np.uint64)),
                    ("upper tail", np.uint64(TOP) - rng.integers(0, 1 << 30, 50_000, dtype=np.uint64))):
        assert_bit_equal(hp.normal_from_p(hn.uniform_from_k(k)), hn.normal_from_k(k), what)


def test_quantile_against_scipy():
    """Relative 4e-15 against scipy.special.ndtri, the bound and derivation of test_restatement_against_scipy (the 1-ulp logarithm,
    whose error the square root halves, two polynomials and a rounded division), on uniform t, on t log-uniform over [2^-1022, 1/2]
    and on the two ends of the clamp.  A general t adds one rounding to it: q = t - 1/2 is not exact below 1/4 (2^-55 absolute on
    |q| >= 1/4).  Measured: uniform 1.04e-15, log-uniform 1.0e-15 (the same below 1e-5), the ends 2.2e-16."""
    from scipy.special import ndtri
    rng = np.random.default_rng(SEED + 1)
    uniform = rng.random(400_000)
    uniform = uniform[(uniform >= hp.T_MIN) & (uniform != 0.5)]
    log_uniform = np.minimum(np.ldexp(1.0 + rng.random(400_000), rng.integers(-1022, -1, 400_000)), 0.5)
    log_uniform = log_uniform[log_uniform != 0.5]
    ends = np.array([hp.T_MIN, hp.T_MAX])
    for what, t in (("uniform", uniform), ("log-uniform", log_uniform), ("below 1e-5", log_uniform[log_uniform < 1e-5]), ("ends", ends)):
        ref = ndtri(t)
        err = np.abs(hp.normal_from_p(t) - ref) / np.abs(ref)
        print(f"{what}: {t.size} arguments, max relative deviation from ndtri {err.max():.3e}")
        assert err.max() <= 4e-15
    z = hp.normal_from_p(ends)
    assert abs(z[0] + 37.52) < 0.01 and abs(z[1] - 8.21) < 0.01 and hp.normal_from_p(0.5)[0] == 0.0


# ---------------------------------------------------------------------------------------------- 2. the table builder
def test_table_of_every_distribution():
    from scipy.stats import lognorm, norm
    priors = {0: Uniform(0.8, 1.5), 2: Normal(8.0, 1.5), 3: Bound(Normal(0.7, 0.2), 0.5, 1.0), 4: Bound(Normal(0.0, 1.0), 6.0, 8.0),
              5: LogNormal(1.1, 0.4), 6: Bound(LogNormal(1.1, 0.4), 2.0, 4.5), 7: Bound(Uniform(0.0, 2.0), 0.5, 3.0),
              8: Bound(LogNormal(1.1, 0.4), 3.5, 9.0), 9: Bound(Normal(0.7, 0.2), 0.7, 1.0), 10: Bound(Normal(0.7, 0.2), -math.inf, 0.6)}
    base = np.arange(11.0) + 100.0
    kind, a, b, p0, p1, lo, hi = prior_table(priors, 11, base)
    assert kind.dtype == np.int32 and all(v.dtype == np.float64 and v.shape == (11,) for v in (a, b, p0, p1, lo, hi))
    R = _lib.PRIOR_REFLECT
    # reflect exactly where the support lies above the centre (row 9: lo == mean counts; row 3 straddles it; row 6: ln 2 < 1.1 < ln 3.5)
    assert kind.tolist() == [0, 0, 1, 1, 1 | R, 2, 2, 0, 2 | R, 1 | R, 1]
    assert (a[0], b[0]) == (0.8, 1.5) and (a[1], b[1]) == (101.0, 101.0) and (a[7], b[7]) == (0.5, 2.0)
    assert (a[2], b[2]) == (8.0, 1.5) and (a[5], b[5]) == (1.1, 0.4) and (a[4], b[4]) == (0.0, 1.0)
    assert (p0[2], p1[2], lo[2], hi[2]) == (0.0, 1.0, -math.inf, math.inf) and (p0[5], p1[5], lo[5], hi[5]) == (0.0, 1.0, -math.inf, math.inf)
    assert (lo[3], hi[3]) == (0.5, 1.0) and (lo[4], hi[4]) == (6.0, 8.0) and (lo[6], hi[6]) == (2.0, 4.5) and (lo[10], hi[10]) == (-math.inf, 0.6)
    want = {3: (norm.cdf(0.5, 0.7, 0.2), norm.cdf(1.0, 0.7, 0.2)), 4: (norm.sf(8.0), norm.sf(6.0)),
            6: (lognorm.cdf(2.0, 0.4, scale=math.exp(1.1)), lognorm.cdf(4.5, 0.4, scale=math.exp(1.1))),
            8: (lognorm.sf(9.0, 0.4, scale=math.exp(1.1)), lognorm.sf(3.5, 0.4, scale=math.exp(1.1))),
            9: (norm.sf(1.0, 0.7, 0.2), norm.sf(0.7, 0.7, 0.2)), 10: (0.0, norm.cdf(0.6, 0.7, 0.2))}
    for j, (w0, w1) in want.items():
        print(f"row {j}: p0 {p0[j]:.17g} (scipy {w0:.17g}), p1 {p1[j]:.17g} (scipy {w1:.17g})")
        assert abs(p0[j] - w0) <= 1e-15 and abs(p1[j] - w1) <= 1e-15 and 0.0 <= p0[j] < p1[j] <= 1.0
    assert p1[9] == 0.5 and p0[4] < 1e-15   # the survival side keeps a far tail's probabilities as small numbers, not as 1 - small


def test_table_refusals():
    class Beta:
        pass
    with pytest.raises(NotImplementedError, match="prior Beta has no device form"):
        prior_table({0: Beta()}, 2, [1.0, 2.0])
    with pytest.raises(NotImplementedError, match="prior Bound has no device form"):
        prior_table({0: Bound(Bound(Normal(0.0, 1.0), -1.0, 1.0), -0.5, 0.5)}, 2, [1.0, 2.0])
    with pytest.raises(ValueError, match="no prior"):
        prior_table({0: Uniform(0.0, 1.0)}, 2)
    with pytest.raises(ValueError, match="one entry per parameter"):
        prior_table({0: Uniform(0.0, 1.0)}, 2, [1.0])
    for row in (-1, 2, 0.5):
        with pytest.raises(ValueError, match="not a parameter row"):
            prior_table({row: Uniform(0.0, 1.0)}, 2, [1.0, 2.0])
    with pytest.raises(ValueError, match="do not meet"):
        prior_table({0: Bound(Uniform(0.0, 1.0), 2.0, 3.0)}, 1, [0.0])
    with pytest.raises(ValueError, match="hold nothing of a LogNormal"):
        prior_table({0: Bound(LogNormal(0.0, 1.0), -2.0, 0.0)}, 1, [0.0])
    with pytest.raises(ValueError, match="no probability"):
        prior_table({0: Bound(Normal(0.0, 1.0), 40.0, 41.0)}, 1, [0.0])   # Phi(-41) and Phi(-40) are both 0
    assert prior_table({0: Uniform(0.0, 1.0), 1: Normal(0.0, 1.0)}, 2)[0].tolist() == [0, 1]   # no base needed when every row has a prior


def test_parameter_set_rows():
    ps = ParameterSet().add("eta", Uniform(0.5, 1.0)).add("forcing_noise|phi", Bound(Normal(0.3, 0.2), 0.0, 0.9))
    ps.add("forcing_scale|aerosol", LogNormal(0.0, 0.3)).add("forcing_noise|sigma", LogNormal(-1.0, 0.5))
    order = ("lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep", "forcing_scale|ghg", "forcing_scale|aerosol",
             "forcing_noise|sigma", "forcing_noise|phi")
    rows = ps.rows(order)
    d = ps.distributions()
    assert rows == {3: d[0], 9: d[1], 7: d[2], 8: d[3]}
    assert ps.rows({n: j for j, n in enumerate(order)}) == rows
    with pytest.raises(KeyError, match="forcing_noise"):
        ps.rows(order[:8])
    assert prior_table(rows, len(order), np.ones(len(order)))[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 2, 2, 1]


# ---------------------------------------------------------------------------------------------- 3. the hypercube
TABLE_PRIORS = {0: Uniform(0.8, 1.5), 2: Normal(8.0, 1.5), 3: Bound(Normal(0.7, 0.2), 0.5, 1.0), 4: Bound(Normal(0.0, 1.0), 6.0, 8.0),
                5: LogNormal(1.1, 0.4), 6: Bound(LogNormal(1.1, 0.4), 2.0, 4.5), 7: Bound(Uniform(0.0, 2.0), 0.5, 3.0)}
TABLE_BASE = np.array([1.0, 0.05, 1.3, 0.7, 8.0, 100.0, 0.4, 0.2])


def test_uniform_rows_are_the_uniform_hypercube():
    table = prior_table(TABLE_PRIORS, 8, TABLE_BASE)
    for n_total, off, n in ((5, 0, 5), (1000, 300, 200)):
        got = hp.lhs_priors_matrix(SEED, table, off, n, n_total)
        want = lhs_matrix(SEED, table[1], table[2], off, n, n_total)
        for j in (0, 1, 7):
            assert same_bits(got[j], want[j]), j
        assert (got[1] == TABLE_BASE[1]).all()
        for j in (2, 3, 4, 5, 6):
            assert not same_bits(got[j], want[j])


@pytest.mark.parametrize("n", [5, 64, 4096])
def test_ranks_bounds_and_recovered_strata(n):
    """Exact, no tolerance: a Normal or centrally truncated column is ordered as its strata, a reflected column in reverse, every
    value lies inside [lo, hi], and floor(Phi((x - a) / b) n) gives the stratum of every member of the plain Normal row back."""
    table = prior_table(TABLE_PRIORS, 8, TABLE_BASE)
    kind, a, b, p0, p1, lo, hi = table
    X, Y = hp.lhs_priors_matrix(SEED, table, 0, n, n, with_y=True)
    for j in range(8):
        strata = hp.lhs_strata(SEED, j, 0, n, n)
        assert sorted(strata.tolist()) == list(range(n))
        if a[j] == b[j] and kind[j] == 0:
            continue
        order = np.argsort(X[j], kind="stable")
        assert np.unique(X[j]).size == n, f"row {j}: {n - np.unique(X[j]).size} ties"
        want = np.argsort(strata)
        assert np.array_equal(order, want[::-1] if kind[j] & _lib.PRIOR_REFLECT else want), f"row {j}"
        if kind[j] != 0:
            assert (X[j] >= lo[j]).all() and (X[j] <= hi[j]).all(), f"row {j}"
    assert kind[4] & _lib.PRIOR_REFLECT and not kind[3] & _lib.PRIOR_REFLECT
    phi = np.array([0.5 * math.erfc(-((x - a[2]) / b[2]) / math.sqrt(2.0)) for x in X[2]])
    assert np.array_equal(np.floor(phi * n).astype(np.int64), hp.lhs_strata(SEED, 2, 0, n, n).astype(np.int64))


def test_a_block_is_the_slice_of_the_whole():
    table = prior_table(TABLE_PRIORS, 8, TABLE_BASE)
    whole = hp.lhs_priors_matrix(SEED, table, 0, 1000, 1000)
    assert same_bits(hp.lhs_priors_matrix(SEED, table, 300, 200, 1000), whole[:, 300:500])


def test_reflection_keeps_the_resolution_of_a_far_tail():
    """Bound(Normal(0, 1), 6, 8) at 1e5 strata: the survival side gives 1e5 distinct values, the CDF side (p0, p1 next to 1) loses some."""
    n = 100_000
    d = Bound(Normal(0.0, 1.0), 6.0, 8.0)
    table = prior_table({0: d}, 1, [0.0])
    assert table[0][0] == _lib.PRIOR_NORMAL | _lib.PRIOR_REFLECT
    assert np.unique(hp.lhs_priors_matrix(SEED, table, 0, n, n)[0]).size == n
    cdf = 0.5 * math.erfc(-6.0 / math.sqrt(2.0)), 0.5 * math.erfc(-8.0 / math.sqrt(2.0))
    plain = (np.array([_lib.PRIOR_NORMAL], dtype=np.int32), table[1], table[2], np.array([cdf[0]]), np.array([cdf[1]]), table[5], table[6])
    distinct = np.unique(hp.lhs_priors_matrix(SEED, plain, 0, n, n)[0]).size
    print(f"unreflected: {distinct} distinct values of {n}")
    assert distinct < n


# ---------------------------------------------------------------------------------------------- 4. the boundary
def test_abi_minor_25_declares_and_binds_the_entry_point():
    header = open(f"{ROOT}/include/rscm_gpu.h").read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", header).group(1)) >= 25
    for name, value in (("UNIFORM", 0), ("NORMAL", 1), ("LOGNORMAL", 2), ("REFLECT", 0x100)):
        assert int(re.search(rf"#define\s+RSCM_PRIOR_{name}\s+(\w+)", header).group(1), 0) == value == getattr(_lib, f"PRIOR_{name}")
        assert getattr(hp, f"PRIOR_{name}") == value
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 25 and hasattr(lib, "rscm_ens_sample_lhs_priors")
