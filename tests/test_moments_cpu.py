"""CPU tier of the exact moments across members (ABI minor 23): the reference of tests/host_moments.py against itself on the
identities that make the integer accumulator worth having, the finishing step rscm_gpu_moment_finish of the built library against
Fractions on synthetic blocks (it needs no device), and the sd / corr rules of rscm_amd.ensemble.moments_result."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import host_moments as hm
from tests.helpers import same_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spread(rng, n, span=60):
    """Full-mantissa doubles of both signs with exponents spread over 2^+-span."""
    return rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-span, span + 1, n)) * rng.choice([-1.0, 1.0], n)


# ---- the reference against itself ---------------------------------------------------------------------------------------------

def test_limb_scheme_is_the_exact_sum_and_a_float_sum_is_not():
    """4099 benign members with 30-bit weights: the canonical value of the limb scheme's block is the exact integer sum, its
    finish is the Fraction's mean, and numpy's dot / sum is another number in the last place."""
    rng = np.random.default_rng(4099)
    x = rng.uniform(0.0, 1.0, 4099)
    w = rng.integers(1, 1 << 30, 4099)
    block = hm.block_of(x, w.tolist())
    value, bad = hm.exact_sum(x, w.tolist())
    W = int(w.sum())
    assert hm.canonical(block) == value and bad == 0 == block[hm.LIMBS]
    assert value == sum(Fraction(float(xi)) * int(wi) for xi, wi in zip(x, w)) * (1 << 1088)
    mean = hm.finish(value, 0, W)
    assert mean == float(sum(Fraction(float(xi)) * int(wi) for xi, wi in zip(x, w)) / W)
    assert abs(np.dot(x, w.astype(np.float64)) / float(W) - mean) <= 4 * np.spacing(mean)
    assert max(abs(v) for v in block[:hm.LIMBS]) < 4099 << 32


def test_permutation_split_and_unit_weights():
    rng = np.random.default_rng(1)
    n = 777
    X = np.stack([_spread(rng, n), _spread(rng, n, 300), rng.standard_normal(n)])
    X[1, 5] = np.nan
    X[2, 700] = -np.inf
    w = rng.integers(0, 1 << 30, n)
    ref = hm.moments(X, w)
    assert ref["count"][0] == n - 2 and ref["weight"][0] == int(w.sum()) - int(w[5]) - int(w[700])
    perm = rng.permutation(n)
    got = hm.moments(X[:, perm], w[perm])
    for k in ("count", "weight", "mean", "cov", "sd", "corr"):
        assert hm.same_bits(np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)), k
    # the raw limbs of two orders differ, their canonical values do not
    a1, a2 = hm.sums_array(X, 1, None, w), hm.sums_array(X[:, perm], 1, None, w[perm])
    assert hm.array_sums(a1, 3, 1) == hm.array_sums(a2, 3, 1) == hm.sums(X, 1, None, w)
    # a split into three parts: the int64 arrays add up element by element, as an all-reduce adds them
    cuts = [0, 100, 101, n]
    for order, c in ((1, None), (2, ref["mean"])):
        parts = [hm.sums_array(X[:, lo:hi], order, c, w[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]
        assert hm.array_sums(sum(parts), 3, order) == hm.sums(X, order, c, w)
    # w = 1 is the unweighted statistic
    ones = hm.moments(X, np.ones(n, dtype=np.int64))
    plain = hm.moments(X)
    for k in ("count", "weight", "mean", "cov", "sd", "corr"):
        assert hm.same_bits(np.asarray(ones[k], dtype=np.float64), np.asarray(plain[k], dtype=np.float64)), k
    assert plain["weight"][0] == plain["count"][0]


def test_ill_conditioned_rows_have_their_exact_remainder():
    from tests import host_reduce as hd
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 1000):
        x = hd.ill_conditioned_row(rng, n)
        got = hm.moments(x[None])
        rem = x[(n - min(n, 2 - n % 2)) // 2:][:min(n, 2 - n % 2)]
        assert got["mean"][0, 0] == float(sum(Fraction(float(v)) for v in rem) / n)
        assert math.isnan(got["cov"][0, 0, 0]) == (n > 2)      # (1e300)^2 overflows: flagged, NaN


# ---- rscm_gpu_moment_finish of the built library --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from rscm_amd import _lib
    return _lib.load()


def _finish(lib, blocks, div, n_terms):
    blocks = np.ascontiguousarray(blocks, dtype=np.int64)
    div = np.ascontiguousarray(div, dtype=np.int64)
    out = np.full(div.size, 123.0)
    i64 = C.POINTER(C.c_int64)
    rc = lib.rscm_gpu_moment_finish(blocks.ctypes.data_as(i64), div.size, div.ctypes.data_as(i64), n_terms, out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def test_abi_minor_23_declares_and_binds_the_entry_points(lib):
    from rscm_amd import _lib
    header = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", header).group(1)) >= 23
    assert lib.rscm_gpu_abi_minor() >= 23
    for name in ("rscm_ens_moment_sums", "rscm_gpu_moment_finish", "rscm_ens_moments"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert int(re.search(r"#define\s+RSCM_MOMENT_BLOCK\s+(\d+)", header).group(1)) == hm.BLOCK == _lib.MOMENT_BLOCK
    assert int(re.search(r"#define\s+RSCM_MOMENT_MAX_VECTORS\s+(\d+)", header).group(1)) == hm.MAX_VECTORS == _lib.MOMENT_MAX_VECTORS


def test_finish_matches_the_fraction_on_synthetic_blocks(lib):
    """Exact ties in both directions, results in the subnormal range and at the largest finite double, negative sums, limbs near
    +-2^62 with carries through every limb, a zero sum, W = 0, a flagged block -- one call per case and all cases in one call."""
    cases = hm.finish_cases()
    names = [c[0] for c in cases]
    for must in ("tie down to even, shift 0", "tie up to even, shift 2000", "subnormal range, 0x2000", "largest finite double",
                 "a zero sum behind deferred carries", "no weight", "a flagged block", "limbs near +-2^62, 0"):
        assert must in names
    for name, block, W, want in cases:
        rc, out = _finish(lib, [block], [W], 1000)
        assert rc == 0 and hm.same_bits(out, [want]), (name, out[0], want)
    rc, out = _finish(lib, [c[1] for c in cases], [c[2] for c in cases], (1 << 31) - 1)
    assert rc == 0 and hm.same_bits(out, [c[3] for c in cases])
    by = dict((c[0], c[3]) for c in cases)
    assert by["subnormal range, 0x2000"] == 0.0 and by["subnormal range, 0x6000"] == 1e-323 and by["subnormal range, 0x2001"] == 5e-324
    assert math.copysign(1.0, by["subnormal range, -0x2000"]) == -1.0                   # a non-zero sum keeps its sign on the way to zero
    assert math.copysign(1.0, by["a zero sum behind deferred carries"]) == 1.0 and by["a zero sum behind deferred carries"] == 0.0
    assert by["largest finite double times 2^63 - 1"] == -np.finfo(np.float64).max
    assert by["half an ulp beyond the largest finite double"] == math.inf and by["just below that"] == np.finfo(np.float64).max
    assert math.isnan(by["no weight"]) and math.isnan(by["a flagged block"]) and math.isnan(by["no weight, zero sum"])


def test_finish_refuses_what_may_have_wrapped(lib):
    from rscm_amd import _lib
    zero = [[0] * hm.BLOCK]
    assert _finish(lib, zero, [1], (1 << 31) - 1)[0] == 0
    for n_terms in (1 << 31, 1 << 40, -1):
        rc, out = _finish(lib, zero, [1], n_terms)
        assert rc == _lib.ERR_INVALID and out[0] == 123.0
        assert b"n_terms" in lib.rscm_gpu_last_error()
    assert _finish(lib, zero, [-1], 0)[0] == _lib.ERR_INVALID
    assert lib.rscm_gpu_moment_finish(None, 1, None, 0, None) == _lib.ERR_INVALID
    assert lib.rscm_gpu_moment_finish(None, 0, None, 0, None) == 0


# ---- moments_result ------------------------------------------------------------------------------------------------------------

def test_moments_result_finishes_reference_sums_to_the_reference(lib):
    from rscm_amd.ensemble import moment_means, moments_result
    rng = np.random.default_rng(8)
    n, K, G = 300, 4, 3
    X = np.stack([_spread(rng, n, 20) for _ in range(K)])
    X[3] = 2.0 * X[0]                               # exactly collinear: cov_03 = 2 cov_00 and cov_33 = 4 cov_00, exactly
    X[2, 17] = np.nan
    w = rng.integers(0, 1 << 30, n)
    groups = rng.integers(-1, G - 1, n)            # the last group stays empty
    ref = hm.moments(X, w, groups, G)
    s1 = hm.sums_array(X, 1, None, w, groups, G)
    mean = moment_means(s1, K, G)
    assert hm.same_bits(mean, ref["mean"])
    s2 = hm.sums_array(X, 2, mean, w, groups, G)
    got = moments_result(s1, s2, K, G)
    for k in ("count", "weight", "mean", "cov", "sd", "corr"):
        assert hm.same_bits(np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)), k
    assert got["count"][G - 1] == 0 and np.isnan(got["mean"][G - 1]).all() and np.isnan(got["corr"][G - 1]).all()
    assert (got["cov"][:G - 1, 0, 3] == 2.0 * got["cov"][:G - 1, 0, 0]).all() and (got["cov"][:G - 1, 3, 3] == 4.0 * got["cov"][:G - 1, 0, 0]).all()
    assert (np.abs(got["corr"][:G - 1, 0, 3] - 1.0) <= 2.0 ** -52).all()     # cov / (sd sd): sd^2 is cov to within an ulp, no more
    assert same_values(got["cov"], got["cov"].transpose(0, 2, 1))


def test_sd_and_corr_rules():
    from rscm_amd.ensemble import moments_dict
    cov = np.array([[[4.0, 1.0, 0.0, 3.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, np.nan, 1.0], [3.0, 2.0, 1.0, 9.0]]])
    d = moments_dict([5], [5], np.zeros((1, 4)), cov)
    assert hm.same_bits(d["sd"], [[2.0, 0.0, np.nan, 3.0]])
    diag = np.einsum("gaa->ga", d["corr"])
    assert hm.same_bits(diag, [[1.0, np.nan, np.nan, 1.0]])           # exactly 1 where the variance is positive, NaN otherwise
    assert d["corr"][0, 0, 3] == 3.0 / (2.0 * 3.0) == d["corr"][0, 3, 0]
    assert d["corr"][0, 0, 1] == math.inf and math.isnan(d["corr"][0, 1, 2]) and math.isnan(d["corr"][0, 2, 3])
    sd, corr = hm.corr_rules(cov[0])
    assert hm.same_bits(d["sd"][0], sd) and hm.same_bits(d["corr"][0], corr)
    flat = moments_dict([5], [5], np.zeros((1, 4)), cov, grouped=False)
    assert flat["cov"].shape == (4, 4) and flat["mean"].shape == (4,) and flat["count"] == 5
