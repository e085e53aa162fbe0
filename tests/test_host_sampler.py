"""tests/host_sampler.py against published answers and analytic targets, no GPU: Philox4x32-10 known answers (Random123,
Salmon et al. 2011), the Feistel map as a bijection, the Latin property of lhs_matrix and its sharding, and the restated
stretch move as a correct MCMC -- moments of analytic posteriors within Monte-Carlo bounds tight enough that the wrong
z exponent fails them, the distribution of z and of the partner index.  The GPU tests pin the device to this restatement."""
import math

import numpy as np
import pytest

from tests.host_sampler import (HostStretchMove, accept_uniform, feistel_perm, lhs_half_bits, lhs_keys, lhs_matrix,
                                philox4x32_10, stretch_draws, u01_from_bits, walker_of)

F = 0xFFFFFFFF


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((F, F, F, F), (F, F), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want
    # vectorised: the same answer in every lane of a broadcast, other lanes independent of it
    c0 = np.array([ctr[0], ctr[0], (ctr[0] + 1) & F], dtype=np.uint64)
    got = philox4x32_10(c0, *ctr[1:], *key)
    assert [int(v[0]) for v in got] == list(want) and [int(v[1]) for v in got] == list(want)
    assert [int(v[2]) for v in got] != list(want)
    assert all((v <= F).all() for v in got)


def test_u01_from_bits():
    assert u01_from_bits(0, 0) == 0.0
    assert u01_from_bits(F, F) == 1.0 - 2.0 ** -53
    assert u01_from_bits(0, 1 << 31) == 0.5
    assert u01_from_bits(1 << 11, 0) == 2.0 ** -53   # the low 11 bits are dropped
    assert u01_from_bits((1 << 11) - 1, 0) == 0.0


def test_lhs_half_bits_restates_launch_lhs():
    assert [lhs_half_bits(n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 4099, 2 ** 20, 2 ** 20 + 1)] == \
        [1, 1, 1, 2, 2, 3, 3, 4, 7, 10, 11]


KEYS = [lhs_keys(0, 0), lhs_keys(20260327, 5), lhs_keys(2 ** 32 + 7, 1), lhs_keys(2 ** 64 - 1, 3)]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099, 2 ** 16 + 1])
def test_feistel_is_a_bijection(n):
    x = np.arange(n, dtype=np.uint64)
    perms = [feistel_perm(x, n, lhs_half_bits(n), k0, k1) for k0, k1 in KEYS]
    for p in perms:
        assert p.dtype == np.uint64 and np.array_equal(np.sort(p), x)
    if n >= 64:  # the keys give different permutations, none of them the identity
        assert all(not np.array_equal(p, x) for p in perms)
        assert len({p.tobytes() for p in perms}) == len(perms)


@pytest.mark.parametrize("n", [2 ** 18 + 3, 2 ** 20])
def test_feistel_is_a_bijection_large(n):
    x = np.arange(n, dtype=np.uint64)
    k0, k1 = lhs_keys(2 ** 64 - 1, 2)
    assert np.array_equal(np.sort(feistel_perm(x, n, lhs_half_bits(n), k0, k1)), x)


def test_lhs_keys_use_both_seed_words():
    assert lhs_keys(7, 0) == lhs_keys(2 ** 64 + 7, 0)           # 64-bit seeds
    assert lhs_keys(7, 0)[0] == lhs_keys(2 ** 32 + 7, 0)[0] and lhs_keys(7, 0)[1] != lhs_keys(2 ** 32 + 7, 0)[1]
    assert lhs_keys(2 ** 64 - 1, 1) == ((F ^ ((0x9E3779B9 * 2) & F)), 0)
    lo, hi = np.zeros(2), np.ones(2)
    assert not np.array_equal(lhs_matrix(7, lo, hi, 0, 64, 64), lhs_matrix(2 ** 32 + 7, lo, hi, 0, 64, 64))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 257, 4099, 2 ** 16 + 1])
def test_lhs_matrix_is_latin_and_shards(n):
    seed = 2 ** 32 + 7 if n % 2 else 2 ** 64 - 1
    lo, hi = np.array([0.0, -2.0, 5.0, 3.0]), np.array([1.0, 3.0, 15.0, 3.0])   # the last row: low == high
    m = lhs_matrix(seed, lo, hi, 0, n, n)
    assert m.shape == (4, n)
    assert (m[3] == 3.0).all()
    for j in range(3):
        u = (m[j] - lo[j]) / (hi[j] - lo[j])
        assert (u >= 0.0).all() and (u < 1.0).all()
        assert np.array_equal(np.sort(np.floor(u * n).astype(np.int64)), np.arange(n)), f"dimension {j}"
    if n >= 64:
        assert not np.array_equal(np.argsort(m[0]), np.argsort(m[1]))
    # uneven shards concatenate to the whole matrix, bit for bit
    cuts = sorted({0, n, min(n, 1), min(n, n // 3 + 1), min(n, (2 * n) // 3 + 5)})
    parts = [lhs_matrix(seed, lo, hi, a, b - a, n) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate(parts, axis=1).view(np.uint64).tobytes() == m.view(np.uint64).tobytes()


# ------------------------------------------------------------------------------------------ the stretch move
def _gaussian(D, cond, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    cov = q @ np.diag(np.geomspace(1.0, cond, D)) @ q.T
    return np.arange(D, dtype=np.float64), cov


def _whitened_moments(D, z_power, seed):
    mu, cov = _gaussian(D, 100.0, 0)
    prec, chol = np.linalg.inv(cov), np.linalg.cholesky(cov)

    def score(x):
        d = x - mu
        return -0.5 * np.einsum("ij,jk,ik->i", d, prec, d)

    W = 256
    s = HostStretchMove(W, D, score, stretch_a=2.0, seed=seed, z_power=z_power)
    s.set_positions(mu + np.random.default_rng(seed).standard_normal((W, D)) @ chol.T)
    samples, _ = s.run(600)
    y = (np.concatenate(samples[100:]) - mu) @ np.linalg.inv(chol).T   # N(0, I) if the chain is right
    return y.mean(axis=0), np.cov(y.T), s


def _gaussian_ok(m, c):
    # 500 kept sweeps x 256 walkers at an integrated autocorrelation time of ~40 sweeps: ~3000 effective draws, a
    # standard error of ~0.02 on a whitened mean, ~0.026 on a variance and ~0.011 on their average -- bounds at ~4 sigma
    D = len(m)
    return np.abs(m).max() < 0.1 and np.abs(c - np.eye(D)).max() < 0.1 and abs(np.trace(c) / D - 1.0) < 0.05


def test_stretch_move_samples_an_ill_conditioned_gaussian():
    """6-D Gaussian, condition number 100: mean and covariance within their Monte-Carlo bounds."""
    m, c, s = _whitened_moments(6, None, 1)
    assert _gaussian_ok(m, c), (m, c)
    assert 0.4 < s.n_accepted.sum() / s.n_proposed.sum() < 0.6 and (s.n_proposed == 600).all()


def test_the_bound_catches_the_wrong_z_exponent():
    """The same bounds fail when the proposal density factor is z^D instead of z^(D-1): the ensemble is ~15% too wide."""
    m, c, _ = _whitened_moments(6, 6, 1)
    assert not _gaussian_ok(m, c)
    assert np.trace(c) / 6 > 1.1


def test_stretch_move_one_dimension():
    """D = 1: z^(D-1) = 1, the move is a plain Metropolis step on a random line; a skewed target (Gamma(3, 1))."""
    def score(x):
        v = x[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(v > 0, 2.0 * np.log(v) - v, -np.inf)

    W = 256
    s = HostStretchMove(W, 1, score, stretch_a=2.0, seed=3)
    s.set_positions(np.random.default_rng(3).gamma(3.0, size=(W, 1)))
    samples, _ = s.run(600)
    x = np.concatenate(samples[100:])[:, 0]
    assert abs(x.mean() - 3.0) < 0.08 and abs(x.var() - 3.0) < 0.25
    assert (x > 0).all()


def test_stretch_move_uniform_box_and_a_walker_outside():
    """A Uniform box: flat inside, -inf outside.  A walker that starts outside the support (score -inf) accepts its first
    proposal that lands inside, whatever its z; the ensemble fills the box with the box's moments."""
    lo, hi = np.array([0.0, -2.0, 10.0]), np.array([1.0, 3.0, 10.5])

    def score(x):
        inside = ((x >= lo) & (x <= hi)).all(axis=1)
        return np.where(inside, -np.log(hi - lo).sum(), -np.inf)

    W = 128
    rng = np.random.default_rng(4)
    pos = lo + 0.5 * (hi - lo) + 0.01 * rng.standard_normal((W, 3))
    pos[[3, 70]] = hi + 0.05 * (hi - lo)
    s = HostStretchMove(W, 3, score, stretch_a=2.0, seed=2 ** 64 - 1)
    s.keep_records = True
    s.set_positions(pos)
    assert s.logp[3] == -np.inf and s.logp[70] == -np.inf
    samples, _ = s.run(400)
    for w in (3, 70):
        first = next(r for r in s.records if w in r[2] and np.isfinite(r[3][np.flatnonzero(r[2] == w)[0]]))
        assert first[4][np.flatnonzero(first[2] == w)[0]]
    x = np.concatenate(samples[100:])
    assert ((x >= lo) & (x <= hi)).all()
    assert np.abs(x.mean(axis=0) - 0.5 * (lo + hi)).max() / (hi - lo).max() < 0.03
    assert np.abs(x.var(axis=0) / ((hi - lo) ** 2 / 12.0) - 1.0).max() < 0.1


@pytest.mark.parametrize("a", [1.5, 2.0, 5.0])
def test_z_follows_the_stretch_density(a):
    """z has density g(z) ~ 1/sqrt(z) on [1/a, a] (Goodman & Weare 2010, eq. 9): a Kolmogorov-Smirnov test."""
    z = np.concatenate([stretch_draws(2 ** 32 + 7, it, half, 4096, a, 2048)[0] for it in (1, 2, 3) for half in (0, 1)])
    assert z.min() >= 1.0 / a and z.max() <= a
    z = np.sort(z)
    n = len(z)
    cdf = (np.sqrt(z) - 1.0 / math.sqrt(a)) / (math.sqrt(a) - 1.0 / math.sqrt(a))
    ks = max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(n) / n).max())
    assert ks * math.sqrt(n) < 1.63   # the 1% point of the Kolmogorov distribution
    # the wrong density is rejected: z uniform on [1/a, a]
    wrong = (z - 1.0 / a) / (a - 1.0 / a)
    assert max((np.arange(1, n + 1) / n - wrong).max(), (wrong - np.arange(n) / n).max()) * math.sqrt(n) > 1.63


@pytest.mark.parametrize("W,groups", [(14, 1), (64, 2), (96, 3)])
def test_partner_is_uniform_over_the_complementary_half_of_its_group(W, groups):
    s = HostStretchMove(W, 1, lambda x: np.zeros(len(x)), seed=11, n_groups=groups)
    s.set_positions(np.zeros((W, 1)))
    Wg, Hg = W // groups, W // groups // 2
    counts = np.zeros((2, W), dtype=np.int64)
    for it in range(1, 301):
        for half in (0, 1):
            st = s.propose(half, iteration=it)
            g = st.active // Wg
            assert np.array_equal(st.active, walker_of(np.arange(W // 2), half, W, groups))
            assert ((st.active % Wg) // Hg == half).all()
            assert (st.comp // Wg == g).all() and ((st.comp % Wg) // Hg == 1 - half).all()
            np.add.at(counts[half], st.comp, 1)
    for half in (0, 1):
        per = counts[half].reshape(groups, 2, Hg)[:, 1 - half].ravel()   # the partners' counts: the other half of every group
        assert (counts[half].reshape(groups, 2, Hg)[:, half] == 0).all()
        exp = per.sum() / per.size
        chi2, dof = ((per - exp) ** 2 / exp).sum(), per.size - 1
        assert chi2 < dof + 5.0 * math.sqrt(2.0 * dof), (chi2, dof)


def test_streams_are_keyed_by_iteration_half_walker_and_both_seed_words():
    base = stretch_draws(5, 1, 0, 64, 2.0, 32)[0]
    for args in ((5, 2, 0), (5, 1, 1), (2 ** 32 + 5, 1, 0)):
        assert not np.array_equal(stretch_draws(*args, 64, 2.0, 32)[0], base)
    assert len(np.unique(base)) == 64
    assert not np.array_equal(accept_uniform(5, 1, 0, 64), accept_uniform(5, 1, 1, 64))
    # the accept stream is not the proposal stream
    z = stretch_draws(5, 1, 0, 64, 2.0, 32)[0]
    assert not np.array_equal(np.sqrt(z * 2.0) - 1.0, accept_uniform(5, 1, 0, 64))
