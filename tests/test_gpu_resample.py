"""GPU tier of the posterior resampling: rscm_ens_weights_stats and rscm_ens_resample (rscm_amd/csrc/resample.hip) against the
integer restatement of tests/host_resample.py, bit for bit -- the CPU tier's cases, a million members, one ensemble's weights
split over three handles -- and the error paths of the two calls."""
import ctypes as C

import numpy as np
import pytest

from tests import host_resample as hr
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.test_host_resample import _cases, _offsets

pytestmark = pytest.mark.gpu

B = np.arange(1750.0, 1754.0)   # a three-step axis: the draw does not depend on it


def _ens(ra, w):
    e = ra.Ensemble(ra.KIND_TWO_LAYER, len(w), B)
    e.set_member_weights(np.asarray(w, dtype=np.int64))
    return e


def test_weights_stats_equal_python_integer_sums(ra):
    rng = np.random.default_rng(3)
    n = 1_000_000
    w = rng.integers(0, (1 << 33) + 1, size=n, dtype=np.int64)
    w[rng.random(n) < 0.2] = 0
    w[12345] = 1 << 33
    with _ens(ra, w) as e:
        got = e.weights_stats()
    want = hr.stats(w)
    print("weights_stats", got)
    assert got == want
    assert isinstance(got["sum_sq"], int) and got["sum_sq"] > 1 << 64     # the high word is in use
    heavy = np.zeros(7, dtype=np.int64)
    heavy[[0, 5]] = 1 << 52                                                # w^2 = 2^104 each
    with _ens(ra, heavy) as e:
        assert e.weights_stats() == hr.stats(heavy)
        assert e.weights_stats()["ess"] == 2.0


@pytest.mark.parametrize("case", range(len(_cases())))
def test_ancestors_are_the_restatement_on_the_cpu_tier_cases(ra, case):
    w, M = _cases()[case]
    W = int(w.sum())
    with _ens(ra, w) as e:
        for s in _offsets(W, np.random.default_rng(case)):
            v = e.resample(M, offset=s)
            k_first, count, want = hr.ancestors(w, M, s)
            assert (v.k_first, len(v)) == (k_first, count) == (0, M)
            assert np.array_equal(v.to_host(), want), (case, s)
        seeded = e.resample(M, seed=99).to_host()
        assert np.array_equal(seeded, hr.ancestors(w, M, hr.offset(99, W))[2])


@pytest.fixture(scope="module")
def million(ra):
    rng = np.random.default_rng(11)
    n = 1_000_000
    w = rng.integers(0, 1 << 33, size=n, dtype=np.int64)
    w[rng.random(n) < 0.35] = 0
    w[rng.integers(0, n, 50)] = 1 << 40                                   # a few members drawn many times
    e = _ens(ra, w)
    yield e, w
    e.close()


@pytest.mark.parametrize("M", [1, 1000, 1_000_000, 3_000_000])
def test_ancestors_at_a_million_members(ra, million, M):
    e, w = million
    W = int(w.sum())
    for s in (0, W - 1, hr.offset(M, W)):
        v = e.resample(M, offset=s)
        k_first, count, want = hr.ancestors_fast(w, M, s)
        assert (v.k_first, len(v)) == (0, M) == (k_first, count)
        got = v.to_host()
        assert np.array_equal(got, want), (M, s, int((got != want).sum()))
        assert np.all(w[got] > 0)


@pytest.mark.parametrize("M", [1000, 1_000_000])
def test_three_handles_of_unequal_size_equal_the_single_handle(ra, million, M):
    e, w = million
    W = int(w.sum())
    s = hr.offset(5, W)
    whole = e.resample(M, offset=s).to_host()
    edges = [0, 1, 333_337, len(w)]
    got, before, k_next = [], 0, 0
    for a, b in zip(edges[:-1], edges[1:]):
        with _ens(ra, w[a:b]) as part:
            v = part.resample(M, offset=s, w_before=before, w_total=W)
            want = hr.ancestors_fast(w[a:b], M, s, before, W)
            assert (v.k_first, len(v)) == want[:2]
            assert len(v) == 0 or v.k_first == k_next
            k_next += len(v)
            got.append(v.to_host() + a)
            before += int(w[a:b].sum())
    assert k_next == M and np.array_equal(np.concatenate(got), whole)


def test_error_paths_return_their_codes_and_keep_earlier_state(ra):
    from rscm_amd._lib import ERR_INVALID, ERR_STATE
    w = np.array([5, 0, 7, 1], dtype=np.int64)
    with ra.Ensemble(ra.KIND_TWO_LAYER, 4, B) as e:
        for call in (e.weights_stats, lambda: e.resample(3, offset=0)):
            assert refusal_code(call) == ERR_STATE                          # no weights set
        e.set_member_weights(w)
        good = e.resample(6, offset=4)
        want = hr.ancestors(w, 6, 4)[2]
        assert np.array_equal(good.to_host(), want)
        for kw in (dict(n_draws=0, offset=0), dict(n_draws=(1 << 31) + 1, offset=0), dict(n_draws=3, offset=13),
                   dict(n_draws=3, offset=-1), dict(n_draws=3, offset=0, w_total=0), dict(n_draws=3, offset=0, w_before=2, w_total=14),
                   dict(n_draws=3, offset=0, w_before=-1, w_total=20)):
            assert refusal_code(e.resample, **kw) == ERR_INVALID, kw
            assert np.array_equal(good.to_host(), want)                  # the earlier draw is still there
        assert e.weights_stats() == hr.stats(w)
        from tests.helpers import f_syn, two_layer_params
        e.set_params(two_layer_params(4))
        e.set_forcing(f_syn(B[:-1]))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.run()
        with e.select(1, [0.5], weighted=True):
            assert refusal_code(e.resample, 3, offset=0) == ERR_STATE                          # a staged select in flight
        assert np.array_equal(e.resample(6, offset=4).to_host(), want)


def test_library_offset_is_the_restatement(ra):
    from rscm_amd.ensemble import resample_offset
    for seed in (0, 7, (1 << 63) + 12345):
        for W in (1, 13, (1 << 53) - 1):
            assert resample_offset(seed, W) == hr.offset(seed, W)
