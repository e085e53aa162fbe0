"""GPU tier of the exact weighted means, covariances and correlations across members (csrc/moments.hip, ABI minor 23) against the
integers and fractions of tests/host_moments.py.  No tolerance anywhere: doubles are compared bit for bit (any NaN for a NaN) and
the device's blocks as canonical integers with their counts of non-finite terms -- never limb by limb, since deferred carries
depend on the order of summation.

The vectors are parameter rows of a two-layer mix ensemble with two forcing components (eight rows of N doubles that take any
bits); nothing is stepped except in the plumbing test."""
import os
import re

import numpy as np
import pytest

from tests import host_moments as hm
from tests import host_reduce as hd
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import f_syn, magicc_chain, two_layer_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B3 = np.arange(1750.0, 1754.0)
DBL_MAX = float(np.finfo(np.float64).max)
KEYS = ("count", "weight", "mean", "cov", "sd", "corr")


def _members_per_pass() -> int:
    """Members one pass of the sum kernel's capped grid takes, read from the code: kMomBlocks blocks of four waves of 64."""
    text = open(os.path.join(ROOT, "rscm_amd", "csrc", "rscm_device.hpp")).read()
    blocks = int(re.search(r"constexpr int kMomBlocks = (\d+);", text).group(1))
    per_pass = int(re.search(r"constexpr int64_t kMomentMembersPerPass = (\d+);", text).group(1))
    hip = open(os.path.join(ROOT, "rscm_amd", "csrc", "moments.hip")).read()
    threads = int(re.search(r"constexpr int kMomThreads = (\d+);", hip).group(1))
    assert per_pass == blocks * threads
    return per_pass


def _spread(rng, n, span=60):
    """Full-mantissa doubles of both signs with exponents spread over 2^+-span."""
    return rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-span, span + 1, n)) * rng.choice([-1.0, 1.0], n)


def _ens(ra, n):
    return ra.Ensemble(ra.KIND_TWO_LAYER, n, B3, forcing_components=2)


def _load(e, X):
    """X[K][n] into the first K parameter rows; their DeviceVectors."""
    X = np.asarray(X, dtype=np.float64)
    assert e.n_params == 8 and X.shape[0] <= 8
    P = np.ones((8, e.n_members))
    P[:X.shape[0]] = X
    e.set_params(P)
    vecs = [e.params_vector(k) for k in range(X.shape[0])]
    assert np.array_equal(vecs[-1].to_host().view(np.uint64), X[-1].view(np.uint64))
    return vecs


def _same_dict(got, ref, grouped, what):
    for k in KEYS:
        want = np.asarray(ref[k], dtype=np.float64)
        if not grouped:
            want = want[0]
        assert hm.same_bits(np.asarray(got[k], dtype=np.float64), want), (what, k, got[k], want)


def _check(e, vecs, X, w=None, groups=None, G=None, what=""):
    """moment_sums of both orders as canonical integers, then moments, against the reference; returns the reference."""
    X = np.asarray(X, dtype=np.float64)
    K = X.shape[0]
    kw = dict(weighted=w is not None, grouped=groups is not None)
    ref, s1, s2 = hm.moments(X, w, groups, G, with_sums=True)
    got1 = e.moment_sums(vecs, 1, **kw)
    assert got1.dtype == np.int64 and got1.shape == (len(s1), 2 + K * hm.BLOCK)
    assert hm.array_sums(got1, K, 1) == s1, (what, "order 1")
    got2 = e.moment_sums(vecs, 2, center=ref["mean"], **kw)
    assert hm.array_sums(got2, K, 2) == s2, (what, "order 2")
    _same_dict(e.moments(vecs, **kw), ref, kw["grouped"], what)
    return ref


# ---- sizes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_and_vector_counts(ra, n):
    """One member, the edges of a wave and of a block, several blocks; K = 1, 2, 8; full-mantissa doubles over 2^+-60; plain,
    weighted with random weights below 2^30, and plain again with those weights still set (they are ignored without the flag)."""
    rng = np.random.default_rng(n)
    X = np.stack([_spread(rng, n) for _ in range(8)])
    X[1] += 3.0 * X[0]                      # something to correlate
    w = rng.integers(0, 1 << 30, n)
    with _ens(ra, n) as e:
        for K in (1, 2, 8):
            vecs = _load(e, X[:K])
            plain = _check(e, vecs, X[:K], what=(n, K, "plain"))
            e.set_member_weights(w)
            _check(e, vecs, X[:K], w, what=(n, K, "weighted"))
            again = e.moments(vecs)
            _same_dict(again, plain, False, (n, K, "weights set, not asked for"))
            assert again["weight"] == again["count"] == n


def test_past_the_grid_cap(ra):
    """One tile and three members past what one pass of the capped grid takes: the grid-stride second pass and its ragged tile, with
    a NaN and the heaviest member in that tail, weighted, in two contiguous groups that meet inside the tail."""
    n = _members_per_pass() + 64 + 3
    rng = np.random.default_rng(11)
    X = np.stack([_spread(rng, n, 40), rng.standard_normal(n)])
    X[0, n - 2] = np.nan
    X[1, n - 70] = np.inf
    w = rng.integers(0, 1 << 20, n)
    w[n - 1] = 1 << 40
    groups = (np.arange(n) >= n - 30).astype(np.int32)
    with _ens(ra, n) as e:
        vecs = _load(e, X)
        e.set_member_weights(w)
        e.set_member_groups(groups, 2)
        ref = _check(e, vecs, X, w, groups, 2, what="past the cap")
        assert ref["count"].tolist() == [n - 30 - 1, 29]


# ---- data -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 1000])
def test_ill_conditioned_rows(ra, n):
    """Pairs +-m up to 1e300 around a remainder in +-[1, 2): the mean is the remainder over n, exactly.  The squares of the 1e300 row
    overflow: its variance is NaN through the count of non-finite terms, which is compared; the same row scaled to 1e150 has a
    finite variance."""
    rng = np.random.default_rng(n)
    x = hd.ill_conditioned_row(rng, n)
    X = np.stack([x, x * 1e-150])
    with _ens(ra, n) as e:
        vecs = _load(e, X)
        ref = _check(e, vecs, X, what="ill-conditioned")
        got = e.moments(vecs)
        rem = x[(n - (2 - n % 2)) // 2:][:2 - n % 2]
        assert 0.0 < abs(got["mean"][0]) < 4.0 / n
        if n % 2:
            assert got["mean"][0] == rem[0] / n          # one member is left: one correctly rounded division
        assert np.isnan(got["cov"][0, 0]) and np.isfinite(got["cov"][1, 1]) and got["cov"][1, 1] > 1e290
        s2 = e.moment_sums(vecs, 2, center=ref["mean"])
        n_bad = hm.array_sums(s2, 2, 2)[0][2][0][1]
        assert 0 < n_bad < n and hm.array_sums(s2, 2, 2)[0][2][2][1] == 0


def test_subnormals_the_first_limb_and_the_last(ra):
    """2^-1074 (the lowest bit of limb 0) and other subnormals beside the largest finite double with weight 2^52 (limbs 64 .. 67):
    both ends of the accumulator in one sum, the heavy member alone carrying half of the weight bound."""
    n = 130
    rng = np.random.default_rng(5)
    x = rng.integers(1, 1 << 52, n).astype(np.float64) * 5e-324          # subnormals
    x[::3] *= -1.0
    x[0], x[64], x[129], x[7] = 5e-324, DBL_MAX, -5e-324, 2.2250738585072014e-308
    y = _spread(rng, n, 1000)
    y[100] = -DBL_MAX
    w = rng.integers(0, 1 << 20, n)
    w[64], w[100], w[0] = 1 << 52, 1 << 51, 1
    X = np.stack([x, y])
    with _ens(ra, n) as e:
        vecs = _load(e, X)
        e.set_member_weights(w)
        ref = _check(e, vecs, X, w, what="both ends, weighted")
        assert np.isfinite(ref["mean"]).all() and ref["mean"][0, 0] > 1e307
        _check(e, vecs, X, what="both ends, plain")
        tiny = np.stack([np.where(np.arange(n) == 64, 0.0, x), np.full(n, 5e-324)])
        vecs = _load(e, tiny)
        ref = _check(e, vecs, tiny, w, what="subnormals only")
        assert ref["mean"][0, 1] == 5e-324 and ref["cov"][0, 1, 1] == 0.0 and 0.0 < abs(ref["mean"][0, 0]) < 2.3e-308


def test_non_finite_members_leave_listwise(ra):
    """NaN, +inf and -inf in ONE vector each take the member out of every sum: a whole tile, the last partial wave, scattered."""
    n = 1000
    rng = np.random.default_rng(6)
    X = np.stack([_spread(rng, n, 10) for _ in range(3)])
    X[0, 64:128] = np.nan
    X[1, 990:] = np.inf
    X[2, rng.choice(900, 40, replace=False)] = -np.inf
    X[1, 3], X[2, 5], X[0, 999] = np.nan, np.inf, -np.inf
    w = rng.integers(1, 1 << 30, n)
    with _ens(ra, n) as e:
        vecs = _load(e, X)
        ref = _check(e, vecs, X, what="listwise")
        assert ref["count"][0] == int(np.isfinite(X).all(axis=0).sum()) < n - 100
        e.set_member_weights(w)
        _check(e, vecs, X, w, what="listwise, weighted")
        X[:, :] = np.nan
        X[1] = 1.0
        vecs = _load(e, X)
        ref = _check(e, vecs, X, w, what="no member counts")
        assert ref["count"][0] == 0 and ref["weight"][0] == 0 and np.isnan(ref["mean"]).all()


def test_weights(ra):
    """All zero: weight 0, NaN, the count still n; one member of 2^52 among zeros: its values are the means, the covariance +0.0."""
    n = 300
    rng = np.random.default_rng(7)
    X = np.stack([_spread(rng, n), _spread(rng, n)])
    with _ens(ra, n) as e:
        vecs = _load(e, X)
        w = np.zeros(n, dtype=np.int64)
        e.set_member_weights(w)
        got = e.moments(vecs, weighted=True)
        _check(e, vecs, X, w, what="all zero")
        assert got["weight"] == 0 and got["count"] == n and np.isnan(got["mean"]).all() and np.isnan(got["cov"]).all()
        w[222] = 1 << 52
        e.set_member_weights(w)
        _check(e, vecs, X, w, what="one member")
        got = e.moments(vecs, weighted=True)
        assert got["weight"] == 1 << 52 and np.array_equal(got["mean"], X[:, 222])
        assert np.array_equal(got["cov"].view(np.uint64), np.zeros((2, 2)).view(np.uint64))
        assert np.isnan(got["corr"]).all()


# ---- groups -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_groups(ra, layout):
    """Five groups: three with members, one empty, one whose only members are non-finite; members of no group (-1) among them."""
    n, G = 1000, 5
    rng = np.random.default_rng(9)
    X = np.stack([_spread(rng, n, 30), rng.standard_normal(n), _spread(rng, n, 5)])
    if layout == "contiguous":
        groups = np.repeat([0, 1, 2, 4], [300, 37, 563, 100]).astype(np.int32)
    else:
        groups = rng.choice([0, 1, 2], n).astype(np.int32)
        groups[rng.choice(n, 50, replace=False)] = 4
    X[1, groups == 4] = np.nan                      # group 4: only non-finite members; group 3: none at all
    groups[rng.choice(np.flatnonzero(groups != 4), 60, replace=False)] = -1
    w = rng.integers(0, 1 << 30, n)
    with _ens(ra, n) as e:
        vecs = _load(e, X)
        e.set_member_groups(groups, G)
        ref = _check(e, vecs, X, None, groups, G, what=(layout, "plain"))
        assert ref["count"][3] == 0 == ref["count"][4] and (ref["count"][:3] > 0).all()
        assert np.isnan(ref["mean"][3:]).all() and np.isfinite(ref["cov"][:3]).all()
        e.set_member_weights(w)
        _check(e, vecs, X, w, groups, G, what=(layout, "weighted"))
        got = e.moments(vecs, weighted=True, grouped=True)
        assert got["mean"].shape == (G, 3) and got["cov"].shape == (G, 3, 3) and got["count"].shape == (G,)
        _same_dict(e.moments(vecs), hm.moments(X), False, (layout, "groups set, not asked for"))
        # a centre that is not finite in one group: that group's blocks stay zero with every term counted, its n and W in place
        c = ref["mean"].copy()
        c[:3] = 0.5
        c[1, 2] = np.inf
        s2 = hm.array_sums(e.moment_sums(vecs, 2, center=c, grouped=True), 3, 2)
        assert s2 == hm.sums(X, 2, c, None, groups, G)
        assert all(b == (0, ref["count"][1]) for b in s2[1][2]) and s2[1][0] == ref["count"][1] and s2[0][2][0][1] == 0


# ---- structure and API ----------------------------------------------------------------------------------------------------------------

def test_two_handles_add_up_to_one(ra):
    """The int64 arrays of two handles of N1 + N2 members, added element by element as an all-reduce adds them, have the canonical
    values of one handle of all members; finished by moments_global's finishing path they are its bits.  moments_global itself,
    in one process, is Ensemble.moments."""
    from rscm_amd import distributed
    from rscm_amd.ensemble import moment_means, moments_result
    n1, n2, K, G = 300, 701, 3, 2
    n = n1 + n2
    rng = np.random.default_rng(10)
    X = np.stack([_spread(rng, n, 50) for _ in range(K)])
    X[2, 5], X[0, 999] = np.nan, np.inf
    w = rng.integers(0, 1 << 30, n)
    groups = rng.choice([-1, 0, 1], n).astype(np.int32)
    with _ens(ra, n) as whole, _ens(ra, n1) as a, _ens(ra, n2) as b:
        parts = [(whole, slice(0, n)), (a, slice(0, n1)), (b, slice(n1, n))]
        vecs = {}
        for e, sl in parts:
            vecs[e] = _load(e, X[:, sl])
            e.set_member_weights(w[sl])
            e.set_member_groups(groups[sl], G)
        for kw in (dict(weighted=True, grouped=True), dict()):
            g = G if kw else 1
            s1 = a.moment_sums(vecs[a], 1, **kw) + b.moment_sums(vecs[b], 1, **kw)
            assert hm.array_sums(s1, K, 1) == hm.array_sums(whole.moment_sums(vecs[whole], 1, **kw), K, 1)
            mean = moment_means(s1, K, g)
            s2 = a.moment_sums(vecs[a], 2, center=mean, **kw) + b.moment_sums(vecs[b], 2, center=mean, **kw)
            assert hm.array_sums(s2, K, 2) == hm.array_sums(whole.moment_sums(vecs[whole], 2, center=mean, **kw), K, 2)
            got = moments_result(s1, s2, K, g, grouped=bool(kw))
            one = whole.moments(vecs[whole], **kw)
            ref = hm.moments(X, w, groups, G) if kw else hm.moments(X)
            _same_dict(got, ref, bool(kw), "two handles")
            _same_dict(one, ref, bool(kw), "one handle")
            _same_dict(distributed.moments_global(whole, vecs[whole], **kw), ref, bool(kw), "moments_global, one process")


def test_a_vector_against_itself(ra):
    """corr of a vector with itself -- the diagonal -- is exactly 1; the same vector passed twice has cov_01 = cov_00 = cov_11 to the
    bit and corr_01 = cov / (sd sd) by the stated rule, which is exactly 1 where the variance is a square (+-2: variance 4)."""
    n = 500
    rng = np.random.default_rng(12)
    v = _spread(rng, n, 8)
    two = np.where(rng.random(n) < 0.5, -2.0, 2.0)
    two[:2] = [2.0, -2.0]
    two[2:] = np.resize([2.0, -2.0], n - 2)         # mean exactly 0, variance exactly 4
    with _ens(ra, n) as e:
        X = np.stack([v, v, two, two])
        vecs = _load(e, X)
        ref = _check(e, vecs, X, what="twice")
        got = e.moments(vecs)
        assert got["corr"][0, 0] == got["corr"][1, 1] == got["corr"][2, 2] == 1.0
        assert got["cov"][0, 1] == got["cov"][0, 0] == got["cov"][1, 1]
        assert got["corr"][0, 1] == got["cov"][0, 1] / (got["sd"][0] * got["sd"][1]) and abs(got["corr"][0, 1] - 1.0) <= 2.0 ** -52
        assert got["mean"][2] == 0.0 and got["cov"][2, 3] == 4.0 and got["corr"][2, 3] == 1.0 == got["corr"][3, 2]
        assert ref["count"][0] == n


def test_parameter_rows_and_an_indicator_after_a_run(ra):
    """The plumbing: parameter rows and an indicator vector of a short two-layer run, one member failed by a NaN parameter."""
    n = 777
    t = np.arange(1750.0, 1771.0)
    P = two_layer_params(n)
    P[0, 13] = np.nan
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0)) as e:
        e.set_params(P)
        e.set_forcing(f_syn(t))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.run()
        d = e.indicators(1, 10, 21)
        vecs = [e.params_vector(0), e.params_vector(4), d["mean"]]
        X = np.stack([v.to_host() for v in vecs])
        assert np.isnan(X[2, 13]) and np.isfinite(np.delete(X, 13, axis=1)).all()
        ref = _check(e, vecs, X, what="plumbing")
        assert ref["count"][0] == n - 1 and np.isfinite(ref["corr"]).all() and abs(ref["corr"][0, 0, 2]) > 0.1


def test_graph_model_moments(ra):
    """GraphModel.moments on indicator vectors of the emissions-driven chain, weighted by the model's member weights."""
    n = 300
    model = magicc_chain().build_chain(n, 20, "topological")
    try:
        model.run()
        ens, _ = model.variable_home("Surface Temperature")
        d = model.indicators("Surface Temperature", 10, ens.n_times, 1, [0.2])
        vecs = [d["mean"], d["peak"]]
        X = np.stack([v.to_host() for v in vecs])
        w = np.random.default_rng(3).integers(0, 1 << 30, n)
        model.set_member_weights(w)
        _same_dict(model.moments(vecs), hm.moments(X), False, "graph")
        _same_dict(model.moments(vecs, weighted=True), hm.moments(X, w), False, "graph, weighted")
    finally:
        model.close()


def test_refusals(ra):
    """Every refusal the header names: the anomaly flag and unknown flags, K outside 1 .. 8, an order outside {1, 2}, order 2 without
    a centre, a NULL out or vector list, a host address as a vector (RSCM_ERR_INVALID); weighted without weights and grouped without
    groups (RSCM_ERR_STATE)."""
    import ctypes as C

    from rscm_amd import _lib
    n = 100
    with _ens(ra, n) as e:
        vecs = _load(e, np.ones((2, n)))
        lib, h = e._lib, e._h
        arr = (C.POINTER(C.c_double) * 9)(*[C.cast(C.c_void_p(e.params_vector(k % 8).ptr), C.POINTER(C.c_double)) for k in range(9)])
        out = np.zeros(2 + 45 * hm.BLOCK, dtype=np.int64)
        po = out.ctypes.data_as(C.POINTER(C.c_int64))
        c = np.zeros(9)
        pc = c.ctypes.data_as(C.POINTER(C.c_double))

        def sums(n_vec=2, a=arr, flags=0, order=1, centre=pc, o=po):
            return lib.rscm_ens_moment_sums(h, n_vec, a, flags, order, centre, o, 0)

        assert sums() == _lib.OK and out[0] == n == out[1]
        assert sums(n_vec=8, order=2) == _lib.OK
        for kw in (dict(flags=_lib.SELECT_ANOMALY), dict(flags=8), dict(flags=_lib.SELECT_WEIGHTED | 16), dict(n_vec=0), dict(n_vec=9),
                   dict(order=0), dict(order=3), dict(order=2, centre=None), dict(o=None), dict(a=None)):
            assert sums(**kw) == _lib.ERR_INVALID, kw
        host = np.ones(n)
        bad = (C.POINTER(C.c_double) * 2)(arr[0], host.ctypes.data_as(C.POINTER(C.c_double)))
        assert sums(a=bad) == _lib.ERR_INVALID
        assert sums(flags=_lib.SELECT_WEIGHTED) == _lib.ERR_STATE and sums(flags=_lib.SELECT_GROUPED) == _lib.ERR_STATE
        mean, cov = np.zeros(2), np.zeros(4)
        pm, pv = mean.ctypes.data_as(C.POINTER(C.c_double)), cov.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.rscm_ens_moments(h, 2, arr, 0, pm, pv, None, None) == _lib.OK and mean.tolist() == [1.0, 1.0] and not cov.any()
        assert lib.rscm_ens_moments(h, 2, arr, _lib.SELECT_ANOMALY, pm, pv, None, None) == _lib.ERR_INVALID
        assert lib.rscm_ens_moments(h, 2, arr, _lib.SELECT_WEIGHTED, pm, pv, None, None) == _lib.ERR_STATE
        assert lib.rscm_ens_moments(h, 2, arr, 0, None, pv, None, None) == _lib.ERR_INVALID
        assert lib.rscm_ens_moments(h, 9, arr, 0, pm, pv, None, None) == _lib.ERR_INVALID
        assert refusal_code(e.moments, vecs, weighted=True) == _lib.ERR_STATE
        assert refusal_code(e.moment_sums, vecs, 1, grouped=True) == _lib.ERR_STATE
        with pytest.raises(ValueError):
            e.moment_sums(vecs, 2)
        with pytest.raises(ValueError):
            e.moments([e.params_vector(k % 8) for k in range(9)])


def test_sums_into_device_memory(ra):
    """on_device != 0: the sums land in device memory of the handle's device (here four spare parameter rows, read back as int64),
    the same integers as through the host; an address too close to the end of its allocation, or host memory, is refused."""
    import ctypes as C

    from rscm_amd import _lib
    n, K = 1000, 2
    rng = np.random.default_rng(13)
    X = np.stack([_spread(rng, n), _spread(rng, n)])
    groups = rng.integers(-1, 3, n).astype(np.int32)
    with _ens(ra, n) as e:
        vecs = _load(e, X)
        e.set_member_groups(groups, 3)
        arr = (C.POINTER(C.c_double) * K)(*[C.cast(C.c_void_p(v.ptr), C.POINTER(C.c_double)) for v in vecs])
        base = e.params_vector(4).ptr                                  # rows 4 .. 7: 4000 spare doubles
        for order, flags, G in ((1, 0, 1), (2, _lib.SELECT_GROUPED, 3)):
            want = e.moment_sums(vecs, order, center=np.full((G, K), 0.25), grouped=G > 1)
            assert want.size <= 4 * n
            c = np.full(G * K, 0.25)
            rc = e._lib.rscm_ens_moment_sums(e._h, K, arr, flags, order, c.ctypes.data_as(C.POINTER(C.c_double)),
                                             C.cast(C.c_void_p(base), C.POINTER(C.c_int64)), 1)
            assert rc == _lib.OK
            got = np.empty(want.size, dtype=np.int64)
            _lib.check(e._lib.rscm_gpu_copy_to_host(e.device, got.ctypes.data_as(C.c_void_p), C.c_void_p(base), got.nbytes))
            assert hm.array_sums(got.reshape(want.shape), K, order) == hm.array_sums(want, K, order)
            assert hm.array_sums(want, K, order) == hm.sums(X, order, np.full((G, K), 0.25), None, groups if G > 1 else None, G if G > 1 else None)
        near_end = e.params_vector(7).ptr + 8 * (n - 10)
        host = np.zeros(2 + K * hm.BLOCK, dtype=np.int64)
        for p in (near_end, host.ctypes.data):
            assert e._lib.rscm_ens_moment_sums(e._h, K, arr, 0, 1, None, C.cast(C.c_void_p(p), C.POINTER(C.c_int64)), 1) == _lib.ERR_INVALID
        assert not host.any()
