"""GPU tier of the exact weighted mean and spread of a stored variable at every row (csrc/moment_rows.hip, ABI minor 24) against the
integers and fractions of tests/host_moment_rows.py.  No tolerance anywhere: doubles are compared bit for bit (any NaN for a NaN)
and the device's blocks as canonical integers with their counts of non-finite terms -- never limb by limb, since deferred carries
depend on the order of summation and on the path a term took (a lane's window or the serial walk).

The rows are those of a small two-layer ensemble, overwritten with set_state so that they take any bits; the member vectors are
parameter rows of a two-layer mix ensemble of the same size (eight rows of N doubles that take any bits)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import host_moment_rows as hr
from tests import host_moments as hm
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import f_syn, magicc_chain, two_layer_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_AXIS = np.arange(1750.0, 1758.0)          # 8 rows
DBL_MAX = float(np.finfo(np.float64).max)


def _members_per_pass() -> int:
    """Members one pass of the kernel's capped grid takes, read from the code: kMomRowBlocks blocks of four waves of 64."""
    text = open(os.path.join(ROOT, "rscm_amd", "csrc", "rscm_device.hpp")).read()
    blocks = int(re.search(r"constexpr int kMomRowBlocks = (\d+);", text).group(1))
    per_pass = int(re.search(r"constexpr int64_t kMomentRowsMembersPerPass = (\d+);", text).group(1))
    hip = open(os.path.join(ROOT, "rscm_amd", "csrc", "moment_rows.hip")).read()
    threads = int(re.search(r"constexpr int kMomRowThreads = (\d+);", hip).group(1))
    assert per_pass == blocks * threads
    return per_pass


def _stats(e):
    out = (C.c_int64 * 3)()
    assert e._lib.rscm_gpu_moment_rows_last_stats(out) == 0
    return list(out)


def _spread(rng, n, span=20):
    """Full-mantissa doubles of both signs with exponents spread over 2^+-span."""
    return rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-span, span + 1, n)) * rng.choice([-1.0, 1.0], n)


def _rows_ens(ra, n, X=None, steps=None, t=T_AXIS, **kw):
    """A two-layer ensemble run to `steps` (None: the end, 0: not at all); X[R][n] then overwrites rows 0 .. R-1 of variable 1."""
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0), **kw)
    e.set_params(two_layer_params(n))
    e.set_forcing(f_syn(t))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    if steps != 0:
        e.run(steps)
    if X is not None:
        _fill(e, X)
    return e


def _fill(e, X, var=1):
    for t, row in enumerate(np.asarray(X, dtype=np.float64)):
        e.set_state(var, t, row)
    got = e.get_series(var, 0, len(X))
    assert np.array_equal(got.view(np.uint64), np.asarray(X, dtype=np.float64).view(np.uint64))


def _vec_ens(ra, n):
    return ra.Ensemble(ra.KIND_TWO_LAYER, n, np.arange(1750.0, 1754.0), forcing_components=2)


def _load(v, V):
    """V[K][n] into the first K parameter rows of the mix ensemble v; their DeviceVectors."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, v.n_members)
    P = np.ones((8, v.n_members))
    P[:V.shape[0]] = V
    v.set_params(P)
    return [v.params_vector(k) for k in range(V.shape[0])]


def _same_dict(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert hm.same_bits(np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)), (what, k, got[k], ref[k])


def _check(e, vecs, X, V=(), w=None, groups=None, G=None, baseline=None, rows=None, what=""):
    """moment_rows_sums of both orders as canonical integers, the path counts of both launches, then moment_rows, against the
    reference over the rows `rows` = (t_begin, t_end, t_stride) of X (default: all of X); returns the reference (group axis kept)."""
    X = np.asarray(X, dtype=np.float64)
    tb, te, ts = rows if rows is not None else (0, X.shape[0], 1)
    Xr = X[tb:te:ts]
    K = len(vecs)
    V = np.asarray(V, dtype=np.float64).reshape(K, X.shape[1])
    kw = dict(weighted=w is not None, grouped=groups is not None, anomaly=baseline is not None)
    hkw = dict(weights=w, groups=groups, n_groups=G, baseline=baseline)
    ref, s1, s2 = hr.moment_rows(Xr, V, with_sums=True, **hkw)
    got1 = e.moment_rows_sums(1, 1, tb, te, ts, vectors=vecs, **kw)
    assert got1.dtype == np.int64 and got1.shape == (Xr.shape[0], G or 1, 2 + (1 + K) * hm.BLOCK)
    assert hr.array_sums(got1, K, 1) == s1, (what, "order 1")
    st = _stats(e)
    assert st[0] + st[1] == hr.n_terms(Xr, 1, V, **hkw), (what, "terms of order 1", st)
    centre = hr.means(s1)
    got2 = e.moment_rows_sums(1, 2, tb, te, ts, vectors=vecs, center=centre, **kw)
    assert hr.array_sums(got2, K, 2) == s2, (what, "order 2")
    st = _stats(e)
    assert st[0] + st[1] == hr.n_terms(Xr, 2, V, centre, **hkw), (what, "terms of order 2", st)
    got = e.moment_rows(1, tb, te, ts, vectors=vecs, **kw)
    _same_dict(got, ref if kw["grouped"] else hr.ungrouped(ref), what)
    return ref


# ---- sizes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_rows_and_vector_counts(ra, n):
    """One member, the edges of a wave and of a block, several blocks; 1, 2 and 5 rows; K = 0, 1, 4 -- against the restatement, and
    every row against ``moments`` of that row (a DeviceVector into the fully stored series) and the vectors: the matching entries
    of mean and cov are equal."""
    rng = np.random.default_rng(n)
    X = np.stack([_spread(rng, n) for _ in range(5)])
    V = np.stack([_spread(rng, n) for _ in range(4)])
    V[0] += 3.0 * X[3]                      # something to co-vary with
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v:
        all_vecs = _load(v, V)
        base = e.series_devptr(1)
        for R in (1, 2, 5):
            for K in (0, 1, 4):
                ref = hr.ungrouped(_check(e, all_vecs[:K], X[:R], V[:K], what=(n, R, K)))
                assert (ref["count"] == n).all()
                for t in range(R):
                    row_t = ra.ensemble.DeviceVector(base + 8 * n * t, n, np.float64, e)
                    m = e.moments([row_t] + all_vecs[:K])
                    assert hm.same_bits(m["mean"][0], ref["mean"][t]) and hm.same_bits(m["cov"][0, 0], ref["var"][t])
                    if K:
                        assert hm.same_bits(m["mean"][1:], ref["vec_mean"][t]) and hm.same_bits(m["cov"][0, 1:], ref["cov"][t])
                        assert hm.same_bits(np.diag(m["cov"])[1:], ref["vec_var"][t])


def test_past_the_grid_cap(ra):
    """One tile and three members past what one pass of the capped grid takes, two rows: the grid-stride second pass and its ragged
    tile, with a NaN and the heaviest member in that tail, weighted, in two contiguous groups that meet inside the tail."""
    n = _members_per_pass() + 64 + 3
    rng = np.random.default_rng(11)
    X = np.stack([_spread(rng, n, 10), rng.standard_normal(n)])
    V = rng.standard_normal((1, n))
    X[0, n - 2] = np.nan
    V[0, n - 70] = np.inf
    w = rng.integers(0, 1 << 20, n)
    w[n - 1] = 1 << 40
    groups = (np.arange(n) >= n - 30).astype(np.int32)
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v:
        vecs = _load(v, V)
        e.set_member_weights(w)
        e.set_member_groups(groups, 2)
        ref = _check(e, vecs, X, V, w, groups, 2, what="past the cap")
        assert ref["count"].tolist() == [[n - 30 - 1, 29], [n - 30 - 1, 30]]


# ---- paths ------------------------------------------------------------------------------------------------------------------------

def test_a_plume_stays_inside_the_window(ra):
    """Values in [1, 4) with weights in [1, 8]: every term of order 1 lies within 5 bits of the largest, far inside the 64 bits the
    window spans below it, so no term may take the serial walk and no window may move."""
    n = 3 * _members_per_pass() + 100          # every wave sees several tiles
    rng = np.random.default_rng(21)
    X = rng.uniform(1.0, 4.0, (2, n))
    X[1, ::5] *= -1.0                          # both signs
    w = rng.integers(1, 9, n)
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        got = e.moment_rows_sums(1, 1, 0, 2, weighted=True)
        assert hr.array_sums(got, 0, 1) == hr.sums(X, 1, weights=w)
        assert _stats(e) == [2 * n, 0, 0]
        _check(e, [], X, w=w, what="plume")


def test_an_ill_conditioned_row_walks_and_rebases(ra):
    """1e300, 1, 1e-300, subnormals and zeros: the first pass of the grid sees 1e-300 only, the second 1e300 only (every window moves
    up), the third 1 only (every term below the window: it moves down), the tail mixes all of them in every tile (the window sits at
    1e300, the rest is walked).  The bits are the restatement's whichever path a term took."""
    p = _members_per_pass()
    n = 3 * p + 1000
    rng = np.random.default_rng(22)
    sign = rng.choice([-1.0, 1.0], n)
    x = np.concatenate([np.full(p, 1e-300), np.full(p, 1e300), np.full(p, 1.0),
                        rng.choice([1e300, 1.0, 1e-300, 5e-324, 3e-310, 0.0], 1000)]) * rng.uniform(1.0, 2.0, n) * sign
    X = np.stack([x, x[::-1]])
    with _rows_ens(ra, n, X) as e:
        got = e.moment_rows_sums(1, 1, 0, 2)
        assert hr.array_sums(got, 0, 1) == hr.sums(X, 1)
        win, walked, rebases = _stats(e)
        assert win + walked == hr.n_terms(X, 1) < 2 * n and walked > 0 and win > walked and rebases >= 1
        ref = hr.ungrouped(_check(e, [], X, what="ill-conditioned"))
        assert np.isfinite(ref["mean"]).all() and np.isnan(ref["var"]).all()       # the squares of 1e300 overflow
        w = rng.integers(0, 1 << 30, n)
        e.set_member_weights(w)
        _check(e, [], X, w=w, what="ill-conditioned, weighted")


def test_both_ends_of_the_accumulator(ra):
    """2^-1074 (the lowest bit of limb 0) beside the largest finite double with weight 2^52 (limbs 64 .. 67) in one row."""
    n = 130
    rng = np.random.default_rng(5)
    x = rng.integers(1, 1 << 52, n).astype(np.float64) * 5e-324
    x[::3] *= -1.0
    x[0], x[64], x[129], x[7] = 5e-324, DBL_MAX, -5e-324, 2.2250738585072014e-308
    w = rng.integers(0, 1 << 20, n)
    w[64], w[0] = 1 << 52, 1
    X = np.stack([x, np.where(np.arange(n) == 64, 0.0, x), np.full(n, 5e-324)])
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        ref = hr.ungrouped(_check(e, [], X, w=w, what="both ends, weighted"))
        assert ref["mean"][0] > 1e307 and 0.0 < abs(ref["mean"][1]) < 2.3e-308 and ref["mean"][2] == 5e-324 and ref["var"][2] == 0.0
        _check(e, [], X, what="both ends, plain")


# ---- which members count ----------------------------------------------------------------------------------------------------------

def test_non_finite_values_per_row(ra):
    """A member that is NaN from row 2 on leaves rows 2 .. only; a NaN in a vector takes its member out of every row; a NaN baseline
    takes its member out under anomaly; products that overflow make that row's var NaN and nothing else."""
    n = 1000
    rng = np.random.default_rng(6)
    X = np.stack([_spread(rng, n, 8) for _ in range(5)])
    V = np.stack([_spread(rng, n, 8) for _ in range(2)])
    X[2:, 17] = np.nan
    X[1, 64:128] = np.inf                   # a whole tile of one row
    X[4, 990:] = -np.inf                    # the last partial wave
    V[1, 500] = np.nan
    X[3, 300], X[3, 301] = 1e200, -1e200    # finite, but the squares are not
    b = X[:2].mean(axis=0)
    b[64:128] = X[0, 64:128]                # (row 1 is infinite there)
    b[40] = np.nan
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v:
        vecs = _load(v, V)
        ref = hr.ungrouped(_check(e, vecs, X, V, what="per row"))
        assert ref["count"].tolist() == [n - 1, n - 1 - 64, n - 2, n - 2, n - 2 - 10]
        assert np.isnan(ref["var"][3]) and np.isfinite(ref["cov"][3]).all() and np.isfinite(ref["mean"][3])
        assert np.isfinite(ref["var"][[0, 1, 2, 4]]).all() and np.isfinite(ref["vec_var"]).all()
        plain = hr.ungrouped(_check(e, [], X, what="per row, no vectors"))
        assert plain["count"][0] == n and plain["count"][2] == n - 1
        e.set_baseline_values(b)
        anom = hr.ungrouped(_check(e, [], X, baseline=b, what="NaN baseline"))
        assert anom["count"][0] == n - 1 and anom["count"][2] == n - 2
        X[:, :] = np.nan
        _fill(e, X)
        ref = hr.ungrouped(_check(e, vecs, X, V, what="no member counts"))
        assert (ref["count"] == 0).all() and (ref["weight"] == 0).all() and np.isnan(ref["mean"]).all() and np.isnan(ref["slope"]).all()


def test_weighted_with_zero_weights(ra):
    n = 777
    rng = np.random.default_rng(7)
    X = np.stack([_spread(rng, n, 4) for _ in range(3)])
    V = rng.standard_normal((2, n))
    w = rng.integers(0, 1 << 30, n)
    w[rng.random(n) < 0.3] = 0
    w[64:128] = 0                           # a tile without weight
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v:
        vecs = _load(v, V)
        plain = hr.ungrouped(_check(e, vecs, X, V, what="plain"))
        e.set_member_weights(w)
        ref = hr.ungrouped(_check(e, vecs, X, V, w, what="weighted"))
        assert (ref["count"] == n).all() and (ref["weight"] == int(w.sum())).all()
        _same_dict(e.moment_rows(1, 0, 3, vectors=vecs), plain, "weights set, not asked for")
        e.set_member_weights(np.zeros(n, dtype=np.int64))
        ref = hr.ungrouped(_check(e, vecs, X, V, np.zeros(n, dtype=np.int64), what="no weight at all"))
        assert (ref["count"] == n).all() and np.isnan(ref["mean"]).all()


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_grouped(ra, layout):
    """Three scenarios, contiguous blocks and posterior()'s i % 3, with members of no group, a group that is empty in row 1 (all its
    values NaN there), weights, two vectors; the group dimension comes after rows."""
    n = 1000
    rng = np.random.default_rng(8)
    groups = (np.arange(n) * 3 // n if layout == "contiguous" else np.arange(n) % 3).astype(np.int32)
    groups[rng.random(n) < 0.05] = -1
    X = np.stack([_spread(rng, n, 4) + g for g in range(3)]) + 0.5 * groups
    X[1, groups == 2] = np.nan
    V = rng.standard_normal((2, n))
    w = rng.integers(0, 1 << 30, n)
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v:
        vecs = _load(v, V)
        e.set_member_groups(groups, 3)
        ref = _check(e, vecs, X, V, groups=groups, G=3, what=layout)
        assert ref["mean"].shape == (3, 3) and ref["slope"].shape == (3, 3, 2)
        assert ref["count"][1, 2] == 0 and np.isnan(ref["mean"][1, 2]) and ref["count"][0, 2] == (groups == 2).sum()
        e.set_member_weights(w)
        _check(e, vecs, X, V, w, groups, 3, what=layout + ", weighted")
        _check(e, [], X, groups=groups, G=3, what=layout + ", no vectors")
        one = e.moment_rows(1, 0, 3, vectors=vecs)                     # groups set, not asked for
        assert one["mean"].shape == (3,) and (one["count"] == [n, n - (groups == 2).sum(), n]).all()


def test_many_groups_split_the_bins(ra):
    """64 groups and four vectors: nine blocks a group do not fit one block's LDS bins, the groups are split over the grid."""
    n = 1000
    rng = np.random.default_rng(9)
    groups = rng.integers(-1, 64, n).astype(np.int32)
    X = np.stack([_spread(rng, n, 4) for _ in range(2)])
    V = rng.standard_normal((4, n))
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v:
        vecs = _load(v, V)
        e.set_member_groups(groups, 64)
        ref = _check(e, vecs, X, V, groups=groups, G=64, what="64 groups")
        assert ref["cov"].shape == (2, 64, 4) and ref["count"].sum() == 2 * (groups >= 0).sum()


def test_anomaly_of_a_reference_period(ra):
    """The baseline is each member's mean over rows 0 .. 2 (set_baseline); the anomaly mean over the reference rows and beyond against
    the restatement, which subtracts the library's baseline once per value."""
    n = 513
    rng = np.random.default_rng(10)
    X = np.cumsum(0.1 + 0.05 * rng.standard_normal((6, n)), axis=0) + 13.0
    with _rows_ens(ra, n, X) as e:
        e.set_baseline(1, 0, 3)
        b = e.baseline()
        ref = hr.ungrouped(_check(e, [], X, baseline=b, what="anomaly"))
        assert abs(ref["mean"][:3].sum()) < 1e-12 and (ref["mean"][3:] > 0.1).all()
        q = e.quantile_rows(1, [0.0, 1.0], 0, 6, anomaly=True)["quantiles"]
        assert (q[:, 0] <= ref["mean"]).all() and (ref["mean"] <= q[:, 1]).all()
        sub = e.moment_rows(1, 1, 6, 2, anomaly=True)
        _same_dict(sub, {k: v[1:6:2] for k, v in ref.items()}, "strided")
        e.clear_baseline()
        assert refusal_code(e.moment_rows, 1, 0, 3, anomaly=True) == 2


# ---- shards, device memory, storage layouts ---------------------------------------------------------------------------------------

def test_two_handles_add_up(ra):
    """The staged sums of two handles over the two parts of a member set add up, element by element, to those of one handle over the
    whole set, as canonical integers, for both orders."""
    n, h = 901, 333
    rng = np.random.default_rng(12)
    X = np.stack([_spread(rng, n, 30) for _ in range(3)])
    V = rng.standard_normal((2, n))
    w = rng.integers(0, 1 << 30, n)
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v, _rows_ens(ra, h, X[:, :h]) as e1, _vec_ens(ra, h) as v1, \
            _rows_ens(ra, n - h, X[:, h:]) as e2, _vec_ens(ra, n - h) as v2:
        parts = ((e, _load(v, V)), (e1, _load(v1, V[:, :h])), (e2, _load(v2, V[:, h:])))
        e.set_member_weights(w), e1.set_member_weights(w[:h]), e2.set_member_weights(w[h:])
        s1 = [x.moment_rows_sums(1, 1, 0, 3, vectors=vv, weighted=True) for x, vv in parts]
        assert hr.array_sums(s1[1] + s1[2], 2, 1) == hr.array_sums(s1[0], 2, 1) == hr.sums(X, 1, V, weights=w)
        c = ra.ensemble.moment_rows_means(s1[1] + s1[2], 2, 1)
        s2 = [x.moment_rows_sums(1, 2, 0, 3, vectors=vv, center=c, weighted=True) for x, vv in parts]
        assert hr.array_sums(s2[1] + s2[2], 2, 2) == hr.array_sums(s2[0], 2, 2) == hr.sums(X, 2, V, c, weights=w)
        got = ra.ensemble.moment_rows_result(s1[1] + s1[2], s2[1] + s2[2], 2, 1, grouped=False)
        _same_dict(got, e.moment_rows(1, 0, 3, vectors=parts[0][1], weighted=True), "two handles")


def test_sums_into_device_memory(ra):
    """on_device != 0: the sums land in device memory of the handle's device (here spare parameter rows of the vector ensemble, read
    back as int64), the same integers as through the host; an address too close to the end of its allocation, or host memory, is
    refused."""
    from rscm_amd import _lib
    n, K = 1000, 1
    rng = np.random.default_rng(13)
    X = np.stack([_spread(rng, n, 30) for _ in range(3)])
    V = rng.standard_normal((1, n))
    with _rows_ens(ra, n, X) as e, _vec_ens(ra, n) as v:
        vecs = _load(v, V)
        arr = (C.POINTER(C.c_double) * K)(C.cast(C.c_void_p(vecs[0].ptr), C.POINTER(C.c_double)))
        base = v.params_vector(2).ptr                                  # rows 2 .. 7: 6000 spare doubles
        i64 = C.POINTER(C.c_int64)
        for order in (1, 2):
            c = np.full((3, 1, 2), 0.25)
            want = e.moment_rows_sums(1, order, 0, 3, vectors=vecs, center=c)
            assert want.size <= 6 * n
            rc = e._lib.rscm_ens_moment_rows_sums(e._h, 1, 0, 3, 1, K, arr, 0, order, c.ctypes.data_as(C.POINTER(C.c_double)),
                                                  C.cast(C.c_void_p(base), i64), 1)
            assert rc == _lib.OK
            got = np.empty(want.size, dtype=np.int64)
            _lib.check(e._lib.rscm_gpu_copy_to_host(e.device, got.ctypes.data_as(C.c_void_p), C.c_void_p(base), got.nbytes))
            assert hr.array_sums(got.reshape(want.shape), K, order) == hr.array_sums(want, K, order) == hr.sums(X, order, V, c)
        near_end = v.params_vector(7).ptr + 8 * (n - 10)
        host = np.zeros(3 * (2 + 2 * hm.BLOCK), dtype=np.int64)
        for p in (near_end, host.ctypes.data):
            assert e._lib.rscm_ens_moment_rows_sums(e._h, 1, 0, 3, 1, K, arr, 0, 1, None, C.cast(C.c_void_p(p), i64), 1) == _lib.ERR_INVALID
        assert not host.any()


def test_windowed_handle(ra):
    """A window of 8 rows and every 5th row in the output store: the resident rows agree with a fully stored twin, bit for bit; a
    row that has slid out and is not kept is RSCM_ERR_STATE."""
    n = 321
    t = np.arange(1750, 1791, dtype=np.float64)
    with _rows_ens(ra, n, t=t) as full, _rows_ens(ra, n, steps=0, t=t, window_rows=8, output_stride=5) as w:
        while w.time_index < len(t) - 1:
            w.run(min(w.time_index + 4, len(t) - 1))
        v = [full.params_vector(0)]
        vw = [w.params_vector(0)]
        want = full.moment_rows(1, vectors=v)
        kept = w.moment_rows(1, 0, 41, 5, vectors=vw)                                  # the output store
        _same_dict(kept, {k: x[0:41:5] for k, x in want.items()}, "output store")
        assert (kept["count"] == n).all() and (kept["slope"][1:, 0] != 0.0).all()
        last = w.moment_rows(1, 36, 41, vectors=vw)                                    # the window's last rows
        _same_dict(last, {k: x[36:41] for k, x in want.items()}, "window")
        assert refusal_code(w.moment_rows, 1, 0, 3) == 2                                      # row 1 is neither in the window nor kept
        assert refusal_code(w.moment_rows_sums, 1, 1, 31, 34) == 2


def test_rows_past_the_time_index(ra):
    n = 100
    with _rows_ens(ra, n, steps=3) as e:
        got = e.moment_rows(1, vectors=[e.params_vector(1)])
        assert got["count"].tolist() == [n] * 4 + [0] * 4 and (got["weight"] == got["count"]).all()
        for k in ("mean", "var", "sd"):
            assert np.isfinite(got[k][:4]).all() and np.isnan(got[k][4:]).all(), k
        for k in ("vec_mean", "vec_var", "cov", "corr", "slope"):
            assert got[k].shape == (8, 1) and np.isnan(got[k][4:]).all(), k
        ref = hr.ungrouped(hr.moment_rows(e.get_series(1, 0, 4), e.get_params()[1:2]))
        _same_dict({k: v[:4] for k, v in got.items()}, ref, "computed rows")
        s = e.moment_rows_sums(1, 1, 4, 8)
        assert not s.any() and _stats(e) == [0, 0, 0]
        assert e.moment_rows(1, 5, 5)["mean"].shape == (0,)


def test_a_diagnostic_by_name(ra):
    """The heat content works once computed -- the restatement over its rows -- and is refused when stale."""
    n = 129
    with _rows_ens(ra, n) as e:
        vid = e.define_heat_content()
        assert refusal_code(e.moment_rows, "Ocean Heat Content") == 2
        e.compute_diagnostic(vid)
        got = e.moment_rows("Ocean Heat Content", vectors=[e.params_vector(4)])
        ref = hr.ungrouped(hr.moment_rows(e.get_series(vid), e.get_params()[4:5]))
        _same_dict(got, ref, "heat content")
        assert (got["count"] == n).all() and (got["var"][2:] > 0).all()   # (the members part from row 2 on)
        e.set_state(1, 0, 0.25)
        assert refusal_code(e.moment_rows, "Ocean Heat Content") == 2
        from rscm_amd._lib import RscmGpuError
        with pytest.raises(RscmGpuError, match="is stale: compute it again"):
            e.moment_rows_sums(vid, 1)


def test_graph_model_moment_rows(ra):
    """By variable name on a graph: the home ensemble's rows, regressed on a parameter of that ensemble; a vector of another
    ensemble raises."""
    mod = magicc_chain()
    n = 257
    model = mod.build_chain(n, 12, "topological")
    try:
        model.run()
        name = "Surface Temperature"
        ens, vid = model.variable_home(name)
        row = 0
        vec = ens.params_vector(row)
        got = model.moment_rows(name, vectors=[vec])
        ref = hr.ungrouped(hr.moment_rows(model.get_series(name), ens.get_params()[row:row + 1]))
        _same_dict(got, ref, "graph")
        assert (got["count"] == n).all()
        _same_dict(model.moment_rows(name, 2, 10, 3), {k: v[2:10:3] for k, v in ref.items() if v.ndim == 1}, "graph, strided")
        other = next(x for x in model.ensembles.values() if x is not ens)
        with pytest.raises(ValueError, match="does not belong to the home ensemble"):
            model.moment_rows(name, vectors=[other.params_vector(0)])
    finally:
        model.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals(ra):
    from rscm_amd import _lib
    n = 70
    rng = np.random.default_rng(14)
    with _rows_ens(ra, n) as e, _vec_ens(ra, n) as v, _vec_ens(ra, n + 1) as longer:
        vecs = _load(v, rng.standard_normal((4, n)))
        lib, h = e._lib, e._h
        arr = (C.POINTER(C.c_double) * 5)(*[C.cast(C.c_void_p(x.ptr), C.POINTER(C.c_double)) for x in vecs + vecs[:1]])
        out = np.zeros(8 * (2 + 9 * hm.BLOCK), dtype=np.int64)
        po = out.ctypes.data_as(C.POINTER(C.c_int64))
        c = np.zeros(8 * 5)
        pc = c.ctypes.data_as(C.POINTER(C.c_double))

        def sums(var=1, tb=0, te=8, ts=1, n_vec=2, a=arr, flags=0, order=1, centre=pc, o=po):
            return lib.rscm_ens_moment_rows_sums(h, var, tb, te, ts, n_vec, a, flags, order, centre, o, 0)

        assert sums() == _lib.OK and out[0] == n == out[1]
        assert sums(n_vec=4, order=2) == _lib.OK and sums(n_vec=0, a=None) == _lib.OK
        for kw in (dict(flags=8), dict(flags=_lib.SELECT_WEIGHTED | 16), dict(n_vec=-1), dict(n_vec=5), dict(n_vec=1, a=None),
                   dict(order=0), dict(order=3), dict(order=2, centre=None), dict(o=None), dict(var=99), dict(tb=-1), dict(te=9),
                   dict(tb=5, te=4), dict(ts=0)):
            assert sums(**kw) == _lib.ERR_INVALID, kw
        for flags in (_lib.SELECT_WEIGHTED, _lib.SELECT_GROUPED, _lib.SELECT_ANOMALY):
            assert sums(flags=flags) == _lib.ERR_STATE, flags
        mean, second = np.zeros(8 * 5), np.zeros(8 * 9)
        pm, ps = mean.ctypes.data_as(C.POINTER(C.c_double)), second.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.rscm_ens_moment_rows(h, 1, 0, 8, 1, 4, arr, 0, pm, ps, None, None) == _lib.OK and np.isfinite(mean).all()
        assert lib.rscm_ens_moment_rows(h, 1, 0, 8, 1, 4, arr, 0, None, ps, None, None) == _lib.ERR_INVALID
        assert lib.rscm_ens_moment_rows(h, 1, 0, 8, 1, 5, arr, 0, pm, ps, None, None) == _lib.ERR_INVALID
        assert lib.rscm_ens_moment_rows(h, 1, 0, 8, 0, 1, arr, 0, pm, ps, None, None) == _lib.ERR_INVALID
        assert lib.rscm_gpu_moment_rows_last_stats(None) == _lib.ERR_INVALID
        # vectors: of another length, of the wrong type, too many; a staged select in flight
        with pytest.raises(ValueError):
            e.moment_rows(1, vectors=[longer.params_vector(0)])
        with pytest.raises(ValueError):
            e.moment_rows(1, vectors=vecs + vecs[:1])
        with pytest.raises(ValueError):
            e.moment_rows_sums(1, 2, vectors=vecs[:1])                 # order 2 without a centre
        with pytest.raises(ValueError):
            e.moment_rows_sums(1, 2, vectors=vecs[:1], center=np.zeros(3))
        near_end = (C.POINTER(C.c_double) * 1)(C.cast(C.c_void_p(v.params_vector(7).ptr + 8 * (n - 10)), C.POINTER(C.c_double)))
        assert sums(n_vec=1, a=near_end) == _lib.ERR_INVALID
        with e.select(1, [0.5], 0, 8):
            assert refusal_code(e.moment_rows, 1) == 2
        e.moment_rows(1)
    # more blocks than one call takes: 751 rows x 64 groups x 9 blocks are within the cap, 1000 rows of them are not; fewer groups are
    assert 751 * 64 * 9 <= (1 << 19) < 1000 * 64 * 9
    with _rows_ens(ra, 8, steps=0, t=np.arange(1000.0)) as e, _vec_ens(ra, 8) as v:
        vecs = _load(v, rng.standard_normal((4, 8)))
        e.set_member_groups(np.arange(8, dtype=np.int32), 64)
        assert refusal_code(e.moment_rows, 1, vectors=vecs, grouped=True) == 1
        assert refusal_code(e.moment_rows_sums, 1, 2, vectors=vecs, center=np.zeros((1000, 64, 5)), grouped=True) == 1
        got = e.moment_rows(1, vectors=vecs)
        assert got["count"].tolist() == [8] + [0] * 999
