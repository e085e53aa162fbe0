"""GPU tier of the kernels that reduce ACROSS the members of an ensemble, at the sizes where their launch shape changes: the plume
summary (summary_rows_partial_kernel / summary_rows_final_kernel, csrc/ensemble_ops.hip), the ungrouped exceedance
(csrc/indicators.hip), the likelihood-to-weights kernels (csrc/weights.hip), and the weight statistics and the scan behind
resampling (csrc/resample.hip).  The first four cap their grid at 1024 blocks of 256, so beyond 262 144 members every thread walks
a grid-stride loop; the scan gains a third level beyond 1024^2 members.

Every comparison is exact or within a bound derived in tests/host_reduce.py from the kernels' addition tree (proved on the CPU by
tests/test_host_reduce.py); none is read off the device.  count, min and max are compared with == by value, so the sign of a zero
is not asserted (the device's fmin / fmax may keep either of -0.0 and 0.0)."""
import math

import numpy as np
import pytest

from tests import host_indicators as hi
from tests import host_reduce as hd
from tests import host_resample as hr
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import f_syn, same_values, two_layer_params

pytestmark = pytest.mark.gpu

GRID = hd.ONE_GRID                    # 262 144 members: one pass of the capped grids
B4 = np.arange(1750.0, 1755.0)        # four time points
B3 = np.arange(1750.0, 1754.0)        # three: the axis of tests/test_gpu_resample.py
VAR = 1                               # Surface Temperature
DBL_MAX = np.finfo(np.float64).max
DENORM_MIN = 5e-324
SUMMARY_SIZES = [1, 63, 64, 65, 255, 256, 257, GRID - 1, GRID, GRID + 1, GRID + 257, 600_001]
NONFINITE_SIZES = [65, 257, GRID + 1, 600_001]


def _bits(x) -> int:
    return int(np.float64(x).view(np.uint64))


def _raw(e, tidx):
    """out[4] = {count, sum, min, max} of rscm_ens_summary: the raw sum, not the mean."""
    from rscm_amd import _lib as L
    out = np.empty(4)
    L.check(e._lib.rscm_ens_summary(e._h, VAR, int(tidx), L.dptr(out)))
    return out


def _raw_series(e, t_begin, t_end):
    from rscm_amd import _lib as L
    out = np.empty((t_end - t_begin, 4))
    L.check(e._lib.rscm_ens_summary_series(e._h, VAR, t_begin, t_end, L.dptr(out)))
    return out


def _check_exact(got, x, what):
    """count, min, max by value and the sum bit for bit against the reference of an exactly summable row."""
    cnt, s, mn, mx = hd.summary(x)
    assert (got[0], got[2], got[3]) == (cnt, mn, mx), (what, got, (cnt, s, mn, mx))
    assert _bits(got[1]) == _bits(s) or (got[1] == 0.0 and s == 0.0), (what, got[1], s)


def _check_bound(got, x, what):
    cnt, s, mn, mx = hd.summary(x)
    bound = hd.sum_bound(x)
    print(what, "sum error", abs(got[1] - s), "bound", bound)
    assert (got[0], got[2], got[3]) == (cnt, mn, mx), (what, got, (cnt, s, mn, mx))
    assert abs(got[1] - s) <= bound, (what, got[1], s, bound)


# ---- 2. plume summary -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SUMMARY_SIZES)
def test_summary_of_exact_and_ill_conditioned_rows(ra, n):
    """One wave, one block, the grid cap and its neighbours, a second stride that ends inside a block (262 144 + 257) and a
    third, partial stride (600 001): on an exactly summable row the sum is math.fsum's bits whatever the tree; on an
    ill-conditioned row (sum x ~ 1, sum |x| ~ 1e302, the last member's partner the first) it is within host_reduce.sum_bound.
    count, min and max exactly, by value (the sign of a zero is not asserted)."""
    rng = np.random.default_rng(n)
    rows = [hd.exact_row(rng, n), hd.ill_conditioned_row(rng, n), hd.exact_row(rng, n)]
    rows[2][rng.random(n) < 0.5] = 0.0          # zeros among the members: they are finite and counted
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, B4) as e:
        for t, x in enumerate(rows):
            e.set_state(VAR, t, x)
        e.set_time_index(2)
        _check_exact(_raw(e, 0), rows[0], (n, "exact"))
        _check_bound(_raw(e, 1), rows[1], (n, "ill-conditioned"))
        _check_exact(_raw(e, 2), rows[2], (n, "exact with zeros"))
        s = e.summary(VAR, 0)                   # the Python front end: one more division
        cnt, want, mn, mx = hd.summary(rows[0])
        assert (s["count"], s["min"], s["max"]) == (cnt, mn, mx) and s["mean"] == want / cnt


def _placements(n):
    """(name, mask of the members made non-finite) for a row of n members."""
    idx = np.arange(n)
    out = [("last partial wave", idx >= (n - 1) // 64 * 64)]
    if n > 256:
        out.append(("block 1", (idx >= 256) & (idx < 512)))
    if n > GRID:
        out.append(("second stride", (idx >= GRID) & (idx < 2 * GRID)))
    return out


@pytest.mark.parametrize("n", NONFINITE_SIZES)
def test_summary_skips_non_finite_members_wherever_they_sit(ra, n):
    """NaN, +inf and -inf (each alone, and cycling) in the last partial wave, a whole block (members 256 .. 511) whose partial is
    the identity {0, 0, +inf, -inf}, every member of the second stride, and every member: the finite ones are counted and summed
    bit for bit, and a row without one is count 0, min +inf, max -inf, mean NaN, as an uncomputed row."""
    rng = np.random.default_rng(7 * n)
    base = hd.exact_row(rng, n)
    cycle = np.resize([np.nan, np.inf, -np.inf], n)
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, B4) as e:
        e.set_time_index(0)
        for name, mask in _placements(n):
            for fill in (np.nan, np.inf, -np.inf, None):
                x = base.copy()
                x[mask] = cycle[mask] if fill is None else fill
                e.set_state(VAR, 0, x)
                _check_exact(_raw(e, 0), x, (n, name, fill))
        e.set_state(VAR, 0, cycle)
        empty = _raw(e, 0)
        assert (empty[0], empty[1], empty[2], empty[3]) == (0.0, 0.0, math.inf, -math.inf)
        assert np.array_equal(empty, _raw(e, 1))                           # row 1 is beyond the time index: uncomputed
        s, u = e.summary(VAR, 0), e.summary(VAR, 1)
        assert (s["count"], s["min"], s["max"]) == (0, math.inf, -math.inf) == (u["count"], u["min"], u["max"])
        assert math.isnan(s["mean"]) and math.isnan(u["mean"])
        x = cycle.copy()
        x[n - 1] = base[n - 1]                                             # one finite member, the very last
        e.set_state(VAR, 0, x)
        _check_exact(_raw(e, 0), x, (n, "only the last member finite"))


@pytest.mark.parametrize("n", [257, 600_001])
def test_summary_at_the_ends_of_the_number_line(ra, n):
    """The smallest denormal is the unique minimum and DBL_MAX the unique maximum, both counted as finite; two DBL_MAX members
    among zeros, a stride apart where the row has strides, overflow the sum to +inf with every member counted."""
    rng = np.random.default_rng(n)
    x = rng.uniform(1.0, 2.0, n)
    x[n - 1] = DENORM_MIN
    x[n - 2 if n < GRID else GRID + 100] = DBL_MAX
    two = np.zeros(n)
    two[[3, n - 1]] = DBL_MAX
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, B4) as e:
        e.set_state(VAR, 0, x)
        e.set_state(VAR, 1, two)
        e.set_time_index(1)
        got = _raw(e, 0)
        assert (got[0], got[2], got[3]) == (n, DENORM_MIN, DBL_MAX) and got[2] > 0.0
        # DBL_MAX dwarfs the rest: the sum is DBL_MAX to within the tree's bound, and finite
        assert math.isfinite(got[1]) and abs(got[1] - math.fsum(x)) <= hd.sum_bound(x)
        got = _raw(e, 1)
        assert (got[0], got[1], got[2], got[3]) == (n, math.inf, 0.0, DBL_MAX)


def test_summary_series_rows_have_the_single_row_bits_beyond_one_grid(ra):
    """262 145 members, three rows of different content and a fourth beyond the time index: every row of summary_series has the
    bits of the single-row summary, equals the reference, and the uncomputed row is empty."""
    n = GRID + 1
    rng = np.random.default_rng(41)
    rows = [hd.exact_row(rng, n), hd.exact_row(rng, n), hd.ill_conditioned_row(rng, n)]
    rows[1][GRID:] = np.nan                                                # the second stride's only member
    rows[1][256:512] = np.inf
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, B4) as e:
        for t, x in enumerate(rows):
            e.set_state(VAR, t, x)
        e.set_time_index(2)
        got = _raw_series(e, 0, 4)
        for t in range(3):
            assert np.array_equal(got[t].view(np.uint64), _raw(e, t).view(np.uint64)), t
        _check_exact(got[0], rows[0], "series row 0")
        _check_exact(got[1], rows[1], "series row 1")
        _check_bound(got[2], rows[2], "series row 2")
        assert got[3].tolist() == [0.0, 0.0, math.inf, -math.inf]
        part = _raw_series(e, 1, 3)                                         # a range that starts inside: the same rows
        assert np.array_equal(part.view(np.uint64), got[1:3].view(np.uint64))
        s = e.summary_series(VAR)
        assert s["count"].tolist() == [n, GRID - 256, n, 0] and math.isnan(s["mean"][3])
        assert s["mean"][0] == got[0, 1] / n and s["min"][1] == got[1, 2] and s["max"][2] == got[2, 3]


# ---- 6. more rows than one grid's y range ---------------------------------------------------------------------------------

def test_summary_series_over_more_rows_than_one_grid_indexes(ra):
    """An axis of 65 537 + 5 points with 3 members: launch_summary_rows goes over the rows in slices of kMaxGridY = 65 535, as the
    select does.  Rows on both sides of the slice edge and the last row hold distinct, exactly summable values (one with a NaN
    member); every row, written or not, must equal the host's count / sum / min / max of what the series holds."""
    T, n = 65_537 + 5, 3
    rng = np.random.default_rng(6)
    written = {0: hd.exact_row(rng, n), 65_534: hd.exact_row(rng, n), 65_535: hd.exact_row(rng, n), 65_536: hd.exact_row(rng, n),
               T - 1: hd.exact_row(rng, n)}
    written[65_535][0] = np.nan
    written[65_536][:] = [np.inf, 0.25, -np.inf]
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, np.arange(T + 1, dtype=np.float64)) as e:
        assert e.n_times == T
        for t, x in written.items():
            e.set_state(VAR, t, x)
        e.set_time_index(T - 1)
        content = e.get_series(VAR)
        got = _raw_series(e, 0, T)
    assert content.shape == (T, n)
    for t, x in written.items():
        assert same_values(content[t], x)
        _check_exact(got[t], x, ("row", t))
    # every row, from what the series holds: the finite values are multiples of 2^-20 below 2^20, so numpy's sum of three is exact
    fin = np.isfinite(content)
    v = np.where(fin, content, 0.0)
    assert np.array_equal(v * 2.0 ** 20, np.rint(v * 2.0 ** 20)) and np.abs(v).max() < 2.0 ** 20
    assert np.array_equal(got[:, 0], fin.sum(axis=1))
    assert np.array_equal(got[:, 1], v.sum(axis=1))
    assert np.array_equal(got[:, 2], np.where(fin, content, np.inf).min(axis=1))
    assert np.array_equal(got[:, 3], np.where(fin, content, -np.inf).max(axis=1))
    assert len({tuple(got[t]) for t in written}) == len(written)           # distinct rows gave distinct summaries


# ---- 3. ungrouped exceedance ------------------------------------------------------------------------------------------------

def _vector(e, values):
    """values as a [N] DeviceVector of e: parameter row 4 of its block."""
    P = two_layer_params(len(values))
    P[4] = values
    e.set_params(P)
    return e.params_vector(4)


@pytest.mark.parametrize("n", [GRID - 1, GRID + 1, 300_001])
def test_ungrouped_exceedance_on_both_sides_of_the_grid_cap(ra, n):
    """Eight thresholds with -inf and +inf among them, ties with a threshold, NaN members only in the second stride, weights up to
    2^33, and (300 001) a total weight of exactly 2^53 carried by two members of the second stride: hits and total are numpy's
    integer sums, the probability is hits / total."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    thr = np.array([-np.inf, -1.5, -0.25, 0.0, 0.25, 1.0, 2.5, np.inf])
    x[rng.integers(0, n, 500)] = 0.25                                      # ties: >= counts them
    x[n - 1] = 2.5
    x[[1, n // 2]] = [np.inf, -np.inf]
    cases = [("finite", x)]
    if n > GRID:
        y = x.copy()
        y[GRID:] = np.where(rng.random(n - GRID) < 0.5, np.nan, y[GRID:])
        y[n - 1] = np.nan
        cases.append(("NaN only in the second stride", y))
    w = rng.integers(0, 1 << 33, n, dtype=np.int64)
    weights = [("random", w)]
    if n == 300_001:
        big = rng.integers(0, 1 << 20, n, dtype=np.int64)
        big[[GRID, n - 2]] = [1 << 52, 0]
        big[n - 2] = (1 << 53) - int(big.sum())                            # the rest of 2^53
        assert int(big.sum()) == 1 << 53 and big[n - 2] > 1 << 51
        weights.append(("W = 2^53", big))
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, B3) as e:
        for name, v in cases:
            dv = _vector(e, v)
            assert same_values(dv.to_host(), v)
            got = e.exceedance(dv, thr)
            hits, total = hi.exceedance_counts(v, thr)
            assert got["hits"].tolist() == hits and got["total"] == total == int((~np.isnan(v)).sum()), name
            assert got["hits"][0] == total and got["hits"][-1] == int((v == np.inf).sum())
            assert np.array_equal(got["probability"], np.array(hits, dtype=np.float64) / float(total))
            for wname, ww in weights:
                e.set_member_weights(ww)
                got = e.exceedance(dv, thr, weighted=True)
                hits, total = hi.exceedance_counts(v, thr, ww)
                assert got["hits"].tolist() == hits and got["total"] == total, (name, wname)
                assert np.array_equal(got["probability"], np.array(hits, dtype=np.float64) / float(total))
                if wname == "W = 2^53" and name == "finite":
                    assert total == 1 << 53 == hits[0]


# ---- 4. likelihood to weights -------------------------------------------------------------------------------------------------

N_LL = 300_001
FAILED = [5, GRID - 1, GRID + 6, N_LL - 2]      # failed members on both sides of the stride edge (besides the random ones)


@pytest.fixture(scope="module")
def stepped(ra):
    """300 001 two-layer members after one step; those with a NaN parameter have status != 0."""
    rng = np.random.default_rng(77)
    P = two_layer_params(N_LL)
    bad = rng.random(N_LL) < 0.01
    bad[FAILED] = True
    bad[[0, GRID, GRID + 3, GRID + 7, N_LL - 1]] = False    # the members the tests below put a maximum on
    P[0, bad] = np.nan
    e = ra.Ensemble(ra.KIND_TWO_LAYER, N_LL, B4)
    e.set_params(P)
    e.set_forcing(f_syn(B4[:-1]))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run(1)
    status = e.status()
    assert ((status != 0) == bad).all()
    yield e, status
    e.close()


def test_loglik_max_wherever_the_maximum_sits(ra, stepped):
    """The maximum at member 0, at the first member of the second stride, at the last member, next to a larger value on a failed
    member, and next to +inf and NaN entries; -inf when every member is failed or non-finite."""
    e, status = stepped
    rng = np.random.default_rng(1)
    base = -1.0 - 20.0 * np.abs(rng.standard_normal(N_LL))
    for pos in (0, GRID, N_LL - 1):
        ll = base.copy()
        ll[pos] = 3.5
        assert e.loglik_max(ll) == 3.5 == hd.loglik_max(ll, status), pos
    ll = base.copy()
    ll[GRID + 6] = 100.0                          # a failed member's value never counts
    ll[GRID + 7] = -0.75
    assert status[GRID + 6] != 0 and status[GRID + 7] == 0
    assert e.loglik_max(ll) == -0.75 == hd.loglik_max(ll, status)
    ll = base.copy()
    ll[[GRID - 2, N_LL - 3]] = np.inf
    ll[[GRID + 2, N_LL - 4]] = np.nan
    ll[[3, GRID + 1]] = -np.inf
    ll[GRID + 3] = -0.5
    assert status[GRID + 3] == 0
    assert e.loglik_max(ll) == -0.5 == hd.loglik_max(ll, status)
    ll = np.where(status != 0, 1.0, np.resize([np.nan, np.inf, -np.inf], N_LL))
    assert e.loglik_max(ll) == -math.inf == hd.loglik_max(ll, status)


def test_weights_from_loglik_in_both_strides(ra, stepped):
    """0 exactly on failed and non-finite members of either stride; elsewhere within one unit of rint(exp(ll - max) * 2^bits), the
    bound test_weights_from_loglik (tests/test_gpu_weighted_quantiles.py) states."""
    e, status = stepped
    rng = np.random.default_rng(2)
    ll = -20.0 * np.abs(rng.standard_normal(N_LL))
    ll[rng.random(N_LL) < 0.01] = -np.inf
    ll[[7, GRID + 9]] = np.nan
    ll[[8, GRID + 10, N_LL - 1]] = np.inf
    ll[FAILED] = 50.0
    ll[GRID + 7] = 1.25                           # the maximum, in the second stride
    ok = hd.loglik_ok(ll, status)
    assert (~ok[:GRID]).sum() > 100 and (~ok[GRID:]).sum() > 100 and ok[GRID + 7]
    got_max, bits = e.set_weights_from_loglik(ll)
    assert got_max == 1.25 == hd.loglik_max(ll, status) and bits == 53 - 19
    w = e.member_weights()
    ref = hd.weights_from_loglik(ll, status, got_max, bits)
    assert (w[~ok] == 0).all() and w[GRID + 7] == 1 << bits == w.max()
    assert np.abs(w[ok] - ref[ok]).max() <= 1
    assert e.weights_stats() == hr.stats(w)


def test_member_weights_are_checked_in_both_strides(ra, stepped):
    """Totals of 2^53 and 2^53 + 1 that differ in one member of the second stride: the first is accepted, the second refused; a
    single -1 at the last member is refused; after each refusal the accepted weights are still in force."""
    from rscm_amd._lib import ERR_INVALID
    e, _status = stepped
    w = np.zeros(N_LL, dtype=np.int64)
    w[0], w[100], w[GRID + 11] = 1 << 52, 5, (1 << 52) - 5
    assert int(w.sum()) == 1 << 53
    e.set_member_weights(w)
    want = hr.stats(w)
    assert e.weights_stats() == want and want["total"] == 1 << 53
    over = w.copy()
    over[GRID + 11] += 1
    neg = w.copy()
    neg[N_LL - 1] = -1
    tail = np.zeros(N_LL, dtype=np.int64)         # the first stride alone is far below the bound
    tail[GRID:] = (1 << 53) // (N_LL - GRID) + 1
    assert int(tail.sum()) > 1 << 53 and int(tail[:GRID].sum()) == 0
    for bad in (over, neg, tail):
        assert refusal_code(e.set_member_weights, bad) == ERR_INVALID
        assert e.weights_stats() == want
    assert np.array_equal(e.member_weights(), w)


# ---- 5. weight statistics, scan and ancestors -------------------------------------------------------------------------------

# 1024 weights per tile.  1 048 577 is the smallest size with three levels (1025 tile totals are scanned in two tiles, whose two
# totals are scanned again).  There the third level runs, but what it adds back changes only the LAST scanned tile total, which no
# tile of the weights reads (tile b takes the entry b - 1): the deepest add reaches a weight from 1024 * 1025 + 1 = 1 049 601
# members on, where tile 1025 takes entry 1024.
SCAN_SIZES = [1023, 1024, 1025, 2048, 2049, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1024 * 1025 + 1, (1 << 20) + 1 + 1025]


def _check_draws(e, w, seed):
    n, W = len(w), int(w.sum())
    assert e.weights_stats() == hr.stats(w)
    for M in (1, 1000, n):
        for s in (0, W - 1, hr.offset(seed + M, W)):
            v = e.resample(M, offset=s)
            k_first, count, want = hr.ancestors_fast(w, M, s)
            assert (v.k_first, len(v)) == (0, M) == (k_first, count)
            got = v.to_host()
            assert np.array_equal(got, want), (n, M, s, int((got != want).sum()))
            assert np.all(w[got] > 0)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_at_tile_edges_and_with_a_third_level(ra, n):
    """Weights below 2^32 with 30 % zeros at sizes on and beside the scan's tile of 1024 and its square, above which the scan
    recurses a third time: the statistics are Python's integer sums and every draw's ancestor is the restatement's."""
    rng = np.random.default_rng(n)
    w = rng.integers(0, 1 << 32, n, dtype=np.int64)
    w[rng.random(n) < 0.3] = 0
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, B3) as e:
        e.set_member_weights(w)
        _check_draws(e, w, n)


@pytest.mark.parametrize("n", SCAN_SIZES[-4:])
def test_scan_of_three_weights_a_million_zeros_apart(ra, n):
    """All weight on members 0, 1 048 575 and n - 1: the running sum of the last tile is nothing but what the levels above add to
    it, so (at the two largest sizes, see SCAN_SIZES) its only positive weight is found only if the deepest add ran."""
    w = np.zeros(n, dtype=np.int64)
    w[0], w[(1 << 20) - 1], w[n - 1] = (1 << 40) + 1, 3, (1 << 41) + 5
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, B3) as e:
        e.set_member_weights(w)
        _check_draws(e, w, n)
        last = e.resample(7, offset=int(w.sum()) - 1).to_host()
        assert last[-1] == n - 1 and set(last.tolist()) <= {0, (1 << 20) - 1, n - 1}
