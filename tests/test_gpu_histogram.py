"""GPU tier of the histograms across members (csrc/histogram.hip, ABI minor 28) against the numpy and Python integers of
tests/host_histogram.py.  Every comparison is of integers, or of doubles that are one exact quotient of those integers rounded once,
so equality is the only tolerance.

The rows are those of a small two-layer ensemble, overwritten with set_state so that they take any bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import host_histogram as hh
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import f_syn, magicc_chain, two_layer_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_AXIS = np.arange(1750.0, 1758.0)          # 8 rows
EDGE_COUNTS = (2, 3, 9, 65, 1025)


def _members_per_pass() -> int:
    """Members one pass of the kernel's capped grid takes, read from the code: kHistBlocks blocks of four waves of 64."""
    text = open(os.path.join(ROOT, "rscm_amd", "csrc", "rscm_device.hpp")).read()
    blocks = int(re.search(r"constexpr int kHistBlocks = (\d+);", text).group(1))
    per_pass = int(re.search(r"constexpr int64_t kHistogramMembersPerPass = (\d+);", text).group(1))
    hip = open(os.path.join(ROOT, "rscm_amd", "csrc", "histogram.hip")).read()
    threads = int(re.search(r"constexpr int kHistThreads = (\d+);", hip).group(1))
    assert per_pass == blocks * threads
    return per_pass


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


def _tied(rng, rows, n):
    """Rows of standard normals rounded to one decimal: a few dozen distinct values, so full of ties."""
    return np.round(rng.standard_normal((rows, n)), 1)


def _weights(rng, n):
    """Weights of 0, values below 2^20 and one of 2^40: a sum truncated to 32 bits anywhere fails."""
    w = rng.integers(0, 1 << 20, n)
    w[rng.random(n) < 0.1] = 0
    w[n // 2] = 1 << 40
    return w


def _edges(E, lo=-2.0, hi=2.0):
    """E ascending edges from lo to hi on a grid of 2^-9 (E = 1025 over four units: exactly that grid), so that the data's tenths sit
    on some of them only after rounding; an edge at 0.0 for odd E."""
    return np.round(np.linspace(lo, hi, E) * 512.0) / 512.0


def _poke_group(e, member, value):
    """Overwrite one member's group id in the handle's device buffer: an id the setter would refuse, which the kernel must leave out."""
    from rscm_amd import _lib as L
    v = np.array([value], dtype=np.int32)
    L.check(L.load().rscm_gpu_copy_to_device(e.device, C.c_void_p(e.member_groups_device().ptr + 4 * member), v.ctypes.data_as(C.c_void_p), 4))


def _check(e, X, edges, w=None, groups=None, G=None, baseline=None, rows=None, what="", var=1):
    """histogram_rows over the rows `rows` = (t_begin, t_end, t_stride) of X (default: all of X) against the restatement."""
    X = np.asarray(X, dtype=np.float64)
    tb, te, ts = rows if rows is not None else (0, X.shape[0], 1)
    want = hh.histogram_rows(X[tb:te:ts], edges, w, groups, G, baseline)
    got = e.histogram_rows(var, edges, tb, te, ts, weighted=w is not None, grouped=groups is not None, anomaly=baseline is not None)
    assert hh.same(got, want), (what, got, want)
    assert (got["below"] + got["counts"].sum(axis=-1) + got["above"] == got["total"]).all()
    return got


# ---- sizes and shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_rows_and_edge_counts(ra, n):
    """One member, the edges of a wave and of a block, several blocks; 1, 2 and 5 rows and a stride of 2 whose end is off the
    stride; E = 2, 3, 9, 65, 1025 -- plain, weighted, grouped (contiguous and i % 3, with a member of group -1 and one whose id is
    past the last group) and as an anomaly with a NaN in the baseline."""
    rng = np.random.default_rng(n)
    X = _tied(rng, 8, n)
    w = _weights(rng, n)
    b = np.round(0.3 * rng.standard_normal(n), 1)
    b[n // 3] = np.nan
    layouts = {"contiguous": (np.arange(n) * 3 // n).astype(np.int32), "interleaved": (np.arange(n) % 3).astype(np.int32)}
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        e.set_baseline_values(b)
        for layout, groups in layouts.items():
            groups = groups.copy()
            groups[0] = -1
            e.set_member_groups(groups, 3)
            groups[n - 1] = 7                     # outside [0, 3): left out like -1
            _poke_group(e, n - 1, 7)
            for rows in ((0, 1, 1), (0, 2, 1), (0, 5, 1), (1, 8, 2)):
                for E in EDGE_COUNTS:
                    edges = _edges(E)
                    _check(e, X, edges, groups=groups, G=3, rows=rows, what=(n, rows, E, layout))
                    _check(e, X, edges, w, groups, 3, rows=rows, what=(n, rows, E, layout, "weighted"))
                    if layout == "contiguous":
                        _check(e, X, edges, rows=rows, what=(n, rows, E, "plain"))
                        _check(e, X, edges, w, rows=rows, what=(n, rows, E, "weighted"))
                        _check(e, X, edges, baseline=b, rows=rows, what=(n, rows, E, "anomaly"))
        got = _check(e, X, _edges(9, -9.0, 9.0))
        assert (got["total"] == n).all() and not got["below"].any() and not got["above"].any()
        assert (_check(e, X, _edges(9, -9.0, 9.0), baseline=b)["total"] == n - 1).all()


def test_past_the_grid_cap(ra):
    """One tile and three members past what one pass of the capped grid takes, two rows: the grid-stride second pass and its ragged
    tile, with a NaN and the heaviest member in that tail, weighted, in two contiguous groups that meet inside the tail; every E."""
    n = _members_per_pass() + 64 + 3
    rng = np.random.default_rng(11)
    X = _tied(rng, 2, n)
    X[0, n - 2] = np.nan
    w = rng.integers(0, 1 << 20, n)
    w[n - 1] = 1 << 40
    X[:, n - 1] = [0.25, -5.0]                # the heaviest member: inside a bin in row 0, below every edge in row 1
    groups = (np.arange(n) >= n - 30).astype(np.int32)
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        e.set_member_groups(groups, 2)
        for E in EDGE_COUNTS:
            edges = _edges(E)
            got = _check(e, X, edges, w, groups, 2, what=("past the cap", E))
            assert got["total"][0, 1] > 1 << 40 and got["below"][1, 1] >= 1 << 40 and got["below"][0, 1] < 1 << 40
            plain = _check(e, X, edges, groups=groups, G=2, what=("past the cap, counts", E))
            assert plain["total"].tolist() == [[n - 30, 29], [n - 30, 30]]
            _check(e, X, edges, w, what=("past the cap, one group", E))
            _check(e, X, edges, what=("past the cap, plain", E))


# ---- contention, both ends --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", EDGE_COUNTS)
def test_every_member_in_one_bin(ra, E):
    """Every member of every wave adds to one slot -- a bin in the middle, the last bin through its closed edge, below and above --
    with a weight of 2^40 among them, so a 32-bit add anywhere fails; three interleaved groups do the same to three slots."""
    n = 2000
    rng = np.random.default_rng(E)
    edges = _edges(E)
    B = E - 1
    mid = B // 2
    X = np.stack([np.full(n, 0.5 * (edges[mid] + edges[mid + 1])), np.full(n, edges[-1]), np.full(n, -7.0), np.full(n, np.inf)])
    w = rng.integers(1, 1 << 20, n)
    w[777] = 1 << 40
    groups = (np.arange(n) % 3).astype(np.int32)
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        e.set_member_groups(groups, 3)
        plain = _check(e, X, edges, what=("one bin", E))
        assert plain["counts"][0, mid] == n and plain["counts"][1, B - 1] == n and plain["below"][2] == n and plain["above"][3] == n
        got = _check(e, X, edges, w, what=("one bin, weighted", E))
        W = int(w.sum())
        assert W > 1 << 40 and got["counts"][0, mid] == W and got["counts"][1, B - 1] == W and got["below"][2] == W and got["above"][3] == W
        _check(e, X, edges, w, groups, 3, what=("one bin, grouped", E))
        _check(e, X, edges, groups=groups, G=3, what=("one bin, grouped counts", E))


def test_every_member_in_its_own_bin(ra):
    """E = 1025 and 1024 members, member i in bin i (and shuffled, so that no wave sees neighbouring bins); then 1500 members over
    the same bins: 64 different slots in a wave, some of them twice."""
    edges = _edges(1025)
    centres = 0.5 * (edges[:-1] + edges[1:])
    rng = np.random.default_rng(21)
    X = np.stack([centres, rng.permutation(centres)])
    w = _weights(rng, 1024)
    with _rows_ens(ra, 1024, X) as e:
        e.set_member_weights(w)
        got = _check(e, X, edges, what="own bin")
        assert (got["counts"] == 1).all()
        got = _check(e, X, edges, w, what="own bin, weighted")
        assert (got["counts"][0] == w).all()
    X = np.stack([rng.choice(centres, 1500), np.sort(rng.choice(centres, 1500))])
    with _rows_ens(ra, 1500, X) as e:
        _check(e, X, edges, what="own bins, 1500 members")


# ---- values -----------------------------------------------------------------------------------------------------------------------

def test_special_values(ra):
    """A value on every edge (the last one closed), the neighbouring doubles of every edge, -0.0 and +0.0 on an edge at 0.0, both
    infinities, a NaN, a whole wave of NaN and a row of NaN."""
    edges = np.array([-1.5, -0.25, 0.0, 0.1 + 0.2, 1.0, 2.5])
    E = edges.size
    n = 300
    rng = np.random.default_rng(2)
    X = _tied(rng, 5, n)
    X[0, :E], X[0, E:2 * E], X[0, 2 * E:3 * E] = edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)
    X[1, :40], X[1, 40:60] = -0.0, 0.0
    X[1, 60], X[1, 61], X[1, 62], X[1, 63] = np.inf, -np.inf, np.nan, 0.3        # 0.3 is below the edge 0.30000000000000004
    X[2, 64:128] = np.nan
    X[3, :] = np.nan
    X[4, :] = edges[-1]
    with _rows_ens(ra, n, X) as e:
        got = _check(e, X, edges, what="special")
        assert got["total"].tolist() == [n, n - 1, n - 64, 0, n]
        assert got["counts"][1, 2] >= 60 and got["counts"][4, E - 2] == n and got["above"][4] == 0
        assert np.isnan(got["probability"][3]).all() and got["probability"][4, E - 2] == 1.0
        only = hh.histogram_rows(X[0:1, :3 * E], edges)
        assert only["below"][0] == 1 and only["above"][0] == 1 and only["counts"][0].tolist() == [3, 3, 3, 3, 4]
        for E2 in (2, 3):
            _check(e, X, edges[1:1 + E2], what=("special", E2))


def test_agrees_with_exceedance_rows(ra):
    """For every edge k < E - 1 the weight at or above it, sum(counts[k:]) + above, is exceedance_rows' hits at that threshold, and
    total is its total: plain, weighted, and as an anomaly."""
    n = 777
    rng = np.random.default_rng(7)
    X = _tied(rng, 3, n)
    X[1, 5] = np.nan
    w = _weights(rng, n)
    b = np.round(0.2 * rng.standard_normal(n), 1)
    edges = _edges(17, -1.6, 1.6)
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        e.set_baseline_values(b)
        for kw in ({}, {"weighted": True}, {"anomaly": True}, {"weighted": True, "anomaly": True}):
            h = e.histogram_rows(1, edges, 0, 3, **kw)
            at_or_above = np.cumsum(h["counts"][:, ::-1], axis=1)[:, ::-1] + h["above"][:, None]
            for k0 in (0, 8):
                x = e.exceedance_rows(1, edges[k0:k0 + 8], 0, 3, **kw)
                assert (x["hits"] == at_or_above[:, k0:k0 + 8]).all() and (x["total"] == h["total"]).all(), (kw, k0)


# ---- the slot cap -----------------------------------------------------------------------------------------------------------------

def test_slot_cap(ra):
    """Exactly 8192 slots are accepted -- 64 groups x (126 + 2), and a joint histogram of 64 x 128 - 1 cells + 1 -- and one more is
    RSCM_ERR_INVALID with the product in the message."""
    from rscm_amd._lib import RscmGpuError
    n = 640
    rng = np.random.default_rng(5)
    X = _tied(rng, 2, n)
    groups = (np.arange(n) % 64).astype(np.int32)
    with _rows_ens(ra, n, X) as e:
        e.set_member_groups(groups, 64)
        _check(e, X, _edges(127), groups=groups, G=64, rows=(0, 2, 1), what="8192 slots")
        with pytest.raises(RscmGpuError, match=r"64 groups x 129 slots \(bins \+ 2\) = 8256 slots") as err:
            e.histogram_rows(1, _edges(128), grouped=True)
        assert err.value.code == 1
        e.set_member_groups(groups % 8, 8)
        _check(e, X, _edges(1023), groups=groups % 8, G=8, rows=(0, 1, 1), what="8 x 1024 slots")
        assert refusal_code(e.histogram_rows, 1, _edges(1024), grouped=True) == 1
        _check(e, X, _edges(1025), what="1025 edges, one group")
        x, y = (ra.ensemble.DeviceVector(e.series_devptr(1) + 8 * n * t, n, np.float64, e) for t in (0, 1))
        ex, ey = _edges(128), _edges(65)                     # 127 x 64 + 1 = 8129
        assert hh.same(e.histogram2d(x, y, ex, ey), hh.histogram2d(X[0], X[1], ex, ey))
        nine = [-1.0, 0.0, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0]
        assert hh.same(e.histogram2d(x, y, _edges(1024), nine), hh.histogram2d(X[0], X[1], _edges(1024), nine))    # 1023 x 8 + 1 = 8185
        with pytest.raises(RscmGpuError, match=r"\(bins of x x bins of y \+ 1\) = 8193 slots") as err:
            e.histogram2d(x, y, _edges(1025), nine)                                                               # 1024 x 8 + 1
        assert err.value.code == 1
        e.set_member_groups(groups % 2, 2)
        ex, ey = _edges(65), _edges(64)                      # 2 x (64 x 63 + 1) = 8066
        assert hh.same(e.histogram2d(x, y, ex, ey, grouped=True), hh.histogram2d(X[0], X[1], ex, ey, None, groups % 2, 2))
        assert refusal_code(e.histogram2d, x, y, _edges(65), _edges(65), grouped=True) == 1                     # 2 x 4097


# ---- vectors ----------------------------------------------------------------------------------------------------------------------

def test_histogram_vectors(ra):
    """Parameter rows and an indicator vector as the rows, with shared and with per-vector edges; NaN is left out per vector."""
    n = 1111
    rng = np.random.default_rng(9)
    X = _tied(rng, 8, n)
    X[3, 100] = np.nan                                       # member 100: NaN in its indicators, not in its parameters
    w = _weights(rng, n)
    groups = (np.arange(n) % 3).astype(np.int32)
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        e.set_member_groups(groups, 3)
        P = e.get_params()
        ind = e.indicators(1, 0, 8)
        vecs = [e.params_vector(0), e.params_vector(3), ind["peak"], ind["mean"]]
        host = np.stack([P[0], P[3], ind["peak"].to_host(), ind["mean"].to_host()])
        assert np.isnan(host[2, 100]) and not np.isnan(host[:2]).any()
        own = np.stack([np.linspace(host[k][~np.isnan(host[k])].min(), host[k][~np.isnan(host[k])].max(), 33) for k in range(4)])
        own[:, 0] -= 1e-9                                    # (the smallest value stays inside after the rounding of linspace)
        shared = _edges(65, -3.0, 3.0)
        for edges in (shared, own):
            for weights, grp in ((None, None), (w, None), (None, groups), (w, groups)):
                got = e.histogram_vectors(vecs, edges, weighted=weights is not None, grouped=grp is not None)
                want = hh.histogram_rows(host, edges, weights, grp, 3 if grp is not None else None)
                assert hh.same(got, want), (edges.shape, weights is not None, grp is not None)
        got = e.histogram_vectors(vecs, own)
        assert got["total"].tolist() == [n, n, n - 1, n - 1] and not got["above"].any() and not got["below"].any()
        one = e.histogram_vectors([vecs[2]], own[2])
        assert hh.same(one, {k: v[2:3] for k, v in got.items()})
        eight = e.histogram_vectors(vecs * 2, shared)
        assert hh.same(eight, hh.histogram_rows(np.concatenate([host, host]), shared))
        record = np.array([own[0, 7], own[1, 20] + 1e-3, np.nan, own[3, 32]])
        bracket = ra.ensemble.crps_bracket(got, own, record)         # per-vector edges: one table per row
        for r in range(4):
            one = hh.crps_bracket({k: v[r:r + 1] for k, v in got.items()}, own[r], record[r:r + 1])
            assert hh.same({k: v[r:r + 1] for k, v in bracket.items()}, one), r
        assert np.isnan(bracket["lower"][2]) and (bracket["lower"][[0, 1, 3]] <= bracket["upper"][[0, 1, 3]]).all()
        from rscm_amd import _lib
        arr, k = e._vectors(vecs)
        i64 = C.POINTER(C.c_int64)
        out = [np.zeros(4 * 64, dtype=np.int64) for _ in range(4)]
        po = [o.ctypes.data_as(i64) for o in out]
        f64 = C.POINTER(C.c_double)
        assert e._lib.rscm_ens_histogram_vectors(e._h, 4, arr, 65, shared.ctypes.data_as(f64), 0, _lib.SELECT_ANOMALY, *po) == _lib.ERR_INVALID
        assert e._lib.rscm_ens_histogram_vectors(e._h, 0, arr, 65, shared.ctypes.data_as(f64), 0, 0, *po) == _lib.ERR_INVALID
        assert e._lib.rscm_ens_histogram_vectors(e._h, 9, arr, 65, shared.ctypes.data_as(f64), 0, 0, *po) == _lib.ERR_INVALID
        bad = own.copy()
        bad[3, 5] = bad[3, 4]
        assert e._lib.rscm_ens_histogram_vectors(e._h, 4, arr, 33, bad.ctypes.data_as(f64), 1, 0, *po) == _lib.ERR_INVALID
        assert e._lib.rscm_ens_histogram_vectors(e._h, 4, arr, 33, bad.ctypes.data_as(f64), 0, 0, *po) == _lib.OK     # only table 0 is read


# ---- two dimensions ---------------------------------------------------------------------------------------------------------------

def test_histogram2d(ra):
    """1 x 1, 3 x 5 and 64 x 64 cells; NaN in either vector; values outside in either vector; weighted and grouped; the transpose
    of (y, x) equals (x, y)."""
    n = 2500
    rng = np.random.default_rng(13)
    X = _tied(rng, 2, n)
    X[0, 10], X[1, 20], X[0, 30], X[1, 30] = np.nan, np.nan, np.nan, np.nan
    X[0, 40], X[1, 41], X[0, 42], X[1, 43] = 50.0, -50.0, -np.inf, np.inf     # outside in x, in y, in x, in y
    w = _weights(rng, n)
    groups = (np.arange(n) % 3).astype(np.int32)
    groups[5] = -1
    with _rows_ens(ra, n, X) as e:
        e.set_member_weights(w)
        e.set_member_groups(groups, 3)
        x, y = (ra.ensemble.DeviceVector(e.series_devptr(1) + 8 * n * t, n, np.float64, e) for t in (0, 1))
        for ex, ey in (([-9.0, 9.0], [-9.0, 9.0]), (_edges(4), _edges(6, -1.0, 1.5)), (_edges(65), _edges(65, -2.5, 2.5))):
            for weights, grp in ((None, None), (w, None), (None, groups), (w, groups)):
                if grp is not None and (len(ex) - 1) * (len(ey) - 1) + 1 > 8192 // 3:
                    continue
                kw = dict(weighted=weights is not None, grouped=grp is not None)
                got = e.histogram2d(x, y, ex, ey, **kw)
                want = hh.histogram2d(X[0], X[1], ex, ey, weights, grp, 3 if grp is not None else None)
                assert hh.same(got, want), (len(ex), len(ey), kw)
                assert (got["counts"].sum(axis=(-2, -1)) + got["outside"] == got["total"]).all()
                swapped = e.histogram2d(y, x, ey, ex, **kw)
                assert (np.swapaxes(swapped["counts"], -1, -2) == got["counts"]).all() and (swapped["outside"] == got["outside"]).all()
        one = e.histogram2d(x, y, [-9.0, 9.0], [-9.0, 9.0])
        assert one["counts"].shape == (1, 1) and one["total"] == n - 3 and one["outside"] == 4 and one["counts"][0, 0] == n - 7
        ok = ~(np.isnan(X[0]) | np.isnan(X[1]))
        np_counts, _, _ = np.histogram2d(X[0][ok], X[1][ok], bins=(_edges(65), _edges(65, -2.5, 2.5)))
        assert (e.histogram2d(x, y, _edges(65), _edges(65, -2.5, 2.5))["counts"] == np_counts.astype(np.int64)).all()
        same_bin = np.full(n, 0.3)
        e.set_state(1, 2, same_bin)
        z = ra.ensemble.DeviceVector(e.series_devptr(1) + 8 * n * 2, n, np.float64, e)
        got = e.histogram2d(z, z, _edges(65), _edges(65), weighted=True)          # every member in one cell, a weight of 2^40 among them
        assert got["counts"].sum() == got["counts"].max() == int(w.sum()) > 1 << 40


# ---- rows, wherever they live -----------------------------------------------------------------------------------------------------

def test_diagnostics_by_name_and_the_stale_refusal(ra):
    """The heat content and a running mean of the surface temperature work once computed -- the restatement over their rows -- and
    the heat content is refused while it is stale."""
    from rscm_amd._lib import RscmGpuError
    n = 129
    with _rows_ens(ra, n) as e:
        vid = e.define_heat_content()
        assert refusal_code(e.histogram_rows, "Ocean Heat Content", [0.0, 1.0]) == 2
        e.compute_diagnostic(vid)
        S = e.get_series(vid)
        edges = np.linspace(S.min(), S.max() * 0.9, 12)
        got = e.histogram_rows("Ocean Heat Content", edges)
        assert hh.same(got, hh.histogram_rows(S, edges)) and (got["total"] == n).all() and got["above"][-1] > 0
        rid = e.define_running_mean("ts3", "Surface Temperature", 3, "trailing")
        e.compute_diagnostic(rid)
        held = e.diagnostics["ts3"]
        tb, te = held["t_begin"], held["t_begin"] + held["rows_held"]
        R = e.get_series(rid, tb, te)
        assert R.shape[0] >= 5
        edges = np.linspace(R.min(), R.max(), 9)
        got = e.histogram_rows("ts3", edges, tb, te)
        assert hh.same(got, hh.histogram_rows(R, edges)) and not got["below"].any() and not got["above"].any()
        assert hh.same(e.histogram_rows(rid, edges, tb, te, 2), hh.histogram_rows(R[::2], edges))
        e.set_state(1, 0, 0.25)
        assert refusal_code(e.histogram_rows, "Ocean Heat Content", edges) == 2
        with pytest.raises(RscmGpuError, match="is stale: compute it again"):
            e.histogram_rows(vid, edges)


def test_rows_past_the_time_index(ra):
    n = 100
    with _rows_ens(ra, n, steps=3) as e:
        S = e.get_series(1, 0, 4)
        edges = np.linspace(S.min(), S.max(), 6)
        got = e.histogram_rows(1, edges)
        assert got["total"].tolist() == [n] * 4 + [0] * 4 and not got["counts"][4:].any() and np.isnan(got["probability"][4:]).all()
        assert not got["below"][4:].any() and not got["above"][4:].any()
        assert hh.same({k: v[:4] for k, v in got.items()}, hh.histogram_rows(S, edges))
        past = e.histogram_rows(1, edges, 4, 8)
        assert not past["total"].any() and not past["counts"].any()
        assert e.histogram_rows(1, edges, 5, 5)["counts"].shape == (0, 5)


def test_windowed_graph_output_store(ra):
    """The MAGICC chain, monthly steps, a 16-row window and every 12th row kept: GraphModel.histogram_rows over the annual rows of
    the output store and over rows still in the window; a row that is in neither is RSCM_ERR_STATE."""
    from rscm_amd import RscmGpuError
    model = magicc_chain().build_chain(257, 6, "topological", steps_per_year=12, series_window=16, output_stride=12)
    try:
        model.run()
        name = "Surface Temperature"
        ser = model.get_series(name, t_stride=12)
        edges = np.linspace(np.nanmin(ser), np.nanmax(ser), 10)
        got = model.histogram_rows(name, edges, t_stride=12)
        assert hh.same(got, hh.histogram_rows(ser, edges)) and got["counts"][-1].sum() == got["total"][-1] == 257
        ti = model.time_index
        win = model.histogram_rows(name, edges, ti - 2, ti + 1)
        assert hh.same(win, hh.histogram_rows(model.get_series(name, t_begin=ti - 2, t_end=ti + 1), edges))
        with pytest.raises(RscmGpuError, match="not resident") as err:
            model.histogram_rows(name, edges, 13, 14)
        assert err.value.code == 2
    finally:
        model.close()


def test_two_handles_add_up(ra):
    """The integers of two handles over the two parts of a member set add up to those of one handle over the whole set."""
    n, h = 901, 333
    rng = np.random.default_rng(12)
    X = _tied(rng, 3, n)
    w = _weights(rng, n)
    groups = (np.arange(n) % 3).astype(np.int32)
    edges = _edges(33)
    with _rows_ens(ra, n, X) as e, _rows_ens(ra, h, X[:, :h]) as e1, _rows_ens(ra, n - h, X[:, h:]) as e2:
        for x, s in ((e, slice(None)), (e1, slice(0, h)), (e2, slice(h, None))):
            x.set_member_weights(w[s])
            x.set_member_groups(groups[s], 3)
        a, b, c = (x.histogram_rows(1, edges, 0, 3, weighted=True, grouped=True) for x in (e, e1, e2))
        keys = ("counts", "below", "above", "total")
        assert all((b[k] + c[k] == a[k]).all() for k in keys)
        assert hh.same(ra.ensemble.histogram_result(*(b[k] + c[k] for k in keys)), a) and hh.same(a, hh.histogram_rows(X, edges, w, groups, 3))
        vecs = [[ra.ensemble.DeviceVector(x.series_devptr(1) + 8 * x.n_members * t, x.n_members, np.float64, x) for t in (0, 2)] for x in (e, e1, e2)]
        a, b, c = (x.histogram2d(v[0], v[1], edges, edges[::4], weighted=True) for x, v in zip((e, e1, e2), vecs))
        keys = ("counts", "outside", "total")
        assert hh.same(ra.ensemble.histogram2d_result(*(b[k] + c[k] for k in keys), grouped=False), a)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals(ra):
    from rscm_amd import _lib
    n = 70
    with _rows_ens(ra, n) as e:
        lib, h = e._lib, e._h
        good = np.array([-1.0, 0.0, 0.5, 2.0])
        i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        counts, below, above, total = (np.zeros(8 * 1024, dtype=np.int64) for _ in range(4))
        pc, pb, pa, po = (a.ctypes.data_as(i64) for a in (counts, below, above, total))

        def call(var=1, tb=0, te=8, ts=1, edges=good, E=None, flags=0, c=pc, b=pb, a=pa, t=po):
            ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
            return lib.rscm_ens_histogram_rows(h, var, tb, te, ts, len(ed) if E is None else E, None if ed is None else ed.ctypes.data_as(f64),
                                               flags, c, b, a, t)

        assert call() == _lib.OK and (total[:8] == n).all()
        assert call(tb=5, te=5) == _lib.OK and call(edges=np.arange(1025.0)) == _lib.OK and call(edges=[0.0, 1.0]) == _lib.OK
        for bad in ([2.0, 1.0], [0.0, 1.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf], [-np.inf, 0.0], [np.nan, 1.0]):
            assert call(edges=bad) == _lib.ERR_INVALID, bad
        assert call(edges=[0.0, 1.0], E=1) == _lib.ERR_INVALID and call(edges=np.arange(1026.0)) == _lib.ERR_INVALID
        assert call(edges=[0.0, 1.0], E=0) == _lib.ERR_INVALID and call(edges=None, E=4) == _lib.ERR_INVALID
        for kw in (dict(tb=-1), dict(te=10), dict(tb=5, te=4), dict(ts=0), dict(ts=-1), dict(flags=8), dict(flags=_lib.SELECT_WEIGHTED | 16),
                   dict(c=None), dict(b=None), dict(a=None), dict(t=None), dict(var=99)):
            assert call(**kw) == _lib.ERR_INVALID, kw
        for flags in (_lib.SELECT_WEIGHTED, _lib.SELECT_GROUPED, _lib.SELECT_ANOMALY):
            assert call(flags=flags) == _lib.ERR_STATE, flags
        assert refusal_code(e.histogram_rows, 1, good, weighted=True) == 2
        assert refusal_code(e.histogram_rows, 1, good, grouped=True) == 2
        assert refusal_code(e.histogram_rows, 1, good, anomaly=True) == 2
        assert refusal_code(e.histogram_rows, 1, good, 0, 10) == 1 and refusal_code(e.histogram_rows, 1, good, 0, 8, 0) == 1
        x = ra.ensemble.DeviceVector(e.series_devptr(1), n, np.float64, e)
        assert refusal_code(e.histogram_vectors, [x], good, weighted=True) == 2 and refusal_code(e.histogram_vectors, [x], good, grouped=True) == 2
        assert refusal_code(e.histogram2d, x, x, good, good, weighted=True) == 2 and refusal_code(e.histogram2d, x, x, good, good, grouped=True) == 2
        px = C.cast(C.c_void_p(x.ptr), f64)
        pg = good.ctypes.data_as(f64)
        descending = np.array([1.0, 0.0]).ctypes.data_as(f64)
        assert lib.rscm_ens_histogram2d(h, px, px, 4, pg, 4, pg, 0, pc, pb, po) == _lib.OK and total[0] == n
        assert lib.rscm_ens_histogram2d(h, px, px, 4, pg, 4, pg, _lib.SELECT_ANOMALY, pc, pb, po) == _lib.ERR_INVALID
        assert lib.rscm_ens_histogram2d(h, px, px, 4, pg, 4, pg, 8, pc, pb, po) == _lib.ERR_INVALID
        assert lib.rscm_ens_histogram2d(h, px, px, 2, descending, 4, pg, 0, pc, pb, po) == _lib.ERR_INVALID
        assert lib.rscm_ens_histogram2d(h, px, px, 4, pg, 2, descending, 0, pc, pb, po) == _lib.ERR_INVALID
        assert lib.rscm_ens_histogram2d(h, px, px, 4, pg, 1, pg, 0, pc, pb, po) == _lib.ERR_INVALID
        assert lib.rscm_ens_histogram2d(h, None, px, 4, pg, 4, pg, 0, pc, pb, po) == _lib.ERR_INVALID
        assert lib.rscm_ens_histogram2d(h, px, px, 4, pg, 4, pg, 0, None, pb, po) == _lib.ERR_INVALID
        host = np.zeros(n)
        assert lib.rscm_ens_histogram2d(h, px, host.ctypes.data_as(f64), 4, pg, 4, pg, 0, pc, pb, po) == _lib.ERR_INVALID   # host memory
        with pytest.raises(ValueError):
            e.histogram_rows(1, [1.0, 0.0])
        with e.select(1, [0.5], 0, 8):
            assert refusal_code(e.histogram_rows, 1, good) == 2
            assert refusal_code(e.histogram_vectors, [x], good) == 2
            assert refusal_code(e.histogram2d, x, x, good, good) == 2
        e.histogram_rows(1, good)
