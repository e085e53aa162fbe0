"""CPU tier of the histograms across members (rscm_ens_histogram_rows, rscm_ens_histogram_vectors, rscm_ens_histogram2d; the
definition is stated in include/rscm_gpu.h).

* tests/host_histogram.py, the restatement in numpy and Python integers, against ``numpy.histogram`` with int64 weights and
  ``numpy.histogram2d`` on tied data and on values sitting on every edge, and against a brute-force Python loop over members on NaN,
  +-Inf, +-0 on an edge at 0.0, a value on the last edge and zero weights beside one of 2^40.
* The finishers ``rscm_amd.ensemble.histogram_result`` / ``histogram2d_result`` against ``fractions.Fraction``; two halves of an
  ensemble add up to the whole; shape and edge errors are raised before the library is touched.
* ``rscm_amd.ensemble.crps_bracket``: it contains a brute-force CRPS that sorts in Fractions, is at most as wide as the widest bin,
  and is NaN in each refused case.
* rscm_amd/csrc/histogram_bin.hpp, the bin function the kernels use, in a stand-alone host program under AddressSanitizer and
  UndefinedBehaviorSanitizer against a linear scan (tests/c_abi/histogram_bin_host.cpp).
* ``rscm_amd.distributed.histogram_rows_global`` / ``histogram_vectors_global`` / ``histogram2d_global`` on stand-in ensembles
  (tests/_dist_histogram_worker.py): alone in one process, and over a real 2-rank gloo group on 127.0.0.1."""
import json
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import host_histogram as hh
from tests._dist_histogram_worker import CALLS, EDGES, N_GROUPS, N_ROWS, StandInEnsemble, bits, global_data, results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=131, rows=5, seed=4):
    """Rows rounded to one decimal (ties, and values on the edges below), with NaN, both infinities and both zeros among them; weights
    with zeros and one of 2^40; groups with members of none and one id past the last group; a baseline with a NaN."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.standard_normal((rows, n)), 1)
    X[2:, 11] = np.nan
    X[1, 20], X[1, 21] = np.inf, -np.inf
    X[0, 30], X[0, 31] = 0.0, -0.0
    X[3, 40], X[3, 41] = 1.5, 1.5                    # on the last edge of EDGES_T
    w = rng.integers(0, 9, n)
    w[rng.random(n) < 0.2] = 0
    w[40] = 1 << 40
    groups = rng.integers(-1, 3, n).astype(np.int32)
    groups[17] = 3                                   # past the last of three groups
    b = np.round(X[:2].mean(axis=0), 1)
    b[50] = np.nan
    return X, w, groups, b


EDGES_T = np.array([-1.5, -0.7, -0.1, 0.0, 0.1, 0.4, 1.5])   # an edge at 0.0, edges on the data's grid of tenths


def _brute(X, edges, w=None, groups=None, G=1, baseline=None):
    """The definition member by member, in Python: (counts[rows][G][B], below, above, total)."""
    R, n = X.shape
    E = len(edges)
    B = E - 1
    counts = [[[0] * B for _ in range(G)] for _ in range(R)]
    below, above, total = ([[0] * G for _ in range(R)] for _ in range(3))
    for r in range(R):
        for i in range(n):
            with np.errstate(invalid="ignore"):      # (an infinity minus an infinity is a NaN, which takes no part)
                v = float(X[r, i]) if baseline is None else float(np.float64(X[r, i]) - np.float64(baseline[i]))
            g = 0 if groups is None else int(groups[i])
            if v != v or not 0 <= g < G:
                continue
            wt = 1 if w is None else int(w[i])
            k = sum(1 for e in edges if float(e) <= v)
            total[r][g] += wt
            if k == 0:
                below[r][g] += wt
            elif k <= B:
                counts[r][g][k - 1] += wt
            elif v == float(edges[-1]):
                counts[r][g][B - 1] += wt
            else:
                above[r][g] += wt
    return tuple(np.array(a, dtype=np.int64) for a in (counts, below, above, total))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def test_restatement_equals_numpy_histogram():
    """numpy.histogram(x, bins=e, weights=w) with int64 weights returns int64 sums; tied data with values on every edge."""
    rng = np.random.default_rng(1)
    for E in (2, 3, 9, 65):
        e = np.round(np.linspace(-2.0, 2.0, E), 3) if E > 3 else np.array([-0.5, 0.5, 1.0][:E])
        x = np.round(rng.standard_normal(500), 1)
        x[:E] = e                                     # a value on every edge, the last one included
        w = rng.integers(0, 1 << 30, 500)
        for weights in (None, w):
            want, _ = np.histogram(x, bins=e, weights=weights)
            counts, below, above, total = hh.sums(x[None, :], e, weights)
            assert want.dtype == np.int64 and (counts[0, 0] == want).all(), E
            assert below[0, 0] == int((np.ones(500, dtype=np.int64) if weights is None else w)[x < e[0]].sum())
            assert above[0, 0] == int((np.ones(500, dtype=np.int64) if weights is None else w)[x > e[-1]].sum())
            assert total[0, 0] == below[0, 0] + counts[0, 0].sum() + above[0, 0]
            right = np.searchsorted(e, x, "right")    # the count of edges at or below the value
            assert ((e[None, :] <= x[:, None]).sum(axis=1) == right).all()


def test_restatement_equals_numpy_histogram2d():
    rng = np.random.default_rng(2)
    x, y = np.round(rng.standard_normal(700), 1), np.round(rng.standard_normal(700), 1)
    ex, ey = np.array([-1.0, -0.3, 0.0, 0.2, 1.1]), np.array([-0.8, 0.0, 0.8])
    x[:5], y[5:8] = ex, ey
    w = rng.integers(0, 1 << 30, 700)
    for weights in (None, w):
        want, _, _ = np.histogram2d(x, y, bins=(ex, ey), weights=weights)
        counts, outside, total = hh.sums2d(x, y, ex, ey, weights)
        assert (counts[0] == want.astype(np.int64)).all() and (want == np.round(want)).all()
        assert total[0] == counts[0].sum() + outside[0] == (700 if weights is None else int(w.sum()))
        assert outside[0] > 0


def test_restatement_equals_the_member_loop():
    X, w, groups, b = _data()
    for weights, grp, base in ((None, None, None), (w, None, None), (None, groups, None), (w, groups, b), (None, None, b)):
        G = 3 if grp is not None else 1
        got = hh.sums(X, EDGES_T, weights, grp, G if grp is not None else None, base)
        want = _brute(X, EDGES_T, weights, grp, G, base)
        for a, c in zip(got, want):
            assert a.dtype == np.int64 and a.shape == c.shape and (a == c).all()
    counts, below, above, total = hh.sums(X, EDGES_T, w)
    assert counts[0, 0, 3] >= int(w[30]) + int(w[31])          # both zeros sit in the bin that starts at 0.0
    assert counts[3, 0, -1] >= 1 << 40 and above[3, 0] < 1 << 40   # 1.5, with the weight of 2^40, is in the closed last bin
    assert above[1, 0] >= int(w[20]) and below[1, 0] >= int(w[21])  # +Inf above, -Inf below
    assert total[2, 0] == int(w.sum()) - int(w[11])             # the NaN takes no part


def test_per_row_edges_and_slot_of():
    X, w, _, _ = _data()
    tables = np.stack([EDGES_T + 0.05 * r for r in range(X.shape[0])])
    got = hh.sums(X, tables, w)
    for r in range(X.shape[0]):
        one = hh.sums(X[r:r + 1], tables[r], w)
        for a, c in zip(got, one):
            assert (a[r] == c[0]).all()
    assert hh.slot_of([0.0, 1.0, 2.0], np.array([-0.0, 0.0, 1.0, 2.0, 2.5, -1.0, np.inf, -np.inf])).tolist() == [0, 0, 1, 1, 3, 2, 3, 2]


# ---- the finishers ------------------------------------------------------------------------------------------------------------------

def test_finishers_against_fractions():
    from rscm_amd.ensemble import histogram2d_result, histogram_result
    X, w, groups, b = _data()
    for weights, grp in ((None, None), (w, None), (w, groups)):
        G = 3 if grp is not None else None
        counts, below, above, total = hh.sums(X, EDGES_T, weights, grp, G)
        got = histogram_result(counts, below, above, total, grouped=grp is not None)
        assert hh.same(got, hh.histogram_rows(X, EDGES_T, weights, grp, G))
        p = np.asarray(got["probability"]).reshape(counts.shape)
        for idx in np.ndindex(*counts.shape):
            t = int(total[idx[:2]])
            assert (math.isnan(p[idx]) if t == 0 else p[idx] == float(Fraction(int(counts[idx]), t)))
        assert got["counts"].dtype == np.int64 and got["total"].shape == ((X.shape[0], 3) if grp is not None else (X.shape[0],))
        c2, o2, t2 = hh.sums2d(X[0], X[1], EDGES_T, EDGES_T[1:5], weights, grp, G)
        got2 = histogram2d_result(c2, o2, t2, grouped=grp is not None)
        assert hh.same(got2, hh.histogram2d(X[0], X[1], EDGES_T, EDGES_T[1:5], weights, grp, G))
        assert got2["counts"].shape == ((3, 6, 3) if grp is not None else (6, 3))
    # quotients beyond 2^53 round the exact quotient once
    big = histogram_result(np.array([[[(1 << 60) + 1, 3]]]), np.array([[0]]), np.array([[0]]), np.array([[(1 << 60) + 4]]), grouped=False)
    assert big["probability"][0, 0] == float(Fraction((1 << 60) + 1, (1 << 60) + 4)) and big["probability"][0, 1] == 3 / ((1 << 60) + 4)
    none = histogram_result(np.zeros((2, 1, 4), dtype=np.int64), *(np.zeros((2, 1), dtype=np.int64),) * 3, grouped=False)
    assert np.isnan(none["probability"]).all() and none["probability"].shape == (2, 4)


def test_two_halves_add_up():
    from rscm_amd.ensemble import histogram2d_result, histogram_result
    X, w, groups, b = _data()
    h = X.shape[1] // 3
    parts = (slice(0, h), slice(h, None))
    whole = hh.sums(X, EDGES_T, w, groups, 3, b)
    halves = [hh.sums(X[:, s], EDGES_T, w[s], groups[s], 3, b[s]) for s in parts]
    for k in range(4):
        assert (halves[0][k] + halves[1][k] == whole[k]).all()
    assert hh.same(histogram_result(*(halves[0][k] + halves[1][k] for k in range(4))), hh.histogram_rows(X, EDGES_T, w, groups, 3, b))
    whole2 = hh.sums2d(X[0], X[4], EDGES_T, EDGES_T, w, groups, 3)
    halves2 = [hh.sums2d(X[0, s], X[4, s], EDGES_T, EDGES_T, w[s], groups[s], 3) for s in parts]
    for k in range(3):
        assert (halves2[0][k] + halves2[1][k] == whole2[k]).all()
    assert hh.same(histogram2d_result(*(halves2[0][k] + halves2[1][k] for k in range(3))), hh.histogram2d(X[0], X[4], EDGES_T, EDGES_T, w, groups, 3))


def test_shape_and_edge_errors_come_before_the_library():
    """The histogram calls check their edges first: with a handle that cannot make any call (no library, no device) bad edges are
    still ValueErrors, and good edges reach the missing library."""
    from rscm_amd.ensemble import DeviceVector, Ensemble, histogram_edges
    e = object.__new__(Ensemble)
    e.n_times, e.n_members = 6, 10

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was touched: {name}")

    e._lib, e._h = NoLibrary(), None
    vec = DeviceVector(8, 10, np.float64, e)
    bad_edges = ([1.0], [], 1.0, [2.0, 1.0], [1.0, 1.0], [0.0, np.nan], [0.0, np.inf], [-np.inf, 0.0], np.arange(1026.0), np.zeros((2, 3)),
                 [[0.0, 1.0], [1.0, 0.0]])
    for bad in bad_edges:
        with pytest.raises(ValueError, match="edges"):
            e.histogram_rows(1, bad)
        with pytest.raises(ValueError, match="edges"):
            e.histogram_vectors([vec], bad)
        with pytest.raises(ValueError, match="edges_x"):
            e.histogram2d(vec, vec, bad, [0.0, 1.0])
        with pytest.raises(ValueError, match="edges_y"):
            e.histogram2d(vec, vec, [0.0, 1.0], bad)
        with pytest.raises(ValueError):
            histogram_edges(bad)
    with pytest.raises(ValueError, match="edges"):
        e.histogram_vectors([vec, vec], np.array([[0.0, 1.0]] * 3))            # two vectors, three tables
    with pytest.raises(ValueError, match="1 to 8 vectors"):
        e.histogram_vectors([], [0.0, 1.0])
    with pytest.raises(ValueError, match="1 to 8 vectors"):
        e.histogram_vectors([vec] * 9, [0.0, 1.0])
    with pytest.raises(ValueError, match="DeviceVectors"):
        e.histogram_vectors([np.zeros(10)], [0.0, 1.0])
    with pytest.raises(ValueError, match="DeviceVectors"):
        e.histogram2d(vec, np.zeros(10), [0.0, 1.0], [0.0, 1.0])
    assert histogram_edges(np.arange(1025.0)).shape == (1025,) and histogram_edges([[0, 1], [5, 7]], tables=2).shape == (2, 2)
    assert histogram_edges([0, 1]).dtype == np.float64
    for call in (lambda: e.histogram_rows(1, [0.0, 1.0]), lambda: e.histogram_vectors([vec], [0.0, 1.0]),
                 lambda: e.histogram2d(vec, vec, [0.0, 1.0], [0.0, 1.0])):
        with pytest.raises(AssertionError, match="the library was touched"):
            call()


# ---- the CRPS bracket ---------------------------------------------------------------------------------------------------------------

def test_crps_bracket_contains_the_sorted_crps():
    """200 random weighted rows: values inside the edges (ties, values on edges), integer weights with zeros; records on an edge,
    on a value, between two, on the first and the last edge.  The bounds are compared as Fractions, so nothing is hidden by
    rounding; what the package returns is each bound rounded once."""
    from rscm_amd.ensemble import crps_bracket
    rng = np.random.default_rng(5)
    rows = 200
    for E in (2, 9, 40):
        edges = np.sort(np.round(rng.uniform(-2.0, 2.0, E), 2))
        edges[0], edges[-1] = -2.5, 2.5
        edges = np.unique(edges)
        n = 30
        X = np.clip(np.round(rng.standard_normal((rows, n)), 1), -2.5, 2.5)
        w = rng.integers(0, 50, n)
        w[3] = 1 << 40
        record = np.round(rng.uniform(-2.5, 2.5, rows), rng.integers(0, 3))
        record[:4] = [edges[0], edges[-1], X[2, 5], edges[len(edges) // 2]]
        hist = hh.histogram_rows(X, edges, w)
        assert not hist["below"].any() and not hist["above"].any()
        got = crps_bracket(hist, edges, record)
        assert hh.same(got, hh.crps_bracket(hist, edges, record))
        widest = max(Fraction(float(b)) - Fraction(float(a)) for a, b in zip(edges[:-1], edges[1:]))
        for r in range(rows):
            lo, hi = hh.crps_bracket_fractions(hist["counts"][r], 0, 0, edges, float(record[r]))
            exact = hh.crps_exact(X[r], w, record[r])
            assert lo <= exact <= hi, (E, r, float(lo), float(exact), float(hi))
            assert hi - lo <= widest, (E, r)
            assert got["lower"][r] == float(lo) and got["upper"][r] == float(hi)
            assert got["lower"][r] <= float(exact) <= got["upper"][r]


def test_crps_bracket_narrows_with_the_grid_and_takes_groups_and_row_edges():
    from rscm_amd.ensemble import crps_bracket, histogram_result
    rng = np.random.default_rng(6)
    X = np.round(rng.standard_normal((3, 50)), 2).clip(-3.0, 3.0)
    record = np.array([0.25, -1.0, 2.0])
    widths = []
    for E in (7, 25, 97):
        edges = np.linspace(-3.0, 3.0, E)
        got = crps_bracket(hh.histogram_rows(X, edges), edges, record)
        widths.append(float((got["upper"] - got["lower"]).max()))
        assert widths[-1] <= 6.0 / (E - 1) * (1 + 1e-12)
    assert widths[0] > widths[1] > widths[2]
    groups = (np.arange(50) % 2).astype(np.int32)
    edges = np.linspace(-3.0, 3.0, 13)
    grouped = crps_bracket(hh.histogram_rows(X, edges, None, groups, 2), edges, record)
    assert grouped["lower"].shape == (3, 2)
    for g in range(2):
        one = hh.crps_bracket(hh.histogram_rows(X[:, groups == g], edges), edges, record)
        assert hh.same({k: v[:, g] for k, v in grouped.items()}, one)
    tables = np.stack([edges, edges * 1.5, edges + 0.125])
    per_row = crps_bracket(hh.histogram_rows(X.clip(-2.8, 2.8), tables), tables, record)
    for r in range(3):
        one = hh.crps_bracket(hh.histogram_rows(X[r:r + 1].clip(-2.8, 2.8), tables[r]), tables[r], record[r:r + 1])
        assert per_row["lower"][r] == one["lower"][0] and per_row["upper"][r] == one["upper"][0]
    # a point mass on the record scores 0, and the bracket says so up to the record's bin
    point = histogram_result(np.array([[0, 7, 0]]), [0], [0], [7], grouped=False)
    got = crps_bracket(point, [0.0, 1.0, 2.0, 3.0], [1.5])
    assert got["lower"][0] == 0.0 and got["upper"][0] == 1.0


def test_crps_bracket_refusals():
    from rscm_amd.ensemble import crps_bracket
    edges = [0.0, 1.0, 2.0]
    ok = {"counts": np.array([[2, 3]] * 7), "below": np.zeros(7, dtype=np.int64), "above": np.zeros(7, dtype=np.int64),
          "total": np.full(7, 5)}
    ok["below"][1], ok["above"][2] = 1, 1
    ok["total"][1:3] = 6
    ok["counts"][3], ok["total"][3] = 0, 0
    record = np.array([0.5, 0.5, 0.5, 0.5, np.nan, -0.1, 2.5])
    got = crps_bracket(ok, edges, record)
    assert np.isfinite([got["lower"][0], got["upper"][0]]).all() and got["lower"][0] <= got["upper"][0]
    for r, why in ((1, "below"), (2, "above"), (3, "no weight"), (4, "NaN record"), (5, "record below"), (6, "record above")):
        assert math.isnan(got["lower"][r]) and math.isnan(got["upper"][r]), why
    assert hh.same(got, hh.crps_bracket(ok, edges, record))
    ends = crps_bracket({k: v[:2] for k, v in ok.items()} | {"below": np.zeros(2, dtype=np.int64), "total": np.full(2, 5)}, edges, [0.0, 2.0])
    assert np.isfinite(ends["lower"]).all()                                     # the first and the last edge are inside
    with pytest.raises(ValueError, match="record"):
        crps_bracket(ok, edges, record[:3])
    with pytest.raises(ValueError, match="edges"):
        crps_bracket(ok, [0.0, 1.0], record)


# ---- the bin function of the kernels, on the host -------------------------------------------------------------------------------------

def test_bin_function_under_sanitizers(tmp_path):
    """histogram_bin.hpp in a stand-alone program with its own main, compiled with -fsanitize=address,undefined and run as a program:
    E = 2, 3, 9, 64, 65, 1025 against a linear scan."""
    out = str(tmp_path / "histogram_bin_host")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "rscm_amd", "csrc"), os.path.join(ROOT, "tests", "c_abi", "histogram_bin_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "histogram_bin ok (" in r.stdout
    with open(os.path.join(ROOT, "rscm_amd", "csrc", "histogram_bin.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_abi_minor_28_declares_and_binds_the_entry_points():
    from rscm_amd import _lib
    header = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", header).group(1)) >= 28
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 28
    for name in ("rscm_ens_histogram_rows", "rscm_ens_histogram_vectors", "rscm_ens_histogram2d"):
        assert name in code and name in _lib.SIGNATURES and hasattr(lib, name)
    assert int(re.search(r"#define\s+RSCM_HISTOGRAM_MAX_EDGES\s+(\d+)", header).group(1)) == 1025 == _lib.HISTOGRAM_MAX_EDGES
    assert int(re.search(r"#define\s+RSCM_HISTOGRAM_MAX_SLOTS\s+(\d+)", header).group(1)) == 8192 == _lib.HISTOGRAM_MAX_SLOTS
    assert int(re.search(r"#define\s+RSCM_HISTOGRAM_MAX_VECTORS\s+(\d+)", header).group(1)) == 8 == _lib.HISTOGRAM_MAX_VECTORS
    device = open(os.path.join(ROOT, "rscm_amd", "csrc", "rscm_device.hpp")).read()
    blocks = int(re.search(r"constexpr int kHistBlocks = (\d+);", device).group(1))
    assert int(re.search(r"constexpr int64_t kHistogramMembersPerPass = (\d+);", device).group(1)) == 256 * blocks


# ---- the sharded route --------------------------------------------------------------------------------------------------------------

def _want(n_total):
    rows, _, w, groups, b = global_data(n_total)
    from tests._dist_histogram_worker import EDGES_PER_VECTOR, EDGES_Y
    full = dict(weights=w, groups=groups, n_groups=N_GROUPS)
    return {"rows_plain": bits(hh.histogram_rows(rows, EDGES)), "rows_full": bits(hh.histogram_rows(rows[1:N_ROWS:2], EDGES, baseline=b, **full)),
            "vectors_plain": bits(hh.histogram_rows(rows[[0, 3]], EDGES_PER_VECTOR)),
            "vectors_full": bits(hh.histogram_rows(rows[[4, 2, 5]], EDGES, **full)),
            "joint_plain": bits(hh.histogram2d(rows[0], rows[3], EDGES, EDGES_Y)),
            "joint_full": bits(hh.histogram2d(rows[4], rows[2], EDGES, EDGES_Y, **full))}


def test_one_process_global():
    from rscm_amd.distributed import ShardedEnsemble
    n_total = 301
    data = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: StandInEnsemble(c, 0, *data), rank=0, world=1)
    got = results(se)
    assert got == _want(n_total)
    assert [list(c) for c in se.ensemble.calls] == CALLS
    plain = se.histogram_rows_global("T", EDGES)
    assert plain["counts"].shape == (N_ROWS, 5) and plain["total"].tolist() == [301, 301, 300, 300, 300, 300]
    assert (plain["below"] + plain["counts"].sum(axis=1) + plain["above"] == plain["total"]).all()
    full = se.histogram_vectors_global([4, 2, 5], EDGES, weighted=True, grouped=True)
    assert full["probability"].shape == (3, N_GROUPS, 5) and int(full["total"].max()) > 1 << 40
    joint = se.histogram2d_global(4, 2, EDGES, [-2.0, 0.2, 0.6], grouped=True)
    assert joint["counts"].shape == (N_GROUPS, 5, 2) and (joint["counts"].sum(axis=(1, 2)) + joint["outside"] == joint["total"]).all()


def test_two_rank_gloo_global(tmp_path):
    n_total = 301
    port = "29883"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_histogram_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    want = _want(n_total)
    assert sum(x["count"] for x in res) == n_total and all(0 < x["count"] < n_total for x in res)
    for x in res:
        assert x["world"] == 2 and x["calls"] == CALLS
        for key, value in want.items():
            assert x[key] == value, key
