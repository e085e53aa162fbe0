"""GPU tier (-m gpu): the uniform year of the EXACT two-layer kernel (csrc/two_layer_body.hpp).  The host tells a stand-alone launch
two facts about its years (csrc/two_layer_year_facts.hpp): the sub-step count all its steps share, and whether every forcing value it
can read lies in the chunk guard's forcing box.  A wavefront under the chunk guard whose launch has ten sub-steps everywhere runs a
year loop without the count's load and test, and without the forcing check if the forcing is vouched for.  Which loop runs is decided
here by construction -- the axis, the table, the pieces a run is made in -- and every comparison is bit for bit: against the CPU
oracle, against the per-numerator guard (rscm_gpu_set_two_layer_guard(1), a path the uniform year is no part of), between the stored
run and the fused likelihood, between a cut run and a plain one."""
import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.helpers import SEED, assert_bit_equal, f_syn, two_layer_params
from tests.test_gpu_two_layer_guard import BASE, _guard

pytestmark = pytest.mark.gpu

TS, TD = "Surface Temperature", "Deep Ocean Temperature"
# the chunk forcing box is [2^-128, 2^13) and +0 (csrc/two_layer_chunk_box.hpp)
EDGE_VALUES = {"minus-zero": -0.0, "2^13": 2.0 ** 13, "below-2^13": np.nextafter(2.0 ** 13, 0.0), "2^-128": 2.0 ** -128,
               "below-2^-128": np.nextafter(2.0 ** -128, 0.0), "denormal": 5e-324, "1e300": 1e300, "inf": np.inf, "nan": np.nan}


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


def _annual(points, start=1750.0, step=1.0):
    return start + step * np.arange(points, dtype=np.float64)


def _ensemble(ra, orc, t, P, F, scen=None, source=0, ts0=0.0, td0=0.0, store=True):
    e = ra.Ensemble(ra.KIND_TWO_LAYER, P.shape[1], orc.bounds_from_values(t), store_series=store)
    e.set_mode(0)
    e.set_params(P)
    e.set_forcing(F, scen, source)
    e.set_initial(TS, ts0)
    e.set_initial(TD, td0)
    return e


def _run(ra, orc, t, P, F, scen=None, source=0, ts0=0.0, td0=0.0, pieces=None):
    """(Ts, Td, status) of one run, whole or in the pieces that end at the given steps"""
    with _ensemble(ra, orc, t, P, F, scen, source, ts0, td0) as e:
        for end in (pieces or ()):
            e.run(end)
        e.run()
        assert e.finished()
        return e.get_series(1), e.get_series(2), e.status()


def _oracle(orc, t, P, F, scen=None, source=0, ts0=0.0, td0=0.0):
    with np.errstate(all="ignore"):
        return orc.two_layer_run(orc.bounds_from_values(t), P, F, ts0, td0, scen=scen, source=source, threads=4)


def _equals(got, want, what):
    assert_bit_equal(got[0], want[0], f"Ts {what}")
    assert_bit_equal(got[1], want[1], f"Td {what}")
    if len(got) > 2:
        with np.errstate(invalid="ignore"):
            bad = ~(np.isfinite(want[0][-1]) & np.isfinite(want[1][-1]))
        assert (got[2].astype(bool) == bad).all(), f"status {what}"


def _counts(enable):
    import ctypes as C
    from rscm_amd import _lib as L
    out = (C.c_int64 * 3)()
    L.check(L.load().rscm_gpu_two_layer_guard_counts(0, enable, out))
    return list(out)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_smallest_shapes(ra, orc, n):
    """One lane, a wavefront short of one, a full one, one and a lane, five: on axes of 2, 3 and 12 points (1, 2 and 11 annual steps
    of ten sub-steps, h = 0.1), from the zero state (the first years replay) and from a warm one."""
    P = two_layer_params(n, seed=SEED + 31)
    for points in (2, 3, 12):
        t = _annual(points)
        F = f_syn(t)
        for ts0, td0 in ((0.0, 0.0), (0.4, 0.1)):
            what = f"{n} members, {points} points, start {ts0}"
            want = _oracle(orc, t, P, F, ts0=ts0, td0=td0)
            _counts(1)
            try:
                got = _run(ra, orc, t, P, F, ts0=ts0, td0=td0)
                assert _counts(1) == [0, 0, (n + 63) // 64], what    # every wavefront under the chunk guard
            finally:
                _counts(0)
            _equals(got, want, what + ": against the oracle")
            try:
                _guard(1)
                old = _run(ra, orc, t, P, F, ts0=ts0, td0=td0)
            finally:
                _guard(0)
            _equals(got, old, what + ": against the per-numerator guard")


def test_one_step_of_another_length_takes_the_uniform_year_away(ra, orc):
    """The same members on an annual axis of 12 points and on that axis with its last step two years long: the second launch is
    told of no common count and runs the loop that loads and tests it.  The first eleven rows are the same bits, each run is the
    oracle's, and the run in pieces gets the uniform year back for the pieces before the long step.  A uniform count other than ten
    (two-year steps, twenty sub-steps each) is the oracle's as well."""
    P = two_layer_params(257, seed=SEED + 37)
    ta = _annual(12)
    tb = ta.copy()
    tb[-1] = tb[-2] + 2.0
    F = f_syn(ta)
    a = _run(ra, orc, ta, P, F, ts0=0.3, td0=0.1)
    b = _run(ra, orc, tb, P, F, ts0=0.3, td0=0.1)
    _equals(a, _oracle(orc, ta, P, F, ts0=0.3, td0=0.1), "annual axis")
    want_b = _oracle(orc, tb, P, F, ts0=0.3, td0=0.1)
    _equals(b, want_b, "long last step")
    assert_bit_equal(a[0][:11], b[0][:11], "Ts, first eleven rows")
    assert_bit_equal(a[1][:11], b[1][:11], "Td, first eleven rows")
    assert not np.array_equal(a[0][11], b[0][11])
    _equals(_run(ra, orc, tb, P, F, ts0=0.3, td0=0.1, pieces=(4, 10)), want_b, "long last step, in pieces")
    t2 = _annual(12, step=2.0)
    _equals(_run(ra, orc, t2, P, f_syn(t2)), _oracle(orc, t2, P, f_syn(t2)), "two-year steps")


def _edge_cases(points):
    """(index of the table, source, pieces): the first, the last and the look-ahead index of a launch -- of the whole run and of the
    pieces [0, 4), [4, 8), [8, end) -- for a table read at n (source 0) and at n + 1 (source 1)"""
    last = points - 2                                  # the last step
    cases = []
    for source in (0, 1):
        # whole run: reads source .. last + source; an index it never reads must not matter either
        for at in (0, 1, last, last + 1):
            cases.append((at, source, None))
        # in pieces: index 4 is the first of [4, 8) (source 0) or the look-ahead of [0, 4) (source 1); 8 likewise; 3 and 7 are a
        # piece's last (source 0)
        for at in (3, 4, 5, 7, 8):
            cases.append((at, source, (4, 8)))
    return cases


@pytest.mark.parametrize("name", list(EDGE_VALUES))
def test_forcing_edges_one_scenario(ra, orc, name):
    """A table inside the box but for one value on or past an edge of it: the launch that can read the value is not told that the
    forcing is boxed and checks it per year, every other launch of the run skips the check."""
    P = two_layer_params(65, seed=SEED + 41)
    t = _annual(13)
    base = f_syn(t)
    base[6] = 0.0                                      # +0 is inside
    for at, source, pieces in _edge_cases(len(t)):
        F = base.copy()
        F[at] = EDGE_VALUES[name]
        want = _oracle(orc, t, P, F, source=source, ts0=0.2, td0=0.1)
        got = _run(ra, orc, t, P, F, source=source, ts0=0.2, td0=0.1, pieces=pieces)
        _equals(got, want, f"{name} at index {at}, source {source}, pieces {pieces}")


@pytest.mark.parametrize("name", list(EDGE_VALUES))
def test_forcing_edges_in_the_second_scenario_only(ra, orc, name):
    """Two scenarios and a scenario map: the bad value in the second row alone takes the verdict from the launch, for both rows."""
    P = two_layer_params(65, seed=SEED + 43)
    t = _annual(13)
    scen = (np.arange(P.shape[1]) % 2).astype(np.int32)
    for at, source, pieces in _edge_cases(len(t)):
        F = np.stack([f_syn(t), 1.5 * f_syn(t)])
        F[1, at] = EDGE_VALUES[name]
        want = _oracle(orc, t, P, F, scen=scen, source=source)
        got = _run(ra, orc, t, P, F, scen=scen, source=source, pieces=pieces)
        _equals(got, want, f"{name} in row 1 at index {at}, source {source}, pieces {pieces}")


def test_a_replaced_table_takes_its_verdict_with_it(ra, orc):
    """A run under a table in the box, a table outside it, a second run: a verdict kept from the first table would skip the check
    the second needs (-0 makes a numerator -0 and 1e300 leaves the window: those years replay).  And back again."""
    P = two_layer_params(130, seed=SEED + 47)
    t = _annual(12)
    good = f_syn(t)
    for bad_value in (-0.0, 1e300, 2.0 ** 13):
        bad = good.copy()
        bad[5] = bad_value
        with _ensemble(ra, orc, t, P, good) as e:
            for F in (good, bad, good):
                e.set_forcing(F)
                e.run()
                _equals((e.get_series(1), e.get_series(2), e.status()), _oracle(orc, t, P, F), f"table with {F[5]!r} at index 5")
                e.clear_series()
            # ... and with another source: the same table is read one index on
            e.set_forcing(bad, None, 1)
            e.run()
            _equals((e.get_series(1), e.get_series(2), e.status()), _oracle(orc, t, P, bad, source=1), f"{bad_value!r}, read at n + 1")


def test_a_wavefront_with_one_member_outside_the_chunk_boxes(ra, orc):
    """Cs = 2 and a = 0.5 are inside the state guard's boxes and outside the chunk's: that member's wavefront takes the state guard
    on an annual axis with a boxed table, the other the uniform year."""
    P = np.repeat(BASE[:, None], 128, axis=1) * np.random.default_rng(7).uniform(0.9, 1.1, (6, 128))
    P[1] = 0.02
    P[4, 70], P[1, 70] = 2.0, 0.5
    t = _annual(12)
    F = f_syn(t)
    _counts(1)
    try:
        got = _run(ra, orc, t, P, F)
        assert _counts(1) == [0, 1, 1]
    finally:
        _counts(0)
    _equals(got, _oracle(orc, t, P, F), "one member outside the chunk boxes")


@pytest.mark.parametrize("period", [False, True], ids=["no-period", "period"])
@pytest.mark.parametrize("boxed", [True, False], ids=["boxed", "minus-zero"])
def test_fused_likelihood_equals_the_stored_path(ra, orc, boxed, period):
    """The fused run + likelihood shares the year loop: on an annual axis it takes the uniform year, with and without the forcing
    check.  Its ln L against the stored series' likelihood of the same handle, as tests/test_gpu_two_layer_dispatch.py compares."""
    n, points = 130, 25
    last = points - 1
    P = two_layer_params(n, seed=SEED + 53)
    t = _annual(points)
    F = f_syn(t)
    if not boxed:
        F[9] = -0.0
    rows = np.array([1, 5, 5, last // 2, last - 1, last, 0, 7, last], dtype=np.int32)
    var = [TS] * 6 + [TD] * 3
    rng = np.random.default_rng(1)
    val, sig = rng.normal(0.4, 0.4, len(rows)), rng.uniform(0.05, 0.5, len(rows))
    kw = {"reference": {TS: (2, 8), TD: (0, last // 2 + 1, 2)}} if period else {}
    with _ensemble(ra, orc, t, P, F) as e:
        e.run()
        _equals((e.get_series(1), e.get_series(2)), _oracle(orc, t, P, F), "the stored run")
        want = [e.loglik(var, rows, val, sig, normalize, **kw) for normalize in (False, True)]
        status = e.status()
        assert np.isfinite(want[0]).all() and not np.array_equal(want[0], want[1])
        e.rewind()
        for normalize in (False, True):
            assert_bit_equal(e.run_loglik(var, rows, val, sig, normalize, **kw), want[normalize],
                             f"boxed {boxed}, period {period}, normalize {normalize}: the handle that holds the series")
    with _ensemble(ra, orc, t, P, F, store=False) as e:
        for normalize in (False, True):
            assert_bit_equal(e.run_loglik(var, rows, val, sig, normalize, **kw), want[normalize],
                             f"boxed {boxed}, period {period}, normalize {normalize}: a handle without series")
        assert np.array_equal(e.status(), status)


def test_a_cut_run_equals_the_plain_one(ra, orc):
    """65 536 + 64 members x 192 annual steps as two member blocks in three chunks of steps (rscm_gpu_set_run_plan(1)) against one
    plain launch: every chunk states the facts of its own steps -- the -0 at index 100 costs the middle chunk of each block the
    forcing's verdict and the plain launch its own -- and the bits are the same; the first and the last wavefront also against the
    oracle."""
    from rscm_amd import _lib as L
    lib = L.load()
    n, points = 65536 + 64, 193
    P = two_layer_params(n, seed=SEED + 59)
    t = _annual(points)
    F = f_syn(t)
    F[100] = -0.0
    out = {}
    try:
        with _ensemble(ra, orc, t, P, F) as e:
            for plan in (0, 1):
                L.check(lib.rscm_gpu_set_run_plan(plan))
                e.run()
                assert e.last_run_plan() == ((2, 3) if plan else (1, 1))
                out[plan] = (e.get_series(1), e.get_series(2), e.status())
                e.clear_series()
    finally:
        L.check(lib.rscm_gpu_set_run_plan(-1))
    assert_bit_equal(out[1][0], out[0][0], "Ts, cut run against the plain run")
    assert_bit_equal(out[1][1], out[0][1], "Td, cut run against the plain run")
    assert np.array_equal(out[1][2], out[0][2])
    ends = np.r_[0:64, n - 64:n]
    want = _oracle(orc, t, np.ascontiguousarray(P[:, ends]), F)
    assert_bit_equal(out[1][0][:, ends], want[0], "Ts, first and last wavefront against the oracle")
    assert_bit_equal(out[1][1][:, ends], want[1], "Td, first and last wavefront against the oracle")
