"""GPU tier (-m gpu): the EXACT two-layer kernel's two guards of a speculative year -- the sub-step states against the boxes of
csrc/two_layer_box.hpp (default where a wavefront's parameters allow it) and every numerator (rscm_gpu_set_two_layer_guard(1)) --
against each other and against the CPU oracle, bit for bit, series and status, on inputs at and across every box edge."""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.helpers import SEED, TL_RANGES, assert_bit_equal, axis_values, f_syn, two_layer_params

pytestmark = pytest.mark.gpu

BASE = np.array([1.0, 0.0, 1.0, 0.7, 8.0, 100.0])
# (lo, hi) exponents of the parameter boxes, in parameter-row order (efficacy * eta is boxed as a product: row 2 is efficacy)
BOXES = {0: (-16, 6), 1: (-64, 2), 3: (-16, 6), 4: (-2, 10), 5: (-2, 14)}


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


def _guard(numerators):
    from rscm_amd import _lib as L
    L.check(L.load().rscm_gpu_set_two_layer_guard(numerators))


def _run(ra, t, P, F, ts0, td0, *, scen=None, h=None, source=0):
    b = np.append(t, t[-1] + (t[-1] - t[-2]))
    with ra.Ensemble(ra.KIND_TWO_LAYER, P.shape[1], b) as e:
        e.set_mode(0)
        if h is not None:
            e.set_step_size(0, h)
        e.set_params(P)
        e.set_forcing(F, scen, source)
        e.set_initial("Surface Temperature", ts0)
        e.set_initial("Deep Ocean Temperature", td0)
        e.run()
        return e.get_series(1), e.get_series(2), e.status()


def _three_ways(ra, orc, t, P, F, ts0=0.0, td0=0.0, *, scen=None, h=None, source=0, what=""):
    """state guard == numerator guard == oracle, series and status."""
    with np.errstate(all="ignore"):
        want = orc.two_layer_run(orc.bounds_from_values(t), P, F, ts0, td0, scen=scen, source=source, h=0.1 if h is None else h,
                                 threads=8)
    try:
        _guard(1)
        old = _run(ra, t, P, F, ts0, td0, scen=scen, h=h, source=source)
    finally:
        _guard(0)
    new = _run(ra, t, P, F, ts0, td0, scen=scen, h=h, source=source)
    for got, name in ((old, "numerator guard"), (new, "state guard")):
        assert_bit_equal(got[0], want[0], f"Ts {name} {what}")
        assert_bit_equal(got[1], want[1], f"Td {name} {what}")
        with np.errstate(invalid="ignore"):
            bad = ~(np.isfinite(want[0][-1]) & np.isfinite(want[1][-1]))
        assert (got[2].astype(bool) == bad).all(), f"status {name} {what}"
    assert (old[2] == new[2]).all()
    return want


def test_switch_is_validated(ra):
    from rscm_amd import RscmGpuError
    from rscm_amd import _lib as L
    with pytest.raises(RscmGpuError):
        L.check(L.load().rscm_gpu_set_two_layer_guard(2))
    _guard(0)


def test_forcing_zeros_denormals_and_extremes(ra, orc):
    """+0 forcing is inside the forcing box, -0, denormals and +-1e300 are not: those years replay (or settle), same bits."""
    t = axis_values(1750, 1900)
    P = two_layer_params(256, seed=SEED + 7)
    F0 = f_syn(t)
    F = np.stack([np.zeros_like(t), np.full_like(t, -0.0), F0 * 5e-324, F0 * 1e-310, np.full_like(t, 1e300), np.full_like(t, -1e300),
                  np.where(np.arange(len(t)) % 3 == 0, -0.0, F0), np.where(np.arange(len(t)) % 5 == 0, 4e-324, -F0),
                  F0 * 2.0 ** -128, F0 * 2.0 ** 11])
    scen = (np.arange(P.shape[1]) % F.shape[0]).astype(np.int32)
    _three_ways(ra, orc, t, P, F, 0.0, 0.0, scen=scen, what="forcing")
    _three_ways(ra, orc, t, P, F, 0.5, 0.2, scen=scen, what="forcing, warm start")


def _edge_values(lo, hi):
    e_lo, e_hi = 2.0 ** lo, 2.0 ** hi
    return [np.nextafter(e_lo, 0.0), e_lo, np.nextafter(e_hi, 0.0), e_hi]


def test_parameters_on_both_sides_of_every_box_edge(ra, orc):
    """Per parameter and edge, one wavefront whose members sit just inside the box at that edge (state guard) next to one whose
    64 members are the same but for one just outside (the whole wavefront takes the numerator guard); a = +0, -0 and efficacy*eta
    at its edges; h at the edges of its box."""
    t = axis_values(1750, 1800)
    rows = []
    rng = np.random.default_rng(3)
    for j, (lo, hi) in BOXES.items():
        below_lo, at_lo, below_hi, at_hi = _edge_values(lo, hi)
        for inside, outside in ((at_lo, below_lo), (below_hi, at_hi)):
            wave = np.repeat(BASE[:, None], 64, axis=1) * rng.uniform(0.9, 1.1, (6, 64))
            wave[1] = rng.uniform(0.0, 0.1, 64)
            wave[j, ::2] = inside
            rows.append(wave.copy())                # all inside
            wave[j, 5] = outside
            rows.append(wave)                       # one outside
    # efficacy * eta (row 2 times row 3) at the edges of its own box
    for target in _edge_values(-16, 6):
        wave = np.repeat(BASE[:, None], 64, axis=1)
        wave[3] = 0.5
        wave[2] = target / 0.5
        rows.append(wave)
    wave = np.repeat(BASE[:, None], 64, axis=1)
    wave[1, 1::2] = -0.0
    rows.append(wave)
    P = np.concatenate(rows, axis=1)
    F = f_syn(t)
    _three_ways(ra, orc, t, P, F, 0.0, 0.0, what="parameter edges")
    _three_ways(ra, orc, t, P, F, 0.3, -0.1, what="parameter edges, warm start")
    # h (and h / 2) at and past the edges of [2^-16, 2^2), on axes that h divides
    for step, hs in ((1.0, (2.0 ** -15, 2.0 ** -16, 2.0 ** -17, 1.0)), (4.0, (2.0, 4.0))):
        tt = np.arange(1750.0, 1750.0 + 3 * step, step)
        for h in hs:
            _three_ways(ra, orc, tt, P[:, :256], f_syn(tt), 0.1, 0.05, h=h, what=f"h={h}")


def test_a_zero_and_trajectories_crossing_zero(ra, orc):
    """a = 0 exactly, and forcings that swing the members through 0 K and back (stage states that cancel to +0 or land near it)."""
    t = axis_values(1750, 2100)
    P = two_layer_params(640, seed=SEED + 11)
    P[1, ::3] = 0.0
    F = np.stack([6.0 * np.sin(2.0 * np.pi * (t - 1750.0) / 7.0), 3.0 * np.cos(2.0 * np.pi * (t - 1750.0) / 3.0) - 0.5,
                  np.where(np.arange(len(t)) % 2 == 0, 4.0, -4.0)])
    scen = (np.arange(P.shape[1]) % 3).astype(np.int32)
    want = _three_ways(ra, orc, t, P, F, 0.0, 0.0, scen=scen, what="crossing 0 K")
    assert (np.diff(np.sign(want[0]), axis=0) != 0).sum(axis=0).min() >= 2   # every member crosses 0 K


def test_states_across_the_state_box_edges(ra, orc):
    """Initial states just below, at and above 2^-128 and 2^26: relaxing members leave the box, tiny ones enter it."""
    t = axis_values(1750, 1850)
    vals = [2.0 ** -129, np.nextafter(2.0 ** -128, 0.0), 2.0 ** -128, 1e-30, -2.0 ** -128, np.nextafter(2.0 ** 26, 0.0), 2.0 ** 26,
            -2.0 ** 26, 3.0 * 2.0 ** 25, 2.0 ** 30, 5e-324, -0.0]
    n = 64 * len(vals)
    P = np.repeat(BASE[:, None], n, axis=1)
    P[0] = 4.0                                       # strong relaxation: a large state comes down through 2^26 within years
    P[4] = 1.0
    ts0 = np.repeat(np.array(vals), 64)
    td0 = np.roll(ts0, 64)
    for F in (np.zeros_like(t), f_syn(t) * 1e-36, f_syn(t)):
        _three_ways(ra, orc, t, P, F, ts0, td0, what="state edges")


def test_headline_draw_including_its_runaway_members(ra, orc):
    """bench.py's workload -- 1e5 members of the seeded Latin hypercube, 750 years, EXACT -- with both guards: the oracle's bits
    everywhere, the 3.4 % of runaway members (overflow to inf / NaN, flagged) included."""
    t = axis_values()
    b = np.append(t, t[-1] + 1.0)
    F = f_syn(t)
    n = 100_000
    lo = np.array([r[0] for r in TL_RANGES])
    hi = np.array([r[1] for r in TL_RANGES])
    got = {}
    for g in (1, 0):
        try:
            _guard(g)
            with ra.Ensemble(ra.KIND_TWO_LAYER, n, b) as e:
                e.set_mode(0)
                e.sample_lhs(SEED, lo, hi)
                P = e.get_params()
                e.set_forcing(F)
                e.set_initial(1, 0.0)
                e.set_initial(2, 0.0)
                e.run()
                got[g] = (e.get_series(1), e.get_series(2), e.status())
        finally:
            _guard(0)
    with np.errstate(all="ignore"):
        want = orc.two_layer_run(orc.bounds_from_values(t), P, F, 0.0, 0.0, threads=8)
        failed = ~(np.isfinite(want[0][-1]) & np.isfinite(want[1][-1]))
    assert 0.02 < failed.mean() < 0.05
    for g in (1, 0):
        assert_bit_equal(got[g][0], want[0], f"Ts guard {g}")
        assert_bit_equal(got[g][1], want[1], f"Td guard {g}")
        assert (got[g][2].astype(bool) == failed).all()


def test_sub_step_counts_other_than_ten(ra, orc):
    """Irregular axes: 5, 10, 50 sub-steps per model step with h = 0.1, and h = 1/120 and 0.25 (the generic loop)."""
    t = np.concatenate([np.arange(1750.0, 1760.0, 0.5), np.arange(1760.0, 1800.0, 1.0), np.arange(1800.0, 1900.0, 5.0)])
    P = two_layer_params(200, seed=SEED + 5)
    for h in (0.1, 1.0 / 120.0, 0.25):
        _three_ways(ra, orc, t, P, f_syn(t), 0.1, 0.0, h=h, what=f"h={h}")


def test_likelihood_only_path(ra):
    """rscm_ens_run_loglik (STORE = false): state guard == numerator guard, bit for bit, on a draw with runaway members."""
    t = axis_values()
    b = np.append(t, t[-1] + 1.0)
    n = 4000
    P, F = two_layer_params(n), f_syn(t)
    ov = np.r_[np.full(5, 2), np.full(19, 1)]
    ot = np.r_[[0, 40, 40, 300, 750], np.arange(100, 271, 10), [750]].astype(np.int32)
    val = np.linspace(0.0, 3.0, len(ot))
    sig = np.linspace(0.05, 0.5, len(ot))
    out = {}
    for g in (1, 0):
        try:
            _guard(g)
            with ra.Ensemble(ra.KIND_TWO_LAYER, n, b, store_series=False) as e:
                e.set_mode(0)
                e.set_params(P)
                e.set_forcing(F)
                e.set_initial(1, 0.1)
                e.set_initial(2, -0.05)
                out[g] = (e.run_loglik(ov, ot, val, sig, True), e.status())
        finally:
            _guard(0)
    assert_bit_equal(out[0][0], out[1][0], "loglik")
    assert (out[0][1] == out[1][1]).all() and (out[0][1] != 0).sum() > 0
    assert np.isfinite(out[0][0]).sum() > n // 2


def test_fused_group_launch(ra, orc):
    """The two-layer body inside the fused lock-step launch (csrc/group.hip), its forcing linked from an Aggregate: state guard ==
    numerator guard == oracle."""
    from rscm_amd import _lib as L
    from rscm_amd.ensemble import run_lockstep
    t = axis_values(1750, 2000)
    b = np.append(t, t[-1] + 1.0)
    T, n = len(t), 700
    P = two_layer_params(n, seed=SEED + 9)
    P[1, :64] = 0.0
    P[1, 64:128] = 2.0                               # runaway within decades
    F = f_syn(t) * 1.5
    F[::17] = 0.0
    lib = L.load()
    got = {}
    stream = C.c_void_p()
    L.check(lib.rscm_gpu_stream_create(0, C.byref(stream)))
    for g in (1, 0):
        ag, tl = ra.Ensemble(ra.KIND_AGGREGATE, n, b), ra.Ensemble(ra.KIND_TWO_LAYER, n, b)
        try:
            _guard(g)
            ag.set_stream(stream.value)
            tl.set_stream(stream.value)
            w = np.zeros((9, n))
            w[0] = 2.0                                # Weighted
            w[1] = 1.0
            ag.set_params(w)
            tab = np.full((8, T), np.nan)
            tab[0] = F
            ag.set_forcing(tab)
            ag.set_initial(1, 0.0)
            tl.set_mode(0)
            tl.set_params(P)
            tl.set_initial(1, 0.0)
            tl.set_initial(2, 0.0)
            tl.link_input(0, ag, 1, ra.SRC_UPSTREAM)
            launches, steps = C.c_int64(), C.c_int64()
            L.check(lib.rscm_gpu_lockstep_stats(C.byref(launches), C.byref(steps)))
            run_lockstep((ag, tl))
            L.check(lib.rscm_gpu_lockstep_stats(C.byref(launches), C.byref(steps)))
            assert launches.value < steps.value      # fused
            got[g] = (tl.get_series(1), tl.get_series(2), tl.status())
            linked = ag.get_series(1)
        finally:
            _guard(0)
            tl.close()
            ag.close()
    L.check(lib.rscm_gpu_stream_destroy(0, stream))
    assert (linked == linked[:, :1]).all()           # the forcing the two-layer model read, one series for every member
    with np.errstate(all="ignore"):
        want = orc.two_layer_run(orc.bounds_from_values(t), P, linked[:, 0], 0.0, 0.0, source=1, threads=8)
    for g in (1, 0):
        assert_bit_equal(got[g][0], want[0], f"Ts guard {g}")
        assert_bit_equal(got[g][1], want[1], f"Td guard {g}")
    assert (got[0][2] == got[1][2]).all()
