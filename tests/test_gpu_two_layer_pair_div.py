"""GPU tier (-m gpu): the pair lane of the EXACT two-layer kernel -- quotients by the heat capacities in two instructions
(csrc/rk4_device.hpp, pair_div) with per-member constants that a verdict has found safe (csrc/pair_div_verdict.hpp), in the wavefronts
of the uniform year whose members all have such constants.  The quotient and the verdict on the device through
rscm_gpu_selftest_pair_div; the stored bits with the lane (rscm_gpu_set_two_layer_pair_lane(1)) against the bits without (0) on
wavefronts that take it, that are kept out by one member and that get in through a neighbouring constant; the constants after every
way of writing a parameter row; cut runs; and who never takes the lane.  Every comparison is bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.helpers import SEED, assert_bit_equal, bits, f_syn, load_script
from tests.test_gpu_two_layer_guard import BASE
from tests.test_gpu_two_layer_uniform_year import TD, TS, _annual, _counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = load_script("pair_div_proof")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pair_div_unsafe.json")))
NUM_LO, NUM_HI, DEEP_LO = P.NUM_LO, 760, P.SURFACE_NUM_FLOOR
DIV_LO, DIV_HI = -2, 14


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


def _lane(mode):
    from rscm_amd import _lib as L
    L.check(L.load().rscm_gpu_set_two_layer_pair_lane(mode))


def _lanes():
    from rscm_amd import _lib as L
    n = C.c_int64()
    L.check(L.load().rscm_gpu_two_layer_pair_lanes(0, C.byref(n)))
    return n.value


def _golden(stays_unsafe, lo=5.0, hi=15.0):
    return [float.fromhex(g["divisor"]) for g in GOLDEN if (g["variant"] < 0) == stays_unsafe and lo <= float.fromhex(g["divisor"]) <= hi]


def _safe(d, num_lo=NUM_LO):
    return P.verdict_f64(d, num_lo)[0] >= 0


# ---------------------------------------------------------------------------------------------------------------- the quotient
def test_golden_pairs_fail_as_defined_and_not_with_the_verdicts_constants(ra):
    from rscm_amd.ensemble import selftest_pair_div
    num = np.array([float.fromhex(g["numerator"]) for g in GOLDEN])
    den = np.array([float.fromhex(g["divisor"]) for g in GOLDEN])
    for scale in (1.0, 2.0 ** -300, -(2.0 ** 500)):   # a failure belongs to the significands: it is there at every exponent
        ieee, plain, tried, variant = selftest_pair_div(num * scale, den)
        assert_bit_equal(ieee, num * scale / den, "device IEEE division vs host IEEE division")
        assert (bits(plain) != bits(ieee)).all(), "a golden pair passes with the constants as defined"
        assert (variant == np.array([g["variant"] for g in GOLDEN])).all()
        ok = variant >= 0
        assert ok.any() and (~ok).any()
        assert_bit_equal(tried[ok], ieee[ok], "the verdict's constants on the golden pairs")
        assert np.isnan(tried[~ok]).all()


def test_the_devices_verdict_is_the_restatements(ra):
    from rscm_amd.ensemble import selftest_pair_div
    rng = np.random.default_rng(3)
    den = np.concatenate([rng.uniform(5.0, 15.0, 700), rng.uniform(50.0, 200.0, 700), np.ldexp(rng.uniform(1, 2, 300), rng.integers(DIV_LO, DIV_HI, 300)),
                          2.0 ** np.arange(DIV_LO - 1, DIV_HI + 2), [float.fromhex(g["divisor"]) for g in GOLDEN],
                          [np.ldexp(float((1 << 52) + 1), -50), 2.0 ** DIV_LO, np.nextafter(2.0 ** DIV_LO, 0.0), np.nextafter(2.0 ** DIV_HI, 0.0)]])
    for num_lo in (NUM_LO, DEEP_LO):
        _, _, tried, variant = selftest_pair_div(np.ones_like(den), den, num_lo)
        for d, v, q in zip(den, variant, tried):
            if not 2.0 ** DIV_LO <= d < 2.0 ** DIV_HI:
                assert v == -2 and np.isnan(q), d.hex()
                continue
            pv, zh, zl = P.verdict_f64(float(d), num_lo)
            assert v == pv, (d.hex(), num_lo)
            if pv >= 0:
                assert q == zh + zl, d.hex()   # 1 * zl and fma(1, zh, .): the constants themselves, summed once
    assert (selftest_pair_div([1.0], [np.ldexp(float((1 << 52) + 1), -50)], DEEP_LO)[3] == -1).all()   # a zl too small for the deeper window


def test_the_window_on_both_sides_of_every_edge(ra):
    """Inside [2^-902, 2^760), at +0, and for divisors up to the box's edges the verdict's constants give the IEEE quotient; the
    deeper window down to 2^-946 where the verdict was asked for it.  Outside, nothing is promised: -0 and the values next to the
    edges are run, and an infinite numerator against a negative zl shows that the window is needed."""
    from rscm_amd.ensemble import selftest_pair_div
    rng = np.random.default_rng(17)
    dens = np.concatenate([[2.0 ** DIV_LO, np.nextafter(2.0 ** DIV_LO, 1.0), np.nextafter(2.0 ** DIV_HI, 0.0), 5.0, 7.0, 15.0, 50.0, 200.0, 3.0, 1.0],
                           rng.uniform(5.0, 15.0, 40), rng.uniform(50.0, 200.0, 40), np.ldexp(rng.uniform(1, 2, 40), rng.integers(DIV_LO, DIV_HI, 40))])
    for num_lo in (NUM_LO, DEEP_LO):
        inside = np.array([2.0 ** num_lo, np.nextafter(2.0 ** num_lo, 1.0), 1.5 * 2.0 ** num_lo, np.nextafter(2.0 ** NUM_HI, 0.0), 2.0 ** (NUM_HI - 1), 0.0, 1.0])
        outside = np.array([np.nextafter(2.0 ** num_lo, 0.0), 2.0 ** (num_lo - 40), 2.0 ** NUM_HI, -0.0, 5e-324, np.inf])
        gn, gd = np.meshgrid(np.concatenate([inside, -inside[:-2], outside, -outside]), dens)
        num, den = gn.ravel(), gd.ravel()
        ieee, _, tried, variant = selftest_pair_div(num, den, num_lo)
        mag = np.abs(num)
        vouched = (variant >= 0) & ((bits(num) == 0) | ((mag >= 2.0 ** num_lo) & (mag < 2.0 ** NUM_HI)))
        assert vouched.sum() > 0.4 * num.size and (~vouched).sum() > 0.3 * num.size
        assert_bit_equal(tried[vouched], ieee[vouched], f"pair_div inside the window from 2^{num_lo}")
        zero = vouched & (num == 0.0)
        assert zero.any() and (bits(tried[zero]) == 0).all()   # +0 / d = +0, sign and all
    # why the window: inf * zh + inf * zl is NaN where zl is negative, and IEEE's quotient is inf
    d = next(x for x in dens if _safe(float(x)) and P.verdict_f64(float(x))[2] < 0)
    ieee, _, tried, _ = selftest_pair_div([np.inf], [d])
    assert np.isinf(ieee[0]) and np.isnan(tried[0])


def test_random_pairs(ra):
    from rscm_amd.ensemble import selftest_pair_div
    rng = np.random.default_rng(29)
    k = 100_000
    den = np.concatenate([rng.uniform(5.0, 15.0, k // 4), rng.uniform(50.0, 200.0, k // 4), np.ldexp(rng.uniform(1, 2, k // 2), rng.integers(DIV_LO, DIV_HI, k // 2))])
    for num_lo in (NUM_LO, DEEP_LO):
        num = np.ldexp(rng.uniform(1, 2, k), rng.integers(num_lo, NUM_HI, k)) * rng.choice([-1.0, 1.0], k)
        ieee, plain, tried, variant = selftest_pair_div(num, den, num_lo)
        with np.errstate(all="ignore"):
            assert_bit_equal(ieee, num / den, "device IEEE division vs host IEEE division")
        ok = variant >= 0
        assert ok.mean() > 0.99
        assert_bit_equal(tried[ok], ieee[ok], "pair_div with the verdict's constants, random pairs")


# ---------------------------------------------------------------------------------------------------------------- the lane
def _members(n, seed):
    """[6][n] inside the chunk boxes around BASE, every heat capacity with safe constants (an unsafe draw moves to the next double
    that has them): the wavefronts of these members take the lane."""
    rng = np.random.default_rng(seed)
    Pm = np.repeat(BASE[:, None], n, axis=1) * rng.uniform(0.8, 1.25, (6, n))
    Pm[1] = rng.uniform(0.0, 0.05, n)
    for row, num_lo in ((4, DEEP_LO), (5, NUM_LO)):
        for i in range(n):
            while not _safe(float(Pm[row, i]), num_lo):
                Pm[row, i] = np.nextafter(Pm[row, i], np.inf)
    return Pm


def _planted(n):
    """The members of _members with, where n allows it: Cs without safe constants in lanes 0 and 63 of wavefront 1; a Cs that only a
    neighbouring constant serves in wavefront 2; a member that runs away to Inf and NaN, the zero initial state, a = 0, in wavefront 0
    (all of which keep their wavefront in the lane).  Returns (params, ts0, td0, wavefronts expected in the lane, of how many)."""
    Pm = _members(n, SEED + n)
    ts0, td0 = np.full(n, 0.3), np.full(n, 0.1)
    unsafe, rescued = _golden(True), _golden(False)
    assert len(unsafe) >= 2 and rescued
    waves = (n + 63) // 64
    in_lane = waves
    Pm[1, min(3, n - 1)] = 0.0                         # a = 0
    ts0[min(5, n - 1)] = td0[min(5, n - 1)] = 0.0      # the zero state: its first year is replayed
    k = min(9, n - 1)                                  # runs away: lambda_eff = 0.3 - 0.12 Ts is negative from the start
    Pm[0, k], Pm[1, k], Pm[4, k], ts0[k] = 0.3, 0.12, 4.5, 20.0
    while not _safe(float(Pm[4, k]), DEEP_LO):
        Pm[4, k] = np.nextafter(Pm[4, k], np.inf)
    if n > 64:
        Pm[4, 64] = unsafe[0]
        if n > 127:
            Pm[4, 127] = unsafe[1]
        in_lane -= 1
    if n > 130:
        Pm[4, 130] = rescued[0]
    return Pm, ts0, td0, in_lane, waves


def _forcing(t):
    F = f_syn(t) + 0.5
    F[min(7, len(t) - 2)] = 0.0                       # a zero forcing year (+0 is inside the box)
    return F


def _ensemble(ra, orc, t, Pm, F, ts0, td0):
    e = ra.Ensemble(ra.KIND_TWO_LAYER, Pm.shape[1], orc.bounds_from_values(t))
    e.set_mode(0)
    e.set_params(Pm)
    e.set_forcing(F)
    e.set_initial(TS, ts0)
    e.set_initial(TD, td0)
    return e


def _stored(e):
    return e.get_series(1), e.get_series(2), e.status()


def _run_with(e, mode):
    """(Ts, Td, status, wavefronts in the lane, guard counts) of a whole run from the start under the switch `mode`"""
    e.rewind()
    e.clear_series()
    _counts(1)
    _lanes()
    try:
        _lane(mode)
        e.run()
        out = _stored(e)
        return out + (_lanes(), _counts(1))
    finally:
        _lane(-1)
        _counts(0)


def _same(got, want, what):
    assert_bit_equal(got[0], want[0], f"Ts, {what}")
    assert_bit_equal(got[1], want[1], f"Td, {what}")
    assert np.array_equal(got[2], want[2]), f"status, {what}"


@pytest.mark.parametrize("n", [192, 257, 63])
def test_bits_with_the_lane_equal_bits_without(ra, orc, n):
    t = _annual(31)
    Pm, ts0, td0, in_lane, waves = _planted(n)
    F = _forcing(t)
    with _ensemble(ra, orc, t, Pm, F, ts0, td0) as e:
        off = _run_with(e, 0)
        on = _run_with(e, 1)
    assert off[3] == 0 and off[4] == [0, 0, waves]
    assert on[3] == in_lane and on[4] == [0, 0, waves], (on[3], on[4])   # a wavefront in the lane still reports the chunk guard
    _same(on, off, f"{n} members: the lane against the three-instruction quotients")
    with np.errstate(all="ignore"):
        want = orc.two_layer_run(orc.bounds_from_values(t), Pm, F, ts0, td0, threads=4)
    _same(on[:2] + (on[2],), (want[0], want[1], on[2]), f"{n} members: against the oracle")
    k = min(9, n - 1)
    assert not np.isfinite(on[0][-1, k]) and on[2][k] == 1     # the runaway member got there, in the lane
    assert np.isfinite(np.delete(on[0][-1], k)).all()


def test_stale_constants(ra, orc):
    """One run in the lane, then Cs of one member changed by each way there is of writing a parameter row, then another run: the bits
    are those of the new parameters without the lane."""
    from rscm_amd import _lib as L
    lib = L.load()
    n = 128
    t = _annual(31)
    F = _forcing(t)
    Pm = _members(n, SEED + 71)
    ts0, td0 = np.full(n, 0.3), np.full(n, 0.1)

    def reference(Pnew):
        with _ensemble(ra, orc, t, Pnew, F, ts0, td0) as r:
            out = _run_with(r, 0)
        assert out[3] == 0
        return out

    def changed(k):
        Pnew = Pm.copy()
        Pnew[4, 17] = _members(1, SEED + 100 + k)[4, 0] * 1.37
        while not _safe(float(Pnew[4, 17]), DEEP_LO):
            Pnew[4, 17] = np.nextafter(Pnew[4, 17], np.inf)
        return Pnew

    def check(e, Pnew, what):
        assert np.array_equal(e.get_params(), Pnew), what
        got = _run_with(e, 1)
        assert got[3] == 2, what
        _same(got, reference(Pnew), what)

    with _ensemble(ra, orc, t, Pm, F, ts0, td0) as e:
        first = _run_with(e, 1)
        assert first[3] == 2
        # rscm_ens_set_params
        Pnew = changed(0)
        e.set_params(Pnew)
        check(e, Pnew, "after set_params")
        # a restore of a checkpoint taken under other parameters
        e.rewind()
        ck = e.checkpoint()
        Pnew = changed(1)
        ck["params"] = Pnew
        e.restore(ck)
        check(e, Pnew, "after a restore")
        # rscm_ens_gather_members into the handle
        Pnew = changed(2)
        with _ensemble(ra, orc, t, Pnew, F, ts0, td0) as src:
            src.branch(e, np.arange(n, dtype=np.int64))
        e.set_initial(TS, ts0)
        e.set_initial(TD, td0)
        check(e, Pnew, "after gather_members")
        # rscm_ens_sample_lhs: every row new; whatever the draw, the bits are the unlaned run's
        lo, hi = BASE * 0.8, BASE * 1.25
        lo[1], hi[1] = 0.0, 0.05
        e.sample_lhs(SEED, lo, hi)
        Pnew = e.get_params()
        assert not np.array_equal(Pnew[4], Pm[4])
        got = _run_with(e, 1)
        _same(got, reference(Pnew), "after sample_lhs")
        # a write through the exposed device pointer: no entry point sees it
        ptr = C.c_void_p()
        L.check(lib.rscm_ens_params_devptr(e._h, C.byref(ptr)))
        _same(_run_with(e, 1), got, "exposed, unchanged")
        for k in (3, 4):   # twice: the constants are formed again before every run of such a handle
            Pnew = np.ascontiguousarray(Pnew.copy())
            Pnew[4, 17] = changed(k)[4, 17]
            L.check(lib.rscm_gpu_copy_to_device(0, ptr, Pnew.ctypes.data_as(C.c_void_p), Pnew.nbytes))
            assert np.array_equal(e.get_params(), Pnew)
            _same(_run_with(e, 1), reference(Pnew), "after a write through the device pointer")

    # a sampler's proposals: the proposal kernel writes the evaluator's block (rows 0 and 4 sampled), then the evaluator runs on its own
    with _ensemble(ra, orc, t, Pm, F, ts0, td0) as ev:
        assert _run_with(ev, 1)[3] == 2
        ev.rewind()
        rows = np.array([0, 4], dtype=np.int32)
        kinds = np.zeros(2, dtype=np.int32)
        a, b = L.f64([0.8, 6.5]), L.f64([1.25, 10.0])
        obs_var = np.array([1, 1], dtype=np.int32)
        obs_t = np.array([5, 20], dtype=np.int32)
        val, sig = L.f64([0.5, 0.9]), L.f64([0.2, 0.2])
        s = C.c_void_p()
        ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        L.check(lib.rscm_sampler_create(ev._h, 2 * n, 2, ip(rows), L.dptr(L.f64(BASE)), ip(kinds), L.dptr(a), L.dptr(b), None, None, 2, ip(obs_var),
                                        ip(obs_t), L.dptr(val), L.dptr(sig), 0, 2.0, 11, C.byref(s)))
        try:
            pos = np.random.default_rng(5).uniform([0.8, 6.5], [1.25, 10.0], (2 * n, 2))
            L.check(lib.rscm_sampler_set_positions(s, L.dptr(L.f64(pos))))
            L.check(lib.rscm_sampler_iterate(s, 1))
            L.check(lib.rscm_sampler_sync(s))
        finally:
            L.check(lib.rscm_sampler_destroy(s))
        Pnew = ev.get_params()
        assert not np.array_equal(Pnew[4], Pm[4])
        ev.set_initial(TS, ts0)
        ev.set_initial(TD, td0)
        got = _run_with(ev, 1)
        _same(got, reference(Pnew), "after a sampler's proposals")


def test_cut_runs_and_defaults(ra, orc):
    """The smallest cut run (65 536 + 64 members, 192 steps, rscm_gpu_set_run_plan(1)) with the lane against the plain launch without
    it -- under the default switch a run of that length does not take the lane, nor does one of 100 steps: no constants are formed;
    a mix handle and the fused likelihood never take the lane."""
    from rscm_amd import _lib as L
    lib = L.load()
    n, points = 65536 + 64, 193
    rng = np.random.default_rng(SEED + 73)
    Pm = np.repeat(BASE[:, None], n, axis=1) * rng.uniform(0.8, 1.25, (6, n))
    Pm[1] = rng.uniform(0.0, 0.05, n)
    t = _annual(points)
    F = _forcing(t)
    ts0, td0 = np.full(n, 0.3), np.full(n, 0.1)
    with _ensemble(ra, orc, t, Pm, F, ts0, td0) as e:
        try:
            L.check(lib.rscm_gpu_set_run_plan(0))
            plain = _run_with(e, 0)
            L.check(lib.rscm_gpu_set_run_plan(1))
            by_default = _run_with(e, -1)
            assert e.last_run_plan() == (2, 3) and by_default[3] == 0   # 192 steps do not earn the constants kernel back
            cut = _run_with(e, 1)
            assert e.last_run_plan() == (2, 3)
        finally:
            L.check(lib.rscm_gpu_set_run_plan(-1))
        waves = (n + 63) // 64
        assert plain[3] == 0 and plain[4] == [0, 0, waves]
        assert cut[4] == [0, 0, 3 * waves]
        assert 0.8 * 3 * waves < cut[3] < 3 * waves and cut[3] % 3 == 0   # most wavefronts, in every chunk alike
        _same(cut, plain, "the cut run in the lane against the plain launch without it")
        _same(by_default, plain, "the cut run under the default switch")
    # a 100-step run under the default switch
    n = 128
    Pm = _members(n, SEED + 79)
    ts0, td0 = np.full(n, 0.3), np.full(n, 0.1)
    t = _annual(101)
    F = _forcing(t)
    with _ensemble(ra, orc, t, Pm, F, ts0, td0) as e:
        short = _run_with(e, -1)
        assert short[3] == 0 and short[4] == [0, 0, 2]
        forced = _run_with(e, 1)
        assert forced[3] == 2
        _same(forced, short, "100 steps: the lane by the switch against the default")
        # the fused likelihood of the same handle
        e.rewind()
        _counts(1)
        _lanes()
        try:
            _lane(1)
            e.run_loglik([TS, TD], np.array([5, 50], dtype=np.int32), np.array([0.5, 0.4]), np.array([0.2, 0.2]), False)
            assert _lanes() == 0 and _counts(1) == [0, 0, 2]
        finally:
            _lane(-1)
            _counts(0)
    # a mix handle
    mix = ra.Ensemble(ra.KIND_TWO_LAYER, n, orc.bounds_from_values(t), forcing_components=2)
    with mix as e:
        e.set_mode(0)
        e.set_params(np.vstack([Pm, np.full((2, n), 0.5)]))
        e.set_forcing(np.stack([F, F])[None])
        e.set_initial(TS, ts0)
        e.set_initial(TD, td0)
        got = _run_with(e, 1)
        assert got[3] == 0
        _same(got, forced, "a mix of two halves of the same forcing")
