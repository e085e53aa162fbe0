"""Reference periods on the device (ABI minor 9; DESIGN.md section 7, "Reference periods"): a target variable observed as an anomaly
from a reference period is scored against x - b, b the member's own mean over the period's rows.

  * the stored path (rscm_ens_loglik_ref, loglik_kernel) against the numpy restatement of tests/host_likelihood.py on the fetched
    series: bit for bit unnormalised (add, subtract, multiply, divide only; the library is built with contraction off), rtol 1e-13
    normalised (the device's log is not glibc's: the tolerance tests/test_gpu_parity.py applies to the normalised likelihood);
  * the fused two-layer run + likelihood (rscm_ens_run_loglik_ref, two_layer_ref_kernel) against the stored path, bit for bit in both
    arithmetic modes;
  * the device sampler (rscm_sampler_set_reference) against log prior + that likelihood, and against the host sampler's posterior.
"""
import ctypes as C

import numpy as np
import pytest

from tests import host_likelihood as hl
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import TL_RANGES, assert_bit_equal, axis_values, emissions_syn, f_syn, two_layer_params
from tests.host_indicators import anomaly, baseline

pytestmark = pytest.mark.gpu

TS, TD = 1, 2
NAMES = ["lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep"]
DEFAULTS = dict(lambda0=1.0, a=0.0, efficacy=1.0, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)


def _rows(a, b, step=1):
    return np.arange(a - 1750, b - 1750 + 1, step, dtype=np.int32)


def _obs(groups, seed=1):
    """(obs_var, obs_tidx, obs_value, obs_sigma) for [(var, rows), ...] in that order; values near typical anomalies"""
    rng = np.random.default_rng(seed)
    ov = np.concatenate([np.full(len(r), v, dtype=np.int32) for v, r in groups])
    ot = np.concatenate([np.asarray(r, dtype=np.int32) for _, r in groups])
    return ov, ot, rng.normal(0.4, 0.4, len(ot)), rng.uniform(0.05, 0.5, len(ot))


# name -> (observation groups, reference); rows on the 1750-2500 axis (row = year - 1750)
CASES = {
    "period 1850-1900, annual observations 1850..2020": ([(TS, _rows(1850, 2020))], {TS: (100, 151)}),
    "observations only after the period": ([(TS, _rows(1910, 2020, 10))], {TS: (100, 151)}),
    "an observation at the period's last row": ([(TS, [150, 200])], {TS: (100, 151)}),
    "a period that starts at row 0": ([(TS, [0, 10, 30, 31, 100])], {TS: (0, 31)}),
    "Ts with a period, Td without": ([(TS, _rows(1800, 2000, 25)), (TD, [0, 100, 125, 400, 750])], {TS: (100, 151)}),
    "both with different periods, the deep group first": ([(TD, [0, 60, 80, 81, 300]), (TS, _rows(1840, 2020, 20))],
                                                            {TS: (100, 151), TD: (50, 81)}),
    "a strided period": ([(TS, [90, 100, 140, 141, 500])], {TS: (100, 151, 10)}),
}


def _ensemble(ra, n, b, P, F, mode=0, store=True, scen=None, init=(0.0, 0.0)):
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, b, store_series=store)
    e.set_mode(mode)
    e.set_params(P)
    e.set_forcing(F, scen)
    e.set_initial(TS, init[0])
    e.set_initial(TD, init[1])
    return e


def _params_with_failures(n):
    """An LHS draw in which some members run away (lambda0 - a Ts < 0 overflows), plus members with +inf / NaN parameters"""
    P = two_layer_params(n)
    P[1, 5] = 5.0          # runaway feedback: overflows within decades
    P[1, 6] = 1.0
    P[4, 7] = np.inf       # infinite heat capacity
    P[0, 8] = np.nan
    P[5, 9] = np.nan
    P[3, 10] = np.inf
    return P


def _check_against_numpy(got, want, normalize, what):
    assert (np.isneginf(got) == np.isneginf(want)).all(), f"{what}: -inf placement"
    assert not np.isnan(got).any() and not np.isposinf(got).any(), what
    if normalize:
        fin = np.isfinite(want)
        assert np.allclose(got[fin], want[fin], rtol=1e-13, atol=0), what
    else:
        assert_bit_equal(got, want, what)


# ------------------------------------------------------------------------------------------------ stored path vs numpy
def test_stored_loglik_with_reference_periods_equals_numpy(ra):
    t = axis_values()
    b = np.append(t, t[-1] + 1.0)
    n = 4000
    P = _params_with_failures(n)
    with _ensemble(ra, n, b, P, f_syn(t), init=(0.1, -0.05)) as e:
        e.run()
        series = {TS: e.get_series(TS), TD: e.get_series(TD)}
        # the baseline of the statistics side: the same bits as the likelihood's b, and left alone by the likelihood
        e.set_baseline(TS, 100, 151)
        assert_bit_equal(e.baseline(), hl.reference_baseline(series[TS], (100, 151)), "b of 1850-1900")
        e.set_baseline(TS, 100, 151, 10)
        assert_bit_equal(e.baseline(), hl.reference_baseline(series[TS], (100, 151, 10)), "b of a strided period")
        e.set_baseline(TD, 10, 20)
        kept = e.baseline()
        n_failed = None
        for name, (groups, reference) in CASES.items():
            ov, ot, val, sig = _obs(groups)
            for normalize in (False, True):
                got = e.loglik(ov, ot, val, sig, normalize, reference=reference)
                want = hl.loglik(series, ov, ot, val, sig, normalize, reference)
                fin = np.isfinite(want) & np.isfinite(got)
                print(f"{name} normalize={normalize}: {np.isneginf(want).sum()} failed members of {n}, "
                      f"max |got - want| = {np.abs(got[fin] - want[fin]).max():.3e}")
                _check_against_numpy(got, want, normalize, f"{name} normalize={normalize}")
                n_failed = int(np.isneginf(want).sum())
                # the conditions on the input set: failed members are in it, and at least half of the members are finite
                assert n_failed >= 1 and np.isfinite(want).sum() >= n // 2
                # ... and the period matters
                assert not np.array_equal(got, e.loglik(ov, ot, val, sig, normalize))
            dev = e.loglik(ov, ot, val, sig, False, on_device=True, reference=reference)
            assert_bit_equal(dev.to_host(), e.loglik(ov, ot, val, sig, False, reference=reference), f"{name}: on_device")
            # the same kernel scores a table without periods: its bits are the restatement's too, group boundaries included
            assert_bit_equal(e.loglik(ov, ot, val, sig, False), hl.loglik(series, ov, ot, val, sig, False, None), f"{name}: no period")
        none = np.empty(0, dtype=np.int32)
        assert_bit_equal(e.loglik(none, none, np.empty(0), np.empty(0), False), hl.loglik(series, none, none, [], [], False, None),
                         "no observations")
        assert_bit_equal(e.baseline(), kept, "the handle's own baseline after likelihood calls")
        # a member that is not finite inside the period only (not at an observed row) is a failed member
        for member, bad in ((42, np.nan), (43, np.inf)):
            row = series[TS][120].copy()
            row[member] = bad
            e.set_state(TS, 120, row)
            series[TS][120] = row
        ov, ot, val, sig = _obs([(TS, [20, 30, 200])])
        plain = e.loglik(ov, ot, val, sig)
        with_period = e.loglik(ov, ot, val, sig, reference={TS: (100, 151)})
        assert np.isfinite(plain[[42, 43]]).all() and np.isneginf(with_period[[42, 43]]).all()
        assert_bit_equal(with_period, hl.loglik(series, ov, ot, val, sig, False, {TS: (100, 151)}), "a NaN and an inf inside the period")


# ------------------------------------------------------------------------------------------------ fused == stored
@pytest.mark.parametrize("mode", [0, 1])
def test_fused_run_loglik_with_reference_periods_equals_stored_path(ra, mode):
    """rscm_ens_run_loglik_ref on a handle without series == rscm_ens_run + rscm_ens_loglik_ref, bit for bit."""
    t = axis_values()
    b = np.append(t, t[-1] + 1.0)
    n = 3000
    P, F = _params_with_failures(n), f_syn(t)
    with _ensemble(ra, n, b, P, F, mode, init=(0.1, -0.05)) as stored, _ensemble(ra, n, b, P, F, mode, store=False, init=(0.1, -0.05)) as fused:
        stored.run()
        st = stored.status()
        for name, (groups, reference) in CASES.items():
            ov, ot, val, sig = _obs(groups)
            for normalize in (False, True):
                want = stored.loglik(ov, ot, val, sig, normalize, reference=reference)
                got = fused.run_loglik(ov, ot, val, sig, normalize, reference=reference)
                assert_bit_equal(got, want, f"mode {mode}, {name}, normalize {normalize}")
                assert (fused.status() == st).all() and fused.time_index == 0
                assert (st != 0).sum() > 0 and np.isneginf(got).sum() >= 1 and np.isfinite(got).sum() >= n // 2
            dev = fused.run_loglik(ov, ot, val, sig, False, on_device=True, reference=reference)
            assert_bit_equal(dev.to_host(), stored.loglik(ov, ot, val, sig, False, reference=reference), f"{name}: on_device")
        # without a period the new keyword and the new entry point return the bits of the old call
        ov, ot, val, sig = _obs(CASES["Ts with a period, Td without"][0])
        old = fused.run_loglik(ov, ot, val, sig)
        assert_bit_equal(fused.run_loglik(ov, ot, val, sig, reference=None), old)
        assert_bit_equal(fused.run_loglik(ov, ot, val, sig, reference={}), old)
        assert_bit_equal(stored.loglik(ov, ot, val, sig, reference=None), stored.loglik(ov, ot, val, sig))
        from rscm_amd import _lib as L
        out = np.empty(n)
        L.check(fused._lib.rscm_ens_run_loglik_ref(fused._h, len(ov), L.iptr(ov), L.iptr(ot), L.dptr(val), L.dptr(sig), 0, 0, None, None,
                                                   None, None, L.dptr(out)))
        assert_bit_equal(out, old, "rscm_ens_run_loglik_ref with n_ref == 0")
        L.check(stored._lib.rscm_ens_loglik_ref(stored._h, len(ov), L.iptr(ov), L.iptr(ot), L.dptr(val), L.dptr(sig), 0, 0, None, None,
                                                None, None, L.dptr(out)))
        assert_bit_equal(out, stored.loglik(ov, ot, val, sig), "rscm_ens_loglik_ref with n_ref == 0")
        assert_bit_equal(fused.run_loglik(ov, ot, val, sig), old, "a period-free call after calls with periods")


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_reference_periods_without_lds_forcing_and_at_1e5_members(ra, mode):
    t = axis_values()
    b = np.append(t, t[-1] + 1.0)
    # more scenarios than fit in LDS (40 * 750 * 8 B = 240 KB): the forcing is read through L2
    n, S = 300, 40
    rng = np.random.default_rng(5)
    P = two_layer_params(n)
    F = np.stack([f_syn(t) * rng.uniform(0.2, 1.2) for _ in range(S)])
    scen = rng.integers(0, S, n).astype(np.int32)
    name = "both with different periods, the deep group first"
    groups, reference = CASES[name]
    ov, ot, val, sig = _obs(groups)
    with _ensemble(ra, n, b, P, F, mode, scen=scen) as stored, _ensemble(ra, n, b, P, F, mode, store=False, scen=scen) as fused:
        stored.run()
        for normalize in (False, True):
            assert_bit_equal(fused.run_loglik(ov, ot, val, sig, normalize, reference=reference),
                             stored.loglik(ov, ot, val, sig, normalize, reference=reference), f"L2 forcing, mode {mode}")
        assert (fused.status() == stored.status()).all() and fused.time_index == 0
    n = 100_000
    P, F = _params_with_failures(n), f_syn(t)   # (the plain draw's runaway members fail after the last observed row)
    groups, reference = CASES["period 1850-1900, annual observations 1850..2020"]
    ov, ot, val, sig = _obs(groups)
    with _ensemble(ra, n, b, P, F, mode) as stored, _ensemble(ra, n, b, P, F, mode, store=False) as fused:
        stored.run()
        want = stored.loglik(ov, ot, val, sig, reference=reference)
        got = fused.run_loglik(ov, ot, val, sig, reference=reference)
        assert_bit_equal(got, want, f"1e5 members, mode {mode}")
        assert (fused.status() == stored.status()).all() and fused.time_index == 0
        assert np.isneginf(got).sum() >= 1 and np.isfinite(got).sum() >= n // 2


# ------------------------------------------------------------------------------------------------ known answer
def test_anomalies_of_a_member_score_zero_for_that_member(ra):
    t = axis_values()
    b = np.append(t, t[-1] + 1.0)
    n = 2000
    P, F = two_layer_params(n), f_syn(t)
    ot = _rows(1850, 2020, 5)
    ov = np.full(len(ot), TS, dtype=np.int32)
    sig = np.full(len(ot), 0.1)
    with _ensemble(ra, n, b, P, F) as e, _ensemble(ra, n, b, P, F, store=False) as fused:
        e.run()
        ts = e.get_series(TS)
        whole = np.flatnonzero(np.isfinite(ts).all(axis=0))   # members that stay finite to the end of the axis
        k = int(whole[len(whole) // 2])
        bk = baseline(ts[100:151])
        val = anomaly(ts[ot], bk)[:, k]
        assert bk[k] != 0.0
        for ll in (e.loglik(ov, ot, val, sig, reference={TS: (100, 151)}), fused.run_loglik(ov, ot, val, sig, reference={TS: (100, 151)})):
            assert ll[k] == 0.0 and int(np.argmax(ll)) == k and (np.delete(ll, k) < 0).all()
        assert e.loglik(ov, ot, val, sig)[k] < 0.0 and fused.run_loglik(ov, ot, val, sig)[k] < 0.0


# ------------------------------------------------------------------------------------------------ errors
def test_reference_period_error_conventions(ra):
    from rscm_amd import RscmGpuError
    from rscm_amd import _lib as L
    t = axis_values(1750, 1900)
    b = np.append(t, t[-1] + 1.0)
    n = 300
    P, F = two_layer_params(n), f_syn(t)
    ov, ot, val, sig = _obs([(TS, [10, 60, 100])])
    with _ensemble(ra, n, b, P, F) as e:
        e.run(110)                                     # rows beyond index 110 are not computed yet
        assert np.isfinite(e.loglik(ov, ot, val, sig, reference={TS: (50, 101)})).any()
        assert np.isneginf(e.loglik(ov, ot, val, sig, reference={TS: (100, 131)})).all()
        assert np.isneginf(e.loglik(ov, ot, val, sig, on_device=True, reference={TS: (100, 131)}).to_host()).all()
        e.run()
        for call in (e.loglik, e.run_loglik):
            with pytest.raises(RscmGpuError, match="has a period already") as err:       # a variable twice
                call(ov, ot, val, sig, reference={TS: (50, 101), "Surface Temperature": (20, 31)})
            assert err.value.code == L.ERR_INVALID
            with pytest.raises(RscmGpuError, match="has no observation") as err:
                call(ov, ot, val, sig, reference={TD: (50, 101)})
            assert err.value.code == L.ERR_INVALID
            for rows in ((50, 50), (-1, 10), (100, 153), (10, 20, 0)):
                with pytest.raises(RscmGpuError, match="bad time range") as err:
                    call(ov, ot, val, sig, reference={TS: rows})
                assert err.value.code == L.ERR_INVALID
            e.rewind()
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, b, window_rows=8, output_stride=5, output_vars=["Surface Temperature"]) as e:
        e.set_params(P)
        e.set_forcing(F)
        e.set_initial(TS, 0.0)
        e.set_initial(TD, 0.0)
        for _ in range(len(t) - 1):
            e.step()
        # the output store holds every fifth row: a period over those rows is resident, one with stride 1 is not
        obs = ([TS, TS], [140, 145], [0.1, 0.2], [0.3, 0.3])
        assert np.isfinite(e.loglik(*obs, reference={TS: (100, 131, 5)})).any()
        with pytest.raises(RscmGpuError, match="not resident") as err:
            e.loglik(*obs, reference={TS: (100, 131)})
        assert err.value.code == L.ERR_STATE


# ------------------------------------------------------------------------------------------------ the sampler at the C level
def _c_sampler(ens, W, rows, base, lo, hi, obs, seed=5, normalize=0):
    from rscm_amd import _lib as L
    ov, ot, val, sig = obs
    rows = np.asarray(rows, dtype=np.int32)
    kinds = np.zeros(len(rows), dtype=np.int32)
    base, lo, hi, val, sig = (L.f64(x) for x in (base, lo, hi, val, sig))
    ov, ot = np.asarray(ov, dtype=np.int32), np.asarray(ot, dtype=np.int32)
    h = C.c_void_p()
    L.check(ens._lib.rscm_sampler_create(ens._h, W, len(rows), L.iptr(rows), L.dptr(base), L.iptr(kinds), L.dptr(lo), L.dptr(hi), None, None,
                                         len(ov), L.iptr(ov), L.iptr(ot), L.dptr(val), L.dptr(sig), normalize, 2.0, C.c_uint64(seed), C.byref(h)))
    return h


def _set_reference(lib, h, reference):
    from rscm_amd import _lib as L
    rv, rb, re_, rs = (np.asarray(x, dtype=np.int32) for x in zip(*[(v, r[0], r[1], r[2] if len(r) > 2 else 1) for v, r in reference.items()]))
    return lib.rscm_sampler_set_reference(h, len(rv), None, L.iptr(rv), L.iptr(rb), L.iptr(re_), L.iptr(rs))


def _log_prob(lib, h, pos):
    from rscm_amd import _lib as L
    pos = L.f64(pos)
    L.check(lib.rscm_sampler_set_positions(h, L.dptr(pos)))
    logp = np.empty(pos.shape[0])
    L.check(lib.rscm_sampler_get(h, None, L.dptr(logp), None, None))
    return logp


def test_sampler_scores_are_log_prior_plus_the_reference_period_likelihood(ra):
    """After rscm_sampler_set_positions the log probabilities are log prior + run_loglik(..., reference=...) of the positions, bit
    for bit: fused two-layer evaluator; rscm_sampler_set_reference after the positions are set is RSCM_ERR_STATE."""
    from rscm_amd import calibrate as cal
    from rscm_amd import _lib as L
    t = axis_values()
    b = np.append(t, t[-1] + 1.0)
    W = 512
    lo, hi = np.array(TL_RANGES).T
    params = cal.ParameterSet()
    for k, (a_, b_) in zip(NAMES, TL_RANGES):
        params.add(k, cal.Uniform(a_, b_))
    pos = params.sample_random(W, np.random.default_rng(4))
    pos[3, 0] = 2.0   # outside the prior
    groups, reference = CASES["both with different periods, the deep group first"]
    obs = _obs(groups)
    base = np.array([DEFAULTS[k] for k in NAMES])
    lp = params.log_prior_batch(pos)
    for normalize in (0, 1):
        with _ensemble(ra, W // 2, b, np.repeat(base[:, None], W // 2, axis=1), f_syn(t), store=False) as ev, \
                _ensemble(ra, W, b, np.ascontiguousarray(pos.T), f_syn(t), store=False) as whole:
            lib = ev._lib
            h = _c_sampler(ev, W, np.arange(6), base, lo, hi, obs, normalize=normalize)
            try:
                L.check(_set_reference(lib, h, reference))
                got = _log_prob(lib, h, pos)
                ll = whole.run_loglik(*obs, bool(normalize), reference=reference)
                with np.errstate(invalid="ignore"):
                    want = np.where(np.isfinite(lp), lp + ll, -np.inf)
                assert_bit_equal(got, want, f"fused evaluator, normalize {normalize}")
                assert got[3] == -np.inf and np.isfinite(got).sum() > W // 2
                assert not np.array_equal(got, np.where(np.isfinite(lp), lp + whole.run_loglik(*obs, bool(normalize)), -np.inf))
                assert _set_reference(lib, h, reference) == L.ERR_STATE          # positions are set
                assert lib.rscm_sampler_set_reference(h, 0, None, None, None, None, None) == L.ERR_STATE
            finally:
                lib.rscm_sampler_destroy(h)
            # set before the positions: a duplicate variable, a variable without observations, an owner on a plain sampler
            h = _c_sampler(ev, W, np.arange(6), base, lo, hi, _obs([(TS, [100, 200])]))
            try:
                one = np.array([TS, TS], dtype=np.int32), np.array([10, 40], dtype=np.int32), np.array([20, 50], dtype=np.int32), np.ones(2, dtype=np.int32)
                assert lib.rscm_sampler_set_reference(h, 2, None, *(L.iptr(x) for x in one)) == L.ERR_INVALID
                assert _set_reference(lib, h, {TD: (10, 20)}) == L.ERR_INVALID
                assert lib.rscm_sampler_set_reference(h, 1, L.iptr(one[3]), *(L.iptr(x) for x in one)) == L.ERR_INVALID
                # n_ref == 0: the scores of a sampler that was never given a period
                L.check(_set_reference(lib, h, {TS: (100, 151)}))
                L.check(lib.rscm_sampler_set_reference(h, 0, None, None, None, None, None))
                got = _log_prob(lib, h, pos)
                ll = whole.run_loglik(*_obs([(TS, [100, 200])]))
                assert_bit_equal(got, np.where(np.isfinite(lp), lp + ll, -np.inf), "periods removed again")
            finally:
                lib.rscm_sampler_destroy(h)


def test_sampler_scores_with_a_stored_series_evaluator(ra):
    """The coupled kind has no fused likelihood: its sampler runs a half and scores the stored series with loglik_kernel, from the
    one table rscm_sampler_set_reference lays out again -- with the periods, and without them once they are removed."""
    from rscm_amd import calibrate as cal
    from rscm_amd import _lib as L
    t = axis_values(1750, 1900)
    b = np.append(t, t[-1] + 1.0)
    W = 256
    base = np.array([1.0, 0.02, 1.2, 0.7, 8.0, 100.0, 25.0, 278.0, 0.02, 3.7])
    rows, lo, hi = [0, 6], np.array([0.8, 15.0]), np.array([1.5, 40.0])
    params = cal.ParameterSet().add("lambda0", cal.Uniform(0.8, 1.5)).add("tau", cal.Uniform(15.0, 40.0))
    pos = params.sample_random(W, np.random.default_rng(7))
    lp = params.log_prior_batch(pos)

    def coupled(n, P):
        e = ra.Ensemble(ra.KIND_COUPLED, n, b)
        e.set_params(P)
        e.set_forcing(emissions_syn(t))
        for v, x in ((1, 0.0), (2, 0.0), (3, 278.0), (4, 0.0), (5, 0.0)):
            e.set_initial(v, x)
        return e

    full = np.repeat(base[:, None], W, axis=1)
    full[rows, :] = pos.T
    with coupled(W // 2, np.repeat(base[:, None], W // 2, axis=1)) as ev, coupled(W, full) as whole:
        ts_id, co2_id = ev._var("Surface Temperature"), ev._var("Atmospheric Concentration|CO2")
        obs = _obs([(ts_id, [40, 80, 100, 120, 150]), (co2_id, [50, 150])])
        obs = (obs[0], obs[1], np.where(obs[0] == co2_id, 300.0, obs[2]), np.where(obs[0] == co2_id, 20.0, obs[3]))
        reference = {ts_id: (80, 111)}
        lib = ev._lib
        h = _c_sampler(ev, W, rows, base, lo, hi, obs)
        try:
            L.check(_set_reference(lib, h, reference))
            got = _log_prob(lib, h, pos)
        finally:
            lib.rscm_sampler_destroy(h)
        h = _c_sampler(ev, W, rows, base, lo, hi, obs)
        try:
            never = _log_prob(lib, h, pos)
        finally:
            lib.rscm_sampler_destroy(h)
        h = _c_sampler(ev, W, rows, base, lo, hi, obs)
        try:
            L.check(_set_reference(lib, h, reference))
            L.check(lib.rscm_sampler_set_reference(h, 0, None, None, None, None, None))
            removed = _log_prob(lib, h, pos)
        finally:
            lib.rscm_sampler_destroy(h)
        whole.run()
        ll = whole.loglik(*obs, reference=reference)
        assert_bit_equal(got, lp + ll, "stored-series evaluator")
        assert np.isfinite(got).all() and not np.array_equal(got, lp + whole.loglik(*obs))
        assert_bit_equal(never, lp + whole.loglik(*obs), "stored-series evaluator: never given a period")
        assert_bit_equal(removed, lp + whole.loglik(*obs), "stored-series evaluator: periods removed again")


# ------------------------------------------------------------------------------------------------ the sampler through the Python front
@pytest.fixture(scope="module")
def problem(ra):
    """tests/test_gpu_sampler.py's problem with the truth run's anomalies from 1800-1850 as the target: 1750-1900 axis, observed
    1780..1900 step 10 -- before, inside and after the period."""
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    t = np.arange(1750.0, 1901.0)
    axis = core.TimeAxis.from_values(t)
    F = 4.0 * (1.0 - np.exp(-(t - 1750.0) / 60.0))
    b = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
         .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(F, axis, "W/m^2", core.InterpolationStrategy.Linear))
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))
    names, ranges = ["lambda0", "efficacy"], [(0.8, 1.5), (1.0, 1.8)]
    runner = cal.ModelRunner(b, names, ["Surface Temperature"])
    truth = runner.run([fixed[k] for k in names])["Surface Temperature"]
    base = baseline(np.array([[truth[float(y)]] for y in range(1800, 1851)]))[0]
    target, absolute = cal.Target(), cal.Target()
    for yr in range(1780, 1901, 10):
        target.add_observation("Surface Temperature", float(yr), truth[float(yr)] - base, 0.05)
        absolute.add_observation("Surface Temperature", float(yr), truth[float(yr)] - base, 0.05)
    target.set_reference_period("Surface Temperature", 1800, 1850)
    params = cal.ParameterSet()
    for k, (lo, hi) in zip(names, ranges):
        params.add(k, cal.Uniform(lo, hi))
    yield cal, runner, target, absolute, params, [fixed[k] for k in names]
    runner.close()


def test_device_sampler_scores_equal_host_scores_with_a_reference_period(problem):
    cal, runner, target, absolute, params, truth = problem
    lik = cal.GaussianLikelihood()
    pos = params.sample_random(64, np.random.default_rng(0))
    pos[5, 0] = 2.0  # outside Uniform(0.8, 1.5)
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target)
    host = cal.EnsembleSampler(params, runner, lik, target)
    want = host.log_posterior_batch(pos)
    assert host.log_posterior_batch(np.array([truth]))[0] == params.log_prior(truth)   # the truth's anomalies fit exactly: ln L = 0
    # one sweep, then compare only the walkers that did not move: their scores are the initial ones
    chain = dev.run(1, cal.WalkerInit.explicit(pos), n_walkers=64, seed=1)
    got_pos, got_lp = chain.flat_samples(), chain.flat_log_probs()
    same = (got_pos == pos).all(axis=1)
    assert same.any() and (~same).any()
    assert np.array_equal(got_lp[same], want[same]) and want[5] == -np.inf
    moved = host.log_posterior_batch(got_pos[~same])
    assert np.array_equal(got_lp[~same], moved) and np.isfinite(moved).all()  # accepted proposals carry their own exact score
    # the same seed gives the same chain; the same target without its period gives another
    a = dev.run(5, cal.WalkerInit.explicit(pos), n_walkers=64, seed=1)
    again = dev.run(5, cal.WalkerInit.explicit(pos), n_walkers=64, seed=1)
    assert np.array_equal(a.flat_samples(), again.flat_samples()) and np.array_equal(a.flat_log_probs(), again.flat_log_probs())
    other = cal.DeviceEnsembleSampler(params, runner, lik, absolute).run(5, cal.WalkerInit.explicit(pos), n_walkers=64, seed=1)
    assert not np.array_equal(other.flat_samples(), a.flat_samples())
    # a period with no row on the model axis: a missing time
    nowhere = cal.Target().add_observation("Surface Temperature", 1800.0, 0.1, 0.1).set_reference_period("Surface Temperature", 1600, 1700)
    with pytest.raises(KeyError):
        cal.DeviceEnsembleSampler(params, runner, lik, nowhere).run(1, cal.WalkerInit.explicit(pos), n_walkers=64, seed=1)
    assert np.isneginf(runner.log_likelihood_batch(pos, nowhere, lik)).all()


def test_device_sampler_recovers_the_truth_from_anomalies(problem):
    """tests/test_gpu_sampler.py::test_device_sampler_matches_host_posterior with the reference-period target: 512 walkers, 300
    sweeps, thin 10, discard 15, the same bands."""
    cal, runner, target, absolute, params, truth = problem
    lik = cal.GaussianLikelihood()
    init = cal.WalkerInit.from_prior()
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target)
    cd = dev.run(300, init, thin=10, n_walkers=512, seed=3, rng=np.random.default_rng(5))
    host = cal.EnsembleSampler(params, runner, lik, target)
    ch = host.run(300, init, thin=10, n_walkers=512, rng=np.random.default_rng(6))
    xd, xh = cd.flat_samples(discard=15), ch.flat_samples(discard=15)
    assert xd.shape == xh.shape == (15 * 512, 2)
    for j in range(2):
        sd = max(xd[:, j].std(), xh[:, j].std())
        print(f"{params.param_names[j]}: device {xd[:, j].mean():.4f} +- {xd[:, j].std():.4f}, host {xh[:, j].mean():.4f} +- {xh[:, j].std():.4f}, "
              f"truth {truth[j]}")
        assert abs(xd[:, j].mean() - truth[j]) < 3 * sd
        assert abs(xd[:, j].mean() - xh[:, j].mean()) < 0.15 * sd
        assert 0.8 < xd[:, j].std() / xh[:, j].std() < 1.25
    again = dev.run(300, init, thin=10, n_walkers=512, seed=3, rng=np.random.default_rng(5))
    assert np.array_equal(again.flat_samples(), cd.flat_samples())


def test_graph_sampler_scores_with_a_reference_period(ra):
    """A graph of linked ensembles as the evaluator (rscm_sampler_create_graph + rscm_sampler_set_reference with owners): the scores
    of walkers that did not move, and of accepted proposals, are log prior + the runner's reference-period likelihood."""
    from rscm_amd import calibrate as cal
    import rscm_amd.core as core
    from rscm_amd.components import CarbonCycleBuilder, CO2ERFBuilder
    from rscm_amd.two_layer import TwoLayerBuilder
    t = np.arange(1750.0, 1851.0)
    axis = core.TimeAxis.from_values(t)
    tl = dict(lambda0=1.1, a=0.0, efficacy=1.2, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    schema = core.VariableSchema()
    for v in ["Emissions|CO2|Anthropogenic", "Surface Temperature", "Deep Ocean Temperature", "Atmospheric Concentration|CO2",
              "Cumulative Land Uptake", "Cumulative Emissions|CO2", "Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other"]:
        schema.add_variable(v, "")
    schema.add_aggregate("Effective Radiative Forcing", "W/m^2", "Sum", ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other"])
    b = (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
         .with_rust_component(CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.05)).build())
         .with_rust_component(CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=278.0)).build())
         .with_rust_component(TwoLayerBuilder.from_parameters(tl).build())
         .with_exogenous_variable("Emissions|CO2|Anthropogenic", core.Timeseries(emissions_syn(t) + 1.0, axis, "", core.InterpolationStrategy.Linear))
         .with_exogenous_variable("Effective Radiative Forcing|Other", core.Timeseries(0.2 * np.sin(t / 9.0), axis, "", core.InterpolationStrategy.Linear))
         .with_initial_values({"Cumulative Land Uptake": 0.0, "Cumulative Emissions|CO2": 0.0, "Atmospheric Concentration|CO2": 278.0,
                               "Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))
    runner = cal.ModelRunner(b, ["TwoLayer.lambda0", "tau"], ["Surface Temperature", "Atmospheric Concentration|CO2"])
    assert runner._graph
    truth = runner.run([1.25, 30.0])
    base = baseline(np.array([[truth["Surface Temperature"][float(y)]] for y in range(1790, 1821)]))[0]
    target, absolute = cal.Target(), cal.Target()
    for tg in (target, absolute):
        for y in range(1780, 1841, 10):   # the period 1790-1820 ends before the last observation; CO2 is observed later still
            tg.add_observation("Surface Temperature", float(y), truth["Surface Temperature"][float(y)] - base, 0.01)
        for y in range(1780, 1851, 10):
            tg.add_observation("Atmospheric Concentration|CO2", float(y), truth["Atmospheric Concentration|CO2"][float(y)], 0.2)
    target.set_reference_period("Surface Temperature", 1790, 1820)
    params = cal.ParameterSet().add("TwoLayer.lambda0", cal.Uniform(0.8, 1.6)).add("tau", cal.Uniform(15.0, 45.0))
    lik = cal.GaussianLikelihood()
    host = cal.EnsembleSampler(params, runner, lik, target)
    assert host.log_posterior_batch(np.array([[1.25, 30.0], [1.25, 30.0]]))[0] == params.log_prior([1.25, 30.0])
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target)
    W = 128
    pos = params.sample_random(W, np.random.default_rng(0))
    pos[7, 1] = 50.0   # outside Uniform(15, 45)
    want = host.log_posterior_batch(pos)
    chain = dev.run(1, cal.WalkerInit.explicit(pos), n_walkers=W, seed=3)
    got_pos, got_lp = chain.flat_samples(), chain.flat_log_probs()
    same = (got_pos == pos).all(axis=1)
    assert same.any() and (~same).any() and want[7] == -np.inf
    assert_bit_equal(got_lp[same], want[same], "graph evaluator: walkers that did not move")
    assert_bit_equal(got_lp[~same], host.log_posterior_batch(got_pos[~same]), "graph evaluator: accepted proposals")
    # the same target without its period: the table of the graph evaluator with no reference entry
    want = cal.EnsembleSampler(params, runner, lik, absolute).log_posterior_batch(pos)
    chain = cal.DeviceEnsembleSampler(params, runner, lik, absolute).run(1, cal.WalkerInit.explicit(pos), n_walkers=W, seed=3)
    same = (chain.flat_samples() == pos).all(axis=1)
    assert same.any() and np.isfinite(want[same]).any()
    assert_bit_equal(chain.flat_log_probs()[same], want[same], "graph evaluator: no period")
    # a period that ends after the last observation: the graph steps on to the period's last row
    late = cal.Target()
    late.add_observation("Surface Temperature", 1780.0, 0.01, 0.05).add_observation("Surface Temperature", 1800.0, 0.02, 0.05)
    late.set_reference_period("Surface Temperature", 1790, 1840)
    host = cal.EnsembleSampler(params, runner, lik, late)
    want = host.log_posterior_batch(pos)
    chain = cal.DeviceEnsembleSampler(params, runner, lik, late).run(1, cal.WalkerInit.explicit(pos), n_walkers=W, seed=3)
    same = (chain.flat_samples() == pos).all(axis=1)
    assert same.any() and np.isfinite(want[same]).any()
    assert_bit_equal(chain.flat_log_probs()[same], want[same], "graph evaluator: a period beyond the last observation")
    runner.close()
