"""GPU tier of the two-layer MIX ensemble (rscm_ens_create_mix; Ensemble(..., forcing_components=K)): member i is forced by
F = S_0 c_0;  F = F + S_k c_k (k = 1 .. K-1), each product and sum rounded on its own, with its coefficients in parameter rows
6 .. 6+K-1.

The reference of every value test: each member's series formed on the host in exactly that order (tests/host_forcing_mix.py,
numpy, which does not fuse) and given to the CPU oracle's plain two-layer run as one scenario per member.  EXACT mode is compared
bit for bit; RSCM_MODE_FAST bit for bit with a PLAIN two-layer handle given the same host-formed series (the forming of F does not
depend on the mode, the rest is the existing kernel) and at the existing FAST tolerance (1e-11 relative to max(1, |oracle|) on
bounded members, tests/test_gpu_parity.py) with the oracle.

N = 130 members (two wavefronts and two lanes) on a 40-step uneven axis unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from tests import host_forcing_mix as hm
from tests import host_resample as hr
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import assert_bit_equal, two_layer_params
from tests.host_sampler import lhs_matrix

pytestmark = pytest.mark.gpu

N = 130
T = 41
BOUNDS = np.concatenate([[1750.0], 1750.0 + np.cumsum(np.where(np.arange(T) % 7 == 3, 0.5, 1.0))])   # uneven steps
FAST_RTOL = 1e-11
TS, TD = "Surface Temperature", "Deep Ocean Temperature"


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


def _block(n_scen, K, n_times=T, scale=1.0):
    """[n_scen][K][n_times] component series: saturating ramps of alternating sign with a ripple, scenario s scaled by 1 + 0.3 s."""
    t = np.arange(n_times, dtype=np.float64)
    S = np.empty((n_scen, K, n_times))
    for s in range(n_scen):
        for k in range(K):
            S[s, k] = scale * (1.0 + 0.3 * s) * ((-1.0) ** k * (1.5 + 0.25 * k) * (1.0 - np.exp(-t / (15.0 + 4.0 * k)))
                                                + 0.2 * np.sin(2.0 * np.pi * t / (7.0 + k)))
    return S


def _params(K, n=N, seed=11, uniform_rows=()):
    """[6 + K][n]: the seeded two-layer draw and coefficients in [0.4, 1.6]; ``uniform_rows`` hold one value for every member."""
    rng = np.random.default_rng(seed)
    P = np.vstack([two_layer_params(n), rng.uniform(0.4, 1.6, (K, n))])
    for j in uniform_rows:
        P[j] = P[j, 0]
    return P


def _scen(n_scen, n=N, seed=5):
    return None if n_scen == 1 else np.random.default_rng(seed).integers(0, n_scen, n).astype(np.int32)


def _mix(ra, P, S, scen=None, source=None, mode=None, bounds=BOUNDS, store_series=True):
    K = P.shape[0] - 6
    e = ra.Ensemble(ra.KIND_TWO_LAYER, P.shape[1], bounds, store_series=store_series, forcing_components=K)
    e.set_mode(ra.MODE_EXACT if mode is None else mode)
    e.set_params(P)
    e.set_forcing(S, scen, ra.SRC_EXOGENOUS if source is None else source)
    e.set_initial(TS, 0.0)
    e.set_initial(TD, 0.0)
    return e


def _plain(ra, P6, F, source=None, mode=None, bounds=BOUNDS):
    """A plain two-layer handle under the members' own series ``F`` [n][T], one scenario per member."""
    n = P6.shape[1]
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, bounds)
    e.set_mode(ra.MODE_EXACT if mode is None else mode)
    e.set_params(P6)
    e.set_forcing(F, np.arange(n, dtype=np.int32), ra.SRC_EXOGENOUS if source is None else source)
    e.set_initial(TS, 0.0)
    e.set_initial(TD, 0.0)
    return e


def _series(e):
    return e.get_series(TS), e.get_series(TD)


def _same(got, want, what):
    assert_bit_equal(got[0], want[0], f"{what}: Ts")
    assert_bit_equal(got[1], want[1], f"{what}: Td")


# ---------------------------------------------------------------------------------------------- 1. EXACT: the oracle's bits
@pytest.mark.parametrize("source", [0, 1], ids=["exogenous", "upstream"])
@pytest.mark.parametrize("n_scen", [1, 2])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_exact_equals_the_oracle_bit_for_bit(ra, orc, K, n_scen, source):
    S, scen = _block(n_scen, K), _scen(n_scen)
    # every row varying; then coefficient rows (and a model row) that hold one value for every member: the uniform read path
    for uniform in ((), (3, 6, 6 + K - 1)):
        P = _params(K, uniform_rows=uniform)
        want = hm.oracle_run(orc, BOUNDS, P, S, scen, source)
        assert np.isfinite(want[0]).all()
        with _mix(ra, P, S, scen, source) as e:
            e.run()
            assert e.finished()
            _same(_series(e), want, f"K={K} S={n_scen} source={source} uniform={uniform}")
            assert not e.status().any()
            assert_bit_equal(e.get_params(), P, "get_params carries the coefficient rows")


@pytest.mark.parametrize("K", [1, 3, 8])
def test_stepwise_and_resumed_runs_equal_one_run(ra, orc, K):
    S, scen, P = _block(2, K), _scen(2), _params(K, uniform_rows=(6,))
    want = hm.oracle_run(orc, BOUNDS, P, S, scen, 1)
    with _mix(ra, P, S, scen, ra.SRC_UPSTREAM) as e:
        while not e.finished():
            e.step()
        _same(_series(e), want, f"K={K} step by step")
    with _mix(ra, P, S, scen, ra.SRC_UPSTREAM) as e:
        e.run(17)
        ck = e.checkpoint()
        assert ck["params"].shape == (6 + K, N)
    # ... into a fresh ensemble whose parameters are all different until restore() puts the checkpoint's 6 + K rows back
    with _mix(ra, _params(K, seed=99), S, scen, ra.SRC_UPSTREAM) as e:
        e.restore(ck)
        assert e.time_index == 17
        e.run()
        got = _series(e)
        assert_bit_equal(got[0][17:], want[0][17:], f"K={K} resumed: Ts")
        assert_bit_equal(got[1][17:], want[1][17:], f"K={K} resumed: Td")


# ---------------------------------------------------------------------------------------------- 2. FAST
@pytest.mark.parametrize("K", [1, 3, 8])
def test_fast_mode_equals_a_plain_handle_under_the_host_formed_series(ra, orc, K):
    S, scen, P = _block(2, K), _scen(2), _params(K)
    F = hm.mix_forcing(S, P[6:], scen)
    with _mix(ra, P, S, scen, mode=ra.MODE_FAST) as e, _plain(ra, P[:6], F, mode=ra.MODE_FAST) as p:
        e.run()
        p.run()
        got = _series(e)
        _same(got, _series(p), f"K={K} FAST mix against FAST plain")
        assert np.array_equal(e.status(), p.status())
    want = hm.oracle_run(orc, BOUNDS, P, S, scen, 0)
    with np.errstate(all="ignore"):
        bounded = np.isfinite(want[0][-1]) & (np.nanmax(np.abs(want[0]), axis=0) < 50.0)
    assert bounded.mean() > 0.9
    for g, w in zip(got, want):
        err = np.abs(g[:, bounded] - w[:, bounded]) / np.maximum(1.0, np.abs(w[:, bounded]))
        print(f"K={K} FAST against the oracle: max deviation {err.max():.3e}")
        assert (err <= FAST_RTOL).all()


# ---------------------------------------------------------------------------------------------- 3. the table read through L2
def _annual(n_times):
    return np.arange(n_times + 1, dtype=np.float64) + 1750.0


def test_table_beyond_the_lds_budget_equals_the_oracle(ra, orc):
    """K = 8, S = 3 on a 900-step annual axis: 3 * 8 * 900 * 8 = 172 800 B, more than the 159 KiB a launch may stage."""
    K, n_scen, nt = 8, 3, 901
    assert n_scen * K * (nt - 1) * 8 > 159 * 1024
    b, S, scen, P = _annual(nt), _block(n_scen, K, nt, scale=0.25), _scen(n_scen), _params(K, uniform_rows=(7,))
    want = hm.oracle_run(orc, b, P, S, scen, 0)
    with _mix(ra, P, S, scen, bounds=b) as e:
        e.run()
        full = _series(e)
        _same(full, want, "K=8 S=3, 900 steps")
        e.rewind()
        e.run(40)   # 40 steps of the same table fit: the staged variant
        head = _series(e)
        assert_bit_equal(head[0][:41], full[0][:41], "first 40 steps, staged against read through L2: Ts")
        assert_bit_equal(head[1][:41], full[1][:41], "first 40 steps, staged against read through L2: Td")


def test_both_variants_agree_on_one_scenario(ra):
    """K = 8, S = 1: a 2600-step axis puts one scenario's table (8 * 2600 * 8 = 166 400 B) beyond the budget; its first 40 steps
    run on their own are staged in LDS.  Same bits."""
    K, nt = 8, 2601
    assert K * (nt - 1) * 8 > 159 * 1024 > K * 40 * 8
    b, S, P = _annual(nt), _block(1, K, nt, scale=0.25), _params(K)
    with _mix(ra, P, S, bounds=b) as e:
        e.run()
        full = (e.get_series(TS, 0, 41), e.get_series(TD, 0, 41))
        e.rewind()
        e.run(40)
        _same((e.get_series(TS, 0, 41), e.get_series(TD, 0, 41)), full, "K=8 S=1, first 40 steps")
        assert np.isfinite(full[0]).all()


# ---------------------------------------------------------------------------------------------- 4. special values
def test_special_values_propagate_as_in_the_oracle(ra, orc):
    K = 3
    S, P = _block(1, K), _params(K)
    S[0, 1, 10] = np.nan            # a NaN in one component row: every member is NaN from there on
    P[6, 5] = np.inf                # an Inf coefficient
    P[6:, 7] = -0.0                 # -0.0 coefficients: a forcing of -0.0 / +0.0 by the signs of the rows
    P[7, 9] = 1.0e5                 # a forcing far outside the guard's box: the year is replayed with the full division
    P[8, 11] = 1.0e-300             # ... and a denormal-sized contribution
    P[7, 13] = 3000.0               # |F| up to 5e3 >= 2^12, outside the box, on a member that stays finite
    for S_case, what in ((S, "NaN row"), (_block(1, K), "finite rows")):
        want = hm.oracle_run(orc, BOUNDS, P, S_case, None, 0)
        F = hm.mix_forcing(S_case, P[6:])
        with _mix(ra, P, S_case) as e, _plain(ra, P[:6], F) as p:
            e.run()
            p.run()
            _same(_series(e), want, what)
            _same(_series(e), _series(p), what + ", plain handle")
            assert np.array_equal(e.status(), p.status()), what
            if what == "NaN row":
                assert e.status().all() and np.isnan(e.get_series(TS, 12, 13)).all()
            else:
                st = e.status()
                assert st[5] == 1 and st[7] == 0 and np.isfinite(want[0][:, 9]).all() == (st[9] == 0)
                assert st[13] == 0 and np.isfinite(want[0][:, 13]).all() and np.abs(F[13]).max() > 4096.0


# ---------------------------------------------------------------------------------------------- 5. the member split
def test_cut_run_equals_uncut_run_and_the_oracle(ra, orc):
    from rscm_amd import _lib as L
    n, nt, K = 65536 + 130, 201, 3
    b, S = _annual(nt), _block(2, K, nt, scale=0.5)
    P, scen = _params(K, n=n, uniform_rows=(8,)), _scen(2, n)
    lib = L.load()
    got = {}
    try:
        for plan in (1, 0):
            L.check(lib.rscm_gpu_set_run_plan(plan))
            with _mix(ra, P, S, scen, bounds=b) as e:
                e.run()
                blocks, chunks = e.last_run_plan()
                assert (blocks, chunks > 1) == ((2, True) if plan else (1, False))
                got[plan] = _series(e)
    finally:
        L.check(lib.rscm_gpu_set_run_plan(-1))
    _same(got[1], got[0], "cut against uncut")
    edge = np.r_[0:130, n - 130:n]
    want = hm.oracle_run(orc, b, P[:, edge], S, scen[edge], 0)
    _same((got[1][0][:, edge], got[1][1][:, edge]), want, "first and last 130 members")


# ---------------------------------------------------------------------------------------------- 6. the fused likelihood
@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fast"])
def test_fused_likelihood_equals_run_then_loglik(ra, mode):
    K = 3
    S, scen, P = _block(2, K), _scen(2), _params(K, uniform_rows=(6,))
    obs_t = [3, 9, 9, 20, 33, 40, 12, 40]
    obs_v = [TS, TS, TS, TS, TS, TS, TD, TD]
    val = [0.1, 0.3, 0.35, 0.8, 1.2, 1.5, 0.05, 0.3]
    sig = [0.1, 0.1, 0.2, 0.15, 0.2, 0.2, 0.05, 0.1]
    for reference in (None, {TS: (5, 15), TD: (0, 11, 2)}):
        kw = {"reference": reference} if reference else {}
        with _mix(ra, P, S, scen, mode=mode) as e:
            e.run()
            stored = e.loglik(obs_v, obs_t, val, sig, True, **kw)
            assert np.isfinite(stored).all()
            e.rewind()
            assert np.array_equal(e.run_loglik(obs_v, obs_t, val, sig, True, **kw), stored), reference
        with _mix(ra, P, S, scen, mode=mode, store_series=False) as e:
            assert np.array_equal(e.run_loglik(obs_v, obs_t, val, sig, True, **kw), stored), reference
    # ... and the likelihood does depend on the coefficients
    P2 = P.copy()
    P2[7] *= 1.1
    with _mix(ra, P2, S, scen, mode=mode, store_series=False) as e:
        assert (e.run_loglik(obs_v, obs_t, val, sig, True) != stored).all()


# ---------------------------------------------------------------------------------------------- 7. Latin hypercube
def test_latin_hypercube_covers_the_coefficient_rows(ra):
    K = 3
    lo = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0, 0.7, -1.6, 0.0])
    hi = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0, 1.3, -0.2, 2.0])
    with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS, forcing_components=K) as e:
        with pytest.raises(ValueError):
            e.sample_lhs(3, lo[:6], hi[:6])
        e.sample_lhs(3, lo, hi)
        P = e.get_params()
    assert P.shape == (6 + K, N)
    for j in range(6 + K):   # exactly one sample per stratum: the r-th smallest lies in stratum r (1e-9 strata of rounding at its edges)
        u = (np.sort(P[j]) - lo[j]) / (hi[j] - lo[j]) * N
        assert ((u >= np.arange(N) - 1e-9) & (u <= np.arange(N) + 1.0 + 1e-9)).all(), f"row {j}: one sample per stratum"
        assert np.unique(P[j]).size == N
    assert_bit_equal(P, lhs_matrix(3, lo, hi, 0, N, N), "the host restatement of the draw, 6 + K rows")
    from rscm_amd.distributed import ShardedEnsemble, shard_bounds
    for rank in range(3):
        sh = ShardedEnsemble(N, lambda count, device: ra.Ensemble(ra.KIND_TWO_LAYER, count, BOUNDS, device=device, forcing_components=K),
                             rank=rank, world=3, device=0)
        sh.sample_lhs(3, lo, hi)
        off, cnt = shard_bounds(N, rank, 3)
        assert_bit_equal(sh.ensemble.get_params(), P[:, off:off + cnt], f"shard {rank}")
        sh.ensemble.close()


# ---------------------------------------------------------------------------------------------- 8. the device sampler
FIXED = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)


@pytest.fixture(scope="module")
def problem(ra):
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    t = np.arange(1750.0, 1831.0)
    axis = core.TimeAxis.from_values(t)
    lin = core.InterpolationStrategy.Linear
    comps = {"ghg": core.Timeseries(3.0 * (1.0 - np.exp(-(t - 1750.0) / 40.0)), axis, "W/m^2", lin),
             "aerosol": core.Timeseries(-1.0 * (1.0 - np.exp(-(t - 1750.0) / 25.0)), axis, "W/m^2", lin),
             "solar": core.Timeseries(0.1 * np.sin(2.0 * np.pi * (t - 1750.0) / 11.0), axis, "W/m^2", lin)}
    b = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(FIXED).build())
         .with_forcing_components("Effective Radiative Forcing", comps, scales={"aerosol": 0.9})
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))
    names = ["lambda0", "forcing_scale|ghg", "forcing_scale|aerosol"]
    runner = cal.ModelRunner(b, names, [TS])
    truth = runner.run([1.1, 1.0, 0.9])[TS]
    target = cal.Target()
    for yr in range(1770, 1831, 10):
        target.add_observation(TS, float(yr), truth[float(yr)], 0.05)
    params = cal.ParameterSet()
    for k, (lo, hi) in zip(names, [(0.8, 1.5), (0.6, 1.4), (0.3, 1.5)]):
        params.add(k, cal.Uniform(lo, hi))
    yield cal, b, runner, target, params
    runner.close()


def test_model_front_end_carries_the_scales(ra, orc, problem):
    cal, b, runner, target, params = problem
    m = runner._model(1)
    assert m.param_order[6:] == ("forcing_scale|ghg", "forcing_scale|aerosol", "forcing_scale|solar")
    assert m.base_params.tolist()[6:] == [1.0, 0.9, 1.0]
    assert m.ensemble.n_params == 9 and m.ensemble.n_inputs == 3 and m.ensemble.coefficient_row("aerosol") == 7
    assert runner._lik_model(4).ensemble.store_series is False
    # run_batch: the members' trajectories are the oracle's under the host-formed series
    sets = np.array([[1.1, 1.0, 0.9], [0.9, 1.3, 0.4], [1.4, 0.7, 1.5]])
    got = runner.run_batch(sets)
    plan = b.forcing_mix_plan()
    P = np.repeat(plan["base_params"][:, None], 3, axis=1)
    P[[0, 6, 7]] = sets.T
    want = hm.oracle_run(orc, m._axis.bounds(), P, plan["block"])[0]
    times = m._axis.values()
    for i in range(3):
        assert [got[i][TS][float(t)] for t in times] == want[:, i].tolist()
    # a TOML text of the model rebuilds a mix ensemble at the same step
    from rscm_amd import core
    m2 = b.build(n_members=2)
    m2.ensemble.set_params(P[:, :2])
    for _ in range(5):
        m2.step()
    m3 = core.Model.from_toml(m2.to_toml())
    assert m3.ensemble.n_forcing_components == 3 and m3.time_index == 5 and m3.param_order == m2.param_order
    m2.run()
    m3.run()
    # the text holds the state at the step it was taken at, not the rows before it: those stay unwritten
    assert_bit_equal(m3.ensemble.get_series(TS)[5:], m2.ensemble.get_series(TS)[5:], "rebuilt from TOML")
    assert np.isnan(m3.ensemble.get_series(TS)[1:5]).all()
    m2.close()
    m3.close()


def test_device_sampler_scores_and_moves_the_coefficient_rows(ra, problem):
    cal, b, runner, target, params = problem
    lik = cal.GaussianLikelihood()
    pos = params.sample_random(64, np.random.default_rng(0))
    pos[5, 1] = 2.0   # outside Uniform(0.6, 1.4)

    def stored_scores(p):
        """log prior + the likelihood of the STORED series of a run with those rows"""
        lp = params.log_prior_batch(p)
        q = np.array(p)
        q[~np.isfinite(lp)] = q[np.flatnonzero(np.isfinite(lp))[0]]
        m = runner._run(q)
        ov, ot, val, sig = [], [], [], []
        for name, vt in target.variables():
            for obs in vt.observations:
                ov.append(name), ot.append(m._axis.index_of(obs.time)), val.append(obs.value), sig.append(obs.uncertainty)
        out = lp + m.ensemble.loglik(ov, ot, val, sig, lik.normalize)
        out[~np.isfinite(lp)] = -np.inf
        return out

    want = stored_scores(pos)
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target)
    chain = dev.run(1, cal.WalkerInit.explicit(pos), n_walkers=64, seed=1)
    got_pos, got_lp = chain.flat_samples(), chain.flat_log_probs()
    same = (got_pos == pos).all(axis=1)
    assert same.any() and (~same).any()
    assert np.array_equal(got_lp[same], want[same]) and want[5] == -np.inf
    assert np.array_equal(got_lp[~same], stored_scores(got_pos[~same])) and np.isfinite(got_lp[~same]).all()
    # accepted proposals moved the coefficient dimensions, not only lambda0
    assert (got_pos[~same][:, 1] != pos[~same][:, 1]).all() and (got_pos[~same][:, 2] != pos[~same][:, 2]).all()
    # a short chain: reproducible by its seed, different for another
    a = dev.run(20, cal.WalkerInit.explicit(pos), thin=5, n_walkers=64, seed=3)
    again = dev.run(20, cal.WalkerInit.explicit(pos), thin=5, n_walkers=64, seed=3)
    other = dev.run(20, cal.WalkerInit.explicit(pos), thin=5, n_walkers=64, seed=4)
    assert np.array_equal(a.flat_samples(), again.flat_samples()) and np.array_equal(a.flat_log_probs(), again.flat_log_probs())
    assert not np.array_equal(a.flat_samples(), other.flat_samples())
    x = a.flat_samples()
    assert x[:, 1].std() > 0 and x[:, 2].std() > 0 and np.unique(x[:, 2]).size > 64


# ---------------------------------------------------------------------------------------------- 9. branch and posterior
def test_branch_and_posterior_carry_the_coefficient_rows(ra):
    from rscm_amd._lib import ERR_INVALID, RscmGpuError
    K, n, M, n_scen, k = 3, 200, 70, 2, 13
    rng = np.random.default_rng(7)
    S, P = _block(1, K), _params(K, n=n, uniform_rows=(6,))
    after = np.stack([S[0], 0.5 * S[0]])                    # the two scenarios the posterior is projected under ...
    after[:, :, :k + 1] = S[0][:, :k + 1]                   # ... spliced to the history at the branch point
    w = rng.integers(0, 1 << 33, size=n, dtype=np.int64)
    w[rng.random(n) < 0.5] = 0
    with _mix(ra, P, S) as src:
        src.run(k)
        src.set_member_weights(w)
        dst, scen = src.posterior(lambda m: ra.Ensemble(ra.KIND_TWO_LAYER, m, BOUNDS, forcing_components=K), M, seed=21, scenarios=n_scen)
        with dst:
            anc = np.tile(hr.ancestors(w, M, hr.offset(21, int(w.sum())))[2], n_scen)
            assert_bit_equal(dst.get_params(), P[:, anc], "the drawn 6 + K rows")
            dst.set_forcing(after, scen)
            dst.run()
            with _mix(ra, P[:, anc], after, scen) as fresh:
                fresh.run()
                for v in (TS, TD):
                    assert_bit_equal(dst.get_series(v, k), fresh.get_series(v, k), f"posterior: {v}")
                assert np.array_equal(dst.status(), fresh.status())
            # the posterior of a coefficient per scenario group, as of any parameter row
            q = dst.quantile_vectors([dst.params_vector(dst.coefficient_row(1))], [0.0, 1.0], grouped=True)
            assert q["quantiles"].shape == (n_scen, 1, 2)
            for g in range(n_scen):   # (minimum and maximum: no interpolation, so the bits of the drawn row)
                assert q["quantiles"][g, 0].tolist() == [P[7, anc[:M]].min(), P[7, anc[:M]].max()] and q["count"][g, 0] == M
            ex = dst.exceedance(dst.params_vector(dst.coefficient_row(1)), [1.0], grouped=True)
            assert ex["hits"][:, 0].tolist() == [int((P[7, anc[:M]] >= 1.0).sum())] * n_scen
        # destinations of another component count, and plain ones, are refused
        for other in (ra.Ensemble(ra.KIND_TWO_LAYER, M, BOUNDS, forcing_components=2), ra.Ensemble(ra.KIND_TWO_LAYER, M, BOUNDS)):
            with other, pytest.raises(RscmGpuError, match="component counts differ") as err:
                src.branch(other, np.arange(M, dtype=np.int64))
            assert err.value.code == ERR_INVALID


# ---------------------------------------------------------------------------------------------- 10. refusals and shapes
def test_shapes_and_refusals(ra):
    from rscm_amd import _lib as L
    from rscm_amd.ensemble import run_lockstep
    lib = L.load()

    def counts(e):
        out = []
        for fn in (lib.rscm_ens_n_params, lib.rscm_ens_n_inputs, lib.rscm_ens_n_forcing_components):
            x = C.c_int32(-1)
            L.check(fn(e._h, C.byref(x)))
            out.append(x.value)
        return tuple(out)

    with ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS) as plain, ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS, forcing_components=1) as one, \
            ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS, forcing_components=("ghg", "aerosol", "solar")) as three, \
            ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS, forcing_components=8, store_series=False) as eight:
        assert counts(plain) == (6, 1, 0) and counts(one) == (7, 1, 1) and counts(three) == (9, 3, 3) and counts(eight) == (14, 8, 8)
        assert (three.n_params, three.n_inputs, three.input_rows) == (9, 3, ("ghg", "aerosol", "solar"))
        assert three.coefficient_row("solar") == 8 and three.coefficient_row(0) == 6
        with pytest.raises(ValueError):
            three.coefficient_row(3)
        with pytest.raises(ValueError):
            plain.coefficient_row(0)
        # set_forcing: [S][K][T] or one scenario's [K][T]; anything else is refused
        three.set_forcing(_block(2, 3))
        three.set_forcing(_block(1, 3)[0])
        one.set_forcing(_block(1, 1)[0, 0])
        for bad in (_block(1, 2), _block(1, 3)[:, :, :-1], _block(1, 3)[0, 0]):
            with pytest.raises(ValueError):
                three.set_forcing(bad)
        with pytest.raises(ValueError):
            three.set_params(np.ones((6, 8)))
        # a mix handle runs on its own
        three.set_params(np.ones((9, 8)))
        with pytest.raises(L.RscmGpuError, match="cannot be linked") as err:
            three.link_input(0, plain, 1)
        assert err.value.code == L.ERR_INVALID
        stream = C.c_void_p()
        L.check(lib.rscm_gpu_stream_create(0, C.byref(stream)))
        try:
            for e in (plain, three):
                e.set_stream(stream.value)
            with pytest.raises(L.RscmGpuError, match="lock-step") as err:
                run_lockstep((plain, three))
            assert err.value.code == L.ERR_INVALID
            h = (C.c_void_p * 1)(three._h)
            i0, d1 = np.zeros(1, dtype=np.int32), np.ones(1)
            s = C.c_void_p()
            rc = lib.rscm_sampler_create_graph(h, 1, 0, 16, 1, L.iptr(i0), L.iptr(i0), L.iptr(i0), L.dptr(0.0 * d1), L.dptr(d1), None, None,
                                               0, None, None, None, None, None, 0, 2.0, 1, 0, 1, C.byref(s))
            assert rc == L.ERR_INVALID and b"graph sampler" in lib.rscm_gpu_last_error() and not s.value
        finally:
            for e in (plain, three):
                e.set_stream(None)
            L.check(lib.rscm_gpu_stream_destroy(0, stream))
    # rscm_ens_create_mix: kind, flags and component count
    b = L.dptr(BOUNDS)
    for kind, flags, k, text in ((L.KIND_COUPLED, 0, 2, b"two-layer kind"), (L.KIND_TWO_LAYER, L.FLAG_WINDOWED, 2, b"windowed"),
                                 (L.KIND_TWO_LAYER, 0, 0, b"n_components"), (L.KIND_TWO_LAYER, 0, 9, b"n_components")):
        h = C.c_void_p()
        assert lib.rscm_ens_create_mix(kind, 8, T, b, 0, flags, k, C.byref(h)) == L.ERR_INVALID and not h.value
        assert text in lib.rscm_gpu_last_error()
    for bad in (0, 9, ("a", "a")):
        with pytest.raises(ValueError):
            ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS, forcing_components=bad)
    with pytest.raises(ValueError):
        ra.Ensemble(ra.KIND_COUPLED, 8, BOUNDS, forcing_components=2)
