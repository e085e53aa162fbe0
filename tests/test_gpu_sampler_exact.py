"""The device stretch-move sampler (csrc/sampler.hip) and Latin hypercube (lhs_kernel, csrc/ensemble_ops.hip) against the
numpy restatement of tests/host_sampler.py, bit for bit.  Every draw is counter-based Philox keyed by values the host
knows, so the restatement predicts every proposal, partner, accept decision and LHS entry:
  * the whole chain, where the device scores equal EnsembleSampler.log_posterior_batch exactly (fused two-layer
    evaluator, Uniform priors): every sweep's positions and log probabilities, the counters, thinning;
  * half-step by half-step from the recorded device state, where the scores agree to a tolerance only (stored-series
    and graph evaluators, Normal / LogNormal / Bound priors): proposals exactly, decisions up to a counted and bounded
    number of marginal ones;
  * Ensemble.sample_lhs at sizes, shard offsets, parameter counts and seeds where a Feistel or keying slip would show."""
import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.helpers import TL_RANGES, SEED, bits, emissions_syn
from tests.host_sampler import HostStretchMove, lhs_matrix, marginal
from tests.test_gpu_sampler import NAMES, _problem, setup  # noqa: F401  (setup: that module's fixture)

pytestmark = pytest.mark.gpu

RANGES = dict(zip(NAMES, TL_RANGES))
DIMS = {1: ["lambda0"], 2: ["lambda0", "efficacy"], 6: NAMES}


def _identical_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ the whole chain
CHAIN_CASES = [  # D, stretch_a, seed, walkers, groups, sweeps
    (2, 2.0, 0, 514, 1, 10),                # a half of kBlock + 1 walkers: the last workgroup holds one lane
    (6, 1.5, 2 ** 32 + 7, 64, 4, 10),
    (1, 5.0, 2 ** 64 - 1, 16, 8, 12),       # Hg = 1: the partner is forced
    (6, 5.0, 0, 2, 1, 12),                  # W = 2
    (1, 2.0, 2 ** 32 + 7, 514, 1, 8),
    (2, 1.5, 2 ** 64 - 1, 96, 2, 10),
]


@pytest.mark.parametrize("D,a,seed,W,G,S", CHAIN_CASES)
def test_device_chain_equals_restatement(setup, D, a, seed, W, G, S):
    """Fused two-layer evaluator, Uniform priors: from the initial positions alone the restatement reproduces every sweep
    of DeviceEnsembleSampler.run bit for bit -- positions, log probabilities, n_accepted / n_proposed -- and what thin = 3
    keeps.  Walkers that start outside the support (-inf) accept their first proposal with a finite score."""
    cal, b = setup
    names = DIMS[D]
    runner, target, params = _problem(cal, b, names, [RANGES[k] for k in names])
    lik = cal.GaussianLikelihood()
    host = cal.EnsembleSampler(params, runner, lik, target)
    rng = np.random.default_rng(seed % 1000 + W)
    pos = params.sample_random(W, rng)
    lo, hi = RANGES[names[0]]
    outside = sorted({0, W // 2 + 1, W - 1}) if W > 2 else [0]
    pos[outside, 0] = hi + 0.02 * (hi - lo)   # just past the upper edge: proposals towards the ensemble land inside
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target, stretch_a=a)
    chain = dev.run(S, cal.WalkerInit.explicit(pos), n_walkers=W, seed=seed, n_groups=G)

    sm = HostStretchMove(W, D, host.log_posterior_batch, stretch_a=a, seed=seed, n_groups=G)
    sm.keep_records = True
    sm.set_positions(pos)
    assert (sm.logp[outside] == -np.inf).all() and np.isfinite(np.delete(sm.logp, outside)).all()
    want_pos, want_lp = sm.run(S)
    assert len(chain) == S and chain.total_iterations == S
    for s in range(S):
        assert _identical_bits(chain._samples[s], want_pos[s]), f"sweep {s + 1}: positions"
        assert _identical_bits(chain._log_probs[s], want_lp[s]), f"sweep {s + 1}: log probabilities"
    assert np.array_equal(dev.n_accepted, sm.n_accepted) and (dev.n_proposed == S).all()
    assert np.array_equal(dev.n_proposed, sm.n_proposed)
    assert sm.n_accepted.sum() < S * W and (W == 2 or sm.n_accepted.sum() > 0)   # some moves rejected, some accepted
    assert sm.n_marginal == 0, "a decision inside the rounding band of log / exp: not a bit-exact case"
    # the walkers outside the support took the first proposal that scored finitely
    for w in outside:
        seen = [(r[3][np.flatnonzero(r[2] == w)[0]], r[4][np.flatnonzero(r[2] == w)[0]]) for r in sm.records if w in r[2]]
        first = next((acc for lp, acc in seen if np.isfinite(lp)), None)
        assert first is None or first
    # thin = 3 keeps sweeps 1, 4, 7, ...
    thin = dev.run(S, cal.WalkerInit.explicit(pos), thin=3, n_walkers=W, seed=seed, n_groups=G)
    assert thin.total_iterations == S and len(thin) == len(range(0, S, 3))
    for k, s in enumerate(range(0, S, 3)):
        assert _identical_bits(thin._samples[k], want_pos[s]) and _identical_bits(thin._log_probs[k], want_lp[s])
    print(f"\nchain D={D} a={a} seed={seed} W={W} groups={G}: {sm.n_decisions} decisions bit-exact, "
          f"acceptance {sm.n_accepted.sum() / sm.n_proposed.sum():.3f}")
    runner.close()


# ------------------------------------------------------------------------------------------ half-step by half-step
def _check_half_steps(chain, D, a, seed, W, score, rtol, atol, G=1):
    """From the device state after sweep s predict sweep s + 1: half 0 from that state, half 1 from it with half 0 replaced
    by what the device recorded (half-0 walkers do not move in half 1).  A recorded position is the old one or the predicted
    proposal, bit for bit; the decision is the predicted one unless marginal; the log probability is the old one, bit for
    bit, or the host's score of the proposal within (rtol, atol).  Returns (decisions, marginal decisions)."""
    sm = HostStretchMove(W, D, score, stretch_a=a, seed=seed, n_groups=G)
    n_dec = n_marg = 0
    for s in range(len(chain) - 1):
        pos, lp = chain._samples[s].copy(), chain._log_probs[s].copy()
        nxt, nlp = chain._samples[s + 1], chain._log_probs[s + 1]
        for half in (0, 1):
            st = sm.propose(half, iteration=s + 2, pos=pos)
            act = st.active
            new = np.asarray(score(st.proposal), dtype=np.float64)
            want, lr = sm.decide(st, new, lp[act])
            with np.errstate(invalid="ignore"):
                tol = atol + rtol * np.abs(new)
            marg = marginal(st.u, lr, new, score_tol=tol)
            rec = nxt[act]
            old = (bits(rec) == bits(pos[act])).all(axis=1)
            prop = (bits(rec) == bits(st.proposal)).all(axis=1)
            assert (old | prop).all(), f"sweep {s + 2} half {half}: a position that is neither the old one nor the proposal"
            moved = ~old
            bad = (moved != want) & ~marg
            assert not bad.any(), (f"sweep {s + 2} half {half}: walkers {act[bad][:8]} decided otherwise "
                                   f"(device moved: {moved[bad][:8]}, scores {new[bad][:8]} vs old {lp[act][bad][:8]})")
            assert _identical_bits(nlp[act][~moved], lp[act][~moved])
            assert np.allclose(nlp[act][moved], new[moved], rtol=rtol, atol=atol) and np.isfinite(nlp[act][moved]).all()
            n_dec += len(act)
            n_marg += int(marg.sum())
            pos[act], lp[act] = rec, nlp[act]
    assert n_marg <= n_dec * 1e-5, f"{n_marg} marginal decisions of {n_dec}"
    return n_dec, n_marg


def test_half_steps_stored_series_evaluator(setup):
    """ClimateUDEB scored from its stored series (the non-fused path): initial scores equal the host's to 1e-9."""
    cal, _ = setup
    from rscm_amd import core
    from rscm_amd.magicc import ClimateUDEBBuilder
    years = np.arange(1850.0, 1911.0)
    axis = core.TimeAxis.from_values(years)
    erf = 3.71 * np.minimum((years - 1850.0) / 40.0, 1.0)
    b = (core.ModelBuilder().with_time_axis(axis)
         .with_rust_component(ClimateUDEBBuilder.from_parameters({"ecs": 3.2, "kappa": 0.9}).build())
         .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(erf, axis, "W/m^2", core.InterpolationStrategy.Previous))
         .with_initial_values({"Surface Temperature": 0.0}))
    runner = cal.ModelRunner(b, ["ecs", "kappa"], ["Sea Surface Temperature"])
    truth = runner.run([3.2, 0.9])["Sea Surface Temperature"]
    target = cal.Target()
    for yr in range(1860, 1911, 5):
        target.add_observation("Sea Surface Temperature", float(yr), truth[float(yr)], 0.02)
    params = cal.ParameterSet().add("ecs", cal.Uniform(1.5, 6.0)).add("kappa", cal.Uniform(0.3, 2.0))
    lik = cal.GaussianLikelihood()
    host = cal.EnsembleSampler(params, runner, lik, target)
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target, stretch_a=2.5)
    W, seed = 256, 2 ** 32 + 7
    chain = dev.run(8, cal.WalkerInit.explicit(params.sample_random(W, np.random.default_rng(9))), n_walkers=W, seed=seed)
    n, m = _check_half_steps(chain, 2, 2.5, seed, W, host.log_posterior_batch, 1e-9, 1e-9)
    print(f"\nstored-series evaluator: {n} decisions, {m} marginal")
    runner.close()


def test_half_steps_graph_evaluator(setup):
    """A graph of linked ensembles as the evaluator (rscm_sampler_create_graph): CarbonCycle -> CO2ERF -> TwoLayer,
    lambda0 and tau sampled in two different components."""
    cal, _ = setup
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
    # a second forcing term and the aggregate keep the three components a graph of linked ensembles (not the fused coupled kind)
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
    target = cal.Target()
    for v, sigma in (("Surface Temperature", 0.01), ("Atmospheric Concentration|CO2", 0.2)):
        for y in range(1780, 1851, 10):
            target.add_observation(v, float(y), truth[v][float(y)], sigma)
    params = cal.ParameterSet().add("TwoLayer.lambda0", cal.Uniform(0.8, 1.6)).add("tau", cal.Uniform(15.0, 45.0))
    lik = cal.GaussianLikelihood()
    host = cal.EnsembleSampler(params, runner, lik, target)
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target)
    W, seed = 128, 2 ** 64 - 1
    pos = params.sample_random(W, np.random.default_rng(0))
    pos[7, 1] = 50.0   # outside Uniform(15, 45)
    chain = dev.run(8, cal.WalkerInit.explicit(pos), n_walkers=W, seed=seed)
    n, m = _check_half_steps(chain, 2, 2.0, seed, W, host.log_posterior_batch, 1e-12, 1e-9)
    print(f"\ngraph evaluator: {n} decisions, {m} marginal")
    runner.close()


def test_half_steps_normal_lognormal_and_bound_priors(setup):
    """No observations: the posterior is the prior, Normal x LogNormal x Bound(Normal), whose device log need not round
    like numpy's.  4096 walkers in 4 groups."""
    cal, b = setup
    runner = cal.ModelRunner(b, ["lambda0", "heat_capacity_surface", "eta"], ["Surface Temperature"])
    params = (cal.ParameterSet().add("lambda0", cal.Normal(1.1, 0.1)).add("heat_capacity_surface", cal.LogNormal(2.0, 0.25))
              .add("eta", cal.Bound(cal.Normal(0.7, 0.2), 0.5, 1.0)))
    dev = cal.DeviceEnsembleSampler(params, runner, cal.GaussianLikelihood(), cal.Target(), stretch_a=1.5)
    W, seed = 4096, 0
    chain = dev.run(10, cal.WalkerInit.explicit(params.sample_random(W, np.random.default_rng(1))), n_walkers=W, seed=seed,
                    n_groups=4)
    n, m = _check_half_steps(chain, 3, 1.5, seed, W, params.log_prior_batch, 1e-13, 1e-13, G=4)
    print(f"\nNormal / LogNormal / Bound priors: {n} decisions, {m} marginal")
    runner.close()


# ------------------------------------------------------------------------------------------ Latin hypercube
LHS_KINDS = [  # kind name, low, high: different parameter counts, one row with low == high in each
    ("KIND_TWO_LAYER", [0.8, 0.0, 1.0, 0.7, 5.0, 50.0], [1.5, 0.1, 1.8, 0.7, 15.0, 200.0]),
    ("KIND_CARBON_CYCLE", [15.0, 278.0, 0.0], [40.0, 278.0, 0.1]),
    ("KIND_COUPLED", [0.8, 0.0, 1.0, 0.5, 5.0, 50.0, 15.0, 278.0, 0.0, 3.7], [1.5, 0.1, 1.8, 1.0, 15.0, 200.0, 40.0, 278.0, 0.1, 3.7]),
    ("KIND_CO2_BUDGET", [-1.0, 2.0], [1.0, 2.0]),
]
LHS_SEEDS = [0, SEED, 2 ** 32 + 7, 2 ** 64 - 1]


def _lhs(ra, kind, n_local, seed, lo, hi, offset, n_total):
    t = np.arange(1750.0, 1753.0)
    with ra.Ensemble(getattr(ra, kind), n_local, np.append(t, t[-1] + 1.0)) as e:
        e.sample_lhs(seed, lo, hi, offset, n_total)
        return e.get_params()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 257, 4099, 65537])
def test_device_lhs_equals_restatement(ra, n):
    """Every entry of Ensemble.sample_lhs is lhs_matrix's, bit for bit, whole and in shards at offsets that are not
    multiples of 64; the kind (parameter count) and seed (high word set or not) vary with n."""
    i = [1, 2, 3, 5, 63, 64, 65, 257, 4099, 65537].index(n)
    kind, lo, hi = LHS_KINDS[i % len(LHS_KINDS)]
    seed = LHS_SEEDS[(i // len(LHS_KINDS) + i) % len(LHS_SEEDS)]
    got = _lhs(ra, kind, n, seed, lo, hi, 0, n)
    assert _identical_bits(got, lhs_matrix(seed, lo, hi, 0, n, n)), f"{kind} n={n} seed={seed}"
    entries = got.size
    if n >= 5:
        cuts = sorted({0, 1, min(n, n // 3 + 5), (2 * n) // 3 - 1, n})
        for a0, a1 in zip(cuts[:-1], cuts[1:]):
            part = _lhs(ra, kind, a1 - a0, seed, lo, hi, a0, n)
            assert _identical_bits(part, got[:, a0:a1]), f"{kind} n={n} members [{a0}, {a1})"
            entries += part.size
    print(f"\nlhs {kind} n={n} seed={seed}: {entries} entries bit-exact")


def test_device_lhs_equals_restatement_1e6(ra):
    n, seed = 1_000_003, 2 ** 64 - 1
    kind, lo, hi = LHS_KINDS[1]
    got = _lhs(ra, kind, n, seed, lo, hi, 0, n)
    assert _identical_bits(got, lhs_matrix(seed, lo, hi, 0, n, n))
    # a block of the same global ensemble at an odd offset
    part = _lhs(ra, kind, 70001, seed, lo, hi, 333_333, n)
    assert _identical_bits(part, got[:, 333_333:403_334])
    print(f"\nlhs {kind} n={n} seed={seed}: {got.size + part.size} entries bit-exact")
