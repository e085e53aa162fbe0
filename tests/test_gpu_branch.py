"""GPU tier of branching (rscm_ens_gather_members, Ensemble.branch / posterior, GraphModel.branch): the device gather pinned by
two oracles, both bit for bit on every row after the branch point k and on the status bytes.

(a) EXACT mode: a member's trajectory depends only on its parameters, initial rows and forcing, so a branch taken at k and run
    to the end under a new post-k forcing equals a fresh ensemble given params[:, anc], run from 0 under the spliced forcing.
(b) Every mode: the device branch equals the host route it replaces -- checkpoint(), take along the member axis, restore()
    into an ensemble of the drawn size.
"""
import numpy as np
import pytest

from tests import host_resample as hr
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import assert_bit_equal, coupled_params, emissions_syn, f_syn, magicc_chain, two_layer_params

pytestmark = pytest.mark.gpu

T = 40
K = 13                                   # odd: inside a split OceanCarbon tile
BOUNDS = np.arange(T + 1, dtype=float) + 1750.0
YR = np.arange(T, dtype=float)


def _defaults(values, n):
    return np.repeat(np.asarray(values, dtype=np.float64).reshape(-1, 1), n, axis=1)


def _spec(ra, name, n, rng):
    """(kind, params [P][n], base forcing, alternative forcing, {variable: initial value(s)}) of a stand-alone ensemble."""
    from rscm_amd import _lib as L
    t = BOUNDS[:-1]
    if name == "two_layer":
        return ra.KIND_TWO_LAYER, two_layer_params(n), f_syn(t), 0.5 * f_syn(t) + 1.0, {1: 0.0, 2: 0.0}
    if name == "coupled":
        init = {1: 0.0, 2: 0.0, 3: 278.0, 4: 0.0, 5: 0.0}
        return ra.KIND_COUPLED, coupled_params(n), emissions_syn(t + 200.0), 2.0 + 0.1 * YR, init
    if name.startswith("udeb"):
        P = _defaults(L.UD_DEFAULTS, n)
        P[0] = float(name[4:])
        P[L.UD_PARAM_NAMES.index("ecs")] = rng.uniform(2.0, 4.5, n)
        P[L.UD_PARAM_NAMES.index("kappa")] = rng.uniform(0.5, 1.2, n)
        return ra.KIND_UDEB, P, 0.08 * YR, 3.0 - 0.02 * YR, {1: 0.0, 2: 0.0, 3: 0.0, 4: 0.0}
    if name == "ocean":
        P = _defaults(L.OC_PRESETS["3D-GFDL"], n)
        P[L.OC_PARAM_NAMES.index("gas_exchange_tau")] = rng.uniform(6.0, 10.0, n)
        base = np.stack([278.0 + 3.0 * YR, 0.01 * YR])
        alt = np.stack([420.0 - 1.0 * YR, 0.5 + 0.0 * YR])
        return ra.KIND_OCEAN_CARBON, P, base, alt, {1: 278.0, 2: 0.0}
    if name == "ch4":
        P = _defaults(L.CH4_DEFAULTS, n)
        P[L.CH4_PARAM_NAMES.index("tau_oh")] = rng.uniform(8.0, 11.0, n)
        base = np.stack([300.0 + 2.0 * YR, 0.01 * YR, 20.0 + 0.0 * YR, 500.0 + YR, 100.0 + 0.0 * YR])
        alt = np.stack([250.0 + 0.0 * YR, 1.0 + 0.0 * YR, 30.0 + 0.0 * YR, 400.0 + 0.0 * YR, 120.0 + 0.0 * YR])
        return ra.KIND_CH4_CHEMISTRY, P, base, alt, {1: rng.uniform(600.0, 900.0, n)}
    if name == "n2o":
        P = _defaults(L.N2O_DEFAULTS, n)
        P[L.N2O_PARAM_NAMES.index("tau_n2o")] = rng.uniform(110.0, 150.0, n)
        P[L.N2O_PARAM_NAMES.index("strat_delay")] = 3.0                   # looks four rows back
        return ra.KIND_N2O_CHEMISTRY, P, 7.0 + 0.2 * YR, 12.0 - 0.1 * YR, {1: rng.uniform(260.0, 280.0, n)}
    if name == "terrestrial":
        P = _defaults(L.TC_DEFAULTS, n)
        P[L.TC_PARAM_NAMES.index("beta")] = rng.uniform(0.3, 0.9, n)
        base = np.stack([278.0 * 1.004 ** YR, 0.02 * YR, np.full(T, 0.3)])
        alt = np.stack([400.0 - YR, 1.0 + 0.0 * YR, np.full(T, 1.0)])
        return ra.KIND_TERRESTRIAL_CARBON, P, base, alt, {v + 1: L.TC_DEFAULTS[8 + v] for v in range(4)}
    if name == "halocarbon":
        P = _defaults(L.HC_DEFAULTS, n)
        P[L.HC_PARAM_NAMES.index("HCFC-22.lifetime")] = rng.uniform(8.0, 16.0, n)
        base = np.outer(1.0 + 0.1 * np.arange(41), 1.0 + 0.05 * YR)
        alt = np.outer(0.5 + 0.2 * np.arange(41), np.ones(T))
        return ra.KIND_HALOCARBON, P, base, alt, {s + 1: 100.0 + s for s in range(41)}
    raise KeyError(name)


def _splice(base, alt, k=K):
    """The base forcing up to and including index k (steps before k read no further), the alternative after it."""
    out = np.array(alt, dtype=np.float64, copy=True)
    out[..., :k + 1] = np.asarray(base)[..., :k + 1]
    return out


def _build(ra, kind, n, forcing, mode, P=None, init=None, scen=None, **kw):
    e = ra.Ensemble(kind, n, BOUNDS, **kw)
    e.set_mode(mode)
    if P is not None:
        e.set_params(P)
    e.set_forcing(forcing, scen)
    for v, x in (init or {}).items():
        e.set_initial(v, x)
    return e


def _take(init, anc):
    return {v: (x[anc] if isinstance(x, np.ndarray) else x) for v, x in init.items()}


def _compare(got, want, n_vars, what, first=K + 1):
    for v in range(1, n_vars):
        assert_bit_equal(got.get_series(v, first), want.get_series(v, first), f"{what}: variable {v}")
    assert np.array_equal(got.status(), want.status()), f"{what}: status bytes"


def _n_vars(e):
    return max(e.var_ids.values()) + 1


KINDS = ["two_layer", "coupled", "udeb50", "udeb30", "ocean", "ch4", "n2o", "terrestrial", "halocarbon"]


@pytest.mark.parametrize("name", KINDS)
def test_branch_equals_a_fresh_run_of_the_drawn_parameters(ra, name):
    """Oracle (a), EXACT mode; more draws than members, repeated ancestors, a destination that never had set_params."""
    rng = np.random.default_rng(KINDS.index(name))
    N, M = 96, 150
    kind, P, base, alt, init = _spec(ra, name, N, rng)
    anc = np.sort(rng.integers(0, N, size=M)).astype(np.int64)
    anc[:3] = anc[3]                                                    # a repeated ancestor for sure
    spliced = _splice(base, alt)
    with _build(ra, kind, N, base, ra.MODE_EXACT, P, init) as src, _build(ra, kind, M, spliced, ra.MODE_EXACT) as dst, \
            _build(ra, kind, M, spliced, ra.MODE_EXACT, P[:, anc], _take(init, anc)) as fresh:
        src.run(K)
        src.branch(dst, anc)
        assert dst.time_index == K
        assert_bit_equal(dst.get_params(), P[:, anc], "parameters")
        dst.run()
        fresh.run()
        _compare(dst, fresh, _n_vars(src), name)
        assert np.isfinite(dst.get_series(1, T - 1)).all()
        # the source is untouched and goes on under its own forcing
        src.run()
        with _build(ra, kind, N, base, ra.MODE_EXACT, P, init) as again:
            again.run()
            _compare(src, again, _n_vars(src), f"{name}: the source afterwards", first=0)


@pytest.mark.parametrize("mode_name", ["MODE_EXACT", "MODE_FAST"])
@pytest.mark.parametrize("name", KINDS)
def test_branch_equals_the_host_route(ra, name, mode_name):
    """Oracle (b): checkpoint() -> take along the member axis -> restore(), in both arithmetic modes; fewer draws than members
    through a device vector of ancestors."""
    mode = getattr(ra, mode_name)
    rng = np.random.default_rng(100 + KINDS.index(name))
    N, M = 128, 70
    kind, P, base, alt, init = _spec(ra, name, N, rng)
    w = rng.integers(0, 1 << 30, size=N, dtype=np.int64)
    w[rng.random(N) < 0.4] = 0
    spliced = _splice(base, alt)
    with _build(ra, kind, N, base, mode, P, init) as src, _build(ra, kind, M, spliced, mode) as dst, \
            _build(ra, kind, M, spliced, mode) as host:
        src.run(K)
        src.set_member_weights(w)
        anc_dev = src.resample(M, seed=4)
        anc = anc_dev.to_host()
        assert np.array_equal(anc, hr.ancestors(w, M, hr.offset(4, int(w.sum())))[2])
        src.branch(dst, anc_dev)
        ck = src.checkpoint(all_variables=True)
        ck["n_members"] = M
        ck["params"] = np.ascontiguousarray(ck["params"][:, anc])
        ck["state"] = {k: np.ascontiguousarray(v[anc]) for k, v in ck["state"].items()}
        ck["history"] = {k: np.ascontiguousarray(v[:, anc]) for k, v in ck["history"].items()}
        if ck["internal"] is not None:
            ck["internal"] = np.ascontiguousarray(ck["internal"].reshape(-1, N)[:, anc]).ravel()
        host.restore(ck)
        dst.run()
        host.run()
        _compare(dst, host, _n_vars(src), f"{name} {mode_name}")


def test_posterior_projects_three_scenarios_in_one_run(ra):
    rng = np.random.default_rng(7)
    N, M, S = 500, 200, 3
    kind, P, base, alt, init = _spec(ra, "two_layer", N, rng)
    w = rng.integers(0, 1 << 33, size=N, dtype=np.int64)
    w[rng.random(N) < 0.5] = 0
    scenarios = np.stack([_splice(base, alt), _splice(base, 2.0 * alt), _splice(base, 0.0 * alt)])
    with _build(ra, kind, N, base, ra.MODE_EXACT, P, init) as src:
        src.run(K)
        src.set_member_weights(w)
        dst, scen = src.posterior(lambda n: ra.Ensemble(kind, n, BOUNDS), M, seed=21, scenarios=S)
        with dst:
            assert dst.n_members == M * S and np.array_equal(scen, np.repeat(np.arange(S), M))
            dst.set_forcing(scenarios, scen)
            dst.run()
            anc = hr.ancestors(w, M, hr.offset(21, int(w.sum())))[2]
            assert np.all(w[anc] > 0)
            three = np.tile(anc, S)
            with _build(ra, kind, M * S, scenarios, ra.MODE_EXACT, P[:, three], init, scen=scen) as fresh:
                fresh.run()
                _compare(dst, fresh, 3, "posterior")
            ts = dst.get_series(1, T - 1)[0].reshape(S, M)
            assert not np.array_equal(ts[0], ts[1]) and not np.array_equal(ts[1], ts[2])


def test_blocks_from_two_calls_and_members_never_written(ra):
    rng = np.random.default_rng(8)
    N = 64
    kind, P, base, alt, init = _spec(ra, "n2o", N, rng)
    a1, a2 = np.array([5, 5, 9], dtype=np.int64), np.array([0, 63], dtype=np.int64)
    # (the members no call writes keep the valid parameters and initial rows given here: running them is the caller's business)
    first8 = _take(init, np.arange(8))
    with _build(ra, kind, N, base, ra.MODE_EXACT, P, init) as src, _build(ra, kind, 8, base, ra.MODE_EXACT, P[:, :8], first8) as dst:
        src.run(K)
        src.branch(dst, a2, dst_offset=6)                                # the first call does not start at member 0
        src.branch(dst, a1, dst_offset=1)
        got = dst.get_params()
        assert_bit_equal(got[:, 1:4], P[:, a1], "first block")
        assert_bit_equal(got[:, 6:8], P[:, a2], "second block")
        dst.run()
        src.run()
        want = src.get_series(1, K + 1)
        assert_bit_equal(dst.get_series(1, K + 1)[:, [1, 2, 3, 6, 7]], want[:, [5, 5, 9, 0, 63]], "written members")
        from rscm_amd._lib import ERR_STATE
        with _build(ra, kind, N, base, ra.MODE_EXACT, P, init) as other, _build(ra, kind, 8, base, ra.MODE_EXACT, P[:, :8], first8) as dst2:
            src.rewind()
            src.run(K)
            other.run(K + 2)
            src.branch(dst2, a1, 0)
            assert refusal_code(other.branch, dst2, a2, 4) == ERR_STATE  # a later block from another time index


@pytest.mark.parametrize("window", [None, 16])
def test_graph_branch_of_the_magicc_chain(ra, window):
    """The linked emissions-driven MAGICC graph: GraphModel.branch into a model of another size, full and windowed storage,
    against a fresh model of the drawn parameters run from the start."""
    mod = magicc_chain()
    years, N, M, k = 60, 200, 300, 23
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1 << 30, size=N, dtype=np.int64)
    w[rng.random(N) < 0.3] = 0
    kw = dict(series_window=window, output_stride=6) if window else {}
    src = mod.build_chain(N, years, "topological", **kw)
    for _ in range(k):
        src.step()
    src.set_member_weights(w)
    anc_dev = src.resample(M, seed=3)
    anc = anc_dev.to_host()
    assert np.array_equal(anc, hr.ancestors(w, M, hr.offset(3, int(w.sum())))[2])
    dst = mod.build_chain(M, years, "topological", **kw)
    src.branch(dst, anc_dev)
    assert dst.time_index == k
    dst.run()
    fresh = mod.build_chain(M, years, "topological")
    for owner in ("ClimateUDEB", "TerrestrialCarbon"):
        fresh.ensembles[owner].set_params(np.ascontiguousarray(src.ensembles[owner].get_params()[:, anc]))
    fresh.run()
    names = ["Atmospheric Concentration|CO2", "Atmospheric Concentration|CH4", "Atmospheric Concentration|N2O", "Sea Surface Temperature",
             "Cumulative Ocean Uptake", "Carbon Pool|Soil", "Effective Radiative Forcing", "Carbon Flux|Ocean",
             "Effective Radiative Forcing|O3|Tropospheric"]
    for name in names:
        if window:
            assert_bit_equal(dst.get_series(name, t_begin=24, t_stride=6), fresh.get_series(name)[24::6], f"windowed: {name}")
        else:
            assert_bit_equal(dst.get_series(name)[k + 1:], fresh.get_series(name)[k + 1:], name)
    assert np.isfinite(fresh.get_series("Sea Surface Temperature")[1:]).all()
    for m in (dst, fresh, src):
        m.close()


def test_mismatches_and_bad_ancestors_are_refused(ra):
    from rscm_amd._lib import ERR_INVALID, ERR_STATE
    rng = np.random.default_rng(9)
    N = 32
    kind, P, base, alt, init = _spec(ra, "two_layer", N, rng)
    anc = np.arange(4, dtype=np.int64)

    def refused(dst, code, a=anc, offset=0):
        assert refusal_code(src.branch, dst, a, offset) == code

    with _build(ra, kind, N, base, ra.MODE_EXACT, P, init) as src:
        src.run(K)
        with ra.Ensemble(ra.KIND_COUPLED, 8, BOUNDS) as d:
            refused(d, ERR_INVALID)                                       # another kind
        with ra.Ensemble(kind, 8, BOUNDS + 1.0) as d:
            refused(d, ERR_INVALID)                                       # another axis
        with ra.Ensemble(kind, 8, BOUNDS[:-1]) as d:
            refused(d, ERR_INVALID)
        with ra.Ensemble(kind, 8, BOUNDS) as d:
            d.set_mode(ra.MODE_FAST)
            refused(d, ERR_INVALID)                                       # another mode
        with ra.Ensemble(kind, 8, BOUNDS) as d:
            d.set_step_size(0, 0.05)
            refused(d, ERR_INVALID)                                       # another RK4 step
        with ra.Ensemble(kind, 8, BOUNDS, store_series=False) as d:
            refused(d, ERR_INVALID)                                       # no stored series
        with _build(ra, kind, 8, base, ra.MODE_EXACT, P[:, :8], init) as d:
            before = d.get_params()
            refused(d, ERR_INVALID, np.array([0, N], dtype=np.int64))    # an ancestor out of range
            refused(d, ERR_INVALID, np.array([-1, 2], dtype=np.int64))
            refused(d, ERR_INVALID, anc, offset=5)                        # the block does not fit
            assert_bit_equal(d.get_params(), before, "a refused call writes nothing")
            assert d.time_index == 0
            d.run()
            with d.select(1, [0.5]):
                refused(d, ERR_STATE)                                     # a select in flight on the destination
            src.branch(d, anc, 4)                                         # and the good call still works
            assert d.time_index == K
