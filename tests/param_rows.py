"""Every parameter row of every kind, for the tests that read each row through the uniform and the per-member path
(tests/test_param_rows_cpu.py on the CPU oracles, tests/test_gpu_param_rows.py on the device).

Per kind of _lib.KIND_TABLE: the default parameter vector (one per configuration), a short uneven axis, two input scenarios and the
initial values of the kind's own GPU test, an oracle runner, the tolerances that test asserts, and a class per row:

  continuous  varied as default * U(0.9, 1.1) (U(0.01, 0.1) where the default is 0)
  switch      a small legal set (booleans, Aggregate's operation, integer counts); a varied row draws from the set
  structural  rows include/rscm_gpu.h marks [u]: one value per ensemble, refused when they vary

Pure numpy + oracle/cbind.py: nothing here touches the device.  The tolerances (and the pointwise inputs) are those of the kinds' own
GPU test modules, imported where a kind's description is built -- importing this module imports none of them."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from rscm_amd import _lib as L
from tests import host_lockstep as H
from tests import helpers

N_MEMBERS = 130          # two wavefronts and two lanes
SEED = 0x9A7A
BIT = 0.0                # a tolerance of 0: the same bits


@dataclass
class Spec:
    kind: int
    name: str
    names: Tuple[str, ...]                     # parameter row names
    configs: List[Tuple[str, np.ndarray]]      # (name, default vector): the first is the library's default
    bounds: np.ndarray                         # [T + 1]
    inputs: np.ndarray                         # [2][rows][T], or [2][T] for the kinds with one shared series
    init: Dict[int, float]                     # row 0 of the state variables
    run: Callable[[np.ndarray, np.ndarray], np.ndarray]   # (P [P][N], scen [N]) -> [V - 1][T][N], variables 1 .. V - 1
    tol: Tuple[float, ...]                     # per stored variable, EXACT mode (0: bit equality)
    fast_tol: Optional[Tuple[float, ...]] = None           # per stored variable in RSCM_MODE_FAST (None: the kind has one arithmetic)
    switch: Dict[str, Tuple[float, ...]] = field(default_factory=dict)
    structural: Tuple[str, ...] = ()
    bounded_only: bool = False                 # two-layer / coupled: the tolerance holds on bounded members (tests/test_gpu_parity.py)

    @property
    def P(self) -> int:
        return len(self.names)

    @property
    def T(self) -> int:
        return len(self.bounds) - 1

    @property
    def n_vars(self) -> int:
        return max(L.KIND_TABLE[self.kind][0].values())

    @property
    def light(self) -> bool:
        return self.kind in H.CATALOGUE and H.CATALOGUE[self.kind].light

    def row_class(self, j: int) -> str:
        nm = self.names[j]
        return "structural" if nm in self.structural else ("switch" if nm in self.switch else "continuous")

    def free_rows(self) -> List[int]:
        return [j for j in range(self.P) if self.row_class(j) != "structural"]

    def default(self, config: int = 0) -> np.ndarray:
        return self.configs[config][1]


def varied_block(spec: Spec, n: int, config: int = 0, seed: int = SEED) -> np.ndarray:
    """[P][n]: every non-structural row drawn per member by its class; member 1 differs from member 0 in every such row."""
    rng = np.random.default_rng([seed, spec.kind, config])
    d = spec.default(config)
    V = np.repeat(d.reshape(-1, 1), n, axis=1)
    for j in range(spec.P):
        cls = spec.row_class(j)
        if cls == "continuous":
            V[j] = d[j] * rng.uniform(0.9, 1.1, n) if d[j] != 0.0 else rng.uniform(0.01, 0.1, n)
        elif cls == "switch":
            legal = np.asarray(spec.switch[spec.names[j]], dtype=np.float64)
            V[j] = rng.choice(legal, n)
            if n > 1:   # (really varied, and the default's neighbour present)
                others = legal[legal != d[j]]
                V[j, 0], V[j, 1] = d[j] if d[j] in legal else legal[0], others[0]
    return V


def block(spec: Spec, V: np.ndarray, varied, config: int = 0) -> np.ndarray:
    """The configuration's defaults for every member, the rows `varied` (indices or a boolean mask) taken from V."""
    P = np.repeat(spec.default(config).reshape(-1, 1), V.shape[1], axis=1)
    rows = np.flatnonzero(varied) if np.asarray(varied).dtype == bool else np.asarray(varied, dtype=np.int64)
    P[rows] = V[rows]
    return np.ascontiguousarray(P)


def scen_map(n: int) -> np.ndarray:
    return (np.arange(n) % 2).astype(np.int32)


def random_masks(spec: Spec, count: int = 8, seed: int = SEED) -> List[np.ndarray]:
    """`count` seeded masks over the non-structural rows and their complements (True: the row varies)."""
    rng = np.random.default_rng([seed, spec.kind, 77])
    free = np.asarray(spec.free_rows())
    out = []
    for _ in range(count):
        m = np.zeros(spec.P, dtype=bool)
        m[free] = rng.random(len(free)) < 0.5
        c = np.zeros(spec.P, dtype=bool)
        c[free] = ~m[free]
        out += [m, c]
    return out


def deviation(spec: Spec, got: np.ndarray, want: np.ndarray, what: str, fast: bool = False) -> float:
    """Asserts the NaN pattern, bit equality for the variables that carry it and the tolerance for the others; returns the worst
    deviation relative to max(1, |oracle|) over the variables with a tolerance."""
    tol = spec.fast_tol if fast else spec.tol
    assert got.shape == want.shape, (what, got.shape, want.shape)
    keep = np.ones(want.shape[2], dtype=bool)
    if spec.bounded_only:
        with np.errstate(all="ignore"):
            keep = np.isfinite(want[0][-1]) & (np.nanmax(np.abs(want[0]), axis=0) < 50.0)
        assert keep.all(), f"{what}: +-10 % around the defaults leaves every member bounded"
    worst = 0.0
    for v in range(want.shape[0]):
        g, w = got[v][:, keep], want[v][:, keep]
        if tol[v] == BIT:
            helpers.assert_bit_equal(g, w, f"{what}: variable {v + 1}")
            continue
        assert (np.isnan(g) == np.isnan(w)).all(), f"{what}: variable {v + 1}: NaN pattern"
        ok = ~np.isnan(w)
        if ok.any():
            err = float((np.abs(g[ok] - w[ok]) / np.maximum(1.0, np.abs(w[ok]))).max())
            assert err <= tol[v], f"{what}: variable {v + 1}: max deviation {err:.3e} > {tol[v]:g}"
            worst = max(worst, err)
    return worst


# ------------------------------------------------------------------------------------------------ the kinds
def _uneven(T: int, every: int, at: int, short: float, start: float = 1750.0) -> np.ndarray:
    return np.concatenate([[start], start + np.cumsum(np.where(np.arange(T) % every == at, short, 1.0))])


def _even(T: int, start: float = 1750.0) -> np.ndarray:
    return np.arange(T + 1, dtype=np.float64) + start


def _with(p: np.ndarray, names, **over) -> np.ndarray:
    q = p.copy()
    for k, v in over.items():
        q[names.index(k)] = v
    return q


def _two_layer() -> Spec:
    from tests.test_gpu_parity import FAST_RTOL
    from oracle import cbind as orc
    T = 25
    t = 1990.0 + np.arange(T, dtype=np.float64)
    F = np.stack([helpers.f_syn(t), 0.6 * helpers.f_syn(t)])
    b = np.append(t, t[-1] + 1.0)
    d = H.default_params(L.KIND_TWO_LAYER, 1, None)[:, 0]

    def run(P, scen):
        return np.stack(orc.two_layer_run(b, P, F, 0.0, 0.0, scen=scen))
    return Spec(L.KIND_TWO_LAYER, "TwoLayer", ("lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep"),
                [("default", d)], b, F, {1: 0.0, 2: 0.0}, run, (BIT, BIT), (FAST_RTOL, FAST_RTOL), bounded_only=True)


CP_STATE_INIT = {1: 0.0, 2: 0.0, 3: 278.0, 4: 0.0, 5: 0.0}


def _coupled() -> Spec:
    from tests.test_gpu_parity import FAST_RTOL
    from oracle import cbind as orc
    T = 25
    t = 1990.0 + np.arange(T, dtype=np.float64)
    E = np.stack([helpers.emissions_syn(t), np.abs(np.random.default_rng(5000).normal(3.0, 3.0, T))])
    b = np.append(t, t[-1] + 1.0)
    tl, cc, ce = (H.default_params(k, 1, None)[:, 0] for k in (L.KIND_TWO_LAYER, L.KIND_CARBON_CYCLE, L.KIND_CO2_ERF))
    d = np.concatenate([tl, cc, ce[:1]])   # the six two-layer rows, tau, conc_pi, alpha_temperature, erf_2xco2 (include/rscm_gpu.h)

    def run(P, scen):
        o = orc.coupled_run(b, P, E, dict(ts=0.0, td=0.0, conc=278.0, cum_uptake=0.0, cum_emis=0.0), scen=scen)
        return np.stack([o[k] for k in orc.COUPLED_VARS])
    tol = tuple(BIT if k == "cum_emis" else FAST_RTOL for k in orc.COUPLED_VARS)   # (test_coupled_vs_oracle, either mode)
    return Spec(L.KIND_COUPLED, "Coupled", ("lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep", "tau",
                                            "conc_pi", "alpha_temperature", "erf_2xco2"),
                [("default", d)], b, E, dict(CP_STATE_INIT), run, tol, tol, bounded_only=True)


UDEB_STRUCTURAL = ("n_layers", "mixed_layer_depth", "layer_thickness", "feedback_cumt_period", "depth_dependent_area",
                   "land_heat_capacity_enabled", "efficacy_apply", "ocean_temp_profile", "steps_per_year")


def udeb_spec(T: int = 13) -> Spec:
    from tests.test_gpu_udeb import RTOL as UDEB_RTOL
    from oracle import cbind as orc
    years = np.arange(1850.0, 1850.0 + T)
    b = np.append(years, years[-1] + 1.0)
    F = np.stack([np.where(years >= 1851, 3.71, 0.0), 3.71 * np.log(np.where(years > 1850, 1.01 ** (years - 1850), 1.0)) / np.log(2.0)])
    names = orc.UDEB_PARAM_NAMES
    d = orc.udeb_default_params()
    # the efficacy rows act when efficacy_apply is on; the floor of kappa and the temperature cap where the run reaches them
    second = _with(d, names, efficacy_apply=1.0, kappa_min=0.9, max_temperature=0.5)

    def run(P, scen):
        o, _ = orc.udeb_run(b, P, F, scen=scen, threads=8)
        return np.stack([o[k] for k in orc.UDEB_VARS])
    return Spec(L.KIND_UDEB, "ClimateUDEB", names, [("default", d), ("efficacy, kappa floor and temperature cap in reach", second)], b, F,
                {k: 0.0 for k in range(1, 5)}, run, (UDEB_RTOL,) * 7, (UDEB_RTOL,) * 7, structural=UDEB_STRUCTURAL)


def _ghg() -> Spec:
    from tests.test_gpu_ghg import TOL as GHG_TOL
    from oracle import cbind as orc
    T = 25
    yr = np.arange(T) * 14.0   # (the span of the 351-year scenarios of tests/test_gpu_ghg.py: all three alpha regimes occur)
    conc = np.stack([np.stack([278.0 * 1.006 ** yr, 722.0 + 6.0 * yr, 270.0 + 0.4 * yr]),
                     np.stack([300.0 - 0.2 * yr, 800.0 - 0.5 * yr, 275.0 - 0.05 * yr])])

    def run(P, scen):
        o = orc.ghg_run(T, P, conc, scen=scen)
        return np.stack([o[k] for k in orc.GHG_VARS])
    return Spec(L.KIND_GHG_FORCING, "GhgForcing", orc.GHG_PARAM_NAMES,
                [("Olbl", orc.ghg_default_params(method="Olbl")), ("Ipcctar", orc.ghg_default_params(method="Ipcctar"))],
                _even(T), conc, {}, run, (GHG_TOL,) * 3, structural=("method",))


def _pointwise(kind: int) -> Spec:
    from tests.test_gpu_pointwise import TOL as PW_TOL
    from tests.test_gpu_pointwise import _inputs as pointwise_inputs
    from oracle import cbind as orc
    T = 25
    inputs = pointwise_inputs(kind, orc, T, None)
    names = orc.PW_PARAM_NAMES[kind]
    d = orc.pointwise_default_params(kind)
    n_out = {orc.PW_OZONE: 3, orc.PW_AEROSOL_DIRECT: 4, orc.PW_AEROSOL_INDIRECT: 1, orc.PW_FOURBOX_OHU: 4, orc.PW_OSPP: 1}[kind]
    # AerosolDirect and FourBoxOHU involve no transcendental, the ozone temperature feedback is one multiply: the same bits
    tol = {orc.PW_OZONE: (PW_TOL, PW_TOL, BIT), orc.PW_AEROSOL_DIRECT: (BIT,) * 4, orc.PW_FOURBOX_OHU: (BIT,) * 4}.get(kind, (PW_TOL,) * n_out)
    configs = [("default", d)]
    # (no configuration with harmonisation on: no solve reads the three harmonize rows, DEAD_ROWS below)
    switch = {"harmonize": (0.0, 1.0)} if kind in (orc.PW_AEROSOL_DIRECT, orc.PW_AEROSOL_INDIRECT) else {}

    def run(P, scen):
        return orc.pointwise_run(kind, T, P, inputs, scen=scen)
    return Spec(kind, H.CATALOGUE[kind].name, names, configs, _even(T), inputs, {}, run, tol, switch=switch)


def _chem(kind: int) -> Spec:
    from tests.test_gpu_chem import TOL as CHEM_TOL
    from oracle import cbind as orc
    T = 25
    yr = np.arange(T, dtype=float)
    b = _uneven(T, 7, 3, 0.5)
    names = orc.CHEM_PARAM_NAMES[kind]
    if kind == orc.CHEM_CH4:
        inputs = np.stack([np.stack([150.0 + 0.8 * yr, 0.008 * yr, 5.0 + 0.1 * yr, 200.0 + yr, 50.0 + 0.2 * yr]),
                           np.stack([400.0 - 0.5 * yr, np.sin(yr / 9.0), 40.0 - 0.05 * yr, 600.0 - yr, 120.0 - 0.1 * yr])])
        c0, switch = 722.0, {"include_temp_feedback": (0.0, 1.0), "include_emissions_feedback": (0.0, 1.0)}
    else:
        inputs = np.stack([(0.02 * yr)[None], (8.0 - 0.01 * yr)[None]])
        c0, switch = 270.0, {"strat_delay": (0.0, 1.0, 2.0, 3.0, 4.0)}

    def run(P, scen):
        return np.stack(orc.chem_run(kind, b, P, inputs, c0, scen=scen))
    return Spec(kind, H.CATALOGUE[kind].name, names, [("default", orc.chem_default_params(kind))], b, inputs, {1: c0}, run,
                (CHEM_TOL, CHEM_TOL), switch=switch)


def _carbon(kind: int) -> Spec:
    from tests.test_gpu_carbon import PI_POOLS
    from tests.test_gpu_carbon import TOL as CARBON_TOL
    from oracle import cbind as orc
    T = 25
    yr = np.arange(T, dtype=float) * 12.0   # (the span of the 301-year scenarios of tests/test_gpu_carbon.py)
    b = _uneven(T, 5, 2, 0.25)
    names = orc.CARBON_PARAM_NAMES[kind]
    if kind == orc.CARBON_BUDGET:
        inputs = np.stack([np.stack([0.03 * yr, 1.0 - 0.002 * yr, 0.01 * yr, 0.012 * yr]),
                           np.stack([np.where(yr < 50, 0.0, 5.0), np.where(yr < 50, 0.0, -6.0 + 0.05 * yr), 0.5 + 0 * yr, 0.7 + 0 * yr])])
        init, tol, switch = {1: 278.0}, (BIT,) * 3, {}
    else:
        inputs = np.stack([np.stack([278.0 * 1.004 ** yr, 0.012 * yr, np.where(yr > 100, 1.5, 0.2)]),
                           np.stack([np.maximum(500.0 - 2.0 * yr, 0.0), 3.0 * np.sin(yr / 15.0), 40.0 + 0 * yr])])
        init, tol = {k + 1: float(PI_POOLS[k]) for k in range(4)}, (CARBON_TOL,) * 5
        switch = {"enable_fertilization": (0.0, 1.0), "enable_temp_feedback": (0.0, 1.0)}
    first = [init[v] for v in sorted(init)]

    def run(P, scen):
        return orc.carbon_run(kind, b, P, inputs, first, scen=scen)
    return Spec(kind, H.CATALOGUE[kind].name, names, [("default", orc.carbon_default_params(kind))], b, inputs, init, run, tol, switch=switch)


OCEAN_STRUCTURAL = ("model", "irf_scale", "steps_per_year", "max_history_months", "irf_switch_time")


def _ocean() -> Spec:
    from tests.test_gpu_ocean import FAST_TOL as OCEAN_FAST_TOL
    from tests.test_gpu_ocean import TOL as OCEAN_TOL
    from oracle import cbind as orc
    T = 13
    yr = np.arange(T, dtype=float) * 5.0
    b = _uneven(T, 6, 1, 0.5)
    inputs = np.stack([np.stack([278.0 * 1.006 ** yr, 0.01 * yr]),
                       np.stack([np.where(yr < 30, 400.0, 300.0), np.where(yr < 30, 1.0, -0.5)])])

    def run(P, scen):
        return orc.ocean_run(b, P, inputs, 278.0, 5.0, scen=scen, threads=8)
    return Spec(L.KIND_OCEAN_CARBON, "OceanCarbon", orc.OCEAN_PARAM_NAMES, [("3D-GFDL", orc.ocean_default_params("3D-GFDL"))], b, inputs,
                {1: 278.0, 2: 5.0}, run, (OCEAN_TOL,) * 3, (OCEAN_FAST_TOL,) * 3, switch={"enable_temp_feedback": (0.0, 1.0)},
                structural=OCEAN_STRUCTURAL)


def _halocarbon() -> Spec:
    from tests.test_gpu_halocarbon import TOL as HALO_TOL
    from oracle import cbind as orc
    T = 25
    rng = np.random.default_rng(1)
    yr = np.arange(T, dtype=float) * 5.0
    b = _uneven(T, 9, 4, 0.5, 1900.0)
    E = np.stack([rng.uniform(0.0, 1.0, (41, 1)) * np.maximum(80.0 - np.abs(yr - 70.0), 0.0), rng.uniform(0.0, 40.0, (41, T))])
    names = tuple(L.HC_PARAM_NAMES)
    d = orc.halo_default_params()
    c0 = np.array([d[orc.halo_index(s, "concentration_pi")] for s in orc.HALO_SPECIES]) + rng.uniform(0.0, 5.0, 41)
    second = d.copy()
    for s in orc.HALO_SPECIES:   # every species releases chlorine and bromine: its three EESC rows all act
        second[orc.halo_index(s, "n_cl")] = second[orc.halo_index(s, "n_br")] = 1.0
        second[orc.halo_index(s, "fractional_release")] = 0.5
    switch = {"eesc_delay": (1.0, 2.0, 3.0, 4.0, 5.0)}
    for s in orc.HALO_SPECIES:
        switch[f"{s}.n_cl"] = (0.0, 1.0, 2.0, 3.0, 4.0)
        switch[f"{s}.n_br"] = (0.0, 1.0, 2.0)

    def run(P, scen):
        return orc.halo_run(b, P, E, c0, scen=scen, threads=4)
    return Spec(L.KIND_HALOCARBON, "HalocarbonChemistry", names, [("default", d), ("every species releases Cl and Br", second)], b, E,
                {s + 1: float(c0[s]) for s in range(41)}, run, (HALO_TOL,) * 45, switch=switch)


def _carbon_cycle() -> Spec:
    from tests.test_gpu_parity import FAST_RTOL
    from oracle import cbind as orc
    T = 25
    rng = np.random.default_rng(9)
    b = 1750.0 + np.concatenate([[0.0], np.cumsum(np.where(np.arange(T) % 4 == 1, 0.5, 1.0))])
    inputs = np.stack([np.stack([np.abs(rng.normal(4.0, 2.0, T)), np.cumsum(rng.normal(0.02, 0.05, T))]) for _ in range(2)])

    def run(P, scen):
        N = P.shape[1]
        out = np.full((3, T, N), np.nan)
        for i in range(N):
            y = np.array([278.0, 0.0, 0.0])
            out[:, 0, i] = y
            for k in range(T - 1):
                y = orc.carbon_cycle_solve(P[:, i], inputs[scen[i], 0, k], inputs[scen[i], 1, k], b[k], b[k + 1], 0.1, y)
                out[:, k + 1, i] = y
        return out
    # the carbon box of the coupled kind on its own: that kind's bar (include/rscm_gpu.h, RSCM_MODE_FAST), cumulative emissions bit for bit
    tol = (FAST_RTOL, FAST_RTOL, BIT)
    return Spec(L.KIND_CARBON_CYCLE, "CarbonCycle", L.CC_PARAM_NAMES, [("default", H.default_params(L.KIND_CARBON_CYCLE, 1, None)[:, 0])], b, inputs,
                {1: 278.0, 2: 0.0, 3: 0.0}, run, tol, tol)


def _co2_erf() -> Spec:
    from oracle import cbind as orc
    T = 25
    yr = np.arange(T, dtype=float)
    inputs = np.stack([(280.0 + 4.0 * yr)[None], (300.0 - 2.0 * yr)[None]])   # above and below the pre-industrial concentration

    def run(P, scen):
        N = P.shape[1]
        out = np.full((1, T, N), np.nan)
        for i in range(N):
            for k in range(T - 1):
                out[0, k + 1, i] = orc.co2_erf(P[0, i], P[1, i], inputs[scen[i], 0, k])
        return out
    tol = H.CATALOGUE[L.KIND_CO2_ERF].tol
    return Spec(L.KIND_CO2_ERF, "CO2ERF", L.CE_PARAM_NAMES, [("default", H.default_params(L.KIND_CO2_ERF, 1, None)[:, 0])], _even(T), inputs, {}, run, (tol,))


def _aggregate() -> Spec:
    T = 25
    yr = np.arange(T, dtype=float)
    rows = np.stack([H.EXO["erf"](yr) * (1.0 + 0.1 * r) for r in range(8)])
    other = np.stack([np.sin(yr / (3.0 + r)) for r in range(8)])
    other[7] = np.nan                       # a contributor that is missing in scenario 1: skipped
    other[2, 5] = np.nan                    # and one missing at a single row
    inputs = np.stack([rows, other])
    d = H.default_params(L.KIND_AGGREGATE, 1, None, op=H.OPS["Sum"])[:, 0]

    def run(P, scen):
        """compute_aggregate restated (host_lockstep.recompute), the operation per member; every contributor read at n + 1."""
        N = P.shape[1]
        out = np.full((1, T, N), np.nan)
        x = inputs[scen]   # [N][8][T]
        op = P[0]
        for n in range(T - 1):
            acc, cnt = np.zeros(N), np.zeros(N)
            for r in range(8):
                v = x[:, r, n + 1]
                ok = ~np.isnan(v)
                acc = np.where(ok, acc + np.where(op == 2.0, v * P[1 + r], v), acc)
                cnt += ok
            out[0, n + 1] = np.where(cnt > 0, np.where(op == 1.0, acc / np.maximum(cnt, 1.0), acc), np.nan)
        return out
    tol = H.CATALOGUE[L.KIND_AGGREGATE].tol
    return Spec(L.KIND_AGGREGATE, "Aggregate", L.AG_PARAM_NAMES, [("Sum", d), ("Weighted", _with(d, L.AG_PARAM_NAMES, operation=2.0))],
                _even(T), inputs, {}, run, (tol,), switch={"operation": (0.0, 1.0, 2.0)})


_BUILDERS = {
    L.KIND_TWO_LAYER: _two_layer, L.KIND_COUPLED: _coupled, L.KIND_UDEB: udeb_spec, L.KIND_GHG_FORCING: _ghg,
    L.KIND_OZONE_FORCING: lambda: _pointwise(L.KIND_OZONE_FORCING), L.KIND_AEROSOL_DIRECT: lambda: _pointwise(L.KIND_AEROSOL_DIRECT),
    L.KIND_AEROSOL_INDIRECT: lambda: _pointwise(L.KIND_AEROSOL_INDIRECT), L.KIND_CH4_CHEMISTRY: lambda: _chem(L.KIND_CH4_CHEMISTRY),
    L.KIND_N2O_CHEMISTRY: lambda: _chem(L.KIND_N2O_CHEMISTRY), L.KIND_CO2_BUDGET: lambda: _carbon(L.KIND_CO2_BUDGET),
    L.KIND_TERRESTRIAL_CARBON: lambda: _carbon(L.KIND_TERRESTRIAL_CARBON), L.KIND_OCEAN_CARBON: _ocean, L.KIND_HALOCARBON: _halocarbon,
    L.KIND_FOURBOX_OHU: lambda: _pointwise(L.KIND_FOURBOX_OHU), L.KIND_OSPP: lambda: _pointwise(L.KIND_OSPP),
    L.KIND_CARBON_CYCLE: _carbon_cycle, L.KIND_CO2_ERF: _co2_erf, L.KIND_AGGREGATE: _aggregate,
}
KINDS = tuple(sorted(_BUILDERS))
KIND_NAMES = {L.KIND_TWO_LAYER: "TwoLayer", L.KIND_COUPLED: "Coupled", L.KIND_UDEB: "ClimateUDEB",
              **{k: v.name for k, v in H.CATALOGUE.items()}}
_SPECS: Dict[int, Spec] = {}


def spec(kind: int) -> Spec:
    if kind not in _SPECS:
        _SPECS[kind] = _BUILDERS[kind]()
    return _SPECS[kind]


# Rows that change no output in any configuration: carried by the parameter block, read by no solve -- neither the oracle's nor the
# reference's (include/rscm_gpu.h: "carried but unused by solve, as upstream").  tests/test_param_rows_cpu.py re-derives these sets.
DEAD_ROWS = {
    L.KIND_AEROSOL_DIRECT: frozenset({"harmonize", "harmonize_year", "harmonize_target"}),
    L.KIND_AEROSOL_INDIRECT: frozenset({"harmonize", "harmonize_year", "harmonize_target"}),
    L.KIND_HALOCARBON: frozenset({"eesc_delay"}),
    L.KIND_CO2_BUDGET: frozenset({"co2_pi"}),
    L.KIND_OCEAN_CARBON: frozenset({"co2_pi"}),
}
# Of these, the rows whose class is continuous: the two settings of a harmonisation no solve performs, and the pre-industrial
# concentration that CO2Budget and OceanCarbon carry without reading it (OceanCarbon works from pco2_pi).
DEAD_CONTINUOUS = {
    L.KIND_AEROSOL_DIRECT: frozenset({"harmonize_year", "harmonize_target"}),
    L.KIND_AEROSOL_INDIRECT: frozenset({"harmonize_year", "harmonize_target"}),
    L.KIND_CO2_BUDGET: frozenset({"co2_pi"}),
    L.KIND_OCEAN_CARBON: frozenset({"co2_pi"}),
}


def liveness(sp: Spec, V: List[np.ndarray], n: int = N_MEMBERS) -> np.ndarray:
    """[configurations][P] bool: varying that row alone changes the oracle's output in that configuration (structural rows: False)."""
    scen = scen_map(n)
    live = np.zeros((len(sp.configs), sp.P), dtype=bool)
    for c in range(len(sp.configs)):
        base = sp.run(block(sp, V[c], [], c), scen)
        for j in sp.free_rows():
            live[c, j] = not helpers.same_values(sp.run(block(sp, V[c], [j], c), scen), base)
    return live


def live_config(live: np.ndarray) -> Dict[int, int]:
    """Per row that is live somewhere: the first configuration in which it is."""
    return {int(j): int(np.argmax(live[:, j])) for j in np.flatnonzero(live.any(axis=0))}
