"""GPU tier (-m gpu): the EXACT year of the coupled chain, bit for bit, for every member.

The fused kind (csrc/coupled.hip, year<SPEC>) and the stand-alone CarbonCycle (csrc/carbon_body.hpp) run every model year
speculatively -- three-instruction quotients, exponent-window tags folded into one accumulator -- and replay the year in IEEE
division when a tag falls outside.  tests/test_gpu_parity.py holds them to the oracle at 1e-11 on bounded members, because one exp
and one log per member-year come from the device and not from glibc.  Here those two values are taken from the device as well
(rscm_amd.ensemble.selftest_math: op 2, the library's exp; op 0, log_f64) and fed into the plain IEEE restatement of the year in
tests/host_coupled.py, which tests/test_host_coupled.py holds to the oracle bit for bit with glibc's exp / log in their place.
Every output row of every member must then carry the restatement's bits (any NaN equals any NaN; zeros and infinities keep their
signs), and the status bytes its flag: no tolerance, no mask.  RSCM_MODE_EXACT only; the FAST arithmetic is its own and stays
with test_gpu_parity.py.

The edge ensemble (host_coupled.edge_ensemble; what it reaches is asserted in tests/test_host_coupled.py) has replays after
year 0, numerators on both sides of 2^-511 and 2^513, lifetimes and heat capacities on both sides of 2^-128 and 2^129, years
that start with Ts = NaN, members that run away through the window to overflow, inf and NaN states and forcings, in lanes that
share wavefronts with members whose speculative years stand."""
import ctypes as C

import numpy as np
import pytest

from tests import host_coupled as hc
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

NAMES = {"ts": "Surface Temperature", "td": "Deep Ocean Temperature", "conc": "Atmospheric Concentration|CO2",
         "cum_uptake": "Cumulative Land Uptake", "cum_emis": "Cumulative Emissions|CO2", "erf_co2": "Effective Radiative Forcing|CO2",
         "erf_total": "Effective Radiative Forcing"}
STATES = ("ts", "td", "conc", "cum_uptake", "cum_emis")


@pytest.fixture(scope="module")
def device_math(ra):
    """exp and log as the kernels evaluate them: the device library's exp and log_f64 through the self-test hook."""
    from rscm_amd.ensemble import selftest_math

    def on_device(op):
        return lambda x: selftest_math(op, np.ascontiguousarray(x, dtype=np.float64)).reshape(np.shape(x))
    return dict(exp=on_device(2), log=on_device(0))


@pytest.fixture(scope="module")
def edge():
    return hc.edge_ensemble()


def _restate(c, device_math, scen="own"):
    return hc.coupled(c["bounds"], c["P"], c["E"], c["init"], scen=c["scen"] if scen == "own" else scen, h_tl=c["h_tl"], h_cc=c["h_cc"],
                      **device_math)


@pytest.fixture(scope="module")
def edge_want(edge, device_math):
    return _restate(edge, device_math)


def _fused(ra, c, scen, cuts=()):
    with ra.Ensemble(ra.KIND_COUPLED, c["N"], c["bounds"]) as e:
        e.set_mode(ra.MODE_EXACT)
        e.set_step_size(0, c["h_tl"])
        e.set_step_size(1, c["h_cc"])
        e.set_params(c["P"])
        e.set_forcing(c["E"], scen)
        for key in STATES:
            e.set_initial(NAMES[key], c["init"][key])
        for cut in cuts:
            if cut > e.time_index:
                e.run(cut)
        e.run()
        assert e.finished()
        return {key: e.get_series(name) for key, name in NAMES.items()}, e.status()


def _assert_is(got, status, want, what):
    for key in hc.SERIES:
        assert_bit_equal(got[key], want[key], f"{what}: {key}")
    assert np.array_equal(status != 0, hc.status(want) != 0), what


# ------------------------------------------------------------------------------------------------ the fused kind
@pytest.mark.parametrize("cuts", [(), (1, 6)], ids=["one launch", "cut at 1 and 6"])
def test_fused_kind_on_the_edge_ensemble(ra, edge, edge_want, cuts):
    """One launch; and cut at steps 1 and 6, where the resumed launches read stored rows that hold inf and NaN."""
    got, st = _fused(ra, edge, edge["scen"], cuts)
    _assert_is(got, st, edge_want, f"fused kind, cuts {cuts}")


def test_fused_kind_on_the_edge_ensemble_without_a_scenario_map(ra, edge, device_math):
    got, st = _fused(ra, edge, None)
    _assert_is(got, st, _restate(edge, device_math, scen=None), "fused kind, no scenario map")


@pytest.mark.parametrize("seed", range(10))
def test_fused_kind_on_the_fuzz_configurations(ra, device_math, seed):
    """The ten configurations of test_gpu_parity.py::test_coupled_chain_fuzz, all members, all seven series, the status bytes."""
    c = hc.fuzz_config(seed)
    got, st = _fused(ra, c, c["scen"], c["cuts"])
    _assert_is(got, st, _restate(c, device_math), f"seed {seed} (T={c['T']}, n={c['N']}, h_tl={c['h_tl']}, h_cc={c['h_cc']}, cuts={c['cuts']})")


# ------------------------------------------------------------------------------------------------ four linked handles
class _Graph:
    """The edge ensemble as CarbonCycle, CO2ERF, Sum and TwoLayer handles wired as tests/test_gpu_links.py::_coupled_graph."""

    def __init__(self, ra, c):
        from rscm_amd import _lib as L
        self.L, self.stream = L, C.c_void_p()
        L.check(L.load().rscm_gpu_stream_create(0, C.byref(self.stream)))
        N, b, P, T = c["N"], c["bounds"], c["P"], c["T"]
        self.cc, self.ce, self.ag, self.tl = (ra.Ensemble(k, N, b) for k in (ra.KIND_CARBON_CYCLE, ra.KIND_CO2_ERF, ra.KIND_AGGREGATE,
                                                                             ra.KIND_TWO_LAYER))
        cc, ce, ag, tl = self.order = (self.cc, self.ce, self.ag, self.tl)
        for e in self.order:
            e.set_stream(self.stream.value)
            e.set_mode(ra.MODE_EXACT)
        cc.set_step_size(1, c["h_cc"])
        tl.set_step_size(0, c["h_tl"])
        cc.set_params(P[[6, 7, 8]])
        ce.set_params(P[[9, 7]])
        ag.set_params(np.zeros((9, N)))   # Sum
        tl.set_params(P[:6])
        cc.set_forcing(np.stack([np.stack([row, np.full(T, np.nan)]) for row in c["E"]]), c["scen"])
        for key in ("conc", "cum_uptake", "cum_emis"):
            cc.set_initial(NAMES[key], c["init"][key])
        for key in ("ts", "td"):
            tl.set_initial(NAMES[key], c["init"][key])
        cc.link_input("Surface Temperature", tl, "Surface Temperature", ra.SRC_EXOGENOUS)
        ce.link_input(0, cc, NAMES["conc"], ra.SRC_UPSTREAM)
        ag.link_input(0, ce, NAMES["erf_co2"], ra.SRC_UPSTREAM)
        tl.link_input(0, ag, "aggregate", ra.SRC_UPSTREAM)

    def fresh(self):
        for e in self.order:
            e.rewind()
            e.clear_series()

    def collect(self):
        return dict(ts=self.tl.get_series(1), td=self.tl.get_series(2), conc=self.cc.get_series(1), cum_uptake=self.cc.get_series(2),
                    cum_emis=self.cc.get_series(3), erf_co2=self.ce.get_series(1), erf_total=self.ag.get_series(1))

    def status(self):
        return self.cc.status() | self.tl.status()

    def close(self):
        self.cc.unlink_input("Surface Temperature")   # the feedback edge is cut by hand, then consumers first
        for e in (self.tl, self.ag, self.ce, self.cc):
            e.close()
        self.L.check(self.L.load().rscm_gpu_stream_destroy(0, self.stream))


def test_four_linked_handles_on_the_edge_ensemble(ra, edge, edge_want):
    """Stepped component by component, and through run_lockstep in every launch shape: one launch per component and step (fusion
    mode 0), the graph's own sequence kernel for all steps in one launch (mode 1: group_seq_kernel<SeqCoupled>), the op interpreter
    for all steps in one launch without and with the device-side op table (modes 2 and 3), and one-step fused launches.  Each time
    the restatement's bits, hence the fused kind's: "linked == fused" for replaying members too, with inf / NaN per-member forcing
    through TwoLayer's linked path."""
    from rscm_amd import _lib as L
    from rscm_amd.ensemble import run_lockstep
    lib = L.load()
    g = _Graph(ra, edge)
    steps = edge["T"] - 1

    def stats():
        a, b = C.c_int64(), C.c_int64()
        L.check(lib.rscm_gpu_lockstep_stats(C.byref(a), C.byref(b)))
        return a.value, b.value

    try:
        for n in range(steps):   # Model::step: every component once, in graph order
            for e in g.order:
                e.run(n + 1, sync=False)
        g.tl.sync()
        _assert_is(g.collect(), g.status(), edge_want, "component by component")
        for mode, launches in ((0, 4 * steps), (1, 1), (2, None), (3, None)):
            g.fresh()
            L.check(lib.rscm_gpu_set_lockstep_fusion(mode))
            stats()
            run_lockstep(g.order)
            counted = stats()
            assert counted[1] == 4 * steps and launches in (None, counted[0]), (mode, counted)
            _assert_is(g.collect(), g.status(), edge_want, f"run_lockstep, fusion mode {mode}")
        g.fresh()
        L.check(lib.rscm_gpu_set_lockstep_fusion(1))
        for n in range(steps):
            run_lockstep(g.order, n + 1, sync=False)
        g.tl.sync()
        _assert_is(g.collect(), g.status(), edge_want, "run_lockstep, one step per call")
    finally:
        L.check(lib.rscm_gpu_set_lockstep_fusion(1))
        g.close()


# ------------------------------------------------------------------------------------------------ the kinds on their own
def test_carbon_cycle_kind_with_table_inputs(ra, edge, device_math):
    """96 members, eight scenarios of (emissions, temperature) rows on the edge ensemble's axis, cut at step 7.  The temperature rows
    hold 0, tame values, +-inf, NaN and +-1e5 (exp(alpha T) overflows / underflows to 0: lifetime inf / 0); tau sits on both sides of
    both edges of the divisor window, with the drawn alpha (the lifetime straddles the edge as T varies) and with alpha = 0 (the
    lifetime is tau, or NaN against an infinite T); a few members start at C == C_pi (a zero numerator)."""
    b, T, N, S, h = edge["bounds"], edge["T"], 96, 8, edge["h_cc"]
    rng = np.random.default_rng(20261021)
    E = np.abs(rng.normal(3.0, 3.0, (S, T)))
    Temp = rng.normal(0.5, 1.0, (S, T))
    Temp[0, 2] = 0.0
    Temp[1, 5], Temp[2, 3], Temp[3, 6], Temp[4, 4], Temp[5, 8] = np.inf, -np.inf, np.nan, 1e5, -1e5
    Temp[7] = 0.0
    scen = (np.arange(N) % S).astype(np.int32)
    P3 = np.stack([rng.uniform(15.0, 40.0, N), rng.uniform(260.0, 300.0, N), rng.uniform(0.0, 0.1, N)])
    edges = (2.0 ** -128, hc.below(2.0 ** -128), 2.0 ** 129, hc.below(2.0 ** 129))
    for i in range(64):
        P3[0, i] = edges[(i // 8) % 4]
        if i >= 32:
            P3[2, i] = 0.0
    init = dict(conc=P3[1] + rng.uniform(1.0, 30.0, N), cum_uptake=rng.uniform(0.0, 5.0, N), cum_emis=1.5)
    init["conc"][64:72] = P3[1, 64:72]
    want = hc.carbon_cycle(b, P3, E[scen].T, Temp[scen].T, init, h=h, exp=device_math["exp"])
    with ra.Ensemble(ra.KIND_CARBON_CYCLE, N, b) as e:
        e.set_mode(ra.MODE_EXACT)
        e.set_params(P3)
        e.set_step_size(1, h)
        e.set_forcing(np.stack([np.stack([E[s], Temp[s]]) for s in range(S)]), scen)
        for key in ("conc", "cum_uptake", "cum_emis"):
            e.set_initial(NAMES[key], init[key])
        e.run(7)
        e.run()
        got = dict(conc=e.get_series(1), cum_uptake=e.get_series(2), cum_emis=e.get_series(3))
        st = e.status()
    for key in got:
        assert_bit_equal(got[key], want[key], key)
    finite = np.all([np.isfinite(want[k][-1]) for k in want], axis=0)
    assert np.array_equal(st == 0, finite)
    assert 16 <= finite.sum() <= N - 16      # both kinds of member in numbers


def test_co2_erf_kind_with_a_table_input(ra, device_math):
    """Concentrations C_pi, its two neighbours, 0, -1, the smallest denormal, 1e308, inf and NaN (and a tame one), every member with its
    own C_pi and erf_2xco2 (two members with erf_2xco2 = +-0): exactly +0 at C_pi, the library's log outside log_f64's fast range."""
    n = 65
    rng = np.random.default_rng(65)
    P2 = np.stack([rng.uniform(3.0, 4.5, n), rng.uniform(260.0, 300.0, n)])
    P2[0, 3], P2[0, 4] = 0.0, -0.0
    pi = P2[1]
    cols = [pi, np.nextafter(pi, 0.0), np.nextafter(pi, 1e3), np.zeros(n), -np.ones(n), np.full(n, 5e-324), np.full(n, 1e308),
            np.full(n, np.inf), np.full(n, np.nan), np.full(n, 400.0)]
    conc = np.stack(cols, axis=1)                                             # [n][T - 1]
    T = conc.shape[1] + 1
    table = np.concatenate([conc, conc[:, -1:]], axis=1)                      # (the last index is never read)
    want = hc.co2_erf(P2, conc.T, log=device_math["log"])                     # [T - 1][n]
    with ra.Ensemble(ra.KIND_CO2_ERF, n, np.arange(T + 1, dtype=float) + 1750.0) as e:
        e.set_mode(ra.MODE_EXACT)
        e.set_params(P2)
        e.set_forcing(table[:, None, :], np.arange(n, dtype=np.int32))
        e.run()
        got = e.get_series(1)                                                 # row k + 1 from concentration k
    assert np.isnan(got[0]).all()
    assert_bit_equal(got[1:], want, "CO2ERF")
    ordinary = np.arange(n) > 4
    assert (got[1, ordinary] == 0.0).all() and not np.signbit(got[1, ordinary]).any()
