"""GPU tier (-m gpu): the FAST year (RSCM_MODE_FAST) of the two-layer kind, the coupled chain and the CarbonCycle kind, bit for bit,
for every member.

The FAST arithmetic is IEEE + - * / rounded one by one and explicit fused multiply-adds (csrc/two_layer_body.hpp: make_fast, rhs_fast,
rk4_year_fast; csrc/carbon_body.hpp: carbon_cycle_year_fast; csrc/coupled.hip: coupled_fast_kernel; the library is built without
contraction), plus one exp and one log_f64 per member-year in the carbon box and CO2ERF.  tests/host_fast.py restates it in numpy with
an exact fma (tests/test_host_fast.py: the fma against rational arithmetic, the restatement within FAST's 1e-11 of the oracle on
bounded members, its status bytes against the oracle's final states, five subtly wrong years told apart).  Here the two
transcendental values are taken from the device (rscm_amd.ensemble.selftest_math: op 2, the library's exp; op 0, log_f64), and every
output row of every member must carry the restatement's bits (any NaN equals any NaN; zeros and infinities keep their signs), the
status bytes its flags: no tolerance, no mask.  What tests/test_gpu_parity.py cannot see -- a stage that is not fused, EXACT's
association in the combination, Td carried instead of w = Ts - Td, a misplaced NaN or inf, a wrong status byte on a member outside
its mask -- fails here.

The edge ensemble (host_fast.edge_ensemble_fast) has 257 members -- a ragged last wave and block -- with heat capacities 0,
+-subnormal, 2^+-130, negative, inf and NaN, runaway feedback up to overflow, inf / NaN / 1e308 parameters, lifetimes 0, inf and
subnormal, an exp that overflows and one that underflows, a zero pre-industrial concentration and inf / NaN emissions, in lanes that
share wavefronts with ordinary members, under forcings scaled from 5e-324 to 1e250."""
import numpy as np
import pytest

from tests import host_coupled as hc
from tests import host_fast as hf
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

NAMES = {"ts": "Surface Temperature", "td": "Deep Ocean Temperature", "conc": "Atmospheric Concentration|CO2",
         "cum_uptake": "Cumulative Land Uptake", "cum_emis": "Cumulative Emissions|CO2", "erf_co2": "Effective Radiative Forcing|CO2",
         "erf_total": "Effective Radiative Forcing"}
STATES = ("ts", "td", "conc", "cum_uptake", "cum_emis")
CARBON = ("conc", "cum_uptake", "cum_emis")


@pytest.fixture(scope="module")
def device_math(ra):
    """exp and log as the kernels evaluate them: the device library's exp and log_f64 through the self-test hook."""
    from rscm_amd.ensemble import selftest_math

    def on_device(op):
        return lambda x: selftest_math(op, np.ascontiguousarray(x, dtype=np.float64)).reshape(np.shape(x))
    return dict(exp=on_device(2), log=on_device(0))


@pytest.fixture(scope="module")
def edge():
    return hf.edge_ensemble_fast()


# ------------------------------------------------------------------------------------------------ the two-layer kind
def _two_layer(ra, bounds, P, F, scen, source, h, ts0, td0, cuts=()):
    with ra.Ensemble(ra.KIND_TWO_LAYER, P.shape[1], bounds) as e:
        e.set_mode(ra.MODE_FAST)
        e.set_step_size(0, h)
        e.set_params(P)
        e.set_forcing(F, scen, source)
        e.set_initial(NAMES["ts"], ts0)
        e.set_initial(NAMES["td"], td0)
        for cut in cuts:
            e.run(cut)
        e.run()
        assert e.finished()
        return e.get_series(NAMES["ts"]), e.get_series(NAMES["td"]), e.status()


def _assert_two_layer(got, want, what):
    assert_bit_equal(got[0], want[0], f"{what}: Ts")
    assert_bit_equal(got[1], want[1], f"{what}: Td")
    assert np.array_equal(got[2] != 0, want[2] != 0), what


@pytest.mark.parametrize("mapped", [True, False], ids=["scenario map", "no map"])
@pytest.mark.parametrize("source", [0, 1])
@pytest.mark.parametrize("h", [0.1, 0.25])
def test_two_layer_on_the_edge_ensemble(ra, edge, h, source, mapped):
    """257 members x 40 steps of 0.5, 1 and 5 years (5 to 50 sub-steps at h = 0.1), the six forcings through the scenario map or the
    ordinary one for everybody, read at index n or n + 1; in one launch, and cut at steps 1 and 6, where the resumed launches read
    stored rows that hold inf and NaN and form w = Ts - Td from them anew (as every model step does)."""
    c = edge
    P, scen = np.ascontiguousarray(c["P"][:6]), c["scen_f"] if mapped else None
    want = hf.two_layer_fast(c["bounds"], P, c["F"], c["ts0"], c["td0"], scen=scen, source=source, h=h)
    assert 0 < want[2].sum() < c["N"]
    for cuts in ((), (1, 6)):
        got = _two_layer(ra, c["bounds"], P, c["F"], scen, source, h, c["ts0"], c["td0"], cuts)
        _assert_two_layer(got, want, f"h {h}, source {source}, cuts {cuts}")


def test_two_layer_with_the_reference_models_finest_step(ra, edge):
    """h = 1/120 over the first six steps of the axis (60 sub-steps each)."""
    c = edge
    bounds, F, P, h = c["bounds"][:8], np.ascontiguousarray(c["F"][:, :7]), np.ascontiguousarray(c["P"][:6]), 1.0 / 120.0
    assert [hf.nsub(bounds[n], bounds[n + 1], h) for n in range(6)] == [60] * 6
    want = hf.two_layer_fast(bounds, P, F, c["ts0"], c["td0"], scen=c["scen_f"], h=h)
    got = _two_layer(ra, bounds, P, F, c["scen_f"], 0, h, c["ts0"], c["td0"])
    _assert_two_layer(got, want, "h 1/120")


@pytest.mark.parametrize("n", [1, 65])
def test_two_layer_smallest_ensembles(ra, edge, n):
    """One member, and a full wave with one lane of the next, on the first eight steps: the edge ensemble's first members (from lane 3
    on every fifth is engineered) -- and for n = 1 its member 28 (Cs = 0) on its own as well."""
    c = edge
    bounds, F = c["bounds"][:10], np.ascontiguousarray(c["F"][:, :9])
    picks = [np.arange(n)] + ([np.array([28])] if n == 1 else [])
    for members in picks:
        P, scen = np.ascontiguousarray(c["P"][:6, members]), np.ascontiguousarray(c["scen_f"][members])
        ts0, td0 = c["ts0"][members], c["td0"][members]
        for source in (0, 1):
            want = hf.two_layer_fast(bounds, P, F, ts0, td0, scen=scen, source=source, h=0.1)
            got = _two_layer(ra, bounds, P, F, scen, source, 0.1, ts0, td0, cuts=(1,))
            _assert_two_layer(got, want, f"n {n}, members {members[:3]}, source {source}")


# ------------------------------------------------------------------------------------------------ the coupled chain
def _restate(c, device_math, scen):
    return hf.coupled_fast(c["bounds"], c["P"], c["E"], c["init"], scen=scen, h_tl=c["h_tl"], h_cc=c["h_cc"], **device_math)


def _fused(ra, c, scen, cuts=()):
    with ra.Ensemble(ra.KIND_COUPLED, c["N"], c["bounds"]) as e:
        e.set_mode(ra.MODE_FAST)
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
    for key in want:
        assert_bit_equal(got[key], want[key], f"{what}: {key}")
    assert np.array_equal(status != 0, hf.status(want) != 0), what


@pytest.mark.parametrize("mapped", [True, False], ids=["scenario map", "no map"])
def test_coupled_chain_on_the_edge_ensemble(ra, edge, device_math, mapped):
    """All seven series and the status bytes; one launch, and cut at steps 1 and 6."""
    scen = edge["scen_e"] if mapped else None
    want = _restate(edge, device_math, scen)
    assert 0 < hf.status(want).sum() < edge["N"]
    for cuts in ((), (1, 6)):
        got, st = _fused(ra, edge, scen, cuts)
        _assert_is(got, st, want, f"coupled chain, cuts {cuts}")


@pytest.mark.parametrize("seed", range(10))
def test_coupled_chain_on_the_fuzz_configurations(ra, device_math, seed):
    """The ten configurations of test_gpu_parity.py::test_coupled_chain_fuzz with their cuts: all members, all seven series, the status
    bytes (uniform conc_pi and erf_2xco2 rows, 1 to 1025 members, 3 to 200 steps of 0.5 to 2 years)."""
    c = hc.fuzz_config(seed)
    got, st = _fused(ra, c, c["scen"], c["cuts"])
    _assert_is(got, st, _restate(c, device_math, c["scen"]),
               f"seed {seed} (T={c['T']}, n={c['N']}, h_tl={c['h_tl']}, h_cc={c['h_cc']}, cuts={c['cuts']})")


# ------------------------------------------------------------------------------------------------ CarbonCycle on its own
def test_carbon_cycle_kind_with_an_exogenous_temperature(ra, edge, device_math):
    """carbon_cycle_body<MODE != 0>: 97 members, eight scenarios of (emissions, temperature) rows on the edge ensemble's axis, cut at step
    7.  The temperature rows hold 0, tame values, +-inf, NaN and +-1e5 (exp(-(alpha T)) underflows to 0 / overflows); tau is 0, +-subnormal,
    2^+-130, inf, NaN and negative in a quarter of the lanes, alpha 0 in another (r = 1/tau, or NaN against an infinite T); a few
    members start at C == C_pi."""
    b, T, N, S, h = edge["bounds"], edge["T"], 97, 8, edge["h_cc"]
    rng = np.random.default_rng(20261022)
    E = np.abs(rng.normal(3.0, 3.0, (S, T)))
    E[6, 5] = np.inf
    Temp = rng.normal(0.5, 1.0, (S, T))
    Temp[0, 2] = 0.0
    Temp[1, 5], Temp[2, 3], Temp[3, 6], Temp[4, 4], Temp[5, 8] = np.inf, -np.inf, np.nan, 1e5, -1e5
    Temp[7] = 0.0
    scen = (np.arange(N) % S).astype(np.int32)
    P3 = np.stack([rng.uniform(15.0, 40.0, N), rng.uniform(260.0, 300.0, N), rng.uniform(0.0, 0.1, N)])
    taus = (0.0, 5e-324, -5e-324, 2.0 ** -130, 2.0 ** 130, np.inf, np.nan, -20.0, 0.05, 0.5)
    for k, v in enumerate(taus):
        P3[0, 3 + 4 * k] = v                      # lanes 3, 7, ... 39: among ordinary members, every scenario met
    P3[2, 48:72] = 0.0
    P3[0, 48:52] = (0.0, np.inf, 5e-324, 2.0)
    init = dict(conc=P3[1] + rng.uniform(1.0, 30.0, N), cum_uptake=rng.uniform(0.0, 5.0, N), cum_emis=1.5)
    init["conc"][72:80] = P3[1, 72:80]
    want = hf.carbon_cycle_fast(b, P3, E[scen].T, Temp[scen].T, init, h=h, exp=device_math["exp"])
    with ra.Ensemble(ra.KIND_CARBON_CYCLE, N, b) as e:
        e.set_mode(ra.MODE_FAST)
        e.set_params(P3)
        e.set_step_size(1, h)
        e.set_forcing(np.stack([np.stack([E[s], Temp[s]]) for s in range(S)]), scen)
        for key in CARBON:
            e.set_initial(NAMES[key], init[key])
        e.run(7)
        e.run()
        got = {key: e.get_series(k + 1) for k, key in enumerate(CARBON)}
        st = e.status()
    for key in CARBON:
        assert_bit_equal(got[key], want[key], key)
    assert np.array_equal(st != 0, hf.status(want) != 0)
    assert 16 <= hf.status(want).sum() <= N - 16      # both kinds of member in numbers
