"""CPU tier: tests/host_coupled.py -- the numpy restatement of the coupled chain's EXACT year -- is the oracle's arithmetic
bit for bit (glibc exp / log on both sides), its exponent windows are the ones csrc/rk4_device.hpp states, its edge
ensemble reaches every replay path of the kernels, and that ensemble tells three subtly wrong years from the right one.
tests/test_gpu_coupled_bits.py then holds the EXACT kernels to the same restatement with the device's exp / log."""
import numpy as np
import pytest

from tests import host_coupled as hc
from tests.helpers import assert_bit_equal, bits


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


@pytest.fixture(scope="module")
def edge():
    return hc.edge_ensemble()


def _args(c):
    return (c["bounds"], c["P"], c["E"], c["init"]), dict(scen=c["scen"], h_tl=c["h_tl"], h_cc=c["h_cc"])


@pytest.fixture(scope="module")
def edge_series(edge):
    a, kw = _args(edge)
    return hc.coupled(*a, **kw)


@pytest.fixture(scope="module")
def edge_causes(edge):
    a, kw = _args(edge)
    return hc.replay_causes(*a, **kw)


@pytest.fixture(scope="module")
def edge_oracle(orc, edge):
    a, kw = _args(edge)
    return orc.coupled_run(*a, **kw, threads=4)


def _differs(got, want):
    """Some bit of some series differs (any NaN equals any NaN, as in assert_bit_equal)."""
    for k in hc.SERIES:
        bad = (bits(got[k]) != bits(want[k])) & ~(np.isnan(got[k]) & np.isnan(want[k]))
        if bad.any():
            return True
    return False


# ------------------------------------------------------------------------------------------------ restatement == oracle
@pytest.mark.parametrize("seed", range(10))
def test_restatement_is_the_oracle_on_the_fuzz_configurations(orc, seed):
    c = hc.fuzz_config(seed)
    a, kw = _args(c)
    want = orc.coupled_run(*a, **kw, threads=4)
    got = hc.coupled(*a, **kw)
    for k in hc.SERIES:
        assert_bit_equal(got[k], want[k], f"seed {seed} {k}")


def test_restatement_is_the_oracle_on_the_edge_ensemble(edge_series, edge_oracle):
    for k in hc.SERIES:
        assert_bit_equal(edge_series[k], edge_oracle[k], k)
    # zeros and infinities keep their signs (assert_bit_equal compares them as bits; only NaNs are pooled)
    assert np.isinf(edge_oracle["erf_total"]).any() and (edge_oracle["erf_total"] == 0.0).any()


def test_edge_ensemble_without_its_scenario_map(orc, edge):
    a, kw = _args(edge)
    kw["scen"] = None
    want = orc.coupled_run(*a, **kw, threads=4)
    got = hc.coupled(*a, **kw)
    for k in hc.SERIES:
        assert_bit_equal(got[k], want[k], k)


def test_carbon_cycle_is_the_oracle_chained_over_the_axis(orc):
    rng = np.random.default_rng(7)
    t = 1750.0 + np.concatenate([[0.0], np.cumsum(np.tile([1.0, 0.5, 1.5], 3))])
    b = np.append(t, t[-1] + (t[-1] - t[-2]))
    T, N, h = len(t), 24, 0.125
    tau_edges = (2.0 ** -128, np.nextafter(2.0 ** -128, 0.0), 2.0 ** 129, np.nextafter(2.0 ** 129, 0.0))
    P3 = np.stack([rng.uniform(15.0, 40.0, N), rng.uniform(260.0, 300.0, N), rng.uniform(0.0, 0.1, N)])
    P3[0, :4] = tau_edges
    P3[2, 4:8] = (0.0, 400.0, -400.0, np.inf)
    E = np.abs(rng.normal(3.0, 3.0, (T, 1)))
    temperature = rng.normal(0.5, 1.0, (T, N))
    temperature[2, 8:14] = (0.0, np.inf, -np.inf, np.nan, 1e5, -1e5)
    init = dict(conc=P3[1] + rng.uniform(-5.0, 30.0, N), cum_uptake=0.0, cum_emis=1.5)
    got = hc.carbon_cycle(b, P3, E, temperature, init, h=h)
    for i in range(N):
        y = np.array([init["conc"][i], 0.0, 1.5])
        for n in range(T - 1):
            y = orc.carbon_cycle_solve(P3[:, i], float(E[n, 0]), float(temperature[n, i]), b[n], b[n + 1], h, y)
            assert_bit_equal(np.array([got[k][n + 1, i] for k in ("conc", "cum_uptake", "cum_emis")]), y, f"member {i} step {n}")
    assert np.isnan(got["conc"][-1]).any() and np.isfinite(got["conc"][-1]).sum() > N // 2


def test_co2_erf_is_the_oracle(orc):
    cpi = 278.0
    conc = np.array([cpi, np.nextafter(cpi, 0.0), np.nextafter(cpi, 1e3), 0.0, -1.0, 5e-324, 1e308, np.inf, np.nan, 400.0, 150.0])
    for e2x in (3.7, 0.0, -0.0, np.inf):
        P2 = np.stack([np.full(conc.size, e2x), np.full(conc.size, cpi)])
        want = np.array([orc.co2_erf(e2x, cpi, float(c)) for c in conc])
        assert_bit_equal(hc.co2_erf(P2, conc), want, f"erf_2xco2 {e2x}")
    assert hc.co2_erf(np.array([[3.7], [cpi]]), np.array([cpi]))[0] == 0.0


# ------------------------------------------------------------------------------------------------ windows
def test_window_predicates_on_both_sides_of_every_edge():
    """csrc/rk4_device.hpp: numerator window |n| in [2^-511, 2^513), divisor window |d| in [2^-128, 2^129)."""
    def below(x):
        return np.nextafter(x, 0.0)
    for s in (1.0, -1.0):
        inside = s * np.array([2.0 ** -511, below(2.0 ** 513), 1.0, 278.0])
        outside = s * np.array([below(2.0 ** -511), 2.0 ** 513, 0.0, 5e-324, 2.2250738585072014e-308, np.inf, np.nan, 1.7976931348623157e308])
        assert not hc.numerator_outside(inside).any() and hc.numerator_outside(outside).all()
        inside = s * np.array([2.0 ** -128, below(2.0 ** 129), 1.0, 8.0])
        outside = s * np.array([below(2.0 ** -128), 2.0 ** 129, 0.0, 5e-324, np.inf, np.nan, 1e45, 1e-45])
        assert not hc.divisor_outside(inside).any() and hc.divisor_outside(outside).all()
    assert list(hc.biased_exponent([2.0 ** -511, 2.0 ** 513, 2.0 ** -128, 2.0 ** 129])) == [512, 1536, 895, 1152]


def test_replay_causes_name_the_year_and_the_cause(edge, edge_causes):
    where = {label: i for i, label in edge["labels"].items()}
    c = edge_causes
    assert c[0, where["equilibrium"]] == hc.CAUSE_NUMERATOR and not c[1:, where["equilibrium"]].any()
    # Ts0 = 2^-510 with eta = 0.5: the deep equation's first numerator is 2^-511, the window's lower edge
    assert not c[:, where[f"eta 0.5, Td0 0, Ts0 {2.0 ** -510!r}"]].any()
    i = where[f"eta 0.5, Td0 0, Ts0 {hc.below(2.0 ** -510)!r}"]
    assert c[0, i] == hc.CAUSE_NUMERATOR and not c[1:, i].any()
    for v, inside in ((2.0 ** -128, True), (hc.below(2.0 ** -128), False), (2.0 ** 129, False), (hc.below(2.0 ** 129), True)):
        assert bool(c[0, where[f"alpha 0, tau {v!r}"]] & hc.CAUSE_LIFETIME) == (not inside), v
        for name in ("cs", "cd"):
            assert bool((c[:, where[f"{name} {v!r}"]] & hc.CAUSE_CAPACITY).all()) == (not inside), (name, v)
            assert bool((c[:, where[f"{name} {v!r}"]] & hc.CAUSE_CAPACITY).any()) == (not inside), (name, v)
    assert (c[:, where["Ts0 NaN"]] & hc.CAUSE_TS_NAN).all()
    i = where["emissions NaN at step 4"]
    assert not c[:4, i].any() and c[4, i] == hc.CAUSE_NUMERATOR and (c[6:, i] & hc.CAUSE_TS_NAN).all()
    i = where["a -5, Ts0 -1.0"]      # runs away through the numerator window to overflow
    assert not c[0, i] and (c[-1, i] & hc.CAUSE_TS_NAN)


def test_edge_ensemble_reaches_every_path(edge, edge_series, edge_causes):
    c, N = edge_causes, edge["N"]
    flagged = c != 0
    per_cause = {bit: int(((c & bit) != 0).any(axis=0).sum()) for bit in (1, 2, 4, 8)}
    years = {bit: int(((c & bit) != 0).sum()) for bit in (1, 2, 4, 8)}
    after_year0 = int(flagged[1:].any(axis=0).sum())
    both = int((flagged.any(axis=0) & ~flagged.all(axis=0)).sum())
    finite = int((np.isfinite(edge_series["ts"][-1]) & np.isfinite(edge_series["conc"][-1])).sum())
    print(f"members per cause {per_cause}; member-years per cause {years}; flagged after year 0: {after_year0} members; both kinds of "
          f"year: {both} members; unflagged member-years {int((~flagged).sum())} of {flagged.size}; finite at the end {finite} of {N}")
    assert all(v >= 4 for v in per_cause.values()), per_cause
    assert after_year0 >= 20
    assert both >= 5
    assert (~flagged).sum() >= 0.8 * flagged.size
    assert not flagged[:, :64].any() and not flagged[:, 256:].any()
    assert finite >= 0.75 * N
    # engineered members sit on every third lane of waves 1-3; the run has all three step lengths
    assert all(64 <= i < 256 and (i - 64) % 3 == 0 for i in edge["labels"])
    assert sorted(set(np.diff(edge["bounds"]))) == [0.5, 1.0, 1.5] and len(edge["bounds"]) == edge["T"] + 1 == 14
    assert hc.status(edge_series).sum() == N - int(np.all([np.isfinite(edge_series[k][-1]) for k in ("ts", "td", "conc", "cum_uptake", "cum_emis")], axis=0).sum())


# ------------------------------------------------------------------------------------------------ discrimination
class _ReciprocalQuotient(hc.Arith):
    div = staticmethod(lambda n, d: n * (1.0 / d))


class _PooledDoubling(hc.Arith):
    combine = staticmethod(lambda y, k1, k2, k3, k4, sixth: y + ((k1 + (k2 + k3) * 2.0) + k4) * sixth)


class _BareAggregate(hc.Arith):
    aggregate = staticmethod(lambda x: np.where(np.isnan(x), np.nan, x))


@pytest.mark.parametrize("wrong", [_ReciprocalQuotient, _PooledDoubling, _BareAggregate], ids=lambda w: w.__name__)
def test_a_subtly_wrong_year_is_told_from_the_oracle(edge, edge_oracle, wrong):
    """Quotients as n * (1/d); the two doublings pooled into (k2 + k3) * 2, one rounding fewer; the Sum without its 0.0 +
    (only the -0.0 forcing of the member with erf_2xco2 = -0.0 shows it)."""
    a, kw = _args(edge)
    assert _differs(hc.coupled(*a, **kw, arith=wrong), edge_oracle)
