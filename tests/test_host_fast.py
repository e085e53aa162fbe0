"""CPU tier: tests/host_fast.py -- the numpy restatement of the FAST year of the two-layer kind, the CarbonCycle kind and the
coupled chain -- rests on an exact fused multiply-add, is within FAST's stated 1e-11 of the oracle on bounded members, flags the
members the oracle's final states flag (but for one listed class), and its ensembles tell five subtly wrong years from the right
one.  tests/test_gpu_fast_bits.py then holds the FAST kernels to the same restatement bit for bit, with the device's exp / log."""
from fractions import Fraction
import math

import numpy as np
import pytest

from tests import host_coupled as hc
from tests import host_fast as hf
from tests.helpers import axis_values, bits, coupled_params, emissions_syn, f_syn, two_layer_params
from tests.test_gpu_parity import FAST_RTOL, _bounded, _close     # the project's own bar and mask, as they stand there


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


@pytest.fixture(scope="module")
def edge():
    return hf.edge_ensemble_fast()


# ------------------------------------------------------------------------------------------------ the fma helper
def _fma_exact(a: float, b: float, c: float) -> float:
    """a*b + c rounded once to nearest-even, from rational arithmetic; IEEE 754's rules where an operand is not finite or the exact
    result is a zero.  NaN stands for every NaN."""
    if math.isnan(a) or math.isnan(b) or math.isnan(c):
        return math.nan
    if math.isinf(a) or math.isinf(b):
        if a == 0.0 or b == 0.0:
            return math.nan                                              # inf * 0
        p = math.copysign(math.inf, math.copysign(1.0, a) * math.copysign(1.0, b))
        return math.nan if math.isinf(c) and c != p else p               # inf - inf
    if math.isinf(c):
        return c
    p, s = Fraction(a) * Fraction(b), Fraction(c)
    if p + s == 0:
        if p != 0:
            return 0.0                                                   # exact cancellation of non-zeros: +0 in round-to-nearest
        p_negative = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -0.0 if p_negative and math.copysign(1.0, c) < 0 else 0.0  # (+-0) + (+-0)
    try:
        return float(p + s)                                              # int / int: correctly rounded, sign kept on underflow
    except OverflowError:
        return math.inf if p + s > 0 else -math.inf


def _fma_triples():
    big, tiny, eps = 1.7976931348623157e308, 5e-324, 2.0 ** -52
    special = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, tiny, -tiny, big, -big, 2.0 ** -1022, 1.0 + eps, 3.0, 2.0 ** -537]
    out = [(a, b, c) for a in special for b in special for c in special]
    rng = np.random.default_rng(20261021)
    for _ in range(1500):                                                # wide exponents, random signs
        out.append(tuple(float(np.ldexp(rng.uniform(1.0, 2.0), int(rng.integers(-600, 600))) * rng.choice([-1.0, 1.0])) for _ in range(3)))
    for _ in range(300):                                                 # c cancels the rounded product: the residual is the product's
        a, b = rng.uniform(1.0, 2.0, 2)                                  # rounding error, a few units of the smallest subnormal
        a, b = float(np.ldexp(a, -510)), float(np.ldexp(b, -510))
        out.append((a, b, -(a * b)))
        out.append((a, -b, a * b))
    for _ in range(300):                                                 # c cancels most of the product at ordinary magnitudes
        a, b = (float(x) for x in rng.uniform(1.0, 2.0, 2))
        out.append((a, b, -(a * b) * float(rng.choice([1.0, 1.0 + eps, 1.0 - eps / 2]))))
    half_ulp = 2.0 ** 970                                                # of the largest finite number
    out += [(big, 1.0, half_ulp), (big, 1.0, float(np.nextafter(half_ulp, 0.0))), (-big, 1.0, -half_ulp),
            (-big, 1.0, -float(np.nextafter(half_ulp, 0.0))), (2.0 ** 512, 2.0 ** 512, -2.0 ** 971), (2.0 ** 512, 2.0 ** 512, -2.0 ** 970),
            (2.0 ** 512, -2.0 ** 512, 2.0 ** 971), (big, 2.0, -big), (big, 2.0, -float(np.nextafter(big, 0.0))), (big, 1.0 + eps, -big * eps)]
    return out


def test_fma_helper_is_exact(orc):
    """orc_fma against a*b + c in rational arithmetic, rounded once: bit for bit where the result is finite (signed zeros, subnormals
    from cancellation, both sides of the overflow threshold), by class and sign where it is not (inf * 0, inf - inf, NaN operands)."""
    triples = _fma_triples()
    a, b, c = (np.array(x) for x in zip(*triples))
    with np.errstate(all="ignore"):
        got = orc.fma(a, b, c)
    want = np.array([_fma_exact(*t) for t in triples])
    assert len(triples) > 5000
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got[ok]), bits(want[ok]))
    # the cases the list is there for are in it: subnormal results, both zeros, both infinities from finite operands, the largest
    # finite number, NaN from inf * 0
    finite_in = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    sub = ok & (want != 0.0) & (np.abs(want) < 2.0 ** -1022)
    assert sub.sum() >= 100 and (finite_in & np.isposinf(want)).any() and (finite_in & np.isneginf(want)).any()
    assert (np.abs(want[ok]) == 1.7976931348623157e308).sum() >= 4
    assert ((want == 0.0) & np.signbit(want)).any() and ((want == 0.0) & ~np.signbit(want)).any()
    assert np.isnan(orc.fma(np.inf, 0.0, 1.0)).all() and orc.fma(2.0, [3.0, 4.0], 1.0).tolist() == [7.0, 9.0]    # broadcasting
    # one rounding, not two: the product's low bits survive
    x = 1.0 + 2.0 ** -30
    assert orc.fma(x, x, -1.0).item() == 2.0 ** -29 + 2.0 ** -60 != x * x - 1.0


# ------------------------------------------------------------------------------------------------ restatement vs oracle
def _rel(a, b):
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def test_two_layer_restatement_is_within_the_fast_bar_of_the_oracle(orc):
    """two_layer_params(2000) over axis_values(), 750 years: the test_two_layer_fast_mode_tolerance inputs.  Bounded share 0.9605;
    maximum deviation relative to max(1, |oracle|) on the bounded members 5.7e-14 (Ts) and 2.3e-14 (Td) against the bar of 1e-11;
    no status byte differs from the oracle's final states, bounded or not."""
    t = axis_values()
    P, F = two_layer_params(2000), f_syn(t)
    b = orc.bounds_from_values(t)
    want_ts, want_td = orc.two_layer_run(b, P, F, 0.0, 0.0, threads=8)
    ts, td, st = hf.two_layer_fast(b, P, F, 0.0, 0.0)
    bounded = _bounded(want_ts)
    worst = _rel(ts[:, bounded], want_ts[:, bounded]), _rel(td[:, bounded], want_td[:, bounded])
    failed = ~(np.isfinite(want_ts[-1]) & np.isfinite(want_td[-1]))
    print(f"two-layer: bounded share {bounded.mean():.4f}, max deviation Ts {worst[0]:.2e} Td {worst[1]:.2e}, "
          f"status disagreements {int((st.astype(bool) != failed).sum())}")
    assert bounded.mean() >= 0.95
    assert _close(ts[:, bounded], want_ts[:, bounded], FAST_RTOL).all() and _close(td[:, bounded], want_td[:, bounded], FAST_RTOL).all()
    assert not st[bounded].any() and np.array_equal(st.astype(bool), failed)


COUPLED_BOUNDED_SHARE = 1.0     # of coupled_params(777) over 750 years, read off the oracle: every member of this draw is bounded


def test_coupled_restatement_is_within_the_fast_bar_of_the_oracle(orc):
    """coupled_params(777) over axis_values(): the test_coupled_vs_oracle inputs, glibc's exp / log on both sides.  Bounded share of
    the oracle's draw 1.0000 (asserted with a margin of 0.01); maximum deviation relative to max(1, |oracle|) on bounded members:
    cumulative uptake 2.1e-13, Td 1.0e-14, Ts 5.6e-15, the two forcings 2.2e-15, concentration 3.3e-16, against the bar of 1e-11;
    cumulative emissions carry the oracle's bits."""
    t = axis_values()
    P, E = coupled_params(777), emissions_syn(t)
    b = orc.bounds_from_values(t)
    init = dict(ts=0.0, td=0.0, conc=278.0, cum_uptake=0.0, cum_emis=0.0)
    want = orc.coupled_run(b, P, E, init, threads=8)
    got = hf.coupled_fast(b, P, E, init)
    bounded = _bounded(want["ts"])
    worst = {k: _rel(got[k][1:, bounded], want[k][1:, bounded]) for k in hf.SERIES}
    print(f"coupled: bounded share {bounded.mean():.4f}, max deviation " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert bounded.mean() >= COUPLED_BOUNDED_SHARE - 0.01
    for k in hf.SERIES:
        assert (np.isnan(got[k][0]) == np.isnan(want[k][0])).all(), k
        assert _close(got[k][1:, bounded], want[k][1:, bounded], FAST_RTOL).all(), k
    assert np.array_equal(bits(got["cum_emis"]), bits(want["cum_emis"]))
    assert not hf.status(got)[bounded].any()


def test_carbon_cycle_restatement_is_the_coupled_chains_carbon_box():
    """The stand-alone kind fed the chain's own Ts rows gives the chain's three carbon series, bit for bit (one year function)."""
    c = hc.fuzz_config(6)
    chain = hf.coupled_fast(c["bounds"], c["P"], c["E"], c["init"], scen=c["scen"], h_tl=c["h_tl"], h_cc=c["h_cc"])
    E = hf._member_rows(c["E"], c["scen"], c["N"])
    alone = hf.carbon_cycle_fast(c["bounds"], c["P"][[6, 7, 8]], E, chain["ts"], {k: c["init"][k] for k in ("conc", "cum_uptake", "cum_emis")},
                                 h=c["h_cc"])
    for k in alone:
        assert np.array_equal(bits(alone[k][1:]), bits(chain[k][1:])), k


# ------------------------------------------------------------------------------------------------ the status contract
# FAST's domain (include/rscm_gpu.h, RSCM_MODE_FAST): finite 1/Cs and eta/Cd.  A subnormal heat capacity is outside it: the
# reference divides 0 by it and keeps a member at rest at exact zeros (or, dividing by Cd alone, finite), while the folded
# coefficients 1/Cs = inf or eta/Cd = inf meet a zero state, inf * 0 = NaN, from the first row on.  The member is flagged; these
# (forcing, member) pairs are the only ones where the restatement's status byte and the oracle's final states part.
OUTSIDE_FASTS_DOMAIN = {
    "all zero": ("cs 5e-324", "cs -5e-324", "cd 5e-324", "cd -5e-324"),
    "* 5e-324": ("cd 5e-324", "cd -5e-324"),     # (with Cs subnormal the reference overflows as well: subnormal / subnormal is no zero)
}


def test_status_contract_on_the_edge_ensemble(orc, edge):
    """Every member under every forcing: the restatement's status byte is `the oracle's final Ts or Td is not finite`, except exactly
    the pairs of OUTSIDE_FASTS_DOMAIN, where the oracle stays finite and FAST flags the member.  Then the coupled chain, where no
    member is excepted (its CO2 forcing is never zero)."""
    c = edge
    where = {label: i for i, label in c["labels"].items()}
    P6 = c["P"][:6]
    with np.errstate(all="ignore"):
        for s, name in enumerate(hf.FORCINGS):
            scen = np.full(c["N"], s, np.int32)
            _, _, st = hf.two_layer_fast(c["bounds"], P6, c["F"], c["ts0"], c["td0"], scen=scen)
            want = orc.two_layer_run(c["bounds"], P6, c["F"], c["ts0"], c["td0"], scen=scen)
            failed = ~(np.isfinite(want[0][-1]) & np.isfinite(want[1][-1]))
            listed = np.zeros(c["N"], dtype=bool)
            listed[[where[label] for label in OUTSIDE_FASTS_DOMAIN.get(name, ())]] = True
            assert np.array_equal(st.astype(bool) != failed, listed), (name, np.flatnonzero((st.astype(bool) != failed) != listed))
            assert st[listed].all() and not failed[listed].any()
            assert name in ("* 1e250", "one NaN year") or 10 <= failed.sum() <= 30       # both kinds of member in numbers
        for scen in (c["scen_e"], None):
            got = hf.coupled_fast(c["bounds"], c["P"], c["E"], c["init"], scen=scen, h_tl=c["h_tl"], h_cc=c["h_cc"])
            want = orc.coupled_run(c["bounds"], c["P"], c["E"], c["init"], scen=scen, h_tl=c["h_tl"], h_cc=c["h_cc"])
            assert np.array_equal(hf.status(got), hc.status(want))
            assert 20 <= hf.status(got).sum() <= 40


def test_edge_ensemble_is_what_it_says(edge):
    c = edge
    assert c["N"] == 257 and c["T"] == 41 and sorted(set(np.diff(c["bounds"]))) == [0.5, 1.0, 5.0]
    assert all(i % 5 == 3 and i < 256 for i in c["labels"]) and len(c["labels"]) == 43
    assert {i // 64 for i in c["labels"]} == {0, 1, 2, 3}                      # in every full wavefront, beside ordinary members
    assert c["F"].shape == (len(hf.FORCINGS), c["T"]) and set(c["scen_f"]) == set(range(len(hf.FORCINGS)))
    assert c["E"].shape == (len(hf.EMISSIONS), c["T"]) and set(c["scen_e"]) == set(range(len(hf.EMISSIONS)))


# ------------------------------------------------------------------------------------------------ discrimination
def _unfused(a, b, c):
    return a * b + c


class _StageUnfused(hf.Arith):
    stage = staticmethod(_unfused)


class _ExactsAssociation(hf.Arith):
    combine = staticmethod(hf.combine_exact)


class _DeepTemperatureCarried(hf.Arith):
    carry_difference = False


class _ForcingDivided(hf.Arith):
    scale_forcing = staticmethod(lambda erf, cs, inv_cs: erf / cs)


class _PhiUnfused(hf.Arith):
    phi = staticmethod(lambda z: _unfused(z, _unfused(z, _unfused(z, -1.0 / 24.0, 1.0 / 6.0), -0.5), 1.0))


def _differs(got, want):
    """Some bit of some series differs (any NaN equals any NaN, as in assert_bit_equal)."""
    return any(((bits(got[k]) != bits(want[k])) & ~(np.isnan(got[k]) & np.isnan(want[k]))).any() for k in want)


def _coupled(c, scen, arith):
    return hf.coupled_fast(c["bounds"], c["P"], c["E"], c["init"], scen=scen, h_tl=c["h_tl"], h_cc=c["h_cc"], arith=arith)


def _two_layer(c, arith):
    ts, td, _ = hf.two_layer_fast(c["bounds"], c["P"][:6], c["F"], c["ts0"], c["td0"], scen=c["scen_f"], arith=arith)
    return dict(ts=ts, td=td)


FUZZ_SEED = 9      # 63 members, 81 steps: the cheapest of the ten on which all five swaps show


@pytest.fixture(scope="module")
def right(edge):
    f = hc.fuzz_config(FUZZ_SEED)
    return dict(edge_coupled=_coupled(edge, edge["scen_e"], hf.Arith), edge_two_layer=_two_layer(edge, hf.Arith), fuzz=_coupled(f, f["scen"], hf.Arith))


@pytest.mark.parametrize("wrong", [_StageUnfused, _ExactsAssociation, _DeepTemperatureCarried, _ForcingDivided, _PhiUnfused],
                         ids=lambda w: w.__name__)
def test_a_subtly_wrong_fast_year_is_told_from_the_right_one(edge, right, wrong):
    """One stage FMA as a product and a sum; the combination in EXACT's association; Td integrated instead of w = Ts - Td; the forcing
    divided by Cs instead of multiplied by 1/Cs; the carbon box's phi(z) as an unfused Horner chain.  Each changes a bit of a series
    on the edge ensemble (the coupled run; for the four two-layer swaps the two-layer run as well) and on a fuzz configuration."""
    f = hc.fuzz_config(FUZZ_SEED)
    assert _differs(_coupled(edge, edge["scen_e"], wrong), right["edge_coupled"])
    assert _differs(_coupled(f, f["scen"], wrong), right["fuzz"])
    if wrong is not _PhiUnfused:
        assert _differs(_two_layer(edge, wrong), right["edge_two_layer"])
    else:       # ... and it changes the carbon series alone of a year (the two-layer half follows through the forcing)
        got = _coupled(f, f["scen"], wrong)
        assert not _differs(dict(cum_emis=got["cum_emis"]), dict(cum_emis=right["fuzz"]["cum_emis"]))
