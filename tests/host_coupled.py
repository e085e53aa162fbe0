"""Host restatement of the coupled chain's EXACT year (CarbonCycle -> CO2ERF -> Sum -> TwoLayer) in numpy float64,
the edge ensemble that drives every replay path of the kernels, and the fuzz recipe of tests/test_gpu_parity.py.

One numpy ufunc call per IEEE operation (numpy neither fuses nor reassociates separate calls), vectorised over
members, Python loops over model steps and RK4 sub-steps.  The expressions are those of oracle/rscm_oracle.c:169-262,
one for one; the two transcendentals are arguments:
  * the defaults are glibc's exp / log through ctypes, which makes the module equal to the oracle bit for bit
    (tests/test_host_coupled.py, no GPU);
  * the GPU tier passes the device's own exp and log_f64 (rscm_amd.ensemble.selftest_math, ops 2 and 0), and then
    every output of the EXACT kernels has to carry this module's bits for every member, replayed years, window edges,
    inf and NaN included (tests/test_gpu_coupled_bits.py).

The exponent windows of replay_causes are restated from the prose of csrc/rk4_device.hpp ("divisor window",
"numerator window"); nothing here is read from the device, and replay_causes is never compared with it: it tells
which paths of the kernels an input reaches.  Pure numpy + ctypes; no oracle, no product code."""
from __future__ import annotations

import ctypes
import ctypes.util
from typing import Callable, Dict

import numpy as np

from tests.helpers import CC_RANGES, TL_RANGES, coupled_params

GTC_PER_PPM = 2.13                                 # crates/rscm-components/src/constants.rs:37
LN2 = float.fromhex("0x1.62e42fefa39efp-1")        # RN(ln 2): 2.0_f64.ln(), log(2.0) folded by the C compiler
SERIES = ("ts", "td", "conc", "cum_uptake", "cum_emis", "erf_co2", "erf_total")

CAUSE_NUMERATOR, CAUSE_LIFETIME, CAUSE_CAPACITY, CAUSE_TS_NAN = 1, 2, 4, 8

_libm = None


def _glibc(name: str) -> Callable[[np.ndarray], np.ndarray]:
    def call(x):
        global _libm
        if _libm is None:
            _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
            for f in ("exp", "log"):
                getattr(_libm, f).argtypes = [ctypes.c_double]
                getattr(_libm, f).restype = ctypes.c_double
        fn = getattr(_libm, name)
        x = np.asarray(x, dtype=np.float64)
        return np.array([fn(v) for v in x.ravel().tolist()], dtype=np.float64).reshape(x.shape)
    return call


glibc_exp = _glibc("exp")
glibc_log = _glibc("log")


# ------------------------------------------------------------------------------------------------ exponent windows
def biased_exponent(x) -> np.ndarray:
    return ((np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)


def numerator_outside(x) -> np.ndarray:
    """Outside |n| in [2^-511, 2^513): biased exponent outside [512, 1535] (zeros, denormals, inf, NaN are outside)."""
    e = biased_exponent(x)
    return (e < 512) | (e > 1535)


def divisor_outside(x) -> np.ndarray:
    """Outside |d| in [2^-128, 2^129): biased exponent outside [895, 1151]."""
    e = biased_exponent(x)
    return (e < 895) | (e > 1151)


# ------------------------------------------------------------------------------------------------ the arithmetic
def rk4_combine(y, k1, k2, k3, k4, sixth):
    """ode_solvers 0.6.1: y + (((k1 + k2*2) + k3*2) + k4) * (h/6)."""
    return y + (((k1 + k2 * 2.0) + k3 * 2.0) + k4) * sixth


def aggregate_sum(x):
    """schema.rs:760-773 over one contributor: NaN when it is NaN, 0.0 + x otherwise."""
    return np.where(np.isnan(x), np.nan, 0.0 + x)


def nsub(t0: float, t1: float, h: float) -> int:
    return int(np.ceil((np.float64(t1) - np.float64(t0)) / np.float64(h)))


class Arith:
    """The three operations a subtly wrong year gets wrong; tests/test_host_coupled.py swaps them one at a time."""
    div = staticmethod(np.divide)
    combine = staticmethod(rk4_combine)
    aggregate = staticmethod(aggregate_sum)


def _carbon_year(ar, lifetime, conc_pi, emis, m, h, conc, cum_u, cum_e, seen):
    half, sixth = h / 2.0, h / 6.0
    e_ppm = emis / GTC_PER_PPM

    def rhs(c):
        n = c - conc_pi
        seen(n)
        up = ar.div(n, lifetime)
        return e_ppm - up, up * GTC_PER_PPM

    for _ in range(m):
        k1c, k1u = rhs(conc)
        k2c, k2u = rhs(conc + k1c * half)
        k3c, k3u = rhs(conc + k2c * half)
        k4c, k4u = rhs(conc + k3c * h)
        conc = ar.combine(conc, k1c, k2c, k3c, k4c, sixth)
        cum_u = ar.combine(cum_u, k1u, k2u, k3u, k4u, sixth)
        cum_e = ar.combine(cum_e, emis, emis, emis, emis, sixth)
    return conc, cum_u, cum_e


def _two_layer_year(ar, P, erf, m, h, ts, td, seen):
    lambda0, a, efficacy, eta, cs, cd = P
    half, sixth = h / 2.0, h / 6.0
    eff_eta = efficacy * eta

    def rhs(s, d):
        diff = s - d
        lambda_eff = lambda0 - a * s
        hx_s = eff_eta * diff
        n_s = erf - lambda_eff * s - hx_s
        n_d = eta * diff
        seen(n_s)
        seen(n_d)
        return ar.div(n_s, cs), ar.div(n_d, cd)

    for _ in range(m):
        k1s, k1d = rhs(ts, td)
        k2s, k2d = rhs(ts + k1s * half, td + k1d * half)
        k3s, k3d = rhs(ts + k2s * half, td + k2d * half)
        k4s, k4d = rhs(ts + k3s * h, td + k3d * h)
        ts = ar.combine(ts, k1s, k2s, k3s, k4s, sixth)
        td = ar.combine(td, k1d, k2d, k3d, k4d, sixth)
    return ts, td


def _co2_erf(ar, erf_2xco2, conc_pi, conc, log):
    return erf_2xco2 / LN2 * log(1.0 + ar.div(conc - conc_pi, conc_pi))


def _member_rows(rows, scen, N):
    """[S][T] with a member -> scenario map (None: scenario 0)  ->  [T][N]."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    s = np.zeros(N, dtype=np.int64) if scen is None else np.asarray(scen, dtype=np.int64)
    return np.ascontiguousarray(rows[s].T)


def _run(bounds, P, E, init, scen, h_tl, h_cc, exp, log, ar):
    bounds = np.asarray(bounds, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    T, N = len(bounds) - 1, P.shape[1]
    emis = _member_rows(E, scen, N)
    assert emis.shape == (T, N) and P.shape[0] == 10
    out = {k: np.full((T, N), np.nan) for k in SERIES}
    for k, v in init.items():
        out[k][0, :] = v
    causes = np.zeros((T - 1, N), dtype=np.int64)
    tau, conc_pi, alpha, erf_2x = P[6], P[7], P[8], P[9]
    capacity = divisor_outside(P[4]) | divisor_outside(P[5])
    with np.errstate(all="ignore"):
        for n in range(T - 1):
            outside = np.zeros(N, dtype=bool)

            def seen(x, outside=outside):
                np.logical_or(outside, numerator_outside(x), out=outside)

            ts, td = out["ts"][n], out["td"][n]
            lifetime = tau * exp(alpha * ts)
            conc, cum_u, cum_e = _carbon_year(ar, lifetime, conc_pi, emis[n], nsub(bounds[n], bounds[n + 1], h_cc), h_cc,
                                              out["conc"][n], out["cum_uptake"][n], out["cum_emis"][n], seen)
            erf_co2 = _co2_erf(ar, erf_2x, conc_pi, conc, log)
            erf = ar.aggregate(erf_co2)
            ts1, td1 = _two_layer_year(ar, P[:6], erf, nsub(bounds[n], bounds[n + 1], h_tl), h_tl, ts, td, seen)
            for k, v in (("ts", ts1), ("td", td1), ("conc", conc), ("cum_uptake", cum_u), ("cum_emis", cum_e),
                         ("erf_co2", erf_co2), ("erf_total", erf)):
                out[k][n + 1] = v
            causes[n] = (CAUSE_NUMERATOR * outside + CAUSE_LIFETIME * divisor_outside(lifetime) + CAUSE_CAPACITY * capacity +
                         CAUSE_TS_NAN * np.isnan(ts))
    return out, causes


def coupled(bounds, P, E, init, scen=None, h_tl=0.1, h_cc=0.1, exp=glibc_exp, log=glibc_log, arith=Arith) -> Dict[str, np.ndarray]:
    """The seven [T][N] series of orc_coupled_run.  P [10][N] as tests/helpers.coupled_params, E [S][T] (or [T]), init the
    values at index 0 (scalar or [N]) of ts, td, conc, cum_uptake, cum_emis."""
    return _run(bounds, P, E, init, scen, h_tl, h_cc, exp, log, arith)[0]


def replay_causes(bounds, P, E, init, scen=None, h_tl=0.1, h_cc=0.1, exp=glibc_exp, log=glibc_log) -> np.ndarray:
    """[T-1][N] bit sets, from the restatement's own numerators and divisors: why the kernels' speculative year of that member
    cannot stand (CAUSE_*: a numerator outside its window, the lifetime outside the divisor window, cs or cd outside it,
    Ts NaN at the start of the year -- the year the fused kernel calls settled)."""
    return _run(bounds, P, E, init, scen, h_tl, h_cc, exp, log, Arith)[1]


def carbon_cycle(bounds, P3, E, temperature, init, h=0.1, exp=glibc_exp, arith=Arith) -> Dict[str, np.ndarray]:
    """CarbonCycle on its own (orc_carbon_cycle_solve chained over the axis): P3 = [tau, conc_pi, alpha][N]; E and temperature
    broadcast to [T][N]; init the values at index 0 of conc, cum_uptake, cum_emis."""
    bounds = np.asarray(bounds, dtype=np.float64)
    P3 = np.asarray(P3, dtype=np.float64)
    T, N = len(bounds) - 1, P3.shape[1]
    E = np.broadcast_to(np.asarray(E, dtype=np.float64).reshape(T, -1), (T, N))
    temperature = np.broadcast_to(np.asarray(temperature, dtype=np.float64).reshape(T, -1), (T, N))
    out = {k: np.full((T, N), np.nan) for k in ("conc", "cum_uptake", "cum_emis")}
    for k, v in init.items():
        out[k][0, :] = v
    with np.errstate(all="ignore"):
        for n in range(T - 1):
            lifetime = P3[0] * exp(P3[2] * temperature[n])
            out["conc"][n + 1], out["cum_uptake"][n + 1], out["cum_emis"][n + 1] = _carbon_year(
                arith, lifetime, P3[1], E[n], nsub(bounds[n], bounds[n + 1], h), h, out["conc"][n], out["cum_uptake"][n],
                out["cum_emis"][n], lambda x: None)
    return out


def co2_erf(P2, conc, log=glibc_log, arith=Arith) -> np.ndarray:
    """orc_co2_erf: P2 = [erf_2xco2, conc_pi][N] (the linked kind's rows), conc [...][N]."""
    P2 = np.asarray(P2, dtype=np.float64)
    with np.errstate(all="ignore"):
        return _co2_erf(arith, P2[0], P2[1], np.asarray(conc, dtype=np.float64), log)


def status(series) -> np.ndarray:
    """The kernels' status byte: 1 when a state variable of the last row is not finite (the two forcings are no states)."""
    ok = np.ones(series["ts"].shape[1], dtype=bool)
    for k in ("ts", "td", "conc", "cum_uptake", "cum_emis"):
        ok &= np.isfinite(series[k][-1])
    return (~ok).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the edge ensemble
def below(x: float) -> float:
    return float(np.nextafter(np.float64(x), np.float64(0.0)))


def edge_ensemble() -> Dict[str, object]:
    """320 members on a 13-point axis with steps of 0.5, 1 and 1.5 years.  Most members are tame draws over the ranges of
    tests/helpers.py started off equilibrium (no numerator is a zero), so that their years stand as speculated.  Every third
    lane of members 64-255 is engineered -- one change each, listed in `labels` -- so that replaying and speculative lanes
    share wavefronts; waves 0 and 4 are tame throughout."""
    N, T = 320, 13
    rng = np.random.default_rng(20261020)
    steps = np.tile([1.0, 0.5, 1.5], 4)
    t = 1750.0 + np.concatenate([[0.0], np.cumsum(steps)])
    bounds = np.append(t, t[-1] + (t[-1] - t[-2]))
    P = np.empty((10, N))
    for j, (lo, hi) in enumerate(TL_RANGES):
        P[j] = rng.uniform(lo, hi, N)
    P[6] = rng.uniform(*CC_RANGES[0], N)
    P[7] = rng.uniform(260.0, 300.0, N)
    P[8] = rng.uniform(*CC_RANGES[1], N)
    P[9] = rng.uniform(3.0, 4.5, N)
    E = np.abs(rng.normal(3.0, 3.0, (4, T)))
    E[3, 4] = np.nan
    scen = rng.integers(0, 3, N).astype(np.int32)     # scenario 3 (the NaN) is for its engineered member alone
    init = dict(ts=rng.uniform(0.05, 0.4, N), td=rng.uniform(-0.2, 0.02, N), conc=P[7] + rng.uniform(1.0, 30.0, N),
                cum_uptake=rng.uniform(0.0, 5.0, N), cum_emis=rng.uniform(0.0, 5.0, N))
    lam0, a_, eta_, cs_, cd_, tau_, cpi_, alpha_, e2x_ = 0, 1, 3, 4, 5, 6, 7, 8, 9
    recipes = [("equilibrium", {}, dict(ts=0.0, td=0.0, conc="pi"))]
    for c0 in (2.0 ** -511, below(2.0 ** -511), 2.0 ** 513, below(2.0 ** 513), 0.0, -0.0, 5e-324):
        recipes.append((f"conc_pi 0, C0 {c0!r}", {cpi_: 0.0}, dict(conc=c0)))
    for ts0 in (2.0 ** -510, below(2.0 ** -510), 5e-324, 1e-300):
        recipes.append((f"eta 0.5, Td0 0, Ts0 {ts0!r}", {eta_: 0.5}, dict(ts=ts0, td=0.0)))
    edges = (2.0 ** -128, below(2.0 ** -128), 2.0 ** 129, below(2.0 ** 129))
    for v in edges:
        recipes.append((f"alpha 0, tau {v!r}", {alpha_: 0.0, tau_: v}, {}))
    for v in edges:
        recipes.append((f"cs {v!r}", {cs_: v}, {}))
    for v in edges:
        recipes.append((f"cd {v!r}", {cd_: v}, {}))
    for v in (400.0, -400.0):
        recipes.append((f"alpha {v!r}, Ts0 2", {alpha_: v}, dict(ts=2.0)))
    recipes.append(("alpha inf, Ts0 0", {alpha_: np.inf}, dict(ts=0.0)))
    recipes.append(("Ts0 NaN", {}, dict(ts=np.nan)))
    recipes.append(("Td0 NaN", {}, dict(td=np.nan)))
    recipes.append(("C0 NaN", {}, dict(conc=np.nan)))
    recipes.append(("C0 inf", {}, dict(conc=np.inf)))
    recipes.append(("Ts0 inf", {}, dict(ts=np.inf)))
    recipes.append(("emissions NaN at step 4", {}, dict(scen=3)))
    for v in (1.0, -1.0):
        recipes.append((f"a -5, Ts0 {v!r}", {a_: -5.0}, dict(ts=v)))
    for v in (1e-45, 1e45):
        recipes.append((f"tau {v!r}", {tau_: v}, {}))
    for v in (0.0, -0.0):
        recipes.append((f"erf_2xco2 {v!r}", {e2x_: v}, {}))
    recipes.append(("lambda0 1e-120, Ts0 1e-200", {lam0: 1e-120}, dict(ts=1e-200)))
    labels = {}
    for k, (label, rows, start) in enumerate(recipes):
        i = 64 + 3 * k
        assert i < 256
        labels[i] = label
        for j, v in rows.items():
            P[j, i] = v
        for key, v in start.items():
            if key == "scen":
                scen[i] = v
            else:
                init[key][i] = P[7, i] if isinstance(v, str) else v
    return dict(N=N, T=T, bounds=bounds, P=P, E=E, scen=scen, init=init, h_tl=0.25, h_cc=0.125, labels=labels)


# ------------------------------------------------------------------------------------------------ the fuzz recipe
def fuzz_config(seed: int) -> Dict[str, object]:
    """The configuration tests/test_gpu_parity.py::test_coupled_chain_fuzz draws for `seed` (same generator, same order)."""
    rng = np.random.default_rng(5000 + seed)
    T = int(rng.integers(3, 200))
    n = int(rng.choice([1, 63, 64, 65, 300, 1025]))
    h_tl = float(rng.choice([0.0625, 0.125, 0.25]))
    h_cc = float(rng.choice([0.0625, 0.125, 0.25, 0.5]))
    lengths = rng.integers(1, 5, T) * 0.5
    b = np.concatenate([[1750.0], 1750.0 + np.cumsum(lengths)])
    S = int(rng.choice([1, 1, 3, 30]))
    E = np.abs(rng.normal(3.0, 3.0, (S, T)))
    scen = rng.integers(0, S, n).astype(np.int32) if (S > 1 or rng.random() < 0.3) else None
    P = coupled_params(n, seed=seed)
    init = dict(ts=rng.normal(0.0, 0.2, n) if rng.random() < 0.5 else 0.0, td=0.0,
                conc=rng.uniform(270.0, 300.0, n) if rng.random() < 0.5 else 278.0, cum_uptake=0.0, cum_emis=1.5)
    cuts = sorted(set(int(x) for x in rng.integers(0, T, int(rng.integers(0, 3)))))
    return dict(N=n, T=T, bounds=b, P=P, E=E, scen=scen, init=init, h_tl=h_tl, h_cc=h_cc, cuts=cuts)
