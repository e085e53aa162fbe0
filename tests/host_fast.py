"""Host restatement of the FAST year (RSCM_MODE_FAST) of the two-layer kind, the CarbonCycle kind and the fused coupled chain in
numpy float64, and the edge ensemble that carries it to the members no tolerance test compares.

Written from the statements of csrc/two_layer_body.hpp (make_fast, rhs_fast, rk4_year_fast), csrc/carbon_body.hpp
(carbon_cycle_year_fast) and csrc/coupled.hip (coupled_fast_kernel): IEEE + - * /, each rounded on its own -- one numpy ufunc call
per operation; numpy neither fuses nor reassociates separate calls -- and explicit fused multiply-adds, C99 fma() over arrays from
the oracle library (oracle.cbind.fma, held to exact rational arithmetic in tests/test_host_fast.py).  Vectorised over members,
Python loops over model steps and RK4 sub-steps.  The two transcendentals of the carbon box and CO2ERF are arguments:
  * the defaults are glibc's exp / log through ctypes; with them the module is within FAST's stated 1e-11 of the oracle on bounded
    members (tests/test_host_fast.py, no GPU);
  * the GPU tier passes the device's own exp and log_f64 (rscm_amd.ensemble.selftest_math, ops 2 and 0), and then every output of
    the FAST kernels has to carry this module's bits for every member, inf and NaN included (tests/test_gpu_fast_bits.py).
Pure numpy + the fma helper; no product code."""
from __future__ import annotations

from typing import Dict

import numpy as np

from oracle.cbind import fma
from tests import host_coupled as hc
from tests.helpers import coupled_params, f_syn

GTC_PER_PPM = 2.13                     # crates/rscm-components/src/constants.rs:37
PPM_PER_GTC = 1.0 / 2.13               # carbon_body.hpp, kPpmPerGtc: the quotient rounded once
LN2 = hc.LN2
SERIES = hc.SERIES
nsub = hc.nsub


# ------------------------------------------------------------------------------------------------ the arithmetic
def combine_fast(y, k1, k2, k3, k4, third, sixth):
    """rk4_year_fast: y + h/6 (k1 + k4) + h/3 (k2 + k3), the inner product-sum fused first."""
    return fma(k2 + k3, third, fma(k1 + k4, sixth, y))


def combine_exact(y, k1, k2, k3, k4, third, sixth):
    """EXACT's association (ode_solvers 0.6.1), which FAST does not use."""
    return hc.rk4_combine(y, k1, k2, k3, k4, sixth)


def phi_fused(z):
    """carbon_cycle_year_fast: 1 - z/2 + z^2/6 - z^3/24 as a Horner chain of three FMAs."""
    return fma(z, fma(z, fma(z, -1.0 / 24.0, 1.0 / 6.0), -0.5), 1.0)


class Arith:
    """The five operations a subtly wrong FAST year gets wrong; tests/test_host_fast.py swaps them one at a time."""
    stage = staticmethod(fma)                     # t = fma(q, Ts, F/Cs), the second operation of every stage
    combine = staticmethod(combine_fast)
    carry_difference = True                       # the second unknown is w = Ts - Td, not Td
    scale_forcing = staticmethod(lambda erf, cs, inv_cs: erf * inv_cs)
    phi = staticmethod(phi_fused)


class Folded:
    """make_fast: lambda0/Cs, a/Cs, efficacy*eta/Cs (the product of the two first), eta/Cd, with 1/Cs formed once."""

    def __init__(self, P):
        lambda0, a, efficacy, eta, cs, cd = (np.ascontiguousarray(r, dtype=np.float64) for r in P[:6])
        self.cs = cs
        self.inv_cs = 1.0 / cs
        self.l0 = lambda0 * self.inv_cs
        self.a = a * self.inv_cs
        self.ee = efficacy * eta * self.inv_cs
        self.ed = eta / cd


def _rhs_fast(ar, p, erf_cs, ts, w):
    q = fma(p.a, ts, -p.l0)
    t = ar.stage(q, ts, erf_cs)
    dts = fma(-p.ee, w, t)
    dw = fma(-p.ed, w, dts)
    return dts, dw


def _two_layer_year(ar, p, erf_cs, m, h, ts, td):
    """rk4_year_fast: m sub-steps of (Ts, w) with w = Ts - Td formed at the start of the model step, Td = Ts - w at its end."""
    half, third, sixth = h / 2.0, h / 3.0, h / 6.0
    if not ar.carry_difference:
        return _two_layer_year_td(ar, p, erf_cs, m, h, ts, td)
    w = ts - td
    for _ in range(m):
        k1s, k1w = _rhs_fast(ar, p, erf_cs, ts, w)
        k2s, k2w = _rhs_fast(ar, p, erf_cs, fma(k1s, half, ts), fma(k1w, half, w))
        k3s, k3w = _rhs_fast(ar, p, erf_cs, fma(k2s, half, ts), fma(k2w, half, w))
        k4s, k4w = _rhs_fast(ar, p, erf_cs, fma(k3s, h, ts), fma(k3w, h, w))
        ts = ar.combine(ts, k1s, k2s, k3s, k4s, third, sixth)
        w = ar.combine(w, k1w, k2w, k3w, k4w, third, sixth)
    return ts, ts - w


def _two_layer_year_td(ar, p, erf_cs, m, h, ts, td):
    """NOT the FAST year: the same fused stages with Td as the second unknown (Td' = ed (Ts - Td)); the swap `carry_difference`."""
    half, third, sixth = h / 2.0, h / 3.0, h / 6.0

    def rhs(s, d):
        w = s - d
        dts, _ = _rhs_fast(ar, p, erf_cs, s, w)
        return dts, p.ed * w

    for _ in range(m):
        k1s, k1d = rhs(ts, td)
        k2s, k2d = rhs(fma(k1s, half, ts), fma(k1d, half, td))
        k3s, k3d = rhs(fma(k2s, half, ts), fma(k2d, half, td))
        k4s, k4d = rhs(fma(k3s, h, ts), fma(k3d, h, td))
        ts = ar.combine(ts, k1s, k2s, k3s, k4s, third, sixth)
        td = ar.combine(td, k1d, k2d, k3d, k4d, third, sixth)
    return ts, td


def _carbon_year(ar, rtau, alpha, conc_pi, emis, temperature, m, h, conc, cum_u, cum_e, exp):
    """carbon_cycle_year_fast: the closed RK4 step of the linear box, m times; one exp per model step, no division."""
    r = rtau * exp(-(alpha * temperature))
    e_ppm = emis * PPM_PER_GTC
    A = fma(conc_pi, r, e_ppm)
    z = h * r
    hphi = h * ar.phi(z)
    inc_e = (((emis + emis * 2.0) + emis * 2.0) + emis) * (h / 6.0)
    dsum = np.zeros_like(conc)
    for _ in range(m):
        k1 = fma(-r, conc, A)
        conc = fma(k1, hphi, conc)
        dsum = fma(k1, hphi, dsum)
        cum_e = cum_e + inc_e
    cum_u = fma(GTC_PER_PPM, fma(float(m) * h, e_ppm, -dsum), cum_u)
    return conc, cum_u, cum_e


def _member_rows(rows, scen, N):
    """[S][T] with a member -> scenario map (None: scenario 0)  ->  [T][N]."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    s = np.zeros(N, dtype=np.int64) if scen is None else np.asarray(scen, dtype=np.int64)
    return np.ascontiguousarray(rows[s].T)


def _start(T, N, value):
    out = np.full((T, N), np.nan)
    out[0, :] = value
    return out


# ------------------------------------------------------------------------------------------------ the three kinds
def two_layer_fast(bounds, P, F, ts0, td0, scen=None, source=0, h=0.1, arith=Arith):
    """The two-layer kind in FAST mode.  P [6][N], F [S][T] (or [T]) read at index n + source (0: exogenous, 1: upstream), ts0 / td0
    scalar or [N].  Returns Ts [T][N], Td [T][N] and the status bytes (a non-finite final Ts or Td)."""
    bounds = np.asarray(bounds, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    T, N = len(bounds) - 1, P.shape[1]
    forcing = _member_rows(F, scen, N)
    assert forcing.shape == (T, N) and P.shape[0] == 6 and source in (0, 1)
    ts, td = _start(T, N, ts0), _start(T, N, td0)
    with np.errstate(all="ignore"):
        p = Folded(P)
        for n in range(T - 1):
            erf_cs = arith.scale_forcing(forcing[n + source], p.cs, p.inv_cs)
            ts[n + 1], td[n + 1] = _two_layer_year(arith, p, erf_cs, nsub(bounds[n], bounds[n + 1], h), h, ts[n].copy(), td[n].copy())
    return ts, td, (~(np.isfinite(ts[-1]) & np.isfinite(td[-1]))).astype(np.uint8)


def carbon_cycle_fast(bounds, P3, E, temperature, init, h=0.1, exp=hc.glibc_exp, arith=Arith) -> Dict[str, np.ndarray]:
    """CarbonCycle on its own in FAST mode (carbon_cycle_body<MODE != 0>): P3 = [tau, conc_pi, alpha][N]; E and temperature broadcast
    to [T][N]; init the values at index 0 of conc, cum_uptake, cum_emis."""
    bounds = np.asarray(bounds, dtype=np.float64)
    P3 = np.ascontiguousarray(P3, dtype=np.float64)
    T, N = len(bounds) - 1, P3.shape[1]
    E = np.ascontiguousarray(np.broadcast_to(np.asarray(E, dtype=np.float64).reshape(T, -1), (T, N)))
    temperature = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float64).reshape(T, -1), (T, N)))
    out = {k: _start(T, N, init[k]) for k in ("conc", "cum_uptake", "cum_emis")}
    with np.errstate(all="ignore"):
        rtau = 1.0 / P3[0]
        for n in range(T - 1):
            out["conc"][n + 1], out["cum_uptake"][n + 1], out["cum_emis"][n + 1] = _carbon_year(
                arith, rtau, P3[2], P3[1], E[n], temperature[n], nsub(bounds[n], bounds[n + 1], h), h, out["conc"][n].copy(),
                out["cum_uptake"][n].copy(), out["cum_emis"][n].copy(), exp)
    return out


def coupled_fast(bounds, P, E, init, scen=None, h_tl=0.1, h_cc=0.1, exp=hc.glibc_exp, log=hc.glibc_log, arith=Arith) -> Dict[str, np.ndarray]:
    """The fused coupled chain in FAST mode (coupled_fast_kernel): the seven [T][N] series.  P [10][N] as tests/helpers.coupled_params,
    E [S][T] (or [T]), init the values at index 0 (scalar or [N]) of ts, td, conc, cum_uptake, cum_emis."""
    bounds = np.asarray(bounds, dtype=np.float64)
    P = np.ascontiguousarray(P, dtype=np.float64)
    T, N = len(bounds) - 1, P.shape[1]
    emis = _member_rows(E, scen, N)
    assert emis.shape == (T, N) and P.shape[0] == 10
    out = {k: _start(T, N, init.get(k, np.nan)) for k in SERIES}
    with np.errstate(all="ignore"):
        p = Folded(P)
        rtau, conc_pi, alpha, erf_scale = 1.0 / P[6], P[7], P[8], P[9] / LN2
        for n in range(T - 1):
            ts, td = out["ts"][n].copy(), out["td"][n].copy()
            conc, cum_u, cum_e = _carbon_year(arith, rtau, alpha, conc_pi, emis[n], ts, nsub(bounds[n], bounds[n + 1], h_cc), h_cc,
                                              out["conc"][n].copy(), out["cum_uptake"][n].copy(), out["cum_emis"][n].copy(), exp)
            erf_co2 = erf_scale * log(1.0 + (conc - conc_pi) / conc_pi)
            erf = hc.aggregate_sum(erf_co2)
            erf_cs = arith.scale_forcing(erf, p.cs, p.inv_cs)
            ts, td = _two_layer_year(arith, p, erf_cs, nsub(bounds[n], bounds[n + 1], h_tl), h_tl, ts, td)
            for k, v in (("ts", ts), ("td", td), ("conc", conc), ("cum_uptake", cum_u), ("cum_emis", cum_e), ("erf_co2", erf_co2),
                         ("erf_total", erf)):
                out[k][n + 1] = v
    return out


def status(series) -> np.ndarray:
    """The kernels' status byte: 1 when a state variable of the last row is not finite (the two forcings are no states).  For the
    coupled chain's seven series, the carbon kind's three, or dict(ts=, td=)."""
    keys = [k for k in ("ts", "td", "conc", "cum_uptake", "cum_emis") if k in series]
    return (~np.all([np.isfinite(series[k][-1]) for k in keys], axis=0)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the edge ensemble
SUBNORMAL = 5e-324
FORCINGS = ("ordinary", "all zero", "* 1e-300", "* 1e250", "* 5e-324", "one NaN year")
EMISSIONS = ("ordinary", "all zero", "inf in one year", "NaN in one year")


def edge_ensemble_fast() -> Dict[str, object]:
    """257 members (four full wavefronts and a lone member: a ragged last wave and last block) on a 41-point axis with steps of
    0.5, 1 and 5 years.  Every fifth lane from 3 on is engineered -- one change each, listed in `labels` -- so that extreme
    members share wavefronts with ordinary ones; the rest is tests/helpers.coupled_params (rows 0-5: the two-layer draw).
    `P` [10][N]; `F` [6][T] the two-layer forcings FORCINGS with the map `scen_f`; `E` [4][T] the emissions EMISSIONS with the map
    `scen_e` (2 and 3 for their engineered members alone); `ts0`, `td0`, `init` the start values.  The heat-capacity members start at
    Ts = Td = 0, where the reference keeps a zero forcing at exact zeros."""
    N = 257
    rng = np.random.default_rng(20261021)
    steps = np.concatenate([np.full(12, 0.5), np.full(20, 1.0), np.full(8, 5.0)])
    t = 1750.0 + np.concatenate([[0.0], np.cumsum(steps)])
    T = len(t)
    bounds = np.append(t, t[-1] + (t[-1] - t[-2]))
    P = coupled_params(N, seed=20261021)
    f = f_syn(t) + 0.25                         # (no exact zero at the first point)
    nan_year = f.copy()
    nan_year[9] = np.nan
    F = np.stack([f, np.zeros(T), f * 1e-300, f * 1e250, f * SUBNORMAL, nan_year])
    E = np.abs(rng.normal(3.0, 3.0, (4, T)))
    E[1] = 0.0
    E[2, 7] = np.inf
    E[3, 11] = np.nan
    scen_f = rng.integers(0, len(FORCINGS), N).astype(np.int32)
    scen_e = rng.integers(0, 2, N).astype(np.int32)
    init = dict(ts=rng.uniform(0.0, 0.4, N), td=rng.uniform(-0.1, 0.1, N), conc=P[7] + rng.uniform(1.0, 30.0, N),
                cum_uptake=rng.uniform(0.0, 5.0, N), cum_emis=rng.uniform(0.0, 5.0, N))
    lam0, a_, eff_, eta_, cs_, cd_, tau_, cpi_, alpha_ = 0, 1, 2, 3, 4, 5, 6, 7, 8
    rest = dict(ts=0.0, td=0.0)
    recipes = [(f"a {v!r}", {a_: v}, {}) for v in (0.0, 0.05, 0.3, 1.0, 5.0)]
    for name, row, tame in (("cs", cs_, 1e-3), ("cd", cd_, 1e3)):
        for v in (0.0, SUBNORMAL, -SUBNORMAL, 2.0 ** -130, 2.0 ** 130, -8.0, np.inf, np.nan, tame):
            recipes.append((f"{name} {v!r}", {row: v}, rest))
    for name, row in (("lambda0", lam0), ("efficacy", eff_), ("eta", eta_)):
        for v in (np.inf, np.nan, 1e308):
            recipes.append((f"{name} {v!r}", {row: v}, {}))
    for v in (0.0, np.inf, SUBNORMAL):
        recipes.append((f"tau {v!r}", {tau_: v}, {}))
    # z = h/lifetime large enough that every term of phi(z) counts, and a pre-industrial level so low that the concentration is
    # all excess and follows each year's emissions: its increments are of its own size, so it shows their last bits
    for v in (0.05, 0.5, 2.0):
        recipes.append((f"tau {v!r}, conc_pi 0.01", {tau_: v, cpi_: 0.01, a_: 0.0, 9: 0.37}, dict(scen_e=0, conc=1.0)))
    for v in (400.0, -400.0):                   # exp(-(alpha Ts)) underflows to 0 / overflows to inf
        recipes.append((f"alpha {v!r}, Ts0 2", {alpha_: v}, dict(ts=2.0)))
    recipes.append(("conc_pi 0.0", {cpi_: 0.0}, {}))
    recipes.append(("emissions inf in one year", {}, dict(scen_e=2)))
    recipes.append(("emissions NaN in one year", {}, dict(scen_e=3)))
    labels = {}
    for k, (label, rows, start) in enumerate(recipes):
        i = 3 + 5 * k
        assert i < N - 1
        labels[i] = label
        for j, v in rows.items():
            P[j, i] = v
        for key, v in start.items():
            if key == "scen_e":
                scen_e[i] = v
            else:
                init[key][i] = v
    return dict(N=N, T=T, t=t, bounds=bounds, P=P, F=F, E=E, scen_f=scen_f, scen_e=scen_e, ts0=init["ts"], td0=init["td"], init=init,
                h_tl=0.25, h_cc=0.125, labels=labels)
