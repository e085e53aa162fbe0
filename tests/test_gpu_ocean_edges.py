"""OceanCarbon's window edges on the GPU against the CPU oracle (oracle.cbind.ocean_run: a plain double O(T^2)
convolution in the reference's order), in both modes.  A short max_history_months makes every edge of csrc/ocean.hip and
csrc/ocean_body.hpp happen inside a 60-year run: the flux-history ring wraps one to five times, pulses leave the
window from year H / 12 on, and

  * the tiled kernel (EXACT; FAST below four times the explicit lags or where the host declines the mode fit) meets windows beside its tiles' pulse counts (12, 24 and
    36 in EXACT, 48 in FAST), where head_end = min(j + K - 1, m0) changes which of the head, bulk and tail loops run;
  * the O(T) recurrence (FAST from 240 months on, 2D-BERN from 480) takes all three of its exit paths, the "straddle" one
    (pulses start leaving inside a model step: H not a multiple of 12) included, preloads its last NEAR pulses across the
    ring's wrap, and joins a run that EXACT began at every stage of the window.

Every case: 130 members (two wavefronts and a ragged tail), 61 years, the two scenarios of test_gpu_ocean._case through a
scenario index.  A window error cannot hide under FAST's bars: on the oracle the outputs for H and H + 1 differ by
8.7e-2 relative or more at every H used here.  The bounds are the ones test_gpu_ocean.py states: bit equality for EXACT
without the temperature feedback (TOL with it), 1e-12 for FAST's fused tiles, FAST_TOL for the recurrence."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import same_values
from tests.test_gpu_ocean import FAST_TOL, TOL, _case, _fast_info, _gpu, orc, ra  # noqa: F401  (ra, orc: fixtures)

pytestmark = pytest.mark.gpu
N, T = 130, 61
FUSED_TOL = 1e-12   # test_ocean_fast_mode_falls_back_when_the_window_is_short's bar
ONES = tuple(range(1, T))
MIXED = (1, 2, 3, 10, 11, 12, 13, 30, 31, 58, 59)   # single steps and longer launches alternate
PATTERNS = {"chunks (3, 20)": (3, 20), "one step per launch": ONES, "mixed": MIXED}
_cases = {}


def _setup(orc, model, H, feedback=False):
    """(bounds, params, inputs, scenario index, oracle result) of one window length, computed once and shared."""
    key = (model, H, feedback)
    if key not in _cases:
        rng = np.random.default_rng(1000 + H)
        b = np.arange(T + 1, dtype=float) + 1750.0
        P, inputs = _case(orc, model, N, T, rng, enable_temp_feedback=0.0, max_history_months=float(H))
        if feedback:   # on half the members
            P[orc.OCEAN_PARAM_NAMES.index("enable_temp_feedback"), ::2] = 1.0
        scen = (np.arange(N) % 2).astype(np.int32)
        want = orc.ocean_run(b, P, inputs, 278.0, 0.0, scen=scen, threads=8)
        for a in (b, P, inputs, scen, want):
            a.flags.writeable = False
        _cases[key] = (b, P, inputs, scen, want)
    return _cases[key]


def _run(ra, case, **kw):
    b, P, inputs, scen, _ = case
    return _gpu(ra, b, P, inputs, 278.0, 0.0, scen=scen, **kw)


def _deviation(got, want):
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    return (np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max()


# ---------------------------------------------------------------------------------------------------------------------
# A. the tiled convolution at window lengths beside the tile widths
BESIDE_TILES = [("HILDA", H) for H in (1, 11, 13, 23, 24, 25, 35, 36, 37, 47, 48, 49)] + \
    [("3D-GFDL", H) for H in (47, 48, 49)]   # its early response is a polynomial
SHORT = [("HILDA", H) for H in (0, 5, 12, 30)]   # test_ocean_gpu_bounded_history's windows, which run EXACT only
# HILDA's short windows past 240 months: the mode fit is there, but too ill-conditioned for the device's double sums (measured
# with the recurrence: test_recurrence_short_window's docstring), so the host declines it and FAST keeps the tiles -- whose
# bulk loop these windows exercise over 20 and 40 years of old pulses, with one wrap of the ring inside the window
ILL_CONDITIONED = [("HILDA", H) for H in (245, 480, 487)]


@pytest.mark.parametrize("model,H", BESIDE_TILES + ILL_CONDITIONED)
def test_tiled_exact_window_beside_a_tile_width(ra, orc, model, H):
    """EXACT (tiles of 36, 24 and 12 pulses; split two-year tiles under one-step launches): the oracle's bits, whatever the
    launches.  The ring has H + 60 rows rounded up to whole years: up to H = 49 it wraps five to eight times in the 720
    months."""
    case = _setup(orc, model, H)
    got = _run(ra, case, mode=ra.MODE_EXACT, recurrence=False)
    assert same_values(got, case[4])
    for what, chunks in PATTERNS.items():
        assert same_values(_run(ra, case, mode=ra.MODE_EXACT, chunks=chunks), got), what


@pytest.mark.parametrize("model,H", SHORT + BESIDE_TILES + ILL_CONDITIONED)
def test_tiled_fast_window_beside_a_tile_width(ra, orc, model, H):
    """FAST below 240 months, or with a declined fit, keeps the tiled kernel, with fused multiply-adds and four-year tiles (48 pulses): within
    FUSED_TOL of the oracle and not equal to it, the same bits under every launch pattern.  With H <= 1 a convolution has no
    term (0) or one (1: fma(f, r, 0) is the rounded product, as 0 + f * r is), so there fusing cannot change a bit and the
    result is the oracle's."""
    case = _setup(orc, model, H)
    got = _run(ra, case, mode=ra.MODE_FAST, recurrence=False)
    dev = _deviation(got, case[4])
    print(f"{model} H = {H}: FAST (fused tiles) vs oracle: max relative deviation {dev:.2e}")
    if H <= 1:
        assert same_values(got, case[4])
    else:
        assert 0.0 < dev <= FUSED_TOL, dev
    for what, chunks in PATTERNS.items():
        assert same_values(_run(ra, case, mode=ra.MODE_FAST, chunks=chunks), got), what


# ---------------------------------------------------------------------------------------------------------------------
# B. the recurrence at short windows: (preset, H, explicit lags NEAR)
RECURRENCE = [("3D-GFDL", 240, 60), ("3D-GFDL", 245, 60), ("3D-GFDL", 251, 60), ("3D-GFDL", 252, 60),
              ("2D-BERN", 480, 120), ("2D-BERN", 487, 120), ("2D-BERN", 493, 120)]


def _wrap_years(H):
    """The model steps at whose start the flux-history ring wraps: it has H + 60 rows rounded up to whole years
    (configure_ocean in csrc/kind_config.cpp), fewer than the run's 720 pulses at every H used here."""
    rows = (H + 60 + 11) // 12 * 12
    assert rows < (T - 1) * 12
    return [y for y in (rows // 12, 2 * rows // 12) if y < T - 1]


def _amplitude(orc, P, H):
    """max |c_q| of the host's mode fit for these parameters (rscm_gpu_ocean_fit_selftest: no GPU call)."""
    from rscm_amd import _lib
    names = orc.OCEAN_PARAM_NAMES
    err, nm, near, nx, mc = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    _lib.check(_lib.load().rscm_gpu_ocean_fit_selftest(int(P[names.index("model"), 0]), P[names.index("irf_scale"), 0],
                                                       P[names.index("irf_switch_time"), 0], H, C.byref(err), C.byref(nm),
                                                       C.byref(near), C.byref(nx), C.byref(mc)))
    return err.value, near.value, nx.value, mc.value


@pytest.mark.parametrize("model,H,near", RECURRENCE)
def test_recurrence_short_window(ra, orc, model, H, near):
    """FAST with the fitted modes at the shortest windows that take them, temperature feedback on half the members: within
    FAST_TOL of the oracle and not equal to it; EXACT gives the oracle's bits (TOL where exp() enters).  At a short window
    nearly every mode carries an exit weight (20 or 21 of 21, against 8 to 14 at 6000 months).
    Measured, max relative deviation of FAST from the oracle (printed per case):
      3D-GFDL 240 / 245 / 251 / 252: 1.33e-11 / 9.10e-12 / 8.08e-12 / 5.85e-12
      2D-BERN 480 / 487 / 493:       3.18e-11 / 2.57e-11 / 3.06e-11
      HILDA 245 / 480 / 487:         2.35e-10 / 4.87e-9 / 3.31e-9 -- over the bar, with amplitudes of 830 / 1.56e4 / 1.04e4:
                                     the host now declines these fits (ILL_CONDITIONED below; kOceanFitMaxCondition in
                                     csrc/kind_config.cpp) and the windows run the fused tiles
    Launch boundaries must not change a bit of FAST's result: one step per launch; a launch that ends at the straddle step
    S = H // 12, one of that step alone and the rest; a boundary at S + 1; launches that start 1, 2, 4 and 5 years (NEAR =
    120: also 9 and 10) after each wrap of the ring, so that the preload of the last NEAR pulses wraps inside it."""
    case = _setup(orc, model, H, feedback=True)
    want = case[4]
    fit, got_near, n_exit, amp = _amplitude(orc, case[1], H)
    assert got_near == near
    exact = _run(ra, case, mode=ra.MODE_EXACT, recurrence=True)
    off = np.arange(N) % 2 == 1   # members without the temperature feedback
    assert same_values(exact[:, :, off], want[:, :, off])
    assert _deviation(exact, want) <= TOL
    fast = _run(ra, case, mode=ra.MODE_FAST, recurrence=True)
    dev, dev_on = _deviation(fast, want), _deviation(fast[:, :, ~off], want[:, :, ~off])
    print(f"{model} H = {H}: fit deviation {fit:.1e}, {n_exit} exit weights, max |c_q| {amp:.4g}; FAST vs oracle: max relative "
          f"deviation {dev:.2e} ({dev_on:.2e} with the temperature feedback)")
    assert 0.0 < dev <= FAST_TOL and 0.0 < dev_on <= FAST_TOL, (dev, dev_on)
    S = H // 12
    # H = 240, 252, 480: step S begins at month 12 S = H, so pulses leave from its first sub-step on (EXIT 1) and every step
    # before it ends at or before month H (EXIT 0) -- no step straddles m = H.  These windows are the control.
    assert (H % 12 == 0) == ((model, H) in (("3D-GFDL", 240), ("3D-GFDL", 252), ("2D-BERN", 480)))
    after_wraps = sorted({w + d for w in _wrap_years(H) for d in (1, 2, 4, 5) + ((9, 10) if near == 120 else ()) if w + d < T - 1})
    assert len(after_wraps) >= 4
    for what, chunks in {"one step per launch": ONES, "step S on its own": (S, S + 1), "a boundary at S + 1": (S + 1,),
                         "launches that start after a wrap": after_wraps}.items():
        assert same_values(_run(ra, case, mode=ra.MODE_FAST, chunks=chunks), fast), (what, chunks)
    # FAST, rewind, FAST: the running sums start from nothing again
    assert same_values(_run(ra, case, mode=ra.MODE_FAST, rewound=True), fast)


@pytest.mark.parametrize("model,H,near", RECURRENCE)
def test_recurrence_joins_a_run_that_exact_began(ra, orc, model, H, near):
    """EXACT up to index k, FAST from there: the running sums are re-formed from the flux history (`rebuild`).  k = 1 .. 4:
    fewer than NEAR months of history, the Horner sum is empty; NEAR / 12 + 1: its first twelve terms; S and S + 1: beside
    the step where pulses start leaving; one year after each wrap of the ring: the walk over the history wraps."""
    case = _setup(orc, model, H, feedback=True)
    want = case[4]
    exact = _run(ra, case, mode=ra.MODE_EXACT)
    S = H // 12
    for k in [1, 2, 3, 4, near // 12 + 1, S, S + 1] + [w + 1 for w in _wrap_years(H)]:
        joined = _run(ra, case, mode=ra.MODE_FAST, recurrence=True, join_at=k)
        assert same_values(joined[:, :k + 1], exact[:, :k + 1]), k
        dev = _deviation(joined, want)
        assert dev <= FAST_TOL, (k, dev)
        assert not same_values(joined[:, k + 1:], exact[:, k + 1:]), k   # the rest did run FAST
