"""GPU tier: what a handle, a sampler and a lock-step plan allocate lazily or allocate again goes with them (csrc/ens.hpp: every d_*
member is an rscm::DevBuf, `delete` is the whole teardown), and a buffer that was replaced serves the results of the new size.

The method and the bound are those of test_gpu_parity.py::test_handle_churn_does_not_leak, which covers the buffers every handle
is created with: one warm-up cycle, free device memory read, 50 cycles, read again, and it may have fallen by less than 64 MB, the
allocator's slack.  A cycle here is create, configure, use, change the size that forces the reallocation, use again, destroy -- at
4096 members on a 20-step axis.  Each test names the smallest buffer it is meant to catch: 50 leaked copies of it are at least twice
the bound.  What is smaller than that -- the row tables, the 3 x kOceanModes table, d_out_vars, the scenario tables, a lock-step
plan's operations, everything a sampler holds at this size -- cannot show in free memory: tests/test_host_dev_buf.py has the owner
itself, failure paths included (no test provokes an allocation failure on the device).  What every cycle does check of those is the
other half: the result after the reallocation equals, bit for bit, that of a fresh handle configured at the second size directly,
so a stale size or a table that was not moved in shows as wrong numbers."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import assert_bit_equal, coupled_params, emissions_syn, f_syn, two_layer_params

pytestmark = pytest.mark.gpu

N = 4096
CYCLES = 50
BOUND = 64 << 20
T_VALUES = np.arange(1750.0, 1771.0)            # 21 points, 20 steps
BOUNDS = np.append(T_VALUES, T_VALUES[-1] + 1.0)
T = T_VALUES.size
CP_INIT = ((1, 0.0), (2, 0.0), (3, 278.0), (4, 0.0), (5, 0.0))


def _churn(cycle, what):
    """cycle() returns the arrays of its second use; they must be the bits of the first call's every time."""
    from rscm_amd import _lib
    want = cycle()                               # the warm-up: whatever the process allocates once is there
    free_before, _ = _lib.mem_info()
    free = [free_before]
    for k in range(CYCLES):
        got = cycle()
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert_bit_equal(g, w, f"{what}: cycle {k}, result {j}")
        free.append(_lib.mem_info()[0])
    fallen = free_before - free[-1]
    steps = {k: (free[k] - free[k + 1]) >> 10 for k in range(CYCLES) if free[k] != free[k + 1]}   # a leak falls every cycle
    print(f"{what}: free device memory fell by {fallen / 1e6:.1f} MB over {CYCLES} cycles")
    assert fallen < BOUND, f"{what}: free device memory fell by {fallen / 1e6:.1f} MB; KiB by cycle: {steps}"
    return want


def _same(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert_bit_equal(g, w, f"{what}, result {j}")


def _constant_rows(defaults, vary=(), seed=3):
    rng = np.random.default_rng(seed)
    P = np.repeat(np.asarray(defaults, dtype=np.float64).reshape(-1, 1), N, axis=1)
    for j in vary:
        P[j] = P[j] * rng.uniform(0.9, 1.1, N)
    return P


def test_ocean_carbon_ring_and_response_table_replaced_at_index_zero():
    """Smallest buffer meant: the first flux-history ring, [120][N] doubles = 3.9 MB a cycle (197 MB over 50).  The second ring
    ([240][N], 7.9 MB), the split-tile sums ([12][N], 0.4 MB) and the FAST mode sums ([21][N], 0.7 MB) ride along; the response
    table and the [3][21] mode table are bytes.

    What this cycle found: the ring used to be cleared with a synchronous hipMemset, which goes through the null stream; with no
    mode table to upload after it (a window too short for the mode fit, as the first one here) that fill stayed the null stream's
    last command and, it seems, kept the block referenced past hipFree (the effect is measured, the mechanism supposed).  In a process that had already run a few hundred GPU tests free
    memory then fell by the ring, 4096 KiB, in every cycle (209.7 MB over the 50, also before the members became owners); the
    ring is now cleared on the handle's own stream (configure_ocean) and the fall is 0.0 MB there as in a fresh process."""
    import rscm_amd as ra
    from rscm_amd import _lib as L
    hist = L.OC_PARAM_NAMES.index("max_history_months")
    P_short = _constant_rows(L.OC_PRESETS["3D-GFDL"], (4, 7))
    P_short[hist] = 60.0                         # a ring of 120 rows, no mode fit (the window is shorter than 4 x 60 months)
    P_long = P_short.copy()
    P_long[hist] = 600.0                         # the ring of the whole axis, 240 rows, and in FAST mode the fitted modes
    yr = T_VALUES - T_VALUES[0]
    inputs = np.stack([300.0 + 2.0 * yr, 0.02 * yr])

    def use(e):
        e.run()
        return [e.get_series(v) for v in (1, 2, 3)]

    def configured(P):
        e = ra.Ensemble(ra.KIND_OCEAN_CARBON, N, BOUNDS)
        e.set_mode(ra.MODE_FAST)
        e.set_params(P)
        e.set_forcing(inputs)
        e.set_initial(1, 290.0)
        e.set_initial(2, 0.0)
        return e

    def cycle():
        with configured(P_short) as e:
            use(e)
            e.rewind()
            e.set_params(P_long)
            return use(e)

    with configured(P_long) as fresh:
        want = use(fresh)
    _same(_churn(cycle, "OceanCarbon"), want, "OceanCarbon against a handle configured at 600 months")


def test_ghg_forcing_tables_of_one_and_then_three_scenarios():
    """Nothing here is large enough for free memory to show: the forcing block is [S][3][T] doubles, the derived rows [S][kGhgRows][T],
    the members' scenario table [N] int32 (16 KB), the member constants [8][N] (0.26 MB).  The cycle is here for the other half: the
    tables of three scenarios are moved in whole, and the members' scenario table goes when it is omitted."""
    import rscm_amd as ra
    from rscm_amd import _lib as L
    yr = T_VALUES - T_VALUES[0]
    conc = np.stack([278.0 * 1.005 ** yr, 722.0 + 10.0 * yr, 270.0 + 0.5 * yr])
    three = np.stack([conc, 1.1 * conc, 0.9 * conc])
    P = _constant_rows(L.GH_DEFAULTS, (1, 4, 18))
    n_vars = len(L.GH_VARS)

    def use(e):
        e.run()
        return [e.get_series(v) for v in range(1, n_vars)]

    def cycle():
        with ra.Ensemble(ra.KIND_GHG_FORCING, N, BOUNDS) as e:
            e.set_params(P)
            e.set_forcing(conc, scenario_of_member=np.zeros(N, dtype=np.int32))
            use(e)
            e.rewind()
            e.set_forcing(three)
            return use(e)

    with ra.Ensemble(ra.KIND_GHG_FORCING, N, BOUNDS) as fresh:
        fresh.set_params(P)
        fresh.set_forcing(three)
        want = use(fresh)
    _same(_churn(cycle, "GhgForcing"), want, "GhgForcing against a handle given the three scenarios directly")


def test_climate_udeb_columns_grow_from_30_to_80_layers_at_index_zero():
    """Smallest buffer meant: the ocean columns as first allocated, [2][64][N] doubles = 4.2 MB a cycle (210 MB over 50); grown they
    are [2][80][N], 5.2 MB.  The work array of the 80-layer kernel, [80][N] = 2.6 MB, would show as well (131 MB) but with less than
    twice the bound to spare; its geometry table is bytes."""
    import rscm_amd as ra
    from rscm_amd import _lib as L
    layers = L.UD_PARAM_NAMES.index("n_layers")
    P30 = _constant_rows(L.UD_DEFAULTS, (3, 10, 12))
    P30[layers] = 30.0
    P80 = P30.copy()
    P80[layers] = 80.0
    F = 3.71 * np.minimum((T_VALUES - T_VALUES[0]) / 15.0, 1.0)
    n_vars = len(L.UD_VARS)

    def use(e):
        e.run()
        return [e.get_series(v) for v in range(1, n_vars)]

    def configured(P):
        e = ra.Ensemble(ra.KIND_UDEB, N, BOUNDS)
        e.set_params(P)
        e.set_forcing(F)
        for v in (1, 2, 3, 4):
            e.set_initial(v, 0.0)
        return e

    def cycle():
        with configured(P30) as e:
            use(e)
            e.rewind()
            e.set_params(P80)
            return use(e)

    with configured(P80) as fresh:
        want = use(fresh)
    _same(_churn(cycle, "ClimateUDEB"), want, "ClimateUDEB against a handle configured at 80 layers")


def test_windowed_handle_with_an_output_list():
    """Smallest buffer meant: the output store of the five variables of the coupled kind, [5][21][N] doubles = 3.4 MB a cycle
    (172 MB over 50).  The saved initial rows ([5][N], 0.16 MB) and the list of output variables (20 bytes) are below what shows.
    Nothing is reallocated here: the cycle is create, step the axis, read the store, destroy."""
    import rscm_amd as ra
    P = coupled_params(N)
    E = emissions_syn(T_VALUES + 200.0)

    def cycle():
        with ra.Ensemble(ra.KIND_COUPLED, N, BOUNDS, window_rows=8, output_stride=1, output_vars=[1, 2, 3, 4, 5]) as e:
            e.set_params(P)
            e.set_forcing(E)
            for v, x in CP_INIT:
                e.set_initial(v, x)
            for _ in range(T - 1):
                e.step()
            return [e.get_series(v, 0, T) for v in (1, 2, 3, 4, 5)]

    _churn(cycle, "windowed coupled handle")


def test_two_layer_likelihood_scratch_resampling_diagnostics_indicators_and_noise():
    """Smallest buffer meant: the ancestors of 2^19 draws, int64 = 4.2 MB a cycle (210 MB over 50), which replace those of 1000.
    The scratch of the deferred observations ([20][N], 0.66 MB), the diagnostic's 20 rows (0.66 MB), the four indicator slots
    ([11][N] each, 1.4 MB together) and the [N] vectors (log-likelihood, running weights, noise state) are each below what shows on
    their own; all of them leaked together, 3 MB a cycle, would show.  The observation and slot tables are bytes."""
    import rscm_amd as ra
    rng = np.random.default_rng(11)
    P = two_layer_params(N)
    F = f_syn(T_VALUES)
    w = rng.integers(1, 1000, N).astype(np.int64)
    few = ([1, 1], [3, 7], [0.2, 0.4], [0.3, 0.3])
    tidx = np.arange(1, T)
    many = ([1] * 20 + [2] * 20, list(tidx) * 2, list(0.02 * tidx) + list(0.005 * tidx), [0.3] * 40)
    few_ref, many_ref = {1: (0, 5)}, {1: (0, 10), 2: (0, 10)}

    def configured():
        e = ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS)
        e.set_params(P)
        e.set_forcing(F)
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        return e

    def use(e, obs, reference, n_draws, diag_rows):
        out = [e.run_loglik(*obs, reference=reference)]
        e.rewind()
        e.set_forcing_noise(0.3, 5, phi=0.5)
        e.run()
        out += [e.get_series(1)]
        e.set_member_weights(w)
        out += [e.resample(n_draws, seed=9).to_host().astype(np.float64)]
        vid = e.var_ids.get("Ocean Heat Content") or e.define_heat_content()
        e.compute_diagnostic(vid, 0, diag_rows)
        out += [e.get_series(vid, 0, diag_rows)]
        for slot in range(4):
            ind = e.indicators(1, 0, T, thresholds=[0.1 * (slot + 1)], slot=slot)
            out += [ind["peak"].to_host(), ind["crossing"][0].to_host()]
        return out

    def cycle():
        with configured() as e:
            use(e, few, few_ref, 1000, 2)
            e.rewind()
            e.clear_forcing_noise()
            return use(e, many, many_ref, 1 << 19, 20)

    with configured() as fresh:
        want = use(fresh, many, many_ref, 1 << 19, 20)
    _same(_churn(cycle, "two-layer handle"), want, "two-layer handle against one used at the second sizes directly")


def _sampler(ens, rows, base, lo, hi, obs, seed=5):
    from rscm_amd import _lib as L
    ov, ot, val, sig = obs
    rows = np.asarray(rows, dtype=np.int32)
    kinds = np.zeros(len(rows), dtype=np.int32)
    base, lo, hi, val, sig = (L.f64(x) for x in (base, lo, hi, val, sig))
    ov, ot = np.asarray(ov, dtype=np.int32), np.asarray(ot, dtype=np.int32)
    h = C.c_void_p()
    L.check(ens._lib.rscm_sampler_create(ens._h, 2 * N, len(rows), L.iptr(rows), L.dptr(base), L.iptr(kinds), L.dptr(lo), L.dptr(hi), None, None,
                                         len(ov), L.iptr(ov), L.iptr(ot), L.dptr(val), L.dptr(sig), 0, 2.0, C.c_uint64(seed), C.byref(h)))
    return h


def test_sampler_on_a_two_layer_evaluator_fused_and_stored():
    """At 8192 walkers in 6 dimensions everything a sampler holds is 1.5 MB (positions [6][8192], proposals and exchange buffers of
    [7][N]): 75 MB over 50 cycles, about the bound, so free memory is no sharp test of it and the owner's host program is.  The cycle
    is here for the two creators and the destructor: the scores of the positions, log prior + ln L, come out the same from every
    sampler, on the fused path (ascending observation times) and on the stored one (its table is the sampler's own buffer)."""
    import rscm_amd as ra
    from rscm_amd import _lib as L
    from tests.helpers import TL_RANGES
    lo, hi = np.array(TL_RANGES).T
    base = 0.5 * (lo + hi)
    pos = np.ascontiguousarray(two_layer_params(2 * N, seed=4).T)      # [W][6]
    ascending = ([1, 1, 2], [4, 12, 9], [0.1, 0.3, 0.02], [0.3, 0.3, 0.1])
    descending = ([1, 1, 2], [12, 4, 9], [0.3, 0.1, 0.02], [0.3, 0.3, 0.1])

    def scores(e, obs):
        h = _sampler(e, np.arange(6), base, lo, hi, obs)
        try:
            L.check(e._lib.rscm_sampler_set_positions(h, L.dptr(pos)))
            logp = np.empty(2 * N)
            L.check(e._lib.rscm_sampler_get(h, None, L.dptr(logp), None, None))
        finally:
            L.check(e._lib.rscm_sampler_destroy(h))
        return logp

    def cycle():
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as e:
            e.set_params(np.repeat(base[:, None], N, axis=1))
            e.set_forcing(f_syn(T_VALUES))
            e.set_initial(1, 0.0)
            e.set_initial(2, 0.0)
            return [scores(e, ascending), scores(e, descending)]

    fused, stored = _churn(cycle, "sampler")
    assert np.isfinite(fused).all() and np.isfinite(stored).all()


def test_lockstep_plan_of_three_handles_and_then_of_two():
    """A plan's operation table is a few hundred bytes a handle and its page-locked ring is host memory: free device memory cannot
    show either.  The cycle is here for the plan's destructor and for the table of the shorter list, built aside and moved in: the
    first two handles' series after the two-handle run are those of two fresh handles run as a pair."""
    import rscm_amd as ra
    from rscm_amd import _lib as L
    from rscm_amd.ensemble import run_lockstep
    Pc = coupled_params(N)
    E = emissions_syn(T_VALUES + 200.0)
    lib = L.load()
    stream = C.c_void_p()
    L.check(lib.rscm_gpu_stream_create(0, C.byref(stream)))

    def graph(n_handles):
        es = [ra.Ensemble(k, N, BOUNDS) for k in (ra.KIND_CARBON_CYCLE, ra.KIND_CO2_ERF, ra.KIND_TWO_LAYER)[:n_handles]]
        for e in es:
            e.set_stream(stream.value)
        cc, ce = es[:2]
        cc.set_params(Pc[[6, 7, 8]])
        ce.set_params(Pc[[9, 7]])
        cc.set_forcing(np.stack([E, np.zeros(T)]))
        for v, x in ((1, 278.0), (2, 0.0), (3, 0.0)):
            cc.set_initial(v, x)
        ce.link_input(0, cc, 1, ra.SRC_UPSTREAM)
        if n_handles == 3:
            tl = es[2]
            tl.set_params(Pc[:6])
            tl.set_initial(1, 0.0)
            tl.set_initial(2, 0.0)
            tl.link_input(0, ce, 1, ra.SRC_UPSTREAM)
        return es

    def close(es):
        for e in reversed(es):                   # consumers before the producers they link to
            e.close()

    def pair(es):
        run_lockstep(es[:2])
        return [es[0].get_series(1), es[1].get_series(1)]

    def cycle():
        es = graph(3)
        try:
            run_lockstep(es)
            assert np.isfinite(es[2].get_series(1)[-1]).all()
            for e in es:
                e.rewind()
            return pair(es)
        finally:
            close(es)

    try:
        es = graph(2)
        try:
            want = pair(es)
        finally:
            close(es)
        _same(_churn(cycle, "lock-step plan"), want, "lock-step pair against two fresh handles")
    finally:
        L.check(lib.rscm_gpu_stream_destroy(0, stream))
