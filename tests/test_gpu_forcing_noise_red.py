"""GPU tier of the red (AR(1)) forcing noise of a two-layer ensemble (rscm_ens_set_forcing_noise_ar1;
Ensemble.set_forcing_noise(..., phi=)): member i is forced at forcing-axis index t by F' = F + e_t, e_0 = sigma z_0,
e_t = (phi e_{t-1}) + ((sigma sqrt(1 - phi^2)) z_t), every operation rounded on its own, z the white tier's deviate.  e is a pure
function of (seed, sigma, phi, member id, t); the handle caches each member's value at the last index it ran and forms it again
from the draws wherever a run starts elsewhere, so every launch plan below must give the bits of one run.

The reference of every value test: each member's series formed on the host (tests/host_forcing_noise_red.py, numpy) and given to
the CPU oracle's plain two-layer run as one scenario per member.  EXACT mode is compared bit for bit; RSCM_MODE_FAST bit for bit
with a PLAIN two-layer handle given the same host-formed series and at the existing FAST tolerance (1e-11 relative to
max(1, |oracle|) on bounded members) with the oracle.

The shapes and helpers are the white tier's (tests/test_gpu_forcing_noise.py): N = 130 members (two wavefronts and two lanes) on a
40-step uneven axis unless a test says otherwise; a noise tuple is (sigma, seed, member_offset, phi)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import host_forcing_mix as hm
from tests import host_forcing_noise as hn
from tests import host_forcing_noise_red as hr
from tests.helpers import assert_bit_equal, two_layer_params
from tests.test_gpu_forcing_noise import (BIG_OFFSET, BOUNDS, FAST_RTOL, N, SEED, SIGMA, T, TD, TS, _annual, _block, _member_series, _mix,  # noqa: F401
                                          _mix_params, _own_series, _plain, _rows, _same, _scen, _series, _status_of, orc, ra)

pytestmark = pytest.mark.gpu

PHIS = (0.7, -0.5)
phis = pytest.mark.parametrize("phi", PHIS)


def _want_rows(offset, phi, n=N, n_times=T):
    return hr.red_noise(SEED, np.arange(n, dtype=np.uint64) + np.uint64(offset), n_times, SIGMA, phi).T


# ---------------------------------------------------------------------------------------------- 1. the term itself
@phis
@pytest.mark.parametrize("offset", [0, BIG_OFFSET], ids=["offset0", "offset2^33+5"])
def test_noise_rows_equal_the_restatement(ra, offset, phi):
    with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as e:
        e.set_forcing_noise(SIGMA, SEED, offset, phi)
        assert e.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": offset, "phi": phi}
        assert e.forcing_noise_cached_index == -1
        want = _want_rows(offset, phi)
        rows = e.forcing_noise_rows()
        assert_bit_equal(rows, want, "all rows")
        assert_bit_equal(e.forcing_noise_rows(5, 9), rows[5:9], "rows 5..8")
        assert e.forcing_noise_rows(5, 5).shape == (0, N)


# ---------------------------------------------------------------------------------------------- 2.-4. EXACT: the oracle's bits
@phis
@pytest.mark.parametrize("source", [0, 1], ids=["exogenous", "upstream"])
@pytest.mark.parametrize("n_scen", [1, 3])
def test_exact_plain_handle_equals_the_oracle(ra, orc, n_scen, source, phi):
    """source = upstream first reads index 1: e_0 is formed from its draw before the first year (a one-draw spin-up)."""
    F, scen, P = _rows(n_scen), _scen(n_scen), two_layer_params(N)
    want = hr.oracle_run_red(orc, BOUNDS, P, _member_series(F, scen), SIGMA, phi, SEED, source=source)
    assert np.isfinite(want[0]).all()
    with _plain(ra, P, F, scen, source, noise=(SIGMA, SEED, 0, phi)) as e:
        e.run()
        assert e.finished() and e.forcing_noise_cached_index == T - 2 + source
        _same(_series(e), want, f"S={n_scen} source={source} phi={phi}")
        assert not e.status().any()


@phis
def test_exact_mix_handle_equals_the_oracle(ra, orc, phi):
    K = 3
    S, scen, P = _block(2, K), _scen(2), _mix_params(K)
    want = hr.oracle_run_red(orc, BOUNDS, P[:6], hm.mix_forcing(S, P[6:], scen), SIGMA, phi, SEED, member_offset=BIG_OFFSET)
    with _mix(ra, P, S, scen, noise=(SIGMA, SEED, BIG_OFFSET, phi)) as e:
        e.run()
        _same(_series(e), want, f"mix K={K} phi={phi}")
        assert not e.status().any()


def test_table_beyond_the_lds_budget_equals_the_oracle(ra, orc):
    """130 scenarios x 200 steps: 130 * 200 * 8 = 208 000 B, more than the 159 KiB a launch may stage, so the rows are read through
    L2; the first 40 steps of the same table run on their own are staged.  Same bits."""
    nt, phi = 201, 0.7
    assert N * (nt - 1) * 8 > 159 * 1024 > N * 40 * 8
    b, F, scen, P = _annual(nt), _rows(N, nt), np.arange(N, dtype=np.int32)[::-1].copy(), two_layer_params(N)
    want = hr.oracle_run_red(orc, b, P, _member_series(F, scen), SIGMA, phi, SEED)
    with _plain(ra, P, F, scen, bounds=b, noise=(SIGMA, SEED, 0, phi)) as e:
        e.run()
        full = _series(e)
        _same(full, want, "130 scenarios, 200 steps")
        e.rewind()
        e.run(40)
        head = _series(e)
        assert_bit_equal(head[0][:41], full[0][:41], "first 40 steps, staged against read through L2: Ts")
        assert_bit_equal(head[1][:41], full[1][:41], "first 40 steps, staged against read through L2: Td")
        e.run()   # ... and the read-through kernel loads what the staged one cached
        assert e.forcing_noise_cached_index == nt - 2
        _same(_series(e), want, "the rest from the cache")


# ---------------------------------------------------------------------------------------------- 5. FAST
@phis
@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
def test_fast_mode_equals_a_plain_handle_under_the_host_formed_series(ra, orc, mix, phi):
    scen, P6 = _scen(2), two_layer_params(N)
    noise = (SIGMA, SEED, 0, phi)
    if mix:
        S, P = _block(2, 3), _mix_params(3)
        Fm = hm.mix_forcing(S, P[6:], scen)
        make = lambda: _mix(ra, P, S, scen, mode=ra.MODE_FAST, noise=noise)
    else:
        F = _rows(2)
        Fm = _member_series(F, scen)
        make = lambda: _plain(ra, P6, F, scen, mode=ra.MODE_FAST, noise=noise)
    Fn = hr.noisy_forcing_red(Fm, SIGMA, phi, SEED)
    with make() as e, _own_series(ra, P6, Fn, mode=ra.MODE_FAST) as p:
        e.run(17)   # the second launch loads the cache
        e.run()
        p.run()
        got = _series(e)
        _same(got, _series(p), "FAST with red noise against FAST plain under the host-formed series")
        assert np.array_equal(e.status(), p.status())
    want = orc.two_layer_run(BOUNDS, P6, Fn, 0.0, 0.0, scen=np.arange(N, dtype=np.int32), source=0)
    with np.errstate(all="ignore"):
        bounded = np.isfinite(want[0][-1]) & (np.nanmax(np.abs(want[0]), axis=0) < 50.0)
    assert bounded.mean() > 0.9
    for g, w in zip(got, want):
        err = np.abs(g[:, bounded] - w[:, bounded]) / np.maximum(1.0, np.abs(w[:, bounded]))
        print(f"FAST against the oracle: max deviation {err.max():.3e}")
        assert (err <= FAST_RTOL).all()


# ---------------------------------------------------------------------------------------------- 6. the launch plan
@phis
@pytest.mark.parametrize("source", [0, 1], ids=["exogenous", "upstream"])
def test_every_launch_plan_equals_one_run(ra, orc, source, phi):
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    noise = (SIGMA, SEED, 3, phi)
    setting = {"sigma": SIGMA, "seed": SEED, "member_offset": 3, "phi": phi}
    want = hr.oracle_run_red(orc, BOUNDS, P, _member_series(F, scen), SIGMA, phi, SEED, member_offset=3, source=source)
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        e.run()
        _same(_series(e), want, "one run")
        e.rewind()   # the cache stands at the last index: the second run starts from e_0 (or its one-draw spin-up) again
        assert e.forcing_noise_cached_index == T - 2 + source
        e.run()
        _same(_series(e), want, "rewind, a second run")
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        while not e.finished():
            e.step()
            assert e.forcing_noise_cached_index == e.time_index - 1 + source
        _same(_series(e), want, "step by step")
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        e.run(17)
        assert e.forcing_noise_cached_index == 16 + source
        e.run()
        _same(_series(e), want, "run(17), run(): from the cache")
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        e.run(17)
        e.set_forcing_noise(*noise)   # any setter of the noise drops the cache
        assert e.forcing_noise_cached_index == -1 and e.forcing_noise == setting
        e.run()
        _same(_series(e), want, "run(17), the noise set again, run(): spun up")
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        e.run(17)
        ck = e.checkpoint()
        assert ck["forcing_noise"] == setting
    # ... into a fresh handle with other parameters and no noise until restore() puts the checkpoint's in place
    with _plain(ra, two_layer_params(N, seed=99), F, scen, source) as e:
        e.restore(ck)
        assert e.time_index == 17 and e.forcing_noise == setting and e.forcing_noise_cached_index == -1
        e.run()
        got = _series(e)
        assert_bit_equal(got[0][17:], want[0][17:], "restored: Ts")
        assert_bit_equal(got[1][17:], want[1][17:], "restored: Td")


def test_cut_run_equals_uncut_run_and_the_oracle(ra, orc):
    """65 536 + 130 members x 201 rows: the run is cut into two member blocks in chunks of steps.  Each block's first chunk starts
    from e_0, every later one loads what the chunk before it stored -- its own members' slots, at the block's offset."""
    from rscm_amd import _lib as L
    n, nt, phi = 65536 + 130, 201, 0.7
    b, F = _annual(nt), _rows(2, nt, scale=0.5)
    P, scen = two_layer_params(n), _scen(2, n)
    lib = L.load()
    got = {}
    try:
        for plan in (1, 0):
            L.check(lib.rscm_gpu_set_run_plan(plan))
            with _plain(ra, P, F, scen, bounds=b, noise=(SIGMA, SEED, 11, phi)) as e:
                e.run()
                blocks, chunks = e.last_run_plan()
                assert (blocks, chunks > 1) == ((2, True) if plan else (1, False))
                assert e.forcing_noise_cached_index == nt - 2
                got[plan] = _series(e)
    finally:
        L.check(lib.rscm_gpu_set_run_plan(-1))
    _same(got[1], got[0], "cut against uncut")
    for edge, off in ((np.r_[0:130], 11), (np.r_[n - 130:n], 11 + n - 130)):
        want = hr.oracle_run_red(orc, b, P[:, edge], _member_series(F, scen[edge]), SIGMA, phi, SEED, member_offset=off)
        _same((got[1][0][:, edge], got[1][1][:, edge]), want, f"members {edge[0]}..{edge[-1]}")


@phis
def test_two_handles_with_offsets_equal_one(ra, phi):
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    with _plain(ra, P, F, scen, noise=(SIGMA, SEED, 0, phi)) as whole:
        whole.run()
        want = _series(whole)
    for lo in (0, 65):
        with _plain(ra, P[:, lo:lo + 65].copy(), F, scen[lo:lo + 65].copy(), noise=(SIGMA, SEED, lo, phi)) as half:
            half.run()
            _same(_series(half), (want[0][:, lo:lo + 65], want[1][:, lo:lo + 65]), f"members {lo}..{lo + 64} as a handle of their own")
    from rscm_amd.distributed import ShardedEnsemble, shard_bounds
    for rank in range(3):
        sh = ShardedEnsemble(N, lambda count, device: ra.Ensemble(ra.KIND_TWO_LAYER, count, BOUNDS, device=device), rank=rank, world=3, device=0)
        sh.set_forcing_noise(SIGMA, SEED, phi=phi)
        off, cnt = shard_bounds(N, rank, 3)
        assert sh.ensemble.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": off, "phi": phi}
        sh.ensemble.close()


# ---------------------------------------------------------------------------------------------- 9. special values
@phis
def test_special_values_propagate_as_in_the_oracle(ra, orc, phi):
    """e does not depend on F: a NaN or Inf in F reaches F' at that index only (the states stay NaN, as in the oracle)."""
    P = two_layer_params(N)
    F = _rows(3)
    F[1, 10] = np.nan
    F[2, 20] = np.inf
    scen = (np.arange(N) % 3).astype(np.int32)
    want = hr.oracle_run_red(orc, BOUNDS, P, _member_series(F, scen), SIGMA, phi, SEED)
    with _plain(ra, P, F, scen, noise=(SIGMA, SEED, 0, phi)) as e:
        e.run()
        _same(_series(e), want, "a NaN and an Inf in F")
        st = e.status()
        assert np.array_equal(st, _status_of(want))
        assert not st[scen == 0].any() and st[scen == 1].all() and st[scen == 2].all()
        assert np.isnan(e.get_series(TS, 12, 13)[0][scen == 1]).all()
        assert_bit_equal(e.forcing_noise_rows(), _want_rows(0, phi), "the term itself stays finite")


def test_large_sigma_leaves_the_guards_box(ra, orc):
    """sigma = 1e4: |F'| beyond 2^12, years outside the state guard's forcing box are replayed with the full division."""
    P, phi = two_layer_params(N), 0.7
    F = _rows(1)
    want = hr.oracle_run_red(orc, BOUNDS, P, _member_series(F, None), 1.0e4, phi, SEED)
    assert np.abs(hr.noisy_forcing_red(_member_series(F, None), 1.0e4, phi, SEED)).max() > 4096.0
    with _plain(ra, P, F, noise=(1.0e4, SEED, 0, phi)) as e:
        e.run()
        _same(_series(e), want, "sigma = 1e4")
        assert np.array_equal(e.status(), _status_of(want))


# ---------------------------------------------------------------------------------------------- 10. phi = 0 and the refusals
def test_phi_zero_is_the_white_setting(ra):
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    F[1, :] = -0.0   # (sigma = 0 below: the formula's 0 * e term would change these zeros' signs)
    for sigma in (SIGMA, 0.0):
        with _plain(ra, P, F, scen, noise=(sigma, SEED, 4)) as white, _plain(ra, P, F, scen, noise=(sigma, SEED, 4, 0.0)) as e:
            white.run()
            e.run()
            _same(_series(e), _series(white), f"phi = 0.0 against the white setter, sigma = {sigma}")
            assert e.forcing_noise == {"sigma": sigma, "seed": SEED, "member_offset": 4} == white.forcing_noise
            assert e.forcing_noise_cached_index == -1
            assert_bit_equal(e.forcing_noise_rows(), white.forcing_noise_rows(), "the term")
            assert "phi" not in e.checkpoint()["forcing_noise"]


def test_refusals(ra):
    from rscm_amd import _lib as L
    from rscm_amd.ensemble import run_lockstep
    lib = L.load()

    def refused(call, text):
        with pytest.raises(L.RscmGpuError, match=text) as err:
            call()
        assert err.value.code == L.ERR_INVALID

    with ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS) as plain, ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS) as red, \
            ra.Ensemble(ra.KIND_COUPLED, 8, BOUNDS) as coupled:
        for phi in (1.0, -1.0, math.nan):
            refused(lambda: plain.set_forcing_noise(0.1, 1, 0, phi), "phi")
        refused(lambda: plain.set_forcing_noise(-0.5, 1, 0, 0.7), "sigma")
        refused(lambda: plain.set_forcing_noise(0.1, 1, -1, 0.7), "member_offset")
        refused(lambda: coupled.set_forcing_noise(0.1, 1, 0, 0.7), "two-layer kind")
        assert plain.forcing_noise is None and plain.forcing_noise_cached_index == -1
        red.set_params(two_layer_params(8))
        red.set_forcing(_rows(1))
        red.set_initial(TS, 0.0)
        red.set_initial(TD, 0.0)
        red.set_forcing_noise(0.1, 1, 0, 0.7)
        refused(lambda: red.link_input(0, plain, TS), "linked input")
        obs = ([TS, TS], [3, 9], [0.1, 0.3], [0.1, 0.1])
        refused(lambda: red.run_loglik(*obs), "fused")
        stream = C.c_void_p()
        L.check(lib.rscm_gpu_stream_create(0, C.byref(stream)))
        try:
            for e in (plain, red):
                e.set_stream(stream.value)
            refused(lambda: run_lockstep((plain, red)), "lock-step")
        finally:
            for e in (plain, red):
                e.set_stream(None)
            L.check(lib.rscm_gpu_stream_destroy(0, stream))
        i0, i1, d0, d1 = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32), np.zeros(1), np.ones(1)
        base = np.ascontiguousarray(two_layer_params(8)[:, 0])
        s = C.c_void_p()
        rc = lib.rscm_sampler_create(red._h, 16, 1, L.iptr(i0), L.dptr(base), L.iptr(i0), L.dptr(d0), L.dptr(d1), None, None,
                                     1, L.iptr(i1), L.iptr(i1), L.dptr(d0), L.dptr(d1), 0, 2.0, 1, C.byref(s))
        assert rc == L.ERR_INVALID and b"forcing noise" in lib.rscm_gpu_last_error() and not s.value
        # ... and the stored likelihood after a run is how it is scored
        red.run()
        ll = red.loglik(*obs)
        assert ll.shape == (8,) and np.isfinite(ll).all()


# ---------------------------------------------------------------------------------------------- 11. branching
@phis
def test_branch_continues_diverges_and_equals_a_restored_plain_handle(ra, phi):
    k = 13
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    ident = np.arange(N, dtype=np.int64)
    with _plain(ra, P, F, scen, noise=(SIGMA, SEED, 0, phi)) as src:
        src.run(k)
        ck = src.checkpoint()
        # the same setting: the copy continues to the source's own bits -- the destination realises its own pure function from 0
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as dst:
            dst.set_forcing(F, scen)
            dst.set_forcing_noise(SIGMA, SEED, 0, phi)
            src.branch(dst, ident)
            assert dst.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": 0, "phi": phi}
            assert dst.forcing_noise_cached_index == -1 and src.forcing_noise_cached_index == k - 1
            dst.run()
            src.run()
            own = _series(src)
            for v, w in zip((TS, TD), own):
                assert_bit_equal(dst.get_series(v, k), w[k:], f"same setting: {v}")
        # another seed and offset: a plain handle restored at k under the host-formed red series
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as dst:
            dst.set_forcing(F, scen)
            dst.set_forcing_noise(SIGMA, SEED + 1, 40, phi)
            src.restore(ck)   # back at k
            src.branch(dst, ident)
            dst.run()
            got = (dst.get_series(TS, k), dst.get_series(TD, k))
            assert (got[0][1:] != own[0][k + 1:]).all()
            plain_ck = {key: val for key, val in ck.items() if key != "forcing_noise"}
            with _own_series(ra, P, hr.noisy_forcing_red(_member_series(F, scen), SIGMA, phi, SEED + 1, 40)) as p:
                p.restore(plain_ck)
                assert p.forcing_noise is None
                p.run()
                assert_bit_equal(got[0], p.get_series(TS, k), "another seed: Ts")
                assert_bit_equal(got[1], p.get_series(TD, k), "another seed: Td")
        # all draws of ONE ancestor diverge from row k + 1 on under the destination's noise
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as dst:
            dst.set_forcing(F[:1])
            dst.set_forcing_noise(SIGMA, SEED, 0, phi)
            src.branch(dst, np.zeros(N, dtype=np.int64))
            dst.run()
            rows = dst.get_series(TS, k)
            assert np.unique(rows[0]).size == 1 and np.unique(rows[1]).size == N and np.unique(rows[-1]).size == N


# ---------------------------------------------------------------------------------------------- 12.-14. clear, the builder, files
def test_clear_and_the_white_setter_after_a_red_setting(ra):
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    with _plain(ra, P, F, scen) as never, _plain(ra, P, F, scen, noise=(SIGMA, SEED)) as white, \
            _plain(ra, P, F, scen, noise=(SIGMA, SEED, 0, 0.7)) as e:
        never.run()
        white.run()
        e.run()
        assert (_series(e)[0][1:] != _series(never)[0][1:]).all() and (_series(e)[0][2:] != _series(white)[0][2:]).all()
        e.clear_forcing_noise()
        assert e.forcing_noise is None and e.forcing_noise_cached_index == -1
        e.rewind()
        e.run()
        _same(_series(e), _series(never), "after clear_forcing_noise")
        assert np.array_equal(e.status(), never.status())
        e.set_forcing_noise(SIGMA, SEED, 0, 0.7)
        e.set_forcing_noise(SIGMA, SEED)   # the three-argument call sets phi = 0
        assert e.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": 0}
        e.rewind()
        e.run()
        _same(_series(e), _series(white), "the white setter after a red setting")
        assert e.forcing_noise_cached_index == -1


def test_model_builder_applies_the_red_noise(ra, orc):
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    t = np.arange(1750.0, 1791.0)
    axis = core.TimeAxis.from_values(t)
    f = 3.0 * (1.0 - np.exp(-(t - 1750.0) / 40.0))
    m = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
         .with_initial_values({TS: 0.0, TD: 0.0}).with_forcing_noise(SIGMA, SEED, phi=0.7)
         .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(f, axis, "W/m^2", core.InterpolationStrategy.Linear))
         .build(n_members=4))
    P6 = np.repeat(np.array([fixed[k] for k in core.TL_PARAM_ORDER])[:, None], 4, axis=1)
    assert m.ensemble.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": 0, "phi": 0.7}
    m.run()
    _same(_series(m.ensemble), hr.oracle_run_red(orc, axis.bounds(), P6, np.repeat(f[None], 4, axis=0), SIGMA, 0.7, SEED), "built model")
    m.close()


def test_checkpoint_file_carries_phi(ra, tmp_path):
    from rscm_amd import core
    setting = {"sigma": SIGMA, "seed": (1 << 64) - 3, "member_offset": BIG_OFFSET, "phi": -0.5}
    with _plain(ra, two_layer_params(N), _rows(1), noise=(SIGMA, (1 << 64) - 3, BIG_OFFSET, -0.5)) as e:
        e.run(5)
        core.save_checkpoint(tmp_path / "ck.npz", e.checkpoint())
        ck = core.load_checkpoint(tmp_path / "ck.npz")
        assert ck["forcing_noise"]["phi"] == -0.5
        e.clear_forcing_noise()
        e.restore(ck)
        assert e.forcing_noise == setting and e.time_index == 5 and e.forcing_noise_cached_index == -1
        # a checkpoint written before there was a phi restores a white handle
        ck["forcing_noise"].pop("phi")
        e.restore(ck)
        assert e.forcing_noise == {key: val for key, val in setting.items() if key != "phi"}
