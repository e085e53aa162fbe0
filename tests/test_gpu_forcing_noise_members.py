"""GPU tier of the per-member forcing noise of a two-layer ensemble (rscm_ens_set_forcing_noise_members;
Ensemble(..., noise_params=True).set_forcing_noise_members): member i is forced at forcing-axis index t by F' = F + e_t with
e_0 = sigma_i z_0 and e_t = (phi_i e_{t-1}) + ((sigma_i sqrt(1 - phi_i^2)) z_t), sigma_i and phi_i the member's own values in
parameter rows 6 + K and 6 + K + 1, every operation rounded on its own, z the white tier's deviate.  e is a pure function of
(seed, sigma_i, phi_i, member id, t) with the rows as they stand at launch: the cache of the red noise is dropped by everything that
writes a parameter row.

The reference of every value test: each member's series formed on the host (tests/host_forcing_noise_members.py, numpy) and given
to the CPU oracle's plain two-layer run as one scenario per member.  EXACT mode is compared bit for bit; RSCM_MODE_FAST bit for bit
with a PLAIN two-layer handle given the same host-formed series and at the existing FAST tolerance (1e-11 relative to
max(1, |oracle|) on bounded members) with the oracle.

The shapes and helpers are the white tier's (tests/test_gpu_forcing_noise.py): N = 130 members (two wavefronts and two lanes) on a
40-step uneven axis unless a test says otherwise.  The rows of ``_noise_rows`` hold negative phi, phi = 0 and sigma = 0."""
import ctypes as C

import numpy as np
import pytest

from tests import host_forcing_mix as hm
from tests import host_forcing_noise_members as hmem
from tests.helpers import assert_bit_equal, two_layer_params
from tests.test_gpu_forcing_noise import (BIG_OFFSET, BOUNDS, FAST_RTOL, N, SEED, T, TD, TS, _annual, _block, _member_series, _mix_params,  # noqa: F401
                                          _own_series, _plain, _rows, _same, _scen, _series, _status_of, orc, ra)

pytestmark = pytest.mark.gpu


def _noise_rows(n=N, seed=21):
    """(sigma [n], phi [n]): amplitudes in [0.05, 0.6) and persistences in (-0.9, 0.9), every 7th member white (phi = 0, one of them
    -0.0), every 11th silent (sigma = 0)."""
    rng = np.random.default_rng(seed)
    sigma, phi = rng.uniform(0.05, 0.6, n), rng.uniform(-0.9, 0.9, n)
    phi[::7] = 0.0
    phi[7] = -0.0
    sigma[3::11] = 0.0
    assert (phi < 0).any() and (phi == 0).any() and (sigma == 0).any()
    return sigma, phi


def _with_rows(P, sigma, phi):
    return np.vstack([P, np.broadcast_to(sigma, P.shape[1:]), np.broadcast_to(phi, P.shape[1:])])


def _flagged(ra, P, F, scen=None, source=None, mode=None, bounds=BOUNDS, noise=None, expose=False):
    """A two-layer handle with the two noise rows: plain with ``P`` [8][n] and rows ``F`` [S][T], mix with ``P`` [6 + K + 2][n] and a
    block ``F`` [S][K][T].  ``noise`` = (seed[, member_offset]); ``expose``: rscm_ens_params_devptr is taken before anything else."""
    K = P.shape[0] - 8
    e = ra.Ensemble(ra.KIND_TWO_LAYER, P.shape[1], bounds, forcing_components=K if K else None, noise_params=True)
    assert e.n_params == 8 + K and e.noise_param_rows == (6 + K, 7 + K)
    if expose:
        e.params_vector(0)
    e.set_mode(ra.MODE_EXACT if mode is None else mode)
    e.set_params(P)
    e.set_forcing(F, scen, ra.SRC_EXOGENOUS if source is None else source)
    e.set_initial(TS, 0.0)
    e.set_initial(TD, 0.0)
    if noise is not None:
        e.set_forcing_noise_members(*noise)
    return e


def _want_rows(sigma, phi, offset=0, n=N, n_times=T):
    return hmem.member_noise(SEED, np.arange(n, dtype=np.uint64) + np.uint64(offset), n_times, sigma, phi).T


@pytest.fixture(scope="module")
def case(orc):
    """The shared case of the launch-plan, cache and shard tests, and its oracle run (computed once, never changed): two scenarios,
    member offset 3."""
    sigma, phi = _noise_rows()
    F, scen, P6 = _rows(2), _scen(2), two_layer_params(N)
    want = hmem.oracle_run_members(orc, BOUNDS, P6, _member_series(F, scen), sigma, phi, SEED, member_offset=3)
    assert np.isfinite(want[0]).all()
    for a in want:
        a.setflags(write=False)
    return dict(sigma=sigma, phi=phi, F=F, scen=scen, P6=P6, P=_with_rows(P6, sigma, phi), want=want, noise=(SEED, 3),
                setting={"per_member": True, "seed": SEED, "member_offset": 3})


# ---------------------------------------------------------------------------------------------- 1. the term itself
@pytest.mark.parametrize("offset", [0, BIG_OFFSET], ids=["offset0", "offset2^33+5"])
def test_noise_rows_equal_the_restatement(ra, offset):
    sigma, phi = _noise_rows()
    with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS, noise_params=True) as e:
        assert e.forcing_noise is None
        e.set_params(_with_rows(two_layer_params(N), sigma, phi))
        e.set_forcing_noise_members(SEED, offset)
        assert e.forcing_noise == {"per_member": True, "seed": SEED, "member_offset": offset}
        assert e.forcing_noise_cached_index == -1
        want = _want_rows(sigma, phi, offset)
        rows = e.forcing_noise_rows()
        assert_bit_equal(rows, want, "all rows")
        assert_bit_equal(e.forcing_noise_rows(5, 9), rows[5:9], "rows 5..8")
        assert_bit_equal(e.forcing_noise_rows(0, 1), rows[:1], "row 0")
        assert e.forcing_noise_rows(5, 5).shape == (0, N)
        white = sigma[None, :] * _want_rows(1.0, 0.0, offset)
        assert np.array_equal(rows[:, phi == 0], white[:, phi == 0]), "phi_i == 0: the white values"
        assert (rows[:, sigma == 0] == 0).all()
        # the rows as they stand: other values, the per-member read path (the block was handed out)
        e.params_vector(6)
        e.set_params(_with_rows(two_layer_params(N), phi * phi + 0.1, -phi))
        assert_bit_equal(e.forcing_noise_rows(), _want_rows(phi * phi + 0.1, -phi, offset), "after set_params with other rows")


# ---------------------------------------------------------------------------------------------- 2. EXACT: the oracle's bits
@pytest.mark.parametrize("source", [0, 1], ids=["exogenous", "upstream"])
@pytest.mark.parametrize("n_scen", [1, 3])
def test_exact_plain_handle_equals_the_oracle(ra, orc, n_scen, source):
    sigma, phi = _noise_rows()
    F, scen, P6 = _rows(n_scen), _scen(n_scen), two_layer_params(N)
    want = hmem.oracle_run_members(orc, BOUNDS, P6, _member_series(F, scen), sigma, phi, SEED, source=source)
    assert np.isfinite(want[0]).all()
    with _flagged(ra, _with_rows(P6, sigma, phi), F, scen, source, noise=(SEED,)) as e:
        e.run()
        assert e.finished() and e.forcing_noise_cached_index == T - 2 + source
        _same(_series(e), want, f"S={n_scen} source={source}")
        assert not e.status().any()


def test_exact_mix_handle_equals_the_oracle(ra, orc):
    K = 3
    sigma, phi = _noise_rows()
    S, scen, P = _block(2, K), _scen(2), _mix_params(K)
    want = hmem.oracle_run_members(orc, BOUNDS, P[:6], hm.mix_forcing(S, P[6:], scen), sigma, phi, SEED, member_offset=BIG_OFFSET)
    with _flagged(ra, _with_rows(P, sigma, phi), S, scen, noise=(SEED, BIG_OFFSET)) as e:
        assert e.noise_param_rows == (9, 10)
        e.run()
        _same(_series(e), want, f"mix K={K}")
        assert not e.status().any()
        assert_bit_equal(e.forcing_noise_rows(), _want_rows(sigma, phi, BIG_OFFSET), "the term of a mix handle: rows 9 and 10")


def test_table_beyond_the_lds_budget_equals_the_oracle(ra, orc):
    """130 scenarios x 200 steps: 130 * 200 * 8 = 208 000 B, more than the 159 KiB a launch may stage, so the rows are read through
    L2; the first 40 steps of the same table run on their own are staged.  Same bits."""
    nt = 201
    assert N * (nt - 1) * 8 > 159 * 1024 > N * 40 * 8
    sigma, phi = _noise_rows()
    b, F, scen, P6 = _annual(nt), _rows(N, nt), np.arange(N, dtype=np.int32)[::-1].copy(), two_layer_params(N)
    want = hmem.oracle_run_members(orc, b, P6, _member_series(F, scen), sigma, phi, SEED)
    with _flagged(ra, _with_rows(P6, sigma, phi), F, scen, bounds=b, noise=(SEED,)) as e:
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


# ---------------------------------------------------------------------------------------------- 3. uniform rows: the handle-wide red bits
@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("expose", [False, True], ids=["uniform-read", "per-member-read"])
def test_uniform_rows_equal_the_handle_wide_red_setting(ra, expose, mode):
    """Once after set_params found the two rows uniform (one element read for the wavefront), once with the block handed out before
    (rscm_ens_params_devptr: no row is ever treated as uniform, every lane reads its own element)."""
    sigma, phi = 0.35, 0.7
    F, scen, P6 = _rows(2), _scen(2), two_layer_params(N)
    with _plain(ra, P6, F, scen, mode=mode, noise=(sigma, SEED, 4, phi)) as red, \
            _flagged(ra, _with_rows(P6, sigma, phi), F, scen, mode=mode, noise=(SEED, 4), expose=expose) as e:
        red.run(17)
        red.run()
        e.run(17)
        e.run()
        _same(_series(e), _series(red), "uniform rows against rscm_ens_set_forcing_noise_ar1")
        assert np.array_equal(e.status(), red.status())
        assert_bit_equal(e.forcing_noise_rows(), red.forcing_noise_rows(), "the term")
        assert e.forcing_noise_cached_index == (-1 if expose else T - 2)


# ---------------------------------------------------------------------------------------------- 4. FAST
@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
def test_fast_mode_equals_a_plain_handle_under_the_host_formed_series(ra, orc, mix):
    sigma, phi = _noise_rows()
    scen, P6 = _scen(2), two_layer_params(N)
    if mix:
        S, P = _block(2, 3), _mix_params(3)
        Fm = hm.mix_forcing(S, P[6:], scen)
        make = lambda: _flagged(ra, _with_rows(P, sigma, phi), S, scen, mode=ra.MODE_FAST, noise=(SEED,))
    else:
        F = _rows(2)
        Fm = _member_series(F, scen)
        make = lambda: _flagged(ra, _with_rows(P6, sigma, phi), F, scen, mode=ra.MODE_FAST, noise=(SEED,))
    Fn = hmem.noisy_forcing_members(Fm, sigma, phi, SEED)
    with make() as e, _own_series(ra, P6, Fn, mode=ra.MODE_FAST) as p:
        e.run(17)   # the second launch loads the cache
        e.run()
        p.run()
        got = _series(e)
        _same(got, _series(p), "FAST with per-member noise against FAST plain under the host-formed series")
        assert np.array_equal(e.status(), p.status())
    want = orc.two_layer_run(BOUNDS, P6, Fn, 0.0, 0.0, scen=np.arange(N, dtype=np.int32), source=0)
    with np.errstate(all="ignore"):
        bounded = np.isfinite(want[0][-1]) & (np.nanmax(np.abs(want[0]), axis=0) < 50.0)
    assert bounded.mean() > 0.9
    for g, w in zip(got, want):
        err = np.abs(g[:, bounded] - w[:, bounded]) / np.maximum(1.0, np.abs(w[:, bounded]))
        print(f"FAST against the oracle: max deviation {err.max():.3e}")
        assert (err <= FAST_RTOL).all()


# ---------------------------------------------------------------------------------------------- 5. the launch plan
def test_every_launch_plan_equals_one_run(ra, case):
    P, F, scen, want, noise = case["P"], case["F"], case["scen"], case["want"], case["noise"]
    with _flagged(ra, P, F, scen, noise=noise) as e:
        e.run()
        _same(_series(e), want, "one run")
        e.rewind()   # the cache stands at the last index: the second run starts from e_0 again
        assert e.forcing_noise_cached_index == T - 2
        e.run()
        _same(_series(e), want, "rewind, a second run")
    with _flagged(ra, P, F, scen, noise=noise) as e:
        while not e.finished():
            e.step()
            assert e.forcing_noise_cached_index == e.time_index - 1
        _same(_series(e), want, "step by step")
    with _flagged(ra, P, F, scen, noise=noise) as e:
        e.run(17)
        assert e.forcing_noise_cached_index == 16
        e.run()
        _same(_series(e), want, "run(17), run(): from the cache")
    with _flagged(ra, P, F, scen, noise=noise) as e:
        e.run(17)
        e.set_forcing_noise_members(*noise)   # any setter of the noise drops the cache
        assert e.forcing_noise_cached_index == -1 and e.forcing_noise == case["setting"]
        e.run()
        _same(_series(e), want, "run(17), the noise set again, run(): spun up")
    with _flagged(ra, P, F, scen, noise=noise) as e:
        e.run(17)
        ck = e.checkpoint()
        assert ck["forcing_noise"] == case["setting"]
    # ... into a fresh flagged handle with other parameters, other rows and no noise until restore() puts the checkpoint's in place
    with _flagged(ra, _with_rows(two_layer_params(N, seed=99), 0.2, 0.3), F, scen) as e:
        e.restore(ck)
        assert e.time_index == 17 and e.forcing_noise == case["setting"] and e.forcing_noise_cached_index == -1
        e.run()
        got = _series(e)
        assert_bit_equal(got[0][17:], want[0][17:], "restored: Ts")
        assert_bit_equal(got[1][17:], want[1][17:], "restored: Td")
    with _plain(ra, case["P6"], F, scen) as e:
        with pytest.raises(ValueError, match="noise_params"):
            e.restore(ck)


# ---------------------------------------------------------------------------------------------- 6.-7. what writes a row drops the cache
def _other_rows(case):
    return _with_rows(two_layer_params(N, seed=5), case["phi"] * case["phi"] + 0.05, -case["sigma"])


@pytest.mark.parametrize("how", ["set_params", "set_params_aos", "sample_lhs", "branch"])
def test_a_written_row_drops_the_cache_and_the_run_continues_under_the_new_rows(ra, case, how):
    """After run(17) the cache stands at index 16.  Each way of writing parameter rows drops it, and the continuation from 17 equals
    a PLAIN handle without noise, restored at 17, under the host-formed series of the NEW rows."""
    P, F, scen, noise = case["P"], case["F"], case["scen"], case["noise"]
    other = _other_rows(case)
    with _flagged(ra, P, F, scen, noise=noise) as e:
        e.run(17)
        assert e.forcing_noise_cached_index == 16
        if how == "set_params":
            e.set_params(other)
        elif how == "set_params_aos":
            e.set_params_aos(np.ascontiguousarray(other.T))
        elif how == "sample_lhs":
            lo = np.r_[P[:6].min(axis=1), 0.05, -0.8]
            hi = np.r_[P[:6].max(axis=1), 0.5, 0.8]
            e.sample_lhs(12, lo, hi)
        else:
            with _flagged(ra, other, F, scen, noise=(SEED + 9, 50)) as src:
                src.run(17)
                src.branch(e, np.arange(N, dtype=np.int64)[::-1].copy())
                assert src.forcing_noise_cached_index == 16   # (the source's own cache is untouched)
        assert e.forcing_noise_cached_index == -1 and e.forcing_noise == case["setting"] and e.time_index == 17
        Pn = e.get_params()
        if how in ("set_params", "set_params_aos"):
            assert_bit_equal(Pn, other, "the rows as set")
        elif how == "branch":
            assert_bit_equal(Pn, other[:, ::-1], "the ancestors' rows")
        else:
            assert (Pn[6] >= 0.05).all() and (Pn[6] <= 0.5).all() and np.unique(Pn[7]).size == N
        ck = e.checkpoint()
        e.run()
        assert e.forcing_noise_cached_index == T - 2
        got = (e.get_series(TS, 17), e.get_series(TD, 17))
        assert_bit_equal(e.forcing_noise_rows(), _want_rows(Pn[6], Pn[7], 3), "the term under the new rows")
    plain_ck = {key: val for key, val in ck.items() if key != "forcing_noise"}
    plain_ck["params"] = Pn[:6].copy()
    with _own_series(ra, Pn[:6].copy(), hmem.noisy_forcing_members(_member_series(F, scen), Pn[6], Pn[7], SEED, 3)) as p:
        p.restore(plain_ck)
        assert p.forcing_noise is None and p.time_index == 17
        p.run()
        assert_bit_equal(got[0], p.get_series(TS, 17), f"{how}: Ts from 17 on")
        assert_bit_equal(got[1], p.get_series(TD, 17), f"{how}: Td from 17 on")
        assert (got[0][1:] != case["want"][0][18:]).all(), "... which is not the continuation under the old rows"


def test_a_handed_out_block_is_never_trusted_across_runs(ra, case):
    """After rscm_ens_params_devptr the caller may write the rows at any time: the index reads -1 after every run, every run spins
    up, and run(17), run() still equals one run."""
    with _flagged(ra, case["P"], case["F"], case["scen"], noise=case["noise"]) as e:
        e.run(5)
        assert e.forcing_noise_cached_index == 4
        v = e.params_vector(e.noise_param_rows[0])
        assert e.forcing_noise_cached_index == -1
        assert_bit_equal(v.to_host(), case["sigma"], "the sigma row as a device vector")
        e.run(17)
        assert e.forcing_noise_cached_index == -1
        e.run()
        assert e.forcing_noise_cached_index == -1
        _same(_series(e), case["want"], "run(5), the block handed out, run(17), run()")
        e.rewind()
        e.step()
        assert e.forcing_noise_cached_index == -1
        e.run()
        _same(_series(e), case["want"], "a step and a run after a rewind")


# ---------------------------------------------------------------------------------------------- 8. the cut run
def test_cut_run_equals_uncut_run_and_the_oracle(ra, orc):
    """65 536 + 130 members x 201 rows: the run is cut into two member blocks in chunks of steps.  Each block reads its members' rows
    and cache slots at the block's offset; its first chunk starts from e_0, every later one loads what the chunk before it stored."""
    from rscm_amd import _lib as L
    n, nt = 65536 + 130, 201
    b, F = _annual(nt), _rows(2, nt, scale=0.5)
    sigma, phi = _noise_rows(n)
    P6, scen = two_layer_params(n), _scen(2, n)
    P = _with_rows(P6, sigma, phi)
    lib = L.load()
    got = {}
    try:
        for plan in (1, 0):
            L.check(lib.rscm_gpu_set_run_plan(plan))
            with _flagged(ra, P, F, scen, bounds=b, noise=(SEED, 11)) as e:
                e.run()
                blocks, chunks = e.last_run_plan()
                assert (blocks, chunks > 1) == ((2, True) if plan else (1, False))
                assert e.forcing_noise_cached_index == nt - 2
                got[plan] = _series(e)
    finally:
        L.check(lib.rscm_gpu_set_run_plan(-1))
    _same(got[1], got[0], "cut against uncut")
    for edge, off in ((np.r_[0:130], 11), (np.r_[n - 130:n], 11 + n - 130)):
        want = hmem.oracle_run_members(orc, b, P6[:, edge], _member_series(F, scen[edge]), sigma[edge], phi[edge], SEED, member_offset=off)
        _same((got[1][0][:, edge], got[1][1][:, edge]), want, f"members {edge[0]}..{edge[-1]}")


# ---------------------------------------------------------------------------------------------- 9. shards
def test_two_handles_with_offsets_and_row_slices_equal_one(ra, case):
    P, F, scen, want = case["P"], case["F"], case["scen"], case["want"]
    for lo in (0, 65):
        with _flagged(ra, P[:, lo:lo + 65].copy(), F, scen[lo:lo + 65].copy(), noise=(SEED, 3 + lo)) as half:
            half.run()
            _same(_series(half), (want[0][:, lo:lo + 65], want[1][:, lo:lo + 65]), f"members {lo}..{lo + 64} as a handle of their own")
    from rscm_amd.distributed import ShardedEnsemble, shard_bounds
    for rank in range(3):
        sh = ShardedEnsemble(N, lambda count, device: ra.Ensemble(ra.KIND_TWO_LAYER, count, BOUNDS, device=device, noise_params=True),
                             rank=rank, world=3, device=0)
        sh.set_forcing_noise_members(SEED)
        off, cnt = shard_bounds(N, rank, 3)
        assert sh.ensemble.forcing_noise == {"per_member": True, "seed": SEED, "member_offset": off}
        sh.set_params_global(P)
        assert_bit_equal(sh.ensemble.forcing_noise_rows(0, 6), _want_rows(case["sigma"], case["phi"])[:6, off:off + cnt], f"rank {rank}: its slice")
        sh.ensemble.close()


# ---------------------------------------------------------------------------------------------- 10.-11. rows nobody validated
def test_special_rows_give_what_the_formula_gives_and_touch_no_other_lane(ra, orc):
    """One member each with a NaN sigma, an Inf sigma, phi = 1, phi = 1.5 and a negative sigma, spread over both full wavefronts and
    the two-lane tail."""
    sigma, phi = _noise_rows()
    F, scen, P6 = _rows(2), _scen(2), two_layer_params(N)
    special = {2: (np.nan, 0.5), 40: (np.inf, 0.5), 64: (0.4, 1.0), 77: (0.4, 1.5), 129: (-0.4, 0.6)}
    s2, p2 = sigma.copy(), phi.copy()
    for i, (s, p) in special.items():
        s2[i], p2[i] = s, p
    want = hmem.oracle_run_members(orc, BOUNDS, P6, _member_series(F, scen), s2, p2, SEED)
    with _flagged(ra, _with_rows(P6, s2, p2), F, scen, noise=(SEED,)) as e, _flagged(ra, _with_rows(P6, sigma, phi), F, scen, noise=(SEED,)) as usual:
        e.run()
        usual.run()
        got = _series(e)
        _same(got, want, "special rows")
        st = e.status()
        assert np.array_equal(st, _status_of(want))
        assert st[[2, 40, 77]].all() and not st[[64, 129]].any() and st.sum() == 3
        assert not np.isfinite(got[0][-1][[2, 40, 77]]).any() and not np.isfinite(got[1][-1][[2, 40, 77]]).any()
        assert_bit_equal(e.forcing_noise_rows(), _want_rows(s2, p2), "the term")
        others = np.setdiff1d(np.arange(N), list(special))
        base = _series(usual)
        assert_bit_equal(got[0][:, others], base[0][:, others], "every other member: Ts of a run without the special rows")
        assert_bit_equal(got[1][:, others], base[1][:, others], "every other member: Td of a run without the special rows")
        assert not usual.status().any()


def test_one_lane_out_of_the_guards_box(ra, orc):
    """sigma_i = 1e4 in one lane among members at 0.1: |F'| beyond 2^12 in that lane alone; it replays its years with the full
    division while its wavefront keeps the state guard."""
    P6, F = two_layer_params(N), _rows(1)
    sigma, phi = np.full(N, 0.1), np.full(N, 0.7)
    sigma[70] = 1.0e4
    Fn = hmem.noisy_forcing_members(_member_series(F, None), sigma, phi, SEED)
    assert np.abs(Fn[70]).max() > 4096.0 and np.abs(np.delete(Fn, 70, axis=0)).max() < 16.0
    want = hmem.oracle_run_members(orc, BOUNDS, P6, _member_series(F, None), sigma, phi, SEED)
    with _flagged(ra, _with_rows(P6, sigma, phi), F, noise=(SEED,)) as e:
        e.run()
        _same(_series(e), want, "one lane at sigma = 1e4")
        assert np.array_equal(e.status(), _status_of(want))


# ---------------------------------------------------------------------------------------------- 12. refusals and inertness
def test_refusals(ra, case):
    from rscm_amd import _lib as L
    from rscm_amd.ensemble import run_lockstep
    lib = L.load()

    def refused(call, text):
        with pytest.raises(L.RscmGpuError, match=text) as err:
            call()
        assert err.value.code == L.ERR_INVALID

    def create(fn, kind, flags, *more):
        h = C.c_void_p()
        rc = fn(kind, 8, T, L.dptr(BOUNDS), 0, flags, *more, C.byref(h))
        if rc == 0:
            L.check(lib.rscm_ens_destroy(h))
        assert (h.value is None) == (rc != 0)
        return rc

    # the flag: two-layer handles that store their whole series, nothing else
    assert create(lib.rscm_ens_create_ex, L.KIND_TWO_LAYER, L.FLAG_NOISE_PARAMS) == 0
    assert create(lib.rscm_ens_create_mix, L.KIND_TWO_LAYER, L.FLAG_NOISE_PARAMS, 2) == 0
    assert create(lib.rscm_ens_create_ex, L.KIND_COUPLED, L.FLAG_NOISE_PARAMS) == L.ERR_INVALID
    assert b"two-layer" in lib.rscm_gpu_last_error()
    assert create(lib.rscm_ens_create_ex, L.KIND_TWO_LAYER, L.FLAG_NOISE_PARAMS | L.FLAG_NO_SERIES) == L.ERR_INVALID
    assert create(lib.rscm_ens_create_mix, L.KIND_TWO_LAYER, L.FLAG_NOISE_PARAMS | L.FLAG_NO_SERIES, 2) == L.ERR_INVALID
    assert create(lib.rscm_ens_create_windowed, L.KIND_TWO_LAYER, L.FLAG_NOISE_PARAMS | L.FLAG_WINDOWED, 8, 0, -1, None) == L.ERR_INVALID
    assert create(lib.rscm_ens_create_windowed, L.KIND_TWO_LAYER, L.FLAG_NOISE_PARAMS | L.FLAG_WINDOWED, T + 5, 0, -1, None) == L.ERR_INVALID
    assert create(lib.rscm_ens_create_ex, L.KIND_TWO_LAYER, 8) == L.ERR_INVALID
    for kw in (dict(kind=ra.KIND_COUPLED), dict(kind=ra.KIND_TWO_LAYER, store_series=False), dict(kind=ra.KIND_TWO_LAYER, window_rows=8)):
        with pytest.raises(ValueError, match="noise_params"):
            ra.Ensemble(kw.pop("kind"), 8, BOUNDS, noise_params=True, **kw)

    P8 = _with_rows(two_layer_params(8), 0.3, 0.5)
    with ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS) as plain, ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS, noise_params=True) as e:
        refused(lambda: plain.set_forcing_noise_members(1), "RSCM_FLAG_NOISE_PARAMS")
        with pytest.raises(ValueError, match="noise_params"):
            plain.noise_param_rows
        assert plain.forcing_noise is None
        refused(lambda: e.set_forcing_noise_members(1, -1), "member_offset")
        assert e.forcing_noise is None and e.forcing_noise_cached_index == -1
        for x in (plain, e):
            x.set_params(P8[:x.n_params])
            x.set_forcing(_rows(1))
            x.set_initial(TS, 0.0)
            x.set_initial(TD, 0.0)
        ident = np.arange(8, dtype=np.int64)
        refused(lambda: plain.branch(e, ident), "RSCM_FLAG_NOISE_PARAMS")
        refused(lambda: e.branch(plain, ident), "RSCM_FLAG_NOISE_PARAMS")
        e.set_forcing_noise_members(1)
        refused(lambda: e.link_input(0, plain, TS), "linked input")
        obs = ([TS, TS], [3, 9], [0.1, 0.3], [0.1, 0.1])
        refused(lambda: e.run_loglik(*obs), "fused")
        stream = C.c_void_p()
        L.check(lib.rscm_gpu_stream_create(0, C.byref(stream)))
        try:
            for x in (plain, e):
                x.set_stream(stream.value)
            refused(lambda: run_lockstep((plain, e)), "lock-step")
        finally:
            for x in (plain, e):
                x.set_stream(None)
            L.check(lib.rscm_gpu_stream_destroy(0, stream))
        i0, i1, d0, d1 = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32), np.zeros(1), np.ones(1)
        base = np.ascontiguousarray(P8[:, 0])
        s = C.c_void_p()
        rc = lib.rscm_sampler_create(e._h, 16, 1, L.iptr(i0), L.dptr(base), L.iptr(i0), L.dptr(d0), L.dptr(d1), None, None,
                                     1, L.iptr(i1), L.iptr(i1), L.dptr(d0), L.dptr(d1), 0, 2.0, 1, C.byref(s))
        assert rc == L.ERR_INVALID and b"forcing noise" in lib.rscm_gpu_last_error() and not s.value
        # the handle-wide setters replace the per-member noise, it replaces them, and clear turns it off
        e.set_forcing_noise(0.2, 5, 0, 0.6)
        assert e.forcing_noise == {"sigma": 0.2, "seed": 5, "member_offset": 0, "phi": 0.6}
        e.set_forcing_noise_members(6, 2)
        assert e.forcing_noise == {"per_member": True, "seed": 6, "member_offset": 2}
        e.clear_forcing_noise()
        assert e.forcing_noise is None
        # ... and with the noise off the flagged handle is accepted by the fused likelihood, to the unflagged handle's bits
        assert_bit_equal(e.run_loglik(*obs), plain.run_loglik(*obs), "run_loglik of a flagged handle with the noise off")


@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fast"])
def test_a_flagged_handle_without_its_noise_is_an_unflagged_handle(ra, case, mode):
    """Noise off, and under the two handle-wide setters: the same bits as a handle without the rows, which stay inert."""
    P, P6, F, scen = case["P"], case["P6"], case["F"], case["scen"]
    with _flagged(ra, P, F, scen, mode=mode) as e, _plain(ra, P6, F, scen, mode=mode) as p:
        for setting in (None, (0.35, SEED, 4), (0.35, SEED, 4, 0.7)):
            for x in (e, p):
                x.rewind()
                if setting:
                    x.set_forcing_noise(*setting)
                x.run(17)
                x.run()
            _same(_series(e), _series(p), f"setting {setting}")
            assert np.array_equal(e.status(), p.status())
            assert e.forcing_noise == p.forcing_noise and e.forcing_noise_cached_index == p.forcing_noise_cached_index
            if setting:
                assert_bit_equal(e.forcing_noise_rows(), p.forcing_noise_rows(), "the term")
                e.set_params(_with_rows(P6, case["phi"], case["sigma"]))   # other inert rows ...
                e.set_params(P)
                assert e.forcing_noise_cached_index == p.forcing_noise_cached_index   # ... drop nothing of a handle-wide setting


# ---------------------------------------------------------------------------------------------- 13. the posterior
def test_posterior_draws_inherit_amplitude_and_persistence_and_realise_their_own_noise(ra, case):
    from tests.test_gpu_weighted_quantiles import _np_weighted
    k, P, F, scen = 17, case["P"], case["F"], case["scen"]
    q = np.array([0.05, 0.25, 0.5, 0.75, 0.95])
    with _flagged(ra, P, F, scen, noise=case["noise"]) as src:
        src.run(k)
        ll = src.loglik([TS, TS, TD], [5, 11, 16], [0.4, 0.9, 0.3], [0.15, 0.15, 0.1])
        assert np.isfinite(ll).all()
        src.set_weights_from_loglik(ll)
        anc = src.resample(N, seed=4).to_host()
        assert np.unique(anc).size < N

        def factory(n):
            dst = ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS, noise_params=True)
            dst.set_forcing(F[:1])
            dst.set_forcing_noise_members(SEED + 1)
            return dst

        dst, _ = src.posterior(factory, N, seed=4)
        with dst:
            got = dst.get_params()
            assert_bit_equal(got, P[:, anc], "the draws' rows are their ancestors', amplitude and persistence included")
            assert dst.forcing_noise == {"per_member": True, "seed": SEED + 1, "member_offset": 0} and dst.forcing_noise_cached_index == -1
            dst.run()
            rows = dst.get_series(TS, k)
            twin = np.flatnonzero((anc[1:] == anc[:-1]) & (P[6, anc[1:]] != 0.0))[0]   # two draws of one ancestor that is not silent
            assert rows[0, twin] == rows[0, twin + 1] and (rows[1:, twin] != rows[1:, twin + 1]).all()
            assert_bit_equal(dst.forcing_noise_rows(), hmem.member_noise(SEED + 1, np.arange(N), T, P[6, anc], P[7, anc]).T,
                             "the term: the ancestors' rows, the draws' own ids and seed")
        # the weighted posterior of the amplitude itself
        sigma_row, phi_row = src.noise_param_rows
        w = src.member_weights()
        res = src.quantile_vectors([src.params_vector(sigma_row), src.params_vector(phi_row)], q, weighted=True)
        want, W = _np_weighted(P[[sigma_row, phi_row]], w, q)
        assert np.array_equal(res["quantiles"], want) and np.array_equal(res["weight"], W)


# ---------------------------------------------------------------------------------------------- 14. the builder, files
def test_model_builder_makes_the_rows_parameters(ra, orc, tmp_path):
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    t = np.arange(1750.0, 1791.0)
    axis = core.TimeAxis.from_values(t)
    f = 3.0 * (1.0 - np.exp(-(t - 1750.0) / 40.0))
    seed = (1 << 64) - 3
    m = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
         .with_initial_values({TS: 0.0, TD: 0.0}).with_forcing_noise_parameters(seed, sigma=0.2, phi=0.5)
         .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(f, axis, "W/m^2", core.InterpolationStrategy.Linear))
         .build(n_members=4))
    assert m.param_order == tuple(core.TL_PARAM_ORDER) + ("forcing_noise|sigma", "forcing_noise|phi")
    assert_bit_equal(m.base_params, np.array([fixed[k] for k in core.TL_PARAM_ORDER] + [0.2, 0.5]), "base values")
    ens = m.ensemble
    assert ens.forcing_noise == {"per_member": True, "seed": seed, "member_offset": 0}
    assert ens.noise_param_rows == (m.param_order.index("forcing_noise|sigma"), m.param_order.index("forcing_noise|phi"))
    P = ens.get_params()
    assert_bit_equal(P, np.repeat(m.base_params[:, None], 4, axis=1), "the base values in every member")
    P[m.param_order.index("forcing_noise|sigma")] = [0.1, 0.2, 0.3, 0.0]
    P[m.param_order.index("forcing_noise|phi")] = [0.9, 0.0, -0.4, 0.7]
    P[m.param_order.index("lambda0")] = [0.9, 1.0, 1.2, 1.3]
    ens.set_params(P)
    m.run()
    want = hmem.oracle_run_members(orc, axis.bounds(), P[:6], np.repeat(f[None], 4, axis=0), P[6], P[7], seed)
    _same(_series(ens), want, "built model, rows set by name")
    # the checkpoint file round-trips the setting; the values travel in the parameter block
    m.ensemble.rewind()
    m.ensemble.run(5)
    core.save_checkpoint(tmp_path / "ck.npz", m.checkpoint())
    ck = core.load_checkpoint(tmp_path / "ck.npz")
    assert ck["forcing_noise"] == {"per_member": True, "seed": seed, "member_offset": 0}
    ens.clear_forcing_noise()
    ens.set_params(np.repeat(m.base_params[:, None], 4, axis=1))
    m.restore(ck)
    assert ens.forcing_noise == {"per_member": True, "seed": seed, "member_offset": 0} and ens.time_index == 5
    assert ens.forcing_noise_cached_index == -1
    assert_bit_equal(ens.get_params(), P, "the restored rows")
    m.run()
    _same(_series(ens), want, "restored from the file at 5 and run on")
    m.close()
