"""GPU tier of the seeded forcing noise of a two-layer ensemble (rscm_ens_set_forcing_noise; Ensemble.set_forcing_noise): member i
is forced at forcing-axis index t by F' = F + sigma * z(seed, member_offset + i, t), product and sum rounded on their own, z a
stateless standard normal deviate.

The reference of every value test: each member's noisy series formed on the host (tests/host_forcing_noise.py, numpy, which does
not fuse) and given to the CPU oracle's plain two-layer run as one scenario per member.  EXACT mode is compared bit for bit;
RSCM_MODE_FAST bit for bit with a PLAIN two-layer handle given the same host-formed series (the forming of F' does not depend on
the mode, the rest is the existing kernel) and at the existing FAST tolerance (1e-11 relative to max(1, |oracle|) on bounded
members, tests/test_gpu_parity.py) with the oracle.

N = 130 members (two wavefronts and two lanes) on a 40-step uneven axis unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from tests import host_forcing_mix as hm
from tests import host_forcing_noise as hn
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import assert_bit_equal, two_layer_params

pytestmark = pytest.mark.gpu

N = 130
T = 41
BOUNDS = np.concatenate([[1750.0], 1750.0 + np.cumsum(np.where(np.arange(T) % 7 == 3, 0.5, 1.0))])   # uneven steps
FAST_RTOL = 1e-11
TS, TD = "Surface Temperature", "Deep Ocean Temperature"
SIGMA, SEED = 0.35, 7
BIG_OFFSET = (1 << 33) + 5


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


def _annual(n_times):
    return np.arange(n_times + 1, dtype=np.float64) + 1750.0


def _rows(n_scen, n_times=T, scale=1.0):
    """[n_scen][n_times] forcing: saturating ramps with a ripple, scenario s scaled by 1 + 0.3 s (bounded by the scale alone)."""
    t = np.arange(n_times, dtype=np.float64)
    return np.stack([scale * (1.0 + 0.3 * (s % 4)) * (2.0 * (1.0 - np.exp(-t / (15.0 + s % 7))) + 0.2 * np.sin(2.0 * np.pi * t / (7.0 + s % 5)))
                     for s in range(n_scen)])


def _block(n_scen, K, n_times=T):
    t = np.arange(n_times, dtype=np.float64)
    S = np.empty((n_scen, K, n_times))
    for s in range(n_scen):
        for k in range(K):
            S[s, k] = (1.0 + 0.3 * s) * ((-1.0) ** k * (1.5 + 0.25 * k) * (1.0 - np.exp(-t / (15.0 + 4.0 * k))) + 0.2 * np.sin(2.0 * np.pi * t / (7.0 + k)))
    return S


def _scen(n_scen, n=N, seed=5):
    return None if n_scen == 1 else np.random.default_rng(seed).integers(0, n_scen, n).astype(np.int32)


def _member_series(F, scen, n=N):
    """The members' noise-free series [n][T] of a plain handle with rows ``F`` [S][T]."""
    return F[np.zeros(n, dtype=np.int64) if scen is None else scen]


def _plain(ra, P6, F, scen=None, source=None, mode=None, bounds=BOUNDS, noise=None):
    """A plain two-layer handle with rows ``F`` [S][T]; ``noise`` = (sigma, seed[, member_offset])."""
    e = ra.Ensemble(ra.KIND_TWO_LAYER, P6.shape[1], bounds)
    e.set_mode(ra.MODE_EXACT if mode is None else mode)
    e.set_params(P6)
    e.set_forcing(F, scen, ra.SRC_EXOGENOUS if source is None else source)
    e.set_initial(TS, 0.0)
    e.set_initial(TD, 0.0)
    if noise is not None:
        e.set_forcing_noise(*noise)
    return e


def _own_series(ra, P6, Fm, source=None, mode=None, bounds=BOUNDS):
    """A plain handle WITHOUT noise under the members' own series ``Fm`` [n][T], one scenario per member."""
    return _plain(ra, P6, Fm, np.arange(P6.shape[1], dtype=np.int32), source, mode, bounds)


def _mix(ra, P, S, scen=None, source=None, mode=None, noise=None):
    e = ra.Ensemble(ra.KIND_TWO_LAYER, P.shape[1], BOUNDS, forcing_components=P.shape[0] - 6)
    e.set_mode(ra.MODE_EXACT if mode is None else mode)
    e.set_params(P)
    e.set_forcing(S, scen, ra.SRC_EXOGENOUS if source is None else source)
    e.set_initial(TS, 0.0)
    e.set_initial(TD, 0.0)
    if noise is not None:
        e.set_forcing_noise(*noise)
    return e


def _mix_params(K, n=N, seed=11):
    return np.vstack([two_layer_params(n), np.random.default_rng(seed).uniform(0.4, 1.6, (K, n))])


def _series(e):
    return e.get_series(TS), e.get_series(TD)


def _same(got, want, what):
    assert_bit_equal(got[0], want[0], f"{what}: Ts")
    assert_bit_equal(got[1], want[1], f"{what}: Td")


def _status_of(want):
    return (~(np.isfinite(want[0][-1]) & np.isfinite(want[1][-1]))).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- 1. the generator
def test_device_deviate_equals_the_restatement_bit_for_bit(ra):
    from rscm_amd import _lib as L
    lib = L.load()
    k = np.concatenate([hn.chosen_k(), np.random.default_rng(3).integers(0, 1 << 52, 4096, dtype=np.uint64)])
    z = np.empty(k.size)
    L.check(lib.rscm_gpu_selftest_normal(k.ctypes.data_as(C.POINTER(C.c_uint64)), k.size, L.dptr(z)))
    assert_bit_equal(z, hn.normal_from_k(k), "device deviate against the numpy restatement")
    assert np.isfinite(z).all() and np.abs(z).max() < 8.21


@pytest.mark.parametrize("offset", [0, BIG_OFFSET], ids=["offset0", "offset2^33+5"])
def test_noise_rows_equal_the_restatement(ra, offset):
    with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as e:
        assert e.forcing_noise is None
        e.set_forcing_noise(SIGMA, SEED, offset)
        assert e.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": offset}
        want = (np.float64(SIGMA) * hn.noise(SEED, np.arange(N, dtype=np.uint64)[:, None] + np.uint64(offset), np.arange(T, dtype=np.uint64)[None, :])).T
        assert_bit_equal(e.forcing_noise_rows(), want, "all rows")
        assert_bit_equal(e.forcing_noise_rows(3, 10), want[3:10], "rows 3..9 (an odd first index)")
        assert e.forcing_noise_rows(5, 5).shape == (0, N)
        e.set_forcing_noise(SIGMA, (1 << 64) - 1, offset)   # the key's high word
        want = (np.float64(SIGMA) * hn.noise((1 << 64) - 1, np.arange(N, dtype=np.uint64)[:, None] + np.uint64(offset), np.arange(2, dtype=np.uint64)[None, :])).T
        assert_bit_equal(e.forcing_noise_rows(0, 2), want, "seed 2^64 - 1")


# ---------------------------------------------------------------------------------------------- 2. EXACT: the oracle's bits
@pytest.mark.parametrize("source", [0, 1], ids=["exogenous", "upstream"])
@pytest.mark.parametrize("n_scen", [1, 2])
def test_exact_plain_handle_equals_the_oracle(ra, orc, n_scen, source):
    F, scen, P = _rows(n_scen), _scen(n_scen), two_layer_params(N)
    want = hn.oracle_run(orc, BOUNDS, P, _member_series(F, scen), SIGMA, SEED, source=source)
    assert np.isfinite(want[0]).all()
    with _plain(ra, P, F, scen, source, noise=(SIGMA, SEED)) as e:
        e.run()
        assert e.finished()
        _same(_series(e), want, f"S={n_scen} source={source}")
        assert not e.status().any()


@pytest.mark.parametrize("source", [0, 1], ids=["exogenous", "upstream"])
@pytest.mark.parametrize("n_scen", [1, 2])
def test_exact_mix_handle_equals_the_oracle(ra, orc, n_scen, source):
    K = 3
    S, scen, P = _block(n_scen, K), _scen(n_scen), _mix_params(K)
    want = hn.oracle_run(orc, BOUNDS, P[:6], hm.mix_forcing(S, P[6:], scen), SIGMA, SEED, member_offset=BIG_OFFSET, source=source)
    with _mix(ra, P, S, scen, source, noise=(SIGMA, SEED, BIG_OFFSET)) as e:
        e.run()
        _same(_series(e), want, f"mix K={K} S={n_scen} source={source}")
        assert not e.status().any()


def test_table_beyond_the_lds_budget_equals_the_oracle(ra, orc):
    """130 scenarios x 200 steps: 130 * 200 * 8 = 208 000 B, more than the 159 KiB a launch may stage, so the rows are read through
    L2; the first 40 steps of the same table run on their own are staged.  Same bits."""
    nt = 201
    assert N * (nt - 1) * 8 > 159 * 1024 > N * 40 * 8
    b, F, scen, P = _annual(nt), _rows(N, nt), np.arange(N, dtype=np.int32)[::-1].copy(), two_layer_params(N)
    want = hn.oracle_run(orc, b, P, _member_series(F, scen), SIGMA, SEED)
    with _plain(ra, P, F, scen, bounds=b, noise=(SIGMA, SEED)) as e:
        e.run()
        full = _series(e)
        _same(full, want, "130 scenarios, 200 steps")
        e.rewind()
        e.run(40)
        head = _series(e)
        assert_bit_equal(head[0][:41], full[0][:41], "first 40 steps, staged against read through L2: Ts")
        assert_bit_equal(head[1][:41], full[1][:41], "first 40 steps, staged against read through L2: Td")


# ---------------------------------------------------------------------------------------------- 3. FAST
@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])
def test_fast_mode_equals_a_plain_handle_under_the_host_formed_series(ra, orc, mix):
    scen, P6 = _scen(2), two_layer_params(N)
    if mix:
        S, P = _block(2, 3), _mix_params(3)
        Fm = hm.mix_forcing(S, P[6:], scen)
        make = lambda: _mix(ra, P, S, scen, mode=ra.MODE_FAST, noise=(SIGMA, SEED))
    else:
        F = _rows(2)
        Fm = _member_series(F, scen)
        make = lambda: _plain(ra, P6, F, scen, mode=ra.MODE_FAST, noise=(SIGMA, SEED))
    Fn = hn.noisy_forcing(Fm, SIGMA, SEED)
    with make() as e, _own_series(ra, P6, Fn, mode=ra.MODE_FAST) as p:
        e.run()
        p.run()
        got = _series(e)
        _same(got, _series(p), "FAST with noise against FAST plain under the host-formed series")
        assert np.array_equal(e.status(), p.status())
    want = orc.two_layer_run(BOUNDS, P6, Fn, 0.0, 0.0, scen=np.arange(N, dtype=np.int32), source=0)
    with np.errstate(all="ignore"):
        bounded = np.isfinite(want[0][-1]) & (np.nanmax(np.abs(want[0]), axis=0) < 50.0)
    assert bounded.mean() > 0.9
    for g, w in zip(got, want):
        err = np.abs(g[:, bounded] - w[:, bounded]) / np.maximum(1.0, np.abs(w[:, bounded]))
        print(f"FAST against the oracle: max deviation {err.max():.3e}")
        assert (err <= FAST_RTOL).all()


# ---------------------------------------------------------------------------------------------- 4. the launch plan
@pytest.mark.parametrize("source", [0, 1], ids=["exogenous", "upstream"])
def test_stepwise_and_resumed_runs_equal_one_run(ra, orc, source):
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    noise = (SIGMA, SEED, 3)
    want = hn.oracle_run(orc, BOUNDS, P, _member_series(F, scen), *noise, source=source)
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        e.run()
        _same(_series(e), want, "one run")
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        while not e.finished():
            e.step()
        _same(_series(e), want, "step by step")
    with _plain(ra, P, F, scen, source, noise=noise) as e:
        e.run(17)
        ck = e.checkpoint()
        assert ck["forcing_noise"] == {"sigma": SIGMA, "seed": SEED, "member_offset": 3}
    # ... into a fresh handle with other parameters and no noise until restore() puts the checkpoint's in place
    with _plain(ra, two_layer_params(N, seed=99), F, scen, source) as e:
        e.restore(ck)
        assert e.time_index == 17 and e.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": 3}
        e.run()
        got = _series(e)
        assert_bit_equal(got[0][17:], want[0][17:], "resumed: Ts")
        assert_bit_equal(got[1][17:], want[1][17:], "resumed: Td")
        # a checkpoint without noise takes it off again
        ck.pop("forcing_noise")
        e.restore(ck)
        assert e.forcing_noise is None


def test_checkpoint_file_carries_the_noise(ra, tmp_path):
    from rscm_amd import core
    with _plain(ra, two_layer_params(N), _rows(1), noise=(SIGMA, (1 << 64) - 3, BIG_OFFSET)) as e:
        e.run(5)
        core.save_checkpoint(tmp_path / "ck.npz", e.checkpoint())
        ck = core.load_checkpoint(tmp_path / "ck.npz")
        e.clear_forcing_noise()
        e.restore(ck)
        assert e.forcing_noise == {"sigma": SIGMA, "seed": (1 << 64) - 3, "member_offset": BIG_OFFSET} and e.time_index == 5


def test_cut_run_equals_uncut_run_and_the_oracle(ra, orc):
    """65 536 + 130 members x 201 rows: the run is cut into two member blocks, whose kernels count members from the block's first.
    A noise that depended on that count would differ between the plans in the second block."""
    from rscm_amd import _lib as L
    n, nt = 65536 + 130, 201
    b, F = _annual(nt), _rows(2, nt, scale=0.5)
    P, scen = two_layer_params(n), _scen(2, n)
    lib = L.load()
    got = {}
    try:
        for plan in (1, 0):
            L.check(lib.rscm_gpu_set_run_plan(plan))
            with _plain(ra, P, F, scen, bounds=b, noise=(SIGMA, SEED, 11)) as e:
                e.run()
                blocks, chunks = e.last_run_plan()
                assert (blocks, chunks > 1) == ((2, True) if plan else (1, False))
                got[plan] = _series(e)
    finally:
        L.check(lib.rscm_gpu_set_run_plan(-1))
    _same(got[1], got[0], "cut against uncut")
    for edge, off in ((np.r_[0:130], 11), (np.r_[n - 130:n], 11 + n - 130)):
        want = hn.oracle_run(orc, b, P[:, edge], _member_series(F, scen[edge]), SIGMA, SEED, member_offset=off)
        _same((got[1][0][:, edge], got[1][1][:, edge]), want, f"members {edge[0]}..{edge[-1]}")


def test_two_handles_with_offsets_equal_one(ra):
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    with _plain(ra, P, F, scen, noise=(SIGMA, SEED)) as whole:
        whole.run()
        want = _series(whole)
    for lo in (0, 65):
        with _plain(ra, P[:, lo:lo + 65].copy(), F, scen[lo:lo + 65].copy(), noise=(SIGMA, SEED, lo)) as half:
            half.run()
            _same(_series(half), (want[0][:, lo:lo + 65], want[1][:, lo:lo + 65]), f"members {lo}..{lo + 64} as a handle of their own")
    from rscm_amd.distributed import ShardedEnsemble, shard_bounds
    for rank in range(3):
        sh = ShardedEnsemble(N, lambda count, device: ra.Ensemble(ra.KIND_TWO_LAYER, count, BOUNDS, device=device), rank=rank, world=3, device=0)
        sh.set_forcing_noise(SIGMA, SEED)
        off, cnt = shard_bounds(N, rank, 3)
        assert sh.ensemble.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": off}
        sh.ensemble.close()


# ---------------------------------------------------------------------------------------------- 5. special values
def test_special_values_propagate_as_in_the_oracle(ra, orc):
    P = two_layer_params(N)
    F = _rows(3)
    F[1, 10] = np.nan
    F[2, 20] = np.inf
    scen = (np.arange(N) % 3).astype(np.int32)
    want = hn.oracle_run(orc, BOUNDS, P, _member_series(F, scen), SIGMA, SEED)
    with _plain(ra, P, F, scen, noise=(SIGMA, SEED)) as e:
        e.run()
        _same(_series(e), want, "a NaN and an Inf in F")
        st = e.status()
        assert np.array_equal(st, _status_of(want))
        assert not st[scen == 0].any() and st[scen == 1].all() and st[scen == 2].all()
        assert np.isnan(e.get_series(TS, 12, 13)[0][scen == 1]).all()


def test_sigma_zero_does_the_arithmetic(ra, orc):
    """sigma = 0 with noise on is still F + 0 * z (off is clear_forcing_noise): a forcing of -0.0 becomes +0.0 where z > 0."""
    P = two_layer_params(N)
    F = _rows(2)
    F[1, :] = -0.0
    F[0, 5] = -0.0
    scen = _scen(2)
    Fn = hn.noisy_forcing(_member_series(F, scen), 0.0, SEED)
    was = np.signbit(_member_series(F, scen))
    assert was.any() and (np.signbit(Fn) != was).any() and np.signbit(Fn[was]).any()   # both signs of zero are in play
    want = hn.oracle_run(orc, BOUNDS, P, _member_series(F, scen), 0.0, SEED)
    with _plain(ra, P, F, scen, noise=(0.0, SEED)) as e:
        e.run()
        assert e.forcing_noise == {"sigma": 0.0, "seed": SEED, "member_offset": 0}
        _same(_series(e), want, "sigma = 0")
        assert_bit_equal(e.forcing_noise_rows(), (np.float64(0.0) * hn.noise(SEED, np.arange(N)[:, None], np.arange(T)[None, :])).T, "0 * z")


def test_large_sigma_leaves_the_guards_box(ra, orc):
    """sigma = 1e4: |F'| up to 8e4 >= 2^12, years outside the state guard's forcing box are replayed with the full division."""
    P = two_layer_params(N)
    F = _rows(1)
    want = hn.oracle_run(orc, BOUNDS, P, _member_series(F, None), 1.0e4, SEED)
    assert np.abs(hn.noisy_forcing(_member_series(F, None), 1.0e4, SEED)).max() > 4096.0
    with _plain(ra, P, F, noise=(1.0e4, SEED)) as e:
        e.run()
        _same(_series(e), want, "sigma = 1e4")
        assert np.array_equal(e.status(), _status_of(want))


# ---------------------------------------------------------------------------------------------- 6. branching
def test_branch_continues_diverges_and_equals_a_restored_plain_handle(ra):
    k = 13
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    ident = np.arange(N, dtype=np.int64)
    with _plain(ra, P, F, scen, noise=(SIGMA, SEED)) as src:
        src.run(k)
        ck = src.checkpoint()
        # the same seed and offset: the copy continues to the source's own bits
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as dst:
            dst.set_forcing(F, scen)
            dst.set_forcing_noise(SIGMA, SEED)
            src.branch(dst, ident)
            assert dst.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": 0}
            dst.run()
            src.run()
            own = _series(src)
            for v, w in zip((TS, TD), own):
                assert_bit_equal(dst.get_series(v, k), w[k:], f"same seed: {v}")
        # another seed: the destination's own noise (a branch leaves it alone) -- a plain handle restored at k under the host-formed series
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as dst:
            dst.set_forcing(F, scen)
            dst.set_forcing_noise(SIGMA, SEED + 1, 40)
            src.restore(ck)   # back at k
            src.branch(dst, ident)
            assert dst.forcing_noise == {"sigma": SIGMA, "seed": SEED + 1, "member_offset": 40}
            dst.run()
            got = (dst.get_series(TS, k), dst.get_series(TD, k))
            assert (got[0][1:] != own[0][k + 1:]).all()
            plain_ck = {key: val for key, val in ck.items() if key != "forcing_noise"}
            with _own_series(ra, P, hn.noisy_forcing(_member_series(F, scen), SIGMA, SEED + 1, 40)) as p:
                p.restore(plain_ck)
                assert p.forcing_noise is None
                p.run()
                assert_bit_equal(got[0], p.get_series(TS, k), "another seed: Ts")
                assert_bit_equal(got[1], p.get_series(TD, k), "another seed: Td")
        # two (here: all) draws of ONE ancestor diverge under the destination's noise and stay identical without it
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as dst:
            dst.set_forcing(F[:1])
            src.branch(dst, np.zeros(N, dtype=np.int64))
            dst.run()
            last = dst.get_series(TS, T - 1)[0]
            assert np.unique(last).size == 1
        with ra.Ensemble(ra.KIND_TWO_LAYER, N, BOUNDS) as dst:
            dst.set_forcing(F[:1])
            dst.set_forcing_noise(SIGMA, SEED)
            src.branch(dst, np.zeros(N, dtype=np.int64))
            dst.run()
            rows = dst.get_series(TS, k)
            assert np.unique(rows[0]).size == 1 and np.unique(rows[1]).size == N and np.unique(rows[-1]).size == N


# ---------------------------------------------------------------------------------------------- 7. shapes and refusals
def test_shapes_and_refusals(ra):
    from rscm_amd import _lib as L
    from rscm_amd.ensemble import run_lockstep
    lib = L.load()

    def refused(call, text):
        with pytest.raises(L.RscmGpuError, match=text) as err:
            call()
        assert err.value.code == L.ERR_INVALID

    with ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS) as plain, ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS) as noisy, \
            ra.Ensemble(ra.KIND_COUPLED, 8, BOUNDS) as coupled, ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS, window_rows=8) as windowed, \
            ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS, store_series=False) as lean, ra.Ensemble(ra.KIND_TWO_LAYER, 8, BOUNDS) as consumer:
        for sigma in (-0.5, np.nan, np.inf):
            refused(lambda: plain.set_forcing_noise(sigma, 1), "sigma")
        refused(lambda: plain.set_forcing_noise(0.1, 1, -1), "member_offset")
        assert plain.forcing_noise is None
        refused(lambda: coupled.set_forcing_noise(0.1, 1), "two-layer kind")
        refused(lambda: windowed.set_forcing_noise(0.1, 1), "whole series")
        refused(lambda: lean.set_forcing_noise(0.1, 1), "whole series")
        consumer.link_input(0, plain, TS)
        refused(lambda: consumer.set_forcing_noise(0.1, 1), "linked input")
        consumer.unlink_input(0)
        with pytest.raises(ValueError):
            plain.set_forcing_noise(0.1, -1)
        assert refusal_code(plain.forcing_noise_rows) == L.ERR_STATE
        # a handle with noise runs on its own
        noisy.set_params(two_layer_params(8))
        noisy.set_forcing(_rows(1))
        noisy.set_initial(TS, 0.0)
        noisy.set_initial(TD, 0.0)
        noisy.set_forcing_noise(0.1, 1)
        for bad in ((-1, 3), (0, T + 1), (5, 4)):
            refused(lambda: noisy.forcing_noise_rows(*bad), "forcing axis")
        refused(lambda: noisy.link_input(0, plain, TS), "linked input")
        obs = ([TS, TS], [3, 9], [0.1, 0.3], [0.1, 0.1])
        refused(lambda: noisy.run_loglik(*obs), "fused")
        refused(lambda: noisy.run_loglik(*obs, reference={TS: (0, 2)}), "fused")
        stream = C.c_void_p()
        L.check(lib.rscm_gpu_stream_create(0, C.byref(stream)))
        try:
            for e in (plain, noisy):
                e.set_stream(stream.value)
            refused(lambda: run_lockstep((plain, noisy)), "lock-step")
        finally:
            for e in (plain, noisy):
                e.set_stream(None)
            L.check(lib.rscm_gpu_stream_destroy(0, stream))
        i0, i1, d0, d1 = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32), np.zeros(1), np.ones(1)
        base = np.ascontiguousarray(two_layer_params(8)[:, 0])
        s = C.c_void_p()
        rc = lib.rscm_sampler_create(noisy._h, 16, 1, L.iptr(i0), L.dptr(base), L.iptr(i0), L.dptr(d0), L.dptr(d1), None, None,
                                     1, L.iptr(i1), L.iptr(i1), L.dptr(d0), L.dptr(d1), 0, 2.0, 1, C.byref(s))
        assert rc == L.ERR_INVALID and b"forcing noise" in lib.rscm_gpu_last_error() and not s.value
        h = (C.c_void_p * 1)(noisy._h)
        rc = lib.rscm_sampler_create_graph(h, 1, 0, 16, 1, L.iptr(i0), L.iptr(i0), L.iptr(i0), L.dptr(d0), L.dptr(d1), None, None,
                                           0, None, None, None, None, None, 0, 2.0, 1, 0, 1, C.byref(s))
        assert rc == L.ERR_INVALID and b"forcing noise" in lib.rscm_gpu_last_error() and not s.value
        # ... and the stored likelihood after a run is how it is scored
        noisy.run()
        ll = noisy.loglik(*obs)
        assert ll.shape == (8,) and np.isfinite(ll).all()


def test_model_builder_applies_the_noise(ra, orc):
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    t = np.arange(1750.0, 1791.0)
    axis = core.TimeAxis.from_values(t)
    lin = core.InterpolationStrategy.Linear
    erf = "Effective Radiative Forcing"
    base = (lambda: core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
            .with_initial_values({TS: 0.0, TD: 0.0}).with_forcing_noise(SIGMA, SEED))
    f = 3.0 * (1.0 - np.exp(-(t - 1750.0) / 40.0))
    plain = base().with_exogenous_variable(erf, core.Timeseries(f, axis, "W/m^2", lin)).build(n_members=4)
    mixed = base().with_forcing_components(erf, {"ghg": core.Timeseries(f, axis, "W/m^2", lin),
                                                 "aerosol": core.Timeseries(-0.3 * f, axis, "W/m^2", lin)}, scales={"aerosol": 0.9}).build(n_members=4)
    P6 = np.repeat(np.array([fixed[k] for k in core.TL_PARAM_ORDER])[:, None], 4, axis=1)
    for m, Fm in ((plain, np.repeat(f[None], 4, axis=0)), (mixed, np.repeat((f * 1.0 + (-0.3 * f) * 0.9)[None], 4, axis=0))):
        assert m.ensemble.forcing_noise == {"sigma": SIGMA, "seed": SEED, "member_offset": 0}
        m.run()
        want = hn.oracle_run(orc, axis.bounds(), P6, Fm, SIGMA, SEED)
        _same(_series(m.ensemble), want, "built model")
        m.close()


# ---------------------------------------------------------------------------------------------- 8. sanity
def test_clear_restores_the_noise_free_bits(ra):
    F, scen, P = _rows(2), _scen(2), two_layer_params(N)
    with _plain(ra, P, F, scen) as never, _plain(ra, P, F, scen, noise=(SIGMA, SEED)) as e:
        never.run()
        e.run()
        noisy = _series(e)
        assert (noisy[0][1:] != _series(never)[0][1:]).all()
        e.clear_forcing_noise()
        assert e.forcing_noise is None
        e.rewind()
        e.run()
        _same(_series(e), _series(never), "after clear_forcing_noise")
        assert np.array_equal(e.status(), never.status())
