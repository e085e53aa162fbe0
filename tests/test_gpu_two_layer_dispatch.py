"""GPU tier of the two-layer launcher's kernel selection (csrc/two_layer.hip): every combination of arithmetic mode, forcing path,
plain or mix forcing and noise kind picks one instantiation from one table, and the files of the single features cover that table
only in part (nothing else runs FAST x mix x through L2 x per-member noise).  Here every entry runs once.

Stored runs, 2 x 2 x 2 x 4 = 32 cases: the handle's series against a PLAIN noise-free handle of the same mode with one scenario per
member, whose table is the host-formed forcing -- the members' series (the mix sum of tests/host_forcing_mix.py for a mix handle)
plus the handle's own rscm_ens_forcing_noise_rows -- bit for bit in both modes (the technique of
test_fast_mode_equals_a_plain_handle_under_the_host_formed_series).  The EXACT cases also against the CPU oracle under the series
formed with the numpy restatements of the noise (tests/host_forcing_noise*.py), bit for bit.

Fused likelihood, 2 x 2 x 2 x 2 = 16 cases (noise-free: a noise handle has no fused likelihood), without and with reference
periods: against the stored-series likelihood of the same handle, bit for bit in both modes and with and without normalisation, the
comparison of tests/test_gpu_reference_period.py.

Shapes: N = 130 members (two wavefronts and two lanes).  "staged": 2 scenarios x 24 uneven steps, the table staged in LDS.
"through L2": 130 scenarios x 200 steps, more than the 159 KiB a launch may stage.  Mix handles have K = 2 components."""
import functools

import numpy as np
import pytest

from tests import host_forcing_mix as hm
from tests import host_forcing_noise_members as hmem
from tests import host_forcing_noise_red as hr
from tests.helpers import assert_bit_equal, two_layer_params
from tests.test_gpu_forcing_noise import N, SEED, SIGMA, TD, TS, _annual, _mix_params, _own_series, _rows, _same, _scen, _series, orc, ra  # noqa: F401
from tests.test_gpu_forcing_noise_members import _noise_rows

pytestmark = pytest.mark.gpu

K = 2
PHI = 0.7
OFFSET = 3
T_STAGED, T_L2 = 25, 201
assert N * K * (T_L2 - 1) * 8 > N * (T_L2 - 1) * 8 > 159 * 1024 > 2 * K * (T_STAGED - 1) * 8

modes = pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fast"])
paths = pytest.mark.parametrize("path", ["staged", "through-L2"])
mixes = pytest.mark.parametrize("mix", [False, True], ids=["plain", "mix"])


@functools.lru_cache(maxsize=None)
def _shape(path, mix):
    """bounds, the handle's table ([S][T], mix: [S][K][T]), scen, its parameter block ([6][N], mix: [6 + K][N]) and the members'
    noise-free series [N][T]; computed once per shape and never changed."""
    if path == "staged":
        nt, n_scen, scen = T_STAGED, 2, _scen(2)
        b = np.concatenate([[1750.0], 1750.0 + np.cumsum(np.where(np.arange(nt) % 7 == 3, 0.5, 1.0))])
    else:
        nt, n_scen, scen = T_L2, N, np.arange(N, dtype=np.int32)[::-1].copy()
        b = _annual(nt)
    if mix:
        F, P = _rows(n_scen * K, nt, scale=0.4).reshape(n_scen, K, nt), _mix_params(K)   # (scaled: no member's sum runs away in 200 years)
        Fm = hm.mix_forcing(F, P[6:], scen)
    else:
        F, P = _rows(n_scen, nt), two_layer_params(N)
        Fm = F[scen]
    for a in (b, F, scen, P, Fm):
        a.setflags(write=False)
    return b, F, scen, P, Fm


@functools.lru_cache(maxsize=None)
def _host_term(path, noise):
    """The numpy restatement of the term e [N][T] that the noise kind adds (member ids OFFSET + i)."""
    nt, g = (T_STAGED if path == "staged" else T_L2), np.arange(N, dtype=np.uint64) + np.uint64(OFFSET)
    if noise == "members":
        return hmem.member_noise(SEED, g, nt, *_noise_rows())
    return hr.red_noise(SEED, g, nt, SIGMA, PHI if noise == "red" else 0.0)


def _handle(ra, mode, path, mix, noise=None, store=True):
    b, F, scen, P, _ = _shape(path, mix)
    if noise == "members":
        P = np.vstack([P, *_noise_rows()])
    e = ra.Ensemble(ra.KIND_TWO_LAYER, N, b, forcing_components=K if mix else None, noise_params=noise == "members", store_series=store)
    e.set_mode(mode)
    e.set_params(P)
    e.set_forcing(F, scen)
    e.set_initial(TS, 0.0)
    e.set_initial(TD, 0.0)
    if noise == "white":
        e.set_forcing_noise(SIGMA, SEED, OFFSET)
    elif noise == "red":
        e.set_forcing_noise(SIGMA, SEED, OFFSET, PHI)
    elif noise == "members":
        e.set_forcing_noise_members(SEED, OFFSET)
    return e


@pytest.mark.parametrize("noise", [None, "white", "red", "members"], ids=["none", "white", "red", "members"])
@mixes
@paths
@modes
def test_stored_run_equals_a_plain_handle_under_the_host_formed_series(ra, orc, mode, path, mix, noise):
    b, _, _, P, Fm = _shape(path, mix)
    with _handle(ra, mode, path, mix, noise) as e:
        e.run()
        assert e.finished()
        got, status = _series(e), e.status()
        with np.errstate(all="ignore"):
            Fn = Fm if noise is None else Fm + e.forcing_noise_rows().T
    with _own_series(ra, P[:6], Fn, mode=mode, bounds=b) as p:
        p.run()
        _same(got, _series(p), f"mode {mode}, {path}, mix {mix}, noise {noise}: against the plain handle")
        assert np.array_equal(status, p.status())
    if mode == 0:
        with np.errstate(all="ignore"):
            Fh = Fm if noise is None else Fm + _host_term(path, noise)
        want = orc.two_layer_run(b, P[:6], Fh, 0.0, 0.0, scen=np.arange(N, dtype=np.int32), source=0)
        assert np.isfinite(want[0]).all()
        _same(got, want, f"{path}, mix {mix}, noise {noise}: against the oracle")
        assert not status.any()


@pytest.mark.parametrize("period", [False, True], ids=["no-period", "period"])
@mixes
@paths
@modes
def test_fused_likelihood_equals_the_stored_path(ra, mode, path, mix, period):
    last = (T_STAGED if path == "staged" else T_L2) - 1
    rows = np.array([1, 5, 5, last // 2, last - 1, last, 0, 7, last], dtype=np.int32)
    var = [TS] * 6 + [TD] * 3
    rng = np.random.default_rng(1)
    val, sig = rng.normal(0.4, 0.4, len(rows)), rng.uniform(0.05, 0.5, len(rows))
    kw = {"reference": {TS: (2, 8), TD: (0, last // 2 + 1, 2)}} if period else {}
    with _handle(ra, mode, path, mix) as e:
        e.run()
        want = [e.loglik(var, rows, val, sig, normalize, **kw) for normalize in (False, True)]
        status = e.status()
        assert np.isfinite(want[0]).all() and not np.array_equal(want[0], want[1])
        if period:
            assert not np.array_equal(want[0], e.loglik(var, rows, val, sig, False))
        e.rewind()
        for normalize in (False, True):
            assert_bit_equal(e.run_loglik(var, rows, val, sig, normalize, **kw), want[normalize],
                             f"mode {mode}, {path}, mix {mix}, period {period}, normalize {normalize}: the handle that holds the series")
            assert e.time_index == 0
    with _handle(ra, mode, path, mix, store=False) as e:
        for normalize in (False, True):
            assert_bit_equal(e.run_loglik(var, rows, val, sig, normalize, **kw), want[normalize],
                             f"mode {mode}, {path}, mix {mix}, period {period}, normalize {normalize}: a handle without series")
        assert np.array_equal(e.status(), status)
