"""The three regimes of the shared-input staging of the two-layer and the coupled kind (csrc/two_layer.hip launch_impl,
csrc/coupled.hip launch_coupled), at their exact edges, in both modes.  The slice n_scen x steps x 8 B of the scenario table is
staged in LDS: within the static 64 KiB as it is, up to 160 KiB - 1 KiB after the launcher has raised the kernel's dynamic limit
(hipFuncSetAttribute), and beyond that it is not staged at all: the <false> instances read it through L2.

33 time points (32 steps, 256 B per scenario), 700 members mapped onto the scenarios by i % S so that the last scenario is read,
S = 256 (65 536 B: the last static size), 257 (the first raised one), 636 (162 816 B: the last LDS size) and 637 (the first L2 size),
in that order on fresh handles and then in reverse -- a raised limit stays with the kernel for the life of the process, so the order
is part of the case.  Which regime a launch took is inferred from the size of its slice (the thresholds the launchers apply to
n_scen x steps x 8, restated below), not observed: the library reports only that the run was one launch.  Against the oracle at the
tolerances of tests/test_gpu_parity.py, and the members whose scenario is the same at every S bit for bit across the four regimes."""
import numpy as np
import pytest

from rscm_amd import _lib as L
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import assert_bit_equal, coupled_params, f_syn, two_layer_params
from tests.test_gpu_parity import CP_INIT, CP_NAMES, FAST_RTOL, _bounded, _close

pytestmark = pytest.mark.gpu

T, N = 33, 700
STEPS = T - 1
STATIC_LDS = 64 * 1024             # kMaxStaticLds (csrc/rscm_device.hpp)
LAST_LDS = 160 * 1024 - 1024       # kMaxLds - 1024: the largest slice that is staged
PER_SCENARIO = STEPS * 8
S_STATIC, S_LAST = STATIC_LDS // PER_SCENARIO, LAST_LDS // PER_SCENARIO
SIZES = (S_STATIC, S_STATIC + 1, S_LAST, S_LAST + 1)
YEARS = 1900.0 + np.arange(T, dtype=np.float64)
BOUNDS = np.append(YEARS, YEARS[-1] + 1.0)
_WANT = {}


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


def test_the_sizes_sit_on_the_intended_side_of_each_edge():
    assert SIZES == (256, 257, 636, 637)
    assert SIZES[0] * PER_SCENARIO == STATIC_LDS == 65_536 and SIZES[1] * PER_SCENARIO > STATIC_LDS
    assert SIZES[2] * PER_SCENARIO == LAST_LDS == 162_816 and SIZES[3] * PER_SCENARIO > LAST_LDS
    assert N > SIZES[3] and all((np.arange(N) % S).max() == S - 1 for S in SIZES)   # the last scenario is read


def _table(kind):
    """[637][T]: scenario s is the same series at every S."""
    rng = np.random.default_rng(637 + kind)
    if kind == L.KIND_TWO_LAYER:
        return f_syn(YEARS + 100.0)[None] * rng.uniform(0.2, 1.2, (SIZES[3], 1)) + rng.normal(0.0, 0.05, (SIZES[3], T))
    return np.abs(rng.normal(3.0, 3.0, (SIZES[3], T)))


def _params(kind):
    return two_layer_params(N) if kind == L.KIND_TWO_LAYER else coupled_params(N)


def _want(orc, kind, S):
    if (kind, S) not in _WANT:
        scen = (np.arange(N) % S).astype(np.int32)
        if kind == L.KIND_TWO_LAYER:
            _WANT[(kind, S)] = dict(zip(("ts", "td"), orc.two_layer_run(BOUNDS, _params(kind), _table(kind)[:S], 0.0, 0.0, scen=scen, threads=8)))
        else:
            _WANT[(kind, S)] = orc.coupled_run(BOUNDS, _params(kind), _table(kind)[:S],
                                               dict(ts=0.0, td=0.0, conc=278.0, cum_uptake=0.0, cum_emis=0.0), scen=scen, threads=8)
    return _WANT[(kind, S)]


def _gpu(ra, kind, S, mode):
    scen = (np.arange(N) % S).astype(np.int32)
    with ra.Ensemble(kind, N, BOUNDS) as e:
        e.set_mode(mode)
        e.set_params(_params(kind))
        e.set_forcing(_table(kind)[:S], scen)
        if kind == L.KIND_TWO_LAYER:
            e.set_initial(1, 0.0)
            e.set_initial(2, 0.0)
            names = {"ts": 1, "td": 2}
        else:
            for name, x in CP_INIT.items():
                e.set_initial(name, x)
            names = CP_NAMES
        e.run()
        assert e.finished() and e.last_run_plan() == (1, 1)   # one launch: the slice is n_scen x 32 steps
        return {k: e.get_series(v) for k, v in names.items()}, e.status()


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_FAST], ids=["exact", "fast"])
@pytest.mark.parametrize("kind", [L.KIND_TWO_LAYER, L.KIND_COUPLED], ids=["two_layer", "coupled"])
def test_staging_regimes_at_their_edges(ra, orc, kind, mode):
    first = None
    worst = 0.0
    for S in SIZES + SIZES[::-1]:
        got, st = _gpu(ra, kind, S, mode)
        want = _want(orc, kind, S)
        what = f"{'two-layer' if kind == L.KIND_TWO_LAYER else 'coupled'} mode {mode} S = {S} ({S * PER_SCENARIO} B)"
        bounded = _bounded(want["ts"])
        assert bounded.mean() > 0.9, what
        for k, w in want.items():
            g = got[k]
            if kind == L.KIND_TWO_LAYER and mode == L.MODE_EXACT:
                assert_bit_equal(g, w, f"{what} {k}")
                continue
            assert (np.isnan(g[:, bounded]) == np.isnan(w[:, bounded])).all(), f"{what} {k}"
            assert _close(g[1:, bounded], w[1:, bounded], FAST_RTOL).all(), f"{what} {k}"
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.nanmax(np.abs(g[1:, bounded] - w[1:, bounded]) / np.maximum(1.0, np.abs(w[1:, bounded])))))
        if kind == L.KIND_COUPLED:
            assert_bit_equal(got["cum_emis"], want["cum_emis"], f"{what} cumulative emissions")
        assert not st[bounded].any(), what
        # members below 256 read scenario i at every S: the regime may not change a bit
        same = {k: g[:, :SIZES[0]] for k, g in got.items()}
        if first is None:
            first = same
        for k in same:
            assert_bit_equal(same[k], first[k], f"{what} {k}: members below {SIZES[0]} against the first run (S = {SIZES[0]})")
    print(f"{'two-layer' if kind == L.KIND_TWO_LAYER else 'coupled'} mode {mode}: 8 runs over S = {SIZES}, largest deviation from the oracle "
          f"{worst:.2e} (tolerance {FAST_RTOL:g}{'; bit equality' if kind == L.KIND_TWO_LAYER and mode == L.MODE_EXACT else ''})")
