"""Every way of putting a handle back at time index 0 leaves a handle that runs like a fresh one, bit for bit.

What a handle remembers from one launch to the next -- OceanCarbon's sums parked for the second year of a split tile, its running
mode sums (RSCM_MODE_FAST), the red forcing noise's cached values -- belongs to the index the handle stands at.  The rule that drops
it when the stepper is put somewhere from outside is one member of the handle (rscm_ens::put_at, csrc/ens.hpp), called by every entry
point that moves the index; rscm_ens_set_initial is the stated exception.  Three subjects are stopped where such a fact is standing,
sent back to 0 by each entry point, run to the end in their own launch pattern and compared with a fresh handle run the same way:
every stored variable and the status bytes, bits not closeness.

65 members: one full wavefront and one lane of the next.  A yearly axis of 8 points: 7 steps, so a two-year tile can start at steps
0 to 5."""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.test_gpu_ocean import _case, _fast_info

pytestmark = pytest.mark.gpu

N, T, STOP = 65, 8, 3
BOUNDS = np.arange(T + 1, dtype=float) + 1850.0


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


class Subject:
    """One kind of handle, how it is set up, its initial values and the launch pattern it is run in."""

    def __init__(self, ra, kind, params, inputs, initial, one_step, setup, standing):
        self.ra, self.kind, self.params, self.inputs, self.initial = ra, kind, params, inputs, initial
        self.one_step, self.setup, self.standing = one_step, setup, standing

    def make(self):
        e = self.ra.Ensemble(self.kind, N, BOUNDS)
        self.setup(e)
        e.set_params(self.params)
        e.set_forcing(self.inputs)
        self.set_initial(e)
        return e

    def set_initial(self, e):
        for v, x in self.initial:
            e.set_initial(v, x)

    def run_to(self, e, end):
        if self.one_step:
            while e.time_index < end:
                e.run(e.time_index + 1)
        else:
            e.run(end)

    def run_out(self, e):
        """[0, STOP) and [STOP, T - 1) in the subject's pattern; every stored variable and the status bytes"""
        assert e.time_index == 0
        self.run_to(e, STOP)
        self.run_to(e, T - 1)
        return np.stack([e.get_series(v) for v in range(1, e.n_vars)]), e.status()


def _ocean(ra, orc, mode, one_step):
    P, inputs = _case(orc, "3D-GFDL", N, T, np.random.default_rng(65))

    def setup(e):
        e.set_mode(mode)

    def standing(e):
        assert _fast_info(e)[0]   # the modes are fitted: RSCM_MODE_FAST runs the recurrence with its running sums

    return Subject(ra, ra.KIND_OCEAN_CARBON, P, inputs[:1], ((1, 278.0), (2, 0.0)), one_step, setup,
                   standing if mode == ra.MODE_FAST else lambda e: None)


def _two_layer_red(ra):
    rng = np.random.default_rng(66)
    lo = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
    hi = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
    P = lo[:, None] + rng.random((6, N)) * (hi - lo)[:, None]
    F = 0.5 * np.arange(T, dtype=float)

    def setup(e):
        e.set_forcing_noise(0.3, seed=11, phi=0.6)

    def standing(e):
        assert e.forcing_noise_cached_index == STOP - 1   # the noise cache stands at the last forcing index the run read

    return Subject(ra, ra.KIND_TWO_LAYER, P, F, ((1, 0.0), (2, 0.0)), False, setup, standing)


@pytest.fixture(scope="module")
def subjects(ra, orc):
    """name -> (subject, what a fresh handle gives), the reference computed once and left unchanged"""
    made = {"ocean_exact_one_step": _ocean(ra, orc, ra.MODE_EXACT, True),   # stopped inside the tile of steps 2 and 3, sums parked
            "ocean_fast": _ocean(ra, orc, ra.MODE_FAST, False),             # the mode sums stand at 3
            "two_layer_red_noise": _two_layer_red(ra)}                      # the noise cache stands at 2
    out = {}
    for name, s in made.items():
        with s.make() as e:
            series, status = s.run_out(e)
        assert not status.any() and not np.isnan(series[:2]).any()
        series.setflags(write=False)
        status.setflags(write=False)
        out[name] = (s, series, status)
    return out


def _set_internal_state_at_0(s, e, state0):
    from rscm_amd import _lib
    _lib.check(e._lib.rscm_ens_set_internal_state(e._h, _lib.dptr(state0), state0.size, 0))


WAYS = {"rewind": lambda s, e, state0: e.rewind(),
        "set_time_index": lambda s, e, state0: e.set_time_index(0),
        "clear_series": lambda s, e, state0: e.clear_series(),
        "set_initial": lambda s, e, state0: s.set_initial(e),
        "set_internal_state": _set_internal_state_at_0}
CASES = [(name, way) for name in ("ocean_exact_one_step", "ocean_fast", "two_layer_red_noise") for way in WAYS
         if way != "set_internal_state" or name.startswith("ocean")]


@pytest.mark.parametrize("name,way", CASES)
def test_a_handle_sent_back_to_index_0_runs_like_a_fresh_one(subjects, name, way):
    from rscm_amd import _lib
    s, want_series, want_status = subjects[name]
    with s.make() as e:
        n = C.c_int64()
        _lib.check(e._lib.rscm_ens_internal_state_size(e._h, C.byref(n)))
        state0 = np.empty(n.value)   # the internal state taken at index 0 (OceanCarbon: no pulse is held yet)
        if n.value:
            _lib.check(e._lib.rscm_ens_get_internal_state(e._h, _lib.dptr(state0)))
        s.run_to(e, STOP)
        assert e.time_index == STOP
        s.standing(e)
        WAYS[way](s, e, state0)
        assert e.time_index == 0
        series, status = s.run_out(e)
    assert np.array_equal(status, want_status)
    assert np.array_equal(series.view(np.uint64), want_series.view(np.uint64))
