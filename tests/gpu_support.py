"""What the GPU test modules share and tests/helpers.py cannot hold, because it needs pytest or the library: the `ra` fixture, the
code of a refused call, the noisy two-layer ensemble of the series statistics' files and the bookkeeping of a `cases` fixture."""
import numpy as np
import pytest

from tests.helpers import two_layer_noise_case


@pytest.fixture(scope="module")
def ra():
    """The package with its HIP library loaded.  A module takes it with `from tests.gpu_support import ra  # noqa: F401`; pytest
    registers an imported fixture in the importing module, so it is set up once per module."""
    import rscm_amd
    from rscm_amd import _lib
    _lib.load()  # fails loudly when the HIP extension is missing
    assert _lib.device_count() >= 1, "no HIP device visible"
    return rscm_amd


def refusal_code(fn, *a, **k):
    """The error code of the call fn(*a, **k), which must be refused with RscmGpuError."""
    from rscm_amd._lib import RscmGpuError
    with pytest.raises(RscmGpuError) as err:
        fn(*a, **k)
    return err.value.code


def noise_ensemble(ra, n, bounds, seed, offset=0, n_total=None, steps=None, **kw):
    """A two-layer ensemble of tests.helpers.two_layer_noise_case(n, offset, n_total) on the axis `bounds`: scenario 0 is zero
    forcing and scenario 1 a ramp, both states start at zero, per-member forcing noise of `seed` from member `offset` of the
    draw; run to `steps` (None: the end)."""
    T = len(bounds) - 1
    P, scen = two_layer_noise_case(n, offset, n_total)
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, bounds, noise_params=True, **kw)
    e.set_params(P)
    e.set_forcing(np.stack([np.zeros(T), 0.05 * np.arange(T)]), scen)
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.set_forcing_noise_members(seed, offset)
    e.run(steps)
    return e


def plant(e, var, member, row, value):
    """Overwrite one member's value in one stored row of variable `var`."""
    x = e.get_series(var, row, row + 1)[0]
    x[member] = value
    e.set_state(var, row, x)


def built_once(build):
    """The body of a module-scoped `cases` fixture (`yield from built_once(build)`): hands the tests get(key), which returns the
    tuple build(key) and builds it at the first request only; at teardown closes the ensemble that leads each tuple."""
    made = {}

    def get(key):
        if key not in made:
            made[key] = build(key)
        return made[key]

    yield get
    for case in made.values():
        case[0].close()
