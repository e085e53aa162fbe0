"""CPU tier of the running-mean diagnostics (ABI minor 27): the boundary declares and binds the new entry points, the front end's
estimator for a record (rscm_amd.variability.series_running_mean) is the restatement of tests/host_running_mean.py bit for bit, the
data the GPU tier (tests/test_gpu_running_mean.py) compares on tells the definition from the reversed order and from a sliding
update, and a non-finite row reaches exactly the windows that hold it.  No device call is made."""
import os
import re

import numpy as np
import pytest

from rscm_amd import _lib
from rscm_amd import variability as va
from tests import host_running_mean as hr
from tests.helpers import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rscm_ens_define_running_mean", "rscm_ens_diagnostic_running_mean")
T, N = 72, 257
WINDOWS = (2, 3, 11, 20, 64)
ALIGNS = ("trailing", "centre")


@pytest.fixture(scope="module")
def rows():
    x = hr.mixed_sign_rows(T, N)
    x.setflags(write=False)
    return x


def test_abi_minor_27_declares_and_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", header).group(1)) >= 27
    for name, value in (("MAX_WINDOW", _lib.RUNMEAN_MAX_WINDOW), ("TRAILING", _lib.RUNMEAN_TRAILING), ("CENTRED", _lib.RUNMEAN_CENTRED)):
        assert int(re.search(r"#define\s+RSCM_RUNMEAN_" + name + r"\s+(\d+)", header).group(1)) == value
    assert _lib.RUNMEAN_ALIGN == {"trailing": 0, "centre": 1}
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 27
    for name in NAMES:
        assert re.search(r"RSCM_API\s+int\s+" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_python_surface_exists():
    import rscm_amd
    from rscm_amd.core import GraphModel, ModelBuilder
    from rscm_amd.distributed import ShardedEnsemble
    for cls, name in ((rscm_amd.Ensemble, "define_running_mean"), (GraphModel, "define_running_mean"),
                      (ModelBuilder, "with_running_mean"), (ShardedEnsemble, "define_running_mean")):
        assert hasattr(cls, name), (cls.__name__, name)
    with pytest.raises(ValueError):
        ModelBuilder().with_running_mean("m", "Surface Temperature", window=65)
    with pytest.raises(ValueError):
        ModelBuilder().with_running_mean("m", "Surface Temperature", align="leading")
    b = ModelBuilder().with_running_mean("m", "Surface Temperature")
    with pytest.raises(ValueError):
        b.with_running_mean("m", "Surface Temperature")


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("step", (1, 3))
def test_series_running_mean_is_the_restatement(rows, window, align, step):
    b = hr.back(window, align)
    n = T - (window - 1) * step
    if n < 1:
        with pytest.raises(ValueError):
            va.series_running_mean(rows, window, align, step)
        return
    got, first = va.series_running_mean(rows, window, align, step)
    want, want_first = hr.all_rows(rows, window, align, step)
    assert first == want_first == b * step and got.shape == want.shape == (n, N)   # first_index and the length
    assert hr.valid_rows(T, window, align, step) == (first, first + n - 1)
    assert same_bits(got, want)
    one, first_one = va.series_running_mean(rows[:, 5], window, align, step)                # a single record
    assert first_one == first and same_bits(one, want[:, 5])
    assert va.running_mean_back(window, align) == b


def test_series_running_mean_refuses_what_the_library_refuses(rows):
    for window in (1, 65):
        with pytest.raises(ValueError):
            va.series_running_mean(rows, window)
    with pytest.raises(ValueError):
        va.series_running_mean(rows, 20, "leading")
    with pytest.raises(ValueError):
        va.series_running_mean(rows, 20, step=0)
    with pytest.raises(ValueError):
        va.series_running_mean(rows[:19], 20)


def test_the_data_tells_the_definition_from_what_it_is_not(rows):
    """On +-uniform(0.01, 5) the reversed order differs from the definition in a good share of the elements for every window
    from 3 on (none at 2: a + b is b + a), and the sliding update for every window from 2 on."""
    for window in range(2, 65):
        first, last = hr.valid_rows(T, window, "centre")
        want = hr.running_mean(rows, window, "centre", 1, first, last + 1, 1)
        rev = hr.reversed_order(rows, window, "centre", 1, first, last + 1, 1)
        differ = (rev.view(np.uint64) != want.view(np.uint64)).mean()
        assert (differ == 0.0) if window == 2 else (differ > 0.2), (window, differ)
        slide = hr.sliding_update(rows, window, "centre", 1, first, last + 1)
        assert same_bits(slide[0], want[0])
        differ = (slide[1:].view(np.uint64) != want[1:].view(np.uint64)).mean()
        assert differ > 0.5, (window, differ)


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("value", (np.inf, -np.inf, np.nan))
def test_a_non_finite_row_reaches_exactly_the_windows_that_hold_it(rows, align, value):
    window, step, k, member = 11, 2, 30, 7
    x = rows.copy()
    x[k, member] = value
    first, last = hr.valid_rows(T, window, align, step)
    got = hr.running_mean(x, window, align, step, first, last + 1, 1)
    clean = hr.running_mean(rows, window, align, step, first, last + 1, 1)
    b = hr.back(window, align)
    holds = np.array([k in range(t - b * step, t + (window - b) * step, step) for t in range(first, last + 1)])
    assert holds.sum() == window
    assert not np.isfinite(got[holds, member]).any() and np.isfinite(got[~holds]).all()
    untouched = np.ones_like(got, dtype=bool)
    untouched[holds, member] = False
    assert same_bits(got[untouched], clean[untouched])
