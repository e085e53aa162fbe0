"""The device Latin hypercube through Normal, LogNormal and truncated priors (include/rscm_gpu.h, rscm_ens_sample_lhs_priors) against
its host restatement tests/host_lhs_priors.py: every entry bit for bit -- the exponential of a log-normal row within the 2 ulp the
device library's exp is held to --, whole and as a block of a larger ensemble; the uniform rows against Ensemble.sample_lhs; the ranks
that make a column a Latin hypercube on the device's own output; the handle's state after the call; the refusals; and one calibration
pass from a ParameterSet to weighted quantiles."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import host_lhs_priors as hp
from tests.gpu_support import ra, refusal_code  # noqa: F401   (ra: the module-scoped fixture)
from tests.helpers import same_bits
from tests.host_math import mp_reference, ulp_error

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 20260117
BOUNDS = np.arange(1850.0, 1872.0)   # 21 steps


def _priors():
    from rscm_amd.calibrate import Bound, LogNormal, Normal, Uniform
    # rows 0 .. 7: Uniform, fixed (absent: a == b), Normal, Bound(Normal) central, Bound(Normal) reflected, LogNormal, Bound(LogNormal),
    # Bound(Uniform)
    return {0: Uniform(0.8, 1.5), 2: Normal(8.0, 1.5), 3: Bound(Normal(0.7, 0.2), 0.5, 1.0), 4: Bound(Normal(0.0, 1.0), 6.0, 8.0),
            5: LogNormal(1.1, 0.4), 6: Bound(LogNormal(1.1, 0.4), 2.0, 4.5), 7: Bound(Uniform(0.0, 2.0), 0.5, 3.0)}


BASE = np.array([1.0, 0.05, 1.3, 0.7, 8.0, 100.0, 0.4, 0.2])
LOG_ROWS = (5, 6)


def _table():
    from rscm_amd.calibrate import prior_table
    return prior_table(_priors(), 8, BASE)


def _draw(ra, n_local, offset, n_total, seed=SEED):
    with ra.Ensemble(ra.KIND_TWO_LAYER, n_local, BOUNDS, noise_params=True) as e:
        assert e.n_params == 8
        e.sample_lhs_priors(seed, _priors(), BASE, offset, n_total)
        return e.get_params()


def _raw(e, table, seed=SEED, offset=0, n_total=None):
    """The entry point itself with a table the builder would not make."""
    from rscm_amd import _lib as L
    kind, a, b, p0, p1, lo, hi = (np.ascontiguousarray(v) for v in table)
    L.check(e._lib.rscm_ens_sample_lhs_priors(e._h, C.c_uint64(seed), L.iptr(kind.astype(np.int32)), L.dptr(a), L.dptr(b), L.dptr(p0),
                                              L.dptr(p1), L.dptr(lo), L.dptr(hi), offset, e.n_members if n_total is None else n_total))


def _assert_equals_restatement(got, offset, n_local, n_total, what):
    """Every row but the log-normal ones bit for bit; those against the correctly rounded exponential of the restated y, moved into
    [lo, hi] as the device moves its own (a 1-Lipschitz map: it cannot widen a distance): at most 2 ulp, the bound
    test_library_log_and_exp_within_two_ulp holds the device's exp to.  Returns the largest distance seen."""
    table = _table()
    want, y = hp.lhs_priors_matrix(SEED, table, offset, n_local, n_total, with_y=True)
    exact = [j for j in range(8) if j not in LOG_ROWS]
    assert same_bits(got[exact], want[exact]), what
    worst = 0.0
    for j in LOG_ROWS:
        true = np.clip(mp_reference("exp", y[j]), table[5][j], table[6][j])
        err = float(ulp_error(got[j], true).max())
        worst = max(worst, err)
        assert err <= 2.0, (what, j, err)
        assert (got[j] >= table[5][j]).all() and (got[j] <= table[6][j]).all()
    return worst


@pytest.mark.parametrize("n", [1, 5, 64, 257, 1000])
def test_every_entry_is_the_restatement(ra, n):
    """n = 1: stratum 0 alone; 64: one wavefront; 257: one member past a block."""
    got = _draw(ra, n, 0, n)
    worst = _assert_equals_restatement(got, 0, n, n, f"n={n}")
    print(f"\nn={n}: six rows bit for bit; the log-normal rows within {worst:.3f} ulp of the correctly rounded exponential")
    assert (got[1] == BASE[1]).all()


def test_a_block_is_the_slice_of_the_whole(ra):
    """Members [300, 500) of 1000 on a handle of 200: the restatement's block, and the slice of the whole draw, bit for bit -- the
    exponential included: the same code on the same y."""
    part = _draw(ra, 200, 300, 1000)
    worst = _assert_equals_restatement(part, 300, 200, 1000, "block [300, 500) of 1000")
    assert same_bits(part, _draw(ra, 1000, 0, 1000)[:, 300:500])
    print(f"\nblock: log-normal rows within {worst:.3f} ulp")


def test_uniform_rows_equal_sample_lhs(ra):
    n = 1000
    table = _table()
    got = _draw(ra, n, 0, n)
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS, noise_params=True) as e:
        e.sample_lhs(SEED, table[1], table[2])
        ref = e.get_params()
        # and a table of uniform rows alone: the whole matrix
        from rscm_amd.calibrate import Uniform
        boxes = {j: Uniform(lo, hi) for j, (lo, hi) in enumerate([(0.8, 1.5), (0.0, 0.1), (1.0, 1.8), (0.5, 1.0), (5.0, 15.0), (50.0, 200.0), (0.1, 0.6)])}
        e.sample_lhs_priors(SEED + 1, boxes, BASE)
        all_uniform = e.get_params()
        e.sample_lhs(SEED + 1, [0.8, 0.0, 1.0, 0.5, 5.0, 50.0, 0.1, BASE[7]], [1.5, 0.1, 1.8, 1.0, 15.0, 200.0, 0.6, BASE[7]])
        assert same_bits(all_uniform, e.get_params())
    uniform = [j for j in range(8) if table[0][j] == 0]
    assert uniform == [0, 1, 7] and same_bits(got[uniform], ref[uniform])


def test_ranks_and_bounds_on_the_device_output(ra):
    """At 4096, exact: a Normal, LogNormal or centrally truncated column is ordered as its strata, a reflected column in reverse,
    and every value of a truncated row lies inside its bounds."""
    n = 4096
    kind, a, b, p0, p1, lo, hi = _table()
    X = _draw(ra, n, 0, n)
    for j in (0, 2, 3, 4, 5, 6, 7):
        strata = hp.lhs_strata(SEED, j, 0, n, n)
        want = np.argsort(strata)
        assert np.unique(X[j]).size == n, f"row {j}: ties"
        assert np.array_equal(np.argsort(X[j], kind="stable"), want[::-1] if kind[j] & hp.PRIOR_REFLECT else want), f"row {j}"
    assert kind[4] & hp.PRIOR_REFLECT
    for j in (3, 4, 6):
        assert (X[j] >= lo[j]).all() and (X[j] <= hi[j]).all(), f"row {j}"
    phi = np.array([0.5 * math.erfc(-((x - a[2]) / b[2]) / math.sqrt(2.0)) for x in X[2]])
    assert np.array_equal(np.floor(phi * n).astype(np.int64), hp.lhs_strata(SEED, 2, 0, n, n).astype(np.int64))


def _runnable_priors():
    from rscm_amd.calibrate import Bound, LogNormal, Normal, Uniform
    return {0: Uniform(0.8, 1.5), 2: Bound(Normal(1.3, 0.2), 1.0, 1.8), 3: Bound(Normal(0.7, 0.2), 0.5, 1.0), 4: Normal(8.0, 0.5),
            5: LogNormal(math.log(100.0), 0.3), 6: Bound(LogNormal(-1.2, 0.4), 0.05, 0.8), 7: Uniform(0.0, 0.9)}


def test_state_after_the_call(ra):
    """As sample_lhs leaves it: a computed diagnostic is stale, the per-member noise cache is dropped, and run() needs no set_params."""
    n, T = 130, len(BOUNDS) - 1
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS, noise_params=True) as e:
        e.set_forcing(0.05 * np.arange(T))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.set_forcing_noise_members(7)
        assert refusal_code(e.run, 10) == 2                                    # parameters not set
        e.sample_lhs_priors(SEED, _runnable_priors(), BASE)
        e.run(10)                                                              # ... and now they are
        assert e.forcing_noise_cached_index == 9
        first = e.get_series(1, 0, 11)
        assert np.isfinite(first).all() and np.unique(first[10]).size == n
        vid = e.define_heat_content()
        e.compute_diagnostic(vid)
        assert e.summary(vid, 10)["count"] == n
        e.sample_lhs_priors(SEED + 1, _runnable_priors(), BASE)
        assert e.forcing_noise_cached_index == -1
        assert refusal_code(e.summary, vid, 10) == 2 and refusal_code(e.get_series, vid, 0, 1) == 2
        from rscm_amd._lib import RscmGpuError
        with pytest.raises(RscmGpuError, match="is stale: compute it again"):
            e.quantile_rows(vid, [0.5], 0, 1)
        e.rewind()
        e.run(10)
        assert not same_bits(e.get_series(1, 0, 11), first)
        e.sample_lhs_priors(SEED, _runnable_priors(), BASE)                    # the first draw again: the first run again
        e.rewind()
        e.run(10)
        assert same_bits(e.get_series(1, 0, 11), first)


def test_refusals(ra):
    from rscm_amd import _lib as L
    from rscm_amd.calibrate import Normal, Uniform

    def changed(row, **kw):
        t = [np.array(v) for v in _table()]
        for name, value in kw.items():
            t[("kind", "a", "b", "p0", "p1", "lo", "hi").index(name)][row] = value
        return t

    with ra.Ensemble(ra.KIND_TWO_LAYER, 64, BOUNDS, noise_params=True) as e:
        _raw(e, _table())                                                      # the table itself passes
        for what, table in {"b = 0": changed(2, b=0.0), "b < 0": changed(5, b=-0.4), "b = inf": changed(2, b=math.inf), "b NaN": changed(2, b=math.nan),
                            "p0 = p1": changed(3, p0=0.25, p1=0.25), "p0 > p1": changed(6, p0=0.75, p1=0.5), "p0 < 0": changed(2, p0=-0.1),
                            "p1 > 1": changed(2, p1=1.5), "p0 NaN": changed(2, p0=math.nan), "lo > hi": changed(3, lo=1.0, hi=0.5),
                            "kind 3": changed(0, kind=3), "kind -1": changed(1, kind=-1), "kind 3 | reflect": changed(2, kind=3 | L.PRIOR_REFLECT),
                            "another flag": changed(2, kind=1 | 0x200), "reflect on kind 0": changed(0, kind=L.PRIOR_REFLECT)}.items():
            assert refusal_code(_raw, e, table) == L.ERR_INVALID, what
        for offset, n_total in ((0, 63), (1, 64), (-1, 100), (37, 100), (0, 0)):
            assert refusal_code(_raw, e, _table(), SEED, offset, n_total) == L.ERR_INVALID, (offset, n_total)
        _raw(e, _table(), SEED, 36, 100)
        assert refusal_code(lambda: L.check(e._lib.rscm_ens_sample_lhs_priors(e._h, C.c_uint64(1), None, None, None, None, None, None, None,
                                                                              0, 64))) == L.ERR_INVALID                  # NULL arrays
        with pytest.raises(ValueError, match="one entry per parameter"):
            e.sample_lhs_priors(SEED, _priors(), BASE[:6])
    with ra.Ensemble(ra.KIND_UDEB, 4, BOUNDS) as e:
        j = L.UD_PARAM_NAMES.index("n_layers")
        assert refusal_code(e.sample_lhs_priors, SEED, {j: Normal(30.0, 2.0)}, L.UD_DEFAULTS) == L.ERR_INVALID
        assert refusal_code(e.sample_lhs_priors, SEED, {j: Uniform(20.0, 30.0)}, L.UD_DEFAULTS) == L.ERR_INVALID
        e.sample_lhs_priors(SEED, {L.UD_PARAM_NAMES.index("ecs"): Normal(3.0, 0.5)}, L.UD_DEFAULTS)   # (a row that is not structural)
    with ra.Ensemble(ra.KIND_N2O_CHEMISTRY, 4, BOUNDS) as e:                   # the delay's row: uniform only, but it may vary
        assert refusal_code(e.sample_lhs_priors, SEED, {4: Normal(3.0, 0.5)}, L.N2O_DEFAULTS) == L.ERR_INVALID
        e.sample_lhs_priors(SEED, {4: Uniform(1.0, 5.0)}, L.N2O_DEFAULTS)
        assert e.get_params()[4].min() >= 1.0 and e.get_params()[4].max() <= 5.0


def test_parameter_set_to_weighted_quantiles(ra):
    """ParameterSet -> sample_lhs_priors -> run -> loglik -> set_weights_from_loglik -> quantile_vectors of a LogNormal row, at 4096
    members; the unweighted mean of the plain Normal row lies within 3 sd / sqrt(n) of its mean (a stratified sample is far inside
    that: this catches a wrong row or scale only)."""
    from rscm_amd.calibrate import ParameterSet
    from rscm_amd.core import ModelBuilder
    n, T = 4096, len(BOUNDS) - 1
    names = ("lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep", "forcing_noise|sigma", "forcing_noise|phi")
    assert names[6:] == ModelBuilder.NOISE_PARAM_NAMES
    ps = ParameterSet()
    for j, d in _runnable_priors().items():
        ps.add(names[j], d)
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS, noise_params=True) as e:
        e.set_forcing(0.1 * np.arange(T))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.set_forcing_noise_members(11)
        e.sample_lhs_priors(SEED, ps.rows(names), BASE)
        e.run()
        assert e.finished()
        ll = e.loglik([1, 1], [10, 20], [0.35, 0.9], [0.15, 0.15], on_device=True)
        e.set_weights_from_loglik(ll)
        cd = e.params_vector(5)
        prior_q = e.quantile_vectors([cd], [0.05, 0.5, 0.95])["quantiles"][0]
        post_q = e.quantile_vectors([cd], [0.05, 0.5, 0.95], weighted=True)["quantiles"][0]
        want = np.exp(math.log(100.0) + 0.3 * np.array([-1.6448536269514722, 0.0, 1.6448536269514722]))
        print(f"\nheat_capacity_deep: prior quantiles {prior_q}, analytic {want}; posterior {post_q}")
        # one stratum of 4096 is 2.4e-4 in probability: at most 2.4e-4 / pdf(1.645) = 2.4e-3 in z, times sigma 0.3 = 7e-4 in ln x
        assert np.allclose(prior_q, want, rtol=2e-3)
        assert np.isfinite(post_q).all() and post_q[0] <= post_q[1] <= post_q[2]
        m = e.moments([e.params_vector(4)])
        assert int(np.ravel(m["count"])[0]) == n and abs(float(np.ravel(m["mean"])[0]) - 8.0) <= 3 * 0.5 / math.sqrt(n)
