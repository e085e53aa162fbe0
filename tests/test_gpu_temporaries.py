"""GPU tier: the host layer's device temporaries do not outlive their call (csrc/dev_buf.hpp, rscm::DevBuf).  Every entry point
that allocates one -- baselines, indicators, variability, spectra, the vector likelihoods, exceedance, the quantile and summary
series, the log-likelihood maximum, member weights and groups, the staged and the one-call select, the forcing-noise rows -- is
called 400 times on one handle of 65 536 members, succeeding and refused after its temporary was allocated, and free device memory
stays where it was.  A refusal leaves the weights, groups and baseline set before in force, bit for bit.

One leaked vector of 65 536 doubles per iteration would be 200 MB over the loop; the margin is the 64 MB that
test_gpu_parity.py::test_handle_churn_does_not_leak allows for allocator slack.  Row-pointer tables and flags are too small to
show in free memory: tests/test_host_dev_buf.py covers the owner itself."""
import numpy as np
import pytest

from tests.helpers import f_syn, two_layer_params

pytestmark = pytest.mark.gpu

N = 65536
ITERATIONS = 400
Q = [0.05, 0.5, 0.95]
THR = [0.1, 0.3]


def _refused(call, *args, **kw):
    from rscm_amd import _lib
    with pytest.raises(_lib.RscmGpuError) as err:
        call(*args, **kw)
    assert err.value.code == _lib.ERR_INVALID, str(err.value)


def test_no_entry_point_leaks_its_device_temporaries_and_refusals_keep_what_was_set():
    import rscm_amd as ra
    from rscm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1
    t = np.arange(1750.0, 1775.0)                  # 24 steps
    b = np.append(t, t[-1] + 1.0)
    T = t.size
    rng = np.random.default_rng(7)
    P = two_layer_params(N)
    w0 = rng.integers(0, 1000, N).astype(np.int64)
    g0 = rng.integers(-1, 3, N).astype(np.int32)
    b0 = rng.normal(0.0, 0.1, N)
    ll = -rng.random(N)
    w_negative = w0.copy()
    w_negative[N // 2] = -1
    w_heavy = np.zeros(N, dtype=np.int64)          # sums to 2^53 + 2
    w_heavy[0], w_heavy[-1] = 1 << 53, 2
    g_bad = g0.copy()
    g_bad[N - 1] = 3                               # == n_groups
    anc_bad = np.arange(8, dtype=np.int64)
    anc_bad[5] = N                                 # == the source's members

    with ra.Ensemble(ra.KIND_TWO_LAYER, N, b) as e, ra.Ensemble(ra.KIND_TWO_LAYER, N, b) as noisy, \
            ra.Ensemble(ra.KIND_TWO_LAYER, 8, b) as dst:
        e.set_params(P)
        e.set_forcing(f_syn(t))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.run()
        noisy.set_params(P)
        noisy.set_forcing_noise(0.3, 11, phi=0.5)

        def one_pass():
            e.set_baseline(1, 0, 5)
            e.set_baseline_values(b0)
            ind = e.indicators(1, 0, T, thresholds=THR, anomaly=True, slot=0)
            var = e.variability(1, 0, T, detrend="linear", slot=1)
            spec = e.spectrum(1, 0, T, detrend="difference", bands=4, slot=2)
            e.loglik_vectors([var["sd"], var["r1"]], [0.1, 0.5], [0.05, 0.2])
            e.loglik_spectrum(spec["power"], np.full(len(spec["power"]), 0.01), spec["counts"])
            e.quantile_series(1, Q, T - 2, T)
            e.summary_series(1, T - 2, T)
            e.loglik_max(ll)
            e.set_weights_from_loglik(ll, bits=20, ll_max=0.0)
            e.set_member_weights(w0)
            e.set_member_groups(g0, 3)
            e.weights_stats()
            e.exceedance(ind["peak"], THR, weighted=True)
            e.exceedance(ind["peak"], THR, weighted=True, grouped=True)
            with e.select(1, Q, T - 2, T, weighted=True, anomaly=True, grouped=True):
                pass
            e.quantile_rows(1, Q, T - 1, T, weighted=True)
            noisy.forcing_noise_rows(3, 5)
            # refused after the temporary is there: ordinary bad input
            _refused(e.set_member_weights, w_negative)
            _refused(e.set_member_weights, w_heavy)
            _refused(e.set_member_groups, g_bad, 3)
            _refused(e.branch, dst, anc_bad)

        def state():
            return e.member_weights(), e.member_groups(), e.baseline().view(np.uint64)

        one_pass()                                 # every lazy allocation is made
        w_set, g_set, b_set = state()
        assert np.array_equal(w_set, w0) and np.array_equal(g_set, g0) and np.array_equal(b_set, b0.view(np.uint64))
        free_before, _ = _lib.mem_info()
        for _ in range(ITERATIONS):
            one_pass()
            w_now, g_now, b_now = state()
            assert np.array_equal(w_now, w_set) and np.array_equal(g_now, g_set) and np.array_equal(b_now, b_set)
            assert e.n_groups == 3
        free_after, _ = _lib.mem_info()
        fallen = free_before - free_after
        print(f"free device memory fell by {fallen / 1e6:.1f} MB over {ITERATIONS} iterations")
        assert fallen < 64e6, f"free device memory fell by {fallen / 1e6:.1f} MB"
