"""CPU tier: the host-side fit behind OceanCarbon's RSCM_MODE_FAST (rscm_gpu_ocean_fit_selftest: no GPU
call).  The scaled mixed-layer impulse response (parameters/ocean_carbon.rs:85-216) beyond the explicit
near lags must be reproduced by the 21 decaying modes to well inside the accepted 5e-10 for the three
presets at the reference's default scale, and the fit must decline windows too short to profit."""
import ctypes as C

import pytest

from rscm_amd import _lib


def _fit(model, scale, switch, H):
    lib = _lib.load()
    err, nm, near, nx, mc = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    _lib.check(lib.rscm_gpu_ocean_fit_selftest(model, scale, switch, H, C.byref(err), C.byref(nm), C.byref(near), C.byref(nx), C.byref(mc)))
    return err.value, nm.value, near.value, nx.value, mc.value


@pytest.mark.parametrize("model,switch,near", [(0, 1.0, 60), (1, 9.9, 120), (2, 2.0, 60)])
def test_default_scale_fits_to_1e_11(model, switch, near):
    err, nm, got_near, n_exit, _ = _fit(model, 0.9492864, switch, 6000)
    assert 0.0 <= err < 1e-11 and nm == 21 and got_near == near and 4 <= n_exit <= 21


@pytest.mark.parametrize("scale", [0.5, 0.7, 1.0, 1.3])
def test_other_scales_stay_inside_the_accepted_deviation(scale):
    for model, switch in ((0, 1.0), (1, 9.9), (2, 2.0)):
        err, nm, _, _, _ = _fit(model, scale, switch, 6000)
        if model == 1 and scale != 1.0:
            # 2D-BERN away from the reference's scale: the table is reproduced to 6e-11 or better, but with amplitudes of
            # 1.8e4 .. 6.4e4 (condition 2e4 .. 2e5, test_ill_conditioned_fits_are_declined): measured on the GPU over 600
            # years, FAST with these fits is 2.6e-9 / 6.7e-10 / 3.7e-10 from EXACT at scale 0.5 / 0.7 / 1.3, over its 2e-10
            assert err < 0.0, (model, scale, err)
            continue
        assert 0.0 <= err <= 5e-10, (model, scale, err)
    assert _fit(0, 1.0, 1.0, 6000)[0] < 1e-15   # unscaled: the response IS a sum of six exponentials


def test_short_windows_and_late_switches_are_declined():
    assert _fit(0, 0.9492864, 1.0, 100)[0] < 0.0
    assert _fit(0, 0.9492864, 1.0, 239)[0] < 0.0
    assert _fit(0, 0.9492864, 1.0, 240)[0] >= 0.0
    assert _fit(0, 0.9492864, 10.5, 6000)[0] < 0.0   # the late regime must begin within the explicit lags


def test_ill_conditioned_fits_are_declined():
    """A short window's fit can reproduce the table to 1e-13 with amplitudes of 1e3 .. 1.5e4 of alternating sign: the
    device's double sum over the modes then loses what the long double check cannot see (HILDA at 480 months: 4.9e-9
    from the oracle on the GPU, FAST's bar is 2e-10).  The host declines a fit whose far sum has a condition
    sum |c_q| G_q / sum r(lag) above 3000 (kOceanFitMaxCondition in csrc/kind_config.cpp has the measurements); such a
    handle keeps the fused tiles.  Conditions of the windows below, in order: 3.3e5, 2.4e4, 9600, 5000 | 2200, 490, 2200,
    1500, 1400, 1300, 1600, 1300, 990 -- none within a quarter of the limit, the amplitudes move by a per cent or so
    with the host's exp()."""
    gfdl, bern, hilda = (0, 1.0), (1, 9.9), (2, 2.0)
    for (model, switch), H in ((hilda, 480), (hilda, 245), (hilda, 600), (hilda, 624)):
        assert _fit(model, 0.9492864, switch, H)[0] < 0.0, (model, H)
    for (model, switch), H in ((hilda, 656), (hilda, 720), (gfdl, 240), (gfdl, 245), (gfdl, 251), (gfdl, 252),
                               (bern, 480), (bern, 487), (bern, 493)):
        err, nm, _, n_exit, amp = _fit(model, 0.9492864, switch, H)
        assert 0.0 <= err <= 1e-12 and nm == 21 and n_exit >= 15 and 10.0 < amp < 200.0, (model, H, err, n_exit, amp)
    # the long windows of the default presets stay accepted: 2D-BERN's amplitudes reach 670 there, in modes of small weight
    for model, switch in (gfdl, bern, hilda):
        assert _fit(model, 0.9492864, switch, 6000)[0] >= 0.0
