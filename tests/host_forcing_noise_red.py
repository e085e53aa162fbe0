"""Host restatement of the red (AR(1)) forcing noise of a two-layer ensemble (include/rscm_gpu.h, rscm_ens_set_forcing_noise_ar1),
built on the white deviate of tests/host_forcing_noise.py: member ``g`` (its index in the whole ensemble) is forced at forcing-axis
index ``t`` by F'_t = F_t + e_t with

    c    = sqrt(1 - phi*phi)          (three roundings)
    s_e  = sigma * c
    e_0  = sigma * z(seed, g, 0)
    e_t  = (phi * e_{t-1}) + (s_e * z(seed, g, t))      t >= 1

-- every operation an IEEE f64 operation rounded on its own (numpy does not fuse).  e is a pure function of
(seed, sigma, phi, g, t).  ``phi == 0`` is the white setting and delegates to the white functions: the formula's 0 * e term would
change signed zeros at sigma == 0.

``oracle_run_red`` gives each member's series to the CPU oracle's plain two-layer run as a scenario of its own: the reference of
every value test of tests/test_gpu_forcing_noise_red.py.  Pure numpy; no product code."""
import numpy as np

from tests import host_forcing_noise as hn


def red_noise(seed, g, T, sigma, phi):
    """e [len(g)][T] of the members with global ids ``g`` at forcing-axis indices 0 .. T-1 (phi == 0: sigma * z)."""
    g = np.atleast_1d(np.asarray(g, dtype=np.uint64))
    z = hn.noise(seed, g[:, None], np.arange(T, dtype=np.uint64)[None, :])
    sigma, phi = np.float64(sigma), np.float64(phi)
    if phi == 0.0:
        return sigma * z
    one = np.float64(1.0)
    c = np.sqrt(one - phi * phi)
    s_e = sigma * c
    e = np.empty_like(z)
    if T > 0:
        e[:, 0] = sigma * z[:, 0]
    for t in range(1, T):
        e[:, t] = (phi * e[:, t - 1]) + (s_e * z[:, t])
    return e


def noisy_forcing_red(F, sigma, phi, seed, member_offset=0):
    """``F`` [N][T], the members' noise-free series over the whole forcing axis -> F + e, [N][T]."""
    if np.float64(phi) == 0.0:
        return hn.noisy_forcing(F, sigma, seed, member_offset)
    F = np.asarray(F, dtype=np.float64)
    N, T = F.shape
    e = red_noise(seed, np.arange(N, dtype=np.uint64) + np.uint64(member_offset), T, sigma, phi)
    with np.errstate(all="ignore"):
        return F + e


def oracle_run_red(orc, bounds, params6, F, sigma, phi, seed, member_offset=0, source=0, ts0=0.0, td0=0.0, **kw):
    """(Ts, Td) [T][N] of the CPU oracle (oracle.cbind): member i runs the plain two-layer model under its own host-formed red-noise
    series, scenario i of N.  ``F`` [N][T] is the members' noise-free forcing (one shared row repeated, or a mix sum)."""
    if np.float64(phi) == 0.0:
        return hn.oracle_run(orc, bounds, params6, F, sigma, seed, member_offset, source, ts0, td0, **kw)
    params6 = np.asarray(params6, dtype=np.float64)
    N = params6.shape[1]
    Fn = noisy_forcing_red(F, sigma, phi, seed, member_offset)
    return orc.two_layer_run(bounds, params6[:6], Fn, ts0, td0, scen=np.arange(N, dtype=np.int32), source=source, **kw)
