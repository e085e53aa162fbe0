"""Host restatement of the per-member forcing noise of a two-layer ensemble (include/rscm_gpu.h, rscm_ens_set_forcing_noise_members),
built on the white deviate of tests/host_forcing_noise.py: member i of the handle has the global id ``g = member_offset + i``, its own
``sigma_i`` and ``phi_i`` (two parameter rows), and is forced at forcing-axis index ``t`` by F'_t = F_t + e_t with

    c_i  = sqrt(1 - phi_i*phi_i)          (three roundings)
    s_i  = sigma_i * c_i
    e_0  = sigma_i * z(seed, g, 0)
    e_t  = (phi_i * e_{t-1}) + (s_i * z(seed, g, t))      t >= 1

-- every operation an IEEE f64 operation rounded on its own (numpy does not fuse).  This is the red formula of
tests/host_forcing_noise_red.py and it is used for EVERY member, ``phi_i == 0`` included: nothing delegates to the white
functions here, so such a member gets the white values with, at most, another sign of a zero.  Nothing validates the rows: NaN, Inf
and ``|phi_i| > 1`` (the square root of a negative number) give that member NaN from the formula itself.

``oracle_run_members`` gives each member's series to the CPU oracle's plain two-layer run as a scenario of its own: the reference
of every value test of tests/test_gpu_forcing_noise_members.py.  Pure numpy; no product code."""
import numpy as np

from tests import host_forcing_noise as hn


def member_noise(seed, g, T, sigma, phi):
    """e [len(g)][T] of the members with global ids ``g``, amplitudes ``sigma`` [len(g)] and persistences ``phi`` [len(g)]."""
    g = np.atleast_1d(np.asarray(g, dtype=np.uint64))
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), g.shape)
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), g.shape)
    z = hn.noise(seed, g[:, None], np.arange(T, dtype=np.uint64)[None, :])
    with np.errstate(all="ignore"):
        c = np.sqrt(np.float64(1.0) - phi * phi)
        s = sigma * c
        e = np.empty_like(z)
        if T > 0:
            e[:, 0] = sigma * z[:, 0]
        for t in range(1, T):
            e[:, t] = (phi * e[:, t - 1]) + (s * z[:, t])
    return e


def noisy_forcing_members(F, sigma, phi, seed, member_offset=0):
    """``F`` [N][T], the members' noise-free series over the whole forcing axis -> F + e, [N][T]."""
    F = np.asarray(F, dtype=np.float64)
    N, T = F.shape
    e = member_noise(seed, np.arange(N, dtype=np.uint64) + np.uint64(member_offset), T, sigma, phi)
    with np.errstate(all="ignore"):
        return F + e


def oracle_run_members(orc, bounds, params6, F, sigma, phi, seed, member_offset=0, source=0, ts0=0.0, td0=0.0, **kw):
    """(Ts, Td) [T][N] of the CPU oracle (oracle.cbind): member i runs the plain two-layer model under its own host-formed series,
    scenario i of N.  ``F`` [N][T] is the members' noise-free forcing (one shared row repeated, or a mix sum); ``sigma`` and ``phi``
    [N] are the two parameter rows."""
    params6 = np.asarray(params6, dtype=np.float64)
    N = params6.shape[1]
    Fn = noisy_forcing_members(F, sigma, phi, seed, member_offset)
    return orc.two_layer_run(bounds, params6[:6], Fn, ts0, td0, scen=np.arange(N, dtype=np.int32), source=source, **kw)
