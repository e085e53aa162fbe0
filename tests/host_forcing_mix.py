"""Host restatement of the forcing a two-layer MIX ensemble forms per member (include/rscm_gpu.h, rscm_ens_create_mix): with K
component rows per scenario and the members' coefficients in parameter rows 6 .. 6+K-1,

    F = S[s][0][n] * c_0[i];   F = F + S[s][k][n] * c_k[i]   for k = 1 .. K-1, in that order,

every product and sum an IEEE f64 operation rounded on its own (numpy ufuncs do not fuse), NaN and Inf propagating, no row
skipped.  ``oracle_run`` gives each member's series to the CPU oracle's plain two-layer run as a scenario of its own: the
reference of every value test of tests/test_gpu_forcing_mix.py.  Pure numpy; no product code."""
import numpy as np


def mix_forcing(S, coeff, scen=None):
    """``S`` [n_scen][K][T] (or one scenario's [K][T]), ``coeff`` [K][N], ``scen`` [N] or None -> the members' series [N][T]."""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim == 2:
        S = S[None]
    coeff = np.asarray(coeff, dtype=np.float64)
    K, N = coeff.shape
    assert S.shape[1] == K
    scen = np.zeros(N, dtype=np.int64) if scen is None else np.asarray(scen, dtype=np.int64)
    with np.errstate(all="ignore"):
        F = S[scen, 0, :] * coeff[0][:, None]
        for k in range(1, K):
            F = F + S[scen, k, :] * coeff[k][:, None]
    return F


def mix_forcing_loop(S, coeff, scen=None):
    """The same in a bare Python loop over members, years and components (Python floats are IEEE f64, one rounding per operator)."""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim == 2:
        S = S[None]
    coeff = np.asarray(coeff, dtype=np.float64)
    K, N = coeff.shape
    T = S.shape[2]
    out = np.empty((N, T))
    for i in range(N):
        s = 0 if scen is None else int(scen[i])
        for n in range(T):
            f = float(S[s, 0, n]) * float(coeff[0, i])
            for k in range(1, K):
                f = f + float(S[s, k, n]) * float(coeff[k, i])
            out[i, n] = f
    return out


def oracle_run(orc, bounds, params, S, scen=None, source=0, ts0=0.0, td0=0.0, **kw):
    """(Ts, Td) [T][N] of the CPU oracle (oracle.cbind) for a mix ensemble with parameter block ``params`` [6+K][N]: member i
    runs the plain two-layer model under its own host-formed series, scenario i of N."""
    params = np.asarray(params, dtype=np.float64)
    N = params.shape[1]
    F = mix_forcing(S, params[6:], scen)
    return orc.two_layer_run(bounds, params[:6], F, ts0, td0, scen=np.arange(N, dtype=np.int32), source=source, **kw)
