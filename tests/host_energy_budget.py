"""The energy-budget diagnostics' definition restated in numpy (include/rscm_gpu.h, "energy-budget diagnostics"): per member and
row, with Ts, Td the stored rows, p the parameter rows 0 .. 5 and F the member's forcing,
    ee = p2 * p3;  d = Ts - Td;  u = p1 * Ts;  lam = p0 - u;  R = lam * Ts;  X = ee * d;  H = p3 * d
    g = F - R;  g = g - X;  N = g + H;   y = scale * q
elementwise in float64, every line one IEEE operation.  F comes from the restatements the forcing already has
(host_forcing_mix, host_forcing_noise, host_forcing_noise_red, host_forcing_noise_members).  Nothing else."""
import numpy as np

from tests import host_forcing_mix as hm
from tests import host_forcing_noise as hn
from tests import host_forcing_noise_members as hnm
from tests import host_forcing_noise_red as hnr

QUANTITIES = ("forcing", "response", "deep_uptake", "imbalance")


def member_forcing(table, P, scen=None, n_comp=0, noise=None, member_offset=0):
    """[N][T]: the forcing of every member at every forcing-axis index.  ``table``: [S][T] (or [T]) of a plain handle, [S][K][T]
    (or [K][T]) of a mix handle with ``n_comp`` = K, whose coefficients are rows 6 .. 6 + K - 1 of ``P``.  ``noise``: None,
    ("white", seed, sigma), ("red", seed, sigma, phi) or ("members", seed) -- the last reads rows 6 + K and 7 + K of ``P``."""
    P = np.asarray(P, dtype=np.float64)
    N = P.shape[1]
    table = np.asarray(table, dtype=np.float64)
    if n_comp:
        F = hm.mix_forcing(table, P[6:6 + n_comp], scen)
    else:
        table = table[None] if table.ndim == 1 else table
        F = table[np.zeros(N, dtype=np.int64) if scen is None else np.asarray(scen, dtype=np.int64)]
    if noise is None:
        return np.array(F, dtype=np.float64)
    if noise[0] == "white":
        return hn.noisy_forcing(F, noise[2], noise[1], member_offset)
    if noise[0] == "red":
        return hnr.noisy_forcing_red(F, noise[2], noise[3], noise[1], member_offset)
    if noise[0] == "members":
        return hnm.noisy_forcing_members(F, P[6 + n_comp], P[7 + n_comp], noise[1], member_offset)
    raise ValueError(noise)


def terms(Ts, Td, P, F):
    """The four quantities, [R][N] each, of the rows ``Ts``, ``Td`` [R][N] under the forcing ``F`` [R][N] (row r: the forcing of the
    step out of that row)."""
    Ts, Td, F = (np.asarray(x, dtype=np.float64) for x in (Ts, Td, F))
    p = np.asarray(P, dtype=np.float64)
    with np.errstate(all="ignore"):
        ee = p[2] * p[3]
        d = Ts - Td
        u = p[1] * Ts
        lam = p[0] - u
        R = lam * Ts
        X = ee * d
        H = p[3] * d
        g = F - R
        g = g - X
        N = g + H
    return {"forcing": F, "response": R, "deep_uptake": H, "imbalance": N}


def budget(quantity, Ts, Td, P, F, scale=1.0):
    """``scale * q`` [R][N]: multiplied even by 1.0."""
    with np.errstate(all="ignore"):
        return np.float64(scale) * terms(Ts, Td, P, F)[quantity]


def imbalance_wrong_association(Ts, Td, P, F):
    """(F - X) - R + H: what the definition is NOT (the same terms, the two subtractions in the other order)."""
    Ts, Td, F = (np.asarray(x, dtype=np.float64) for x in (Ts, Td, F))
    p = np.asarray(P, dtype=np.float64)
    with np.errstate(all="ignore"):
        ee = p[2] * p[3]
        d = Ts - Td
        R = (p[0] - p[1] * Ts) * Ts
        X = ee * d
        H = p[3] * d
        return ((F - X) - R) + H


def rows_forcing(F_axis, t_begin, t_end, t_stride, source_offset=0):
    """[R][N]: the forcing of the rows t_begin, t_begin + t_stride, ... < t_end from ``F_axis`` [N][T]: index t + source_offset."""
    idx = np.arange(t_begin, t_end, t_stride) + source_offset
    return np.ascontiguousarray(np.asarray(F_axis)[:, idx].T)
