"""Host restatement of the device Latin hypercube through the rows' priors (include/rscm_gpu.h, rscm_ens_sample_lhs_priors;
rscm_amd/csrc/ensemble_ops.hip, lhs_priors_kernel): the uniform hypercube of tests/host_sampler.py, then per row

    kind 0 (uniform)            x = a + u (b - a)
    kind 1, 2 (normal, log)     t = p0 + u (p1 - p0), moved into [2^-1022, 1 - 2^-53];  z = Q(t), negated under PRIOR_REFLECT;
                                y = a + b z;  x = y or exp(y);  x below lo becomes lo, x above hi becomes hi

with Q = normal_from_p, AS241 PPND16 on a double in the order of noise::normal_from_p (rscm_amd/csrc/forcing_noise.hpp): the
polynomials and the written-out logarithm are those of tests/host_forcing_noise.py, whose normal_from_k it equals bit for bit on
t = (2k + 1) 2^-53.  Everything up to y is f64 + - * / and sqrt rounded one by one, so it predicts the device's bits; the exponential of
a log-normal row is numpy's here and the device library's there (within 2 ulp of each other's true value, not the same bits), which
is why lhs_priors_matrix also returns y.  Pure numpy; no product code."""
import numpy as np

from tests.host_forcing_noise import A, B, C, D, E, F, _horner, ln_small
from tests.host_sampler import feistel_perm, lhs_half_bits, lhs_keys, lhs_matrix

PRIOR_UNIFORM, PRIOR_NORMAL, PRIOR_LOGNORMAL, PRIOR_REFLECT = 0, 1, 2, 0x100   # RSCM_PRIOR_* of include/rscm_gpu.h
T_MIN = 2.0 ** -1022
T_MAX = 1.0 - 2.0 ** -53


def normal_from_p(t):
    """Q(t) for doubles t in [T_MIN, T_MAX].  Both branches are evaluated for every element and selected, as the device does."""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    q = t - 0.5
    central = np.abs(q) <= 0.425
    with np.errstate(all="ignore"):
        r = 0.180625 - q * q
        z_central = (_horner(A, r) * q) / _horner(B, r)
        p = np.where(q < 0.0, t, 1.0 - t)
        p = np.where(central, 0.0625, p)   # (the tail's arithmetic on a harmless argument where it is not selected)
        rt = np.sqrt(-ln_small(p))
        r1 = rt - 1.6
        r2 = rt - 5.0
        z_mid = _horner(C, r1) / _horner(D, r1)
        z_far = _horner(E, r2) / _horner(F, r2)
        z_tail = np.where(rt <= 5.0, z_mid, z_far)
        z_tail = np.where(q < 0.0, -z_tail, z_tail)
    return np.where(central, z_central, z_tail)


def lhs_strata(seed: int, j: int, member_offset: int, n_local: int, n_total: int) -> np.ndarray:
    """The stratum of row j for members [member_offset, member_offset + n_local) of n_total."""
    g = np.arange(member_offset, member_offset + n_local, dtype=np.uint64)
    k0, k1 = lhs_keys(seed, j)
    return feistel_perm(g, n_total, lhs_half_bits(n_total), k0, k1)


def lhs_priors_matrix(seed: int, table, member_offset: int, n_local: int, n_total: int, with_y: bool = False):
    """[P][n_local] float64: what rscm_ens_sample_lhs_priors writes for members [member_offset, member_offset + n_local) of an
    ensemble of n_total under table = (kind, a, b, p0, p1, lo, hi), in the kernel's expression order.  with_y: also the matrix of
    y = a + b z (the argument of the exponential on a log-normal row; x itself on every other row)."""
    kind, a, b, p0, p1, lo, hi = (np.asarray(v) for v in table)
    P = len(kind)
    U = lhs_matrix(seed, np.zeros(P), np.ones(P), member_offset, n_local, n_total)   # 0 + u * (1 - 0) is u, exactly
    out = lhs_matrix(seed, a, b, member_offset, n_local, n_total)                    # the uniform rows; the others are replaced
    ys = out.copy()
    for j in range(P):
        family = int(kind[j]) & ~PRIOR_REFLECT
        if family == PRIOR_UNIFORM:
            continue
        u = U[j]
        t = p0[j] + u * (p1[j] - p0[j])
        t = np.where(t < T_MIN, T_MIN, t)
        t = np.where(t > T_MAX, T_MAX, t)
        z = normal_from_p(t)
        if int(kind[j]) & PRIOR_REFLECT:
            z = -z
        y = a[j] + b[j] * z
        with np.errstate(over="ignore"):
            x = np.exp(y) if family == PRIOR_LOGNORMAL else y
        x = np.where(x < lo[j], lo[j], x)
        out[j] = np.where(x > hi[j], hi[j], x)
        ys[j] = y
    return (out, ys) if with_y else out
