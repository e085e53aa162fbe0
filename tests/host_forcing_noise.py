"""Host restatement of the seeded forcing noise of a two-layer ensemble (include/rscm_gpu.h, rscm_ens_set_forcing_noise): member
``g`` (its index in the whole ensemble) is forced at forcing-axis index ``t`` by

    F' = F + sigma * z(seed, g, t)

-- the product and the sum each an IEEE f64 operation rounded on its own.  z is a standard normal deviate that is a pure function
of (seed, g, t):

* Philox4x32-10 with counter (lo32(g), hi32(g), t >> 1, NOISE_STREAM_TAG) and key (lo32(seed), hi32(seed)); even t takes words
  (0, 1) as (lo, hi), odd t words (2, 3);
* k = ((hi << 32) | lo) >> 12, u = (2k + 1) * 2^-53 in (0, 1), q = u - 0.5 (both exact);
* Wichura's AS241 PPND16 in Horner form; its tails need ln(p) for p in [2^-53, 0.075], written out in + - * / so that numpy, a
  bare Python loop and the device form the same bits: p = m 2^e, m in (1/sqrt 2, sqrt 2], s = (m - 1)/(m + 1), w = s s,
  ln m = 2s + 2s (w P(w)) with P the odd series 1/3 + w/5 + ... + w^11/25, ln p = e ln2 + ln m.

``oracle_run`` gives each member's series to the CPU oracle's plain two-layer run as a scenario of its own: the reference of every
value test of tests/test_gpu_forcing_noise.py.  Pure numpy; no product code."""
import numpy as np

from tests.host_sampler import philox4x32_10

NOISE_STREAM_TAG = 0x4E5A   # RSCM_NOISE_STREAM_TAG of include/rscm_gpu.h ("NZ")
M32 = np.uint64(0xFFFFFFFF)

# AS241 PPND16 (Wichura 1988), highest degree first
A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
     1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
     5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
     3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
     6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
     2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
     1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)

SQRT2 = 1.4142135623730951
LN2 = 0.6931471805599453
LN_ODD = tuple(1.0 / (2 * j + 1) for j in range(12, 0, -1))   # 1/25, 1/23, ..., 1/3: each the f64 nearest the fraction


def _horner(c, r):
    p = c[0] * r + c[1]
    for x in c[2:]:
        p = p * r + x
    return p


def ln_small(p):
    """ln(p) for p in [2^-53, 0.075] (normal f64), in + - * / only."""
    p = np.asarray(p, dtype=np.float64)
    bits = p.view(np.uint64)
    e = (bits >> np.uint64(52)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > SQRT2
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    w = s * s
    P = np.full_like(w, LN_ODD[0])
    for c in LN_ODD[1:]:
        P = P * w + c
    s2 = s + s
    r = s2 + s2 * (w * P)
    return e.astype(np.float64) * LN2 + r


def uniform_from_k(k):
    """u = (2k + 1) 2^-53 for a 52-bit k: exact, in (0, 1), symmetric about 1/2."""
    k = np.asarray(k, dtype=np.uint64)
    return (np.uint64(2) * k + np.uint64(1)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normal_from_k(k):
    """The deviate of the 52-bit integer(s) k.  Both branches are evaluated for every element and selected, as the device does."""
    u = np.atleast_1d(uniform_from_k(k))
    q = u - 0.5
    with np.errstate(all="ignore"):
        r = 0.180625 - q * q
        z_central = (_horner(A, r) * q) / _horner(B, r)
        p = np.where(q < 0.0, u, 1.0 - u)
        p = np.where(np.abs(q) <= 0.425, 0.0625, p)   # (the tail's arithmetic on a harmless argument where it is not selected)
        rt = np.sqrt(-ln_small(p))
        r1 = rt - 1.6
        r2 = rt - 5.0
        z_mid = _horner(C, r1) / _horner(D, r1)
        z_far = _horner(E, r2) / _horner(F, r2)
        z_tail = np.where(rt <= 5.0, z_mid, z_far)
        z_tail = np.where(q < 0.0, -z_tail, z_tail)
    return np.where(np.abs(q) <= 0.425, z_central, z_tail)


def normal_from_k_loop(k):
    """The same for one k in bare Python floats and integers, with real branches."""
    k = int(k)
    u = float(2 * k + 1) * 2.0 ** -53
    q = u - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        num = A[0] * r + A[1]
        den = B[0] * r + B[1]
        for a, b in zip(A[2:], B[2:]):
            num = num * r + a
            den = den * r + b
        return (num * q) / den
    p = u if q < 0.0 else 1.0 - u
    bits = int(np.float64(p).view(np.uint64))
    e = (bits >> 52) - 1023
    m = float(np.uint64((bits & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000).view(np.float64))
    if m > SQRT2:
        m, e = m * 0.5, e + 1
    s = (m - 1.0) / (m + 1.0)
    w = s * s
    P = LN_ODD[0]
    for c in LN_ODD[1:]:
        P = P * w + c
    s2 = s + s
    ln = float(e) * LN2 + (s2 + s2 * (w * P))
    r = float(np.sqrt(np.float64(-ln)))
    if r <= 5.0:
        r, cn, cd = r - 1.6, C, D
    else:
        r, cn, cd = r - 5.0, E, F
    num, den = cn[0] * r + cn[1], cd[0] * r + cd[1]
    for a, b in zip(cn[2:], cd[2:]):
        num = num * r + a
        den = den * r + b
    z = num / den
    return -z if q < 0.0 else z


def k52(seed, g, t, tag=NOISE_STREAM_TAG):
    """The 52-bit integer of (seed, g, t): broadcasts g against t."""
    g = np.asarray(g, dtype=np.uint64)
    t = np.asarray(t, dtype=np.uint64)
    g, t = np.broadcast_arrays(g, t)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c0, c1, c2, c3 = philox4x32_10(g & M32, g >> np.uint64(32), t >> np.uint64(1), tag, seed & 0xFFFFFFFF, seed >> 32)
    odd = (t & np.uint64(1)) == 1
    lo = np.where(odd, c2, c0)
    hi = np.where(odd, c3, c1)
    return ((hi << np.uint64(32)) | lo) >> np.uint64(12)


def noise(seed, g, t, tag=NOISE_STREAM_TAG):
    """z(seed, g, t), g and t broadcast against each other."""
    k = k52(seed, g, t, tag)
    return normal_from_k(k.ravel()).reshape(k.shape)


def noisy_forcing(F, sigma, seed, member_offset=0, tag=NOISE_STREAM_TAG):
    """``F`` [N][T], the members' noise-free series over the whole forcing axis -> F + sigma * z(seed, member_offset + i, t), [N][T]."""
    F = np.asarray(F, dtype=np.float64)
    N, T = F.shape
    z = noise(seed, (np.arange(N, dtype=np.uint64) + np.uint64(member_offset))[:, None], np.arange(T, dtype=np.uint64)[None, :], tag)
    with np.errstate(all="ignore"):
        return F + np.float64(sigma) * z


def oracle_run(orc, bounds, params6, F, sigma, seed, member_offset=0, source=0, ts0=0.0, td0=0.0, **kw):
    """(Ts, Td) [T][N] of the CPU oracle (oracle.cbind): member i runs the plain two-layer model under its own host-formed noisy
    series, scenario i of N.  ``F`` [N][T] is the members' noise-free forcing (one shared row repeated, or a mix sum)."""
    params6 = np.asarray(params6, dtype=np.float64)
    N = params6.shape[1]
    Fn = noisy_forcing(F, sigma, seed, member_offset)
    return orc.two_layer_run(bounds, params6[:6], Fn, ts0, td0, scen=np.arange(N, dtype=np.int32), source=source, **kw)


def _tail_r(k):
    """r = sqrt(-ln p) of the lower-tail integer(s) k (u < 1/2, p = u)."""
    return np.sqrt(-ln_small(uniform_from_k(k)))


def chosen_k():
    """52-bit integers that put every branch of the deviate in play: the ends (|z| = 8.2095...), the two next to u = 1/2, both
    sides of |q| = 0.425 in either half, and both sides of r = 5 (p near e^-25) in either half -- random draws do not reach r > 5."""
    top = (1 << 52) - 1
    ks = [0, 1, top - 1, top, 1 << 51, (1 << 51) - 1]
    # |q| <= 0.425  <=>  u >= 0.075 in the lower half: the first k inside the central branch (q is exact, so is the comparison)
    lo, hi = 0, 1 << 51   # lo outside, hi inside
    while hi - lo > 1:
        mid = (lo + hi) // 2
        inside = abs(float(uniform_from_k(mid)) - 0.5) <= 0.425
        lo, hi = (lo, mid) if inside else (mid, hi)
    ks += [lo - 1, lo, hi, hi + 1]
    # r > 5 for the smallest k: the last k of the far tail
    a, b = 0, 1 << 20     # a far, b near
    assert _tail_r(np.uint64(a))[()] > 5.0 >= _tail_r(np.uint64(b))[()]
    while b - a > 1:
        mid = (a + b) // 2
        a, b = (mid, b) if _tail_r(np.uint64(mid))[()] > 5.0 else (a, mid)
    ks += [a // 2, a - 1, a, b, b + 1, 2 * b]
    ks += [top - k for k in ks[6:]]
    return np.array(ks, dtype=np.uint64)
