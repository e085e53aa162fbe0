#!/usr/bin/env python3
"""Division by a constant in two instructions (rscm_amd/csrc/pair_div_verdict.hpp, rk4_device.hpp pair_div): the argument, and its
check in integer arithmetic.

    zh = RN(1/d)     zl = RN(1/d - zh)          once per divisor          (zl may be moved k ulps: the "variant" constants)
    t  = RN(n zl)    q  = RN(n zh + t)          per division

Precision p (53 for f64), everything normal; a power of two moves every quantity exactly, so take d = Y 2^(1-p) and n = X 2^(1-p) in
[1, 2) with integer significands X, Y in [2^(p-1), 2^p).

The error.  1/d lies in (1/2, 1], where doubles are 2^-p apart: |1/d - zh| <= 2^-(p+1).  Rounding is monotone and 2^-(p+1) is a
double, so |zl| <= 2^-(p+1), an ulp of zl is at most 2^-2p, and |1/d - zh - zl| <= 2^-(2p+1) (half an ulp of zl), plus k 2^-2p when zl
is moved k ulps.  |t - n zl| <= 2^-p |n zl| <= |n| 2^-(2p+1) (1 + k 2^(1-p)).  The fma forms n zh + t exactly before it rounds, so

    n zh + t = n/d + e,     |e| <= |n| 2^-2p (1 + k) (1 + 2^-p)                                                     (1)

The boundaries.  q = RN(n zh + t) and RN(n/d) differ only if a rounding boundary of the quotient's binade -- a midpoint
(2Q + 1) / 2^s of two neighbouring doubles, s = p for X >= Y (quotient in [1, 2)) and s = p + 1 for X < Y (quotient in (1/2, 1)) --
lies between n/d and the sum or on the sum.  X/Y is never such a midpoint itself (2^s X = (2Q + 1) Y: the left side has at least p
trailing zero bits and 2Q + 1 is odd, so Y would need p of them, and 0 < Y < 2^p has fewer), so

    X/Y - (2Q + 1)/2^s = j / (2^s Y),      j = 2^s X - (2Q + 1) Y  a non-zero integer,

and a failure needs |j| / (2^s Y) <= |e|, that is with (1) and n = X 2^(1-p):

    |j| <= 2^s X Y 2^(1-3p) (1 + k)(1 + 2^-p) < 2^(s - p + 1) (1 + k)         since X Y <= (2^p - 1)^2                            (2)

((2^p - 1)^2 (1 + 2^-p) = 2^2p (1 - 2^-p - 2^-2p + 2^-3p) < 2^2p.)  So J(s, k) = 2^(s - p + 1) (1 + k) - 1:

              k = 0    k = 1
    s = p       1        3
    s = p + 1   3        7

The header forms its candidates with kJ = 8 for both s: a superset, and every candidate is tried.  Given s and j, 2^s X = j (mod Y)
is a linear congruence in X (candidates() below restates how the header solves it); a divisor whose candidates all give the IEEE
quotient is safe for every numerator of the window.

The check.  exhaustive(p) tries EVERY divisor against EVERY numerator at precision p, for the constants as defined and for zl's two
neighbours, and reports each failure with its (s, |j|): every one must lie within J(s, k) -- and lowering a J by one where a failure
sits on it leaves that failure uncovered.  verdict() restates the header at any precision in integers.

Run as a program: prints the J table, the exhaustive summary at 8, 9 and 10 bits, and, with --unsafe N, N divisors of the
benchmark's ranges whose constants as defined fail, each with a failing numerator (tests/golden/pair_div_unsafe.json).
"""
import json
import random
import struct
import sys


# ------------------------------------------------------------------------------------------------------------------ integer floats
# A value is (m, e): m 2^e with m an integer (any sign, any size); rnd() brings it to p bits, round to nearest even, no exponent range.
def rnd(num, den, p):
    """RN_p(num / den) as (m, e) with |m| in [2^(p-1), 2^p), or (0, 0)."""
    if num == 0:
        return (0, 0)
    sign = -1 if (num < 0) != (den < 0) else 1
    num, den = abs(num), abs(den)
    sh = p + 2 + den.bit_length() - num.bit_length()   # the shifted quotient has p + 2 or p + 3 bits
    q, r = divmod(num << sh, den) if sh >= 0 else divmod(num, den << -sh)
    drop = q.bit_length() - p
    low, q, half = q & ((1 << drop) - 1), q >> drop, 1 << (drop - 1)
    if low > half or (low == half and (r != 0 or (q & 1))):
        q += 1
        if q == (1 << p):
            q >>= 1
            drop += 1
    return (sign * q, drop - sh)


def mul(a, b, p):
    return rnd_pow2(a[0] * b[0], a[1] + b[1], p)


def rnd_pow2(m, e, p):
    """RN_p(m 2^e)."""
    r = rnd(m, 1, p)
    return (r[0], r[1] + e) if r[0] else r


def fma(a, b, c, p):
    """RN_p(a b + c), the sum formed exactly."""
    pe = a[1] + b[1]
    pm = a[0] * b[0]
    if c[0] == 0:
        return rnd_pow2(pm, pe, p)
    lo = min(pe, c[1])
    return rnd_pow2((pm << (pe - lo)) + (c[0] << (c[1] - lo)), lo, p)


def step_ulps(z, k, p):
    """z moved one ulp away from zero (k = +1) or towards it (k = -1), as the integer representation +- 1 does; z non-zero."""
    m, e = z
    s = -1 if m < 0 else 1
    m = abs(m) + k
    if m == (1 << p):
        return (s * (1 << (p - 1)), e + 1)
    if m < (1 << (p - 1)):     # the binade below: half the ulp
        return (s * ((1 << p) - 1), e - 1)
    return (s * m, e)


# ------------------------------------------------------------------------------------------------------------------ the constants
def constants(Y, p, k=0):
    """(zh, zl) for d = Y 2^(1-p); zl moved k ulps in magnitude (k = 0: as defined)."""
    one = 1 << (p - 1)
    zh = rnd(one, Y, p)                         # d = Y / one
    # 1/d - zh = (one - Y zh) / Y: formed exactly, rounded once
    zm, ze = zh
    num = (one << -ze) - Y * zm                 # (one - Y zh) 2^-ze, an integer (ze < 0)
    zl = rnd(num, Y << -ze, p)
    if k and zl[0]:
        zl = step_ulps(zl, k, p)
    return zh, zl


def quotient(X, zh, zl, p):
    n = (X, 1 - p)
    return fma(n, zh, mul(n, zl, p), p)


def ieee(X, Y, p):
    return rnd(X, Y, p)


def J(s_minus_p, k):
    """The bound (2) of the module text: a failure with zl moved k ulps has |j| <= J."""
    return (1 << (s_minus_p + 1)) * (1 + abs(k)) - 1


def j_of(X, Y, p):
    """(s - p, j) of the midpoint nearest X/Y in the quotient's binade."""
    s = p if X >= Y else p + 1
    r = ((X << s) - Y) % (2 * Y)                # 2^s X - (2Q + 1) Y over all Q: residues mod 2Y, shifted by Y
    j = r if r <= Y else r - 2 * Y
    return s - p, j


# ------------------------------------------------------------------------------------------------------------------ the header's search
K_J = 8
MAX_TRAILING = 3
VARIANT_STEPS = (0, 1, -1)   # the header's order: zl, zl + ulp, zl - ulp
NUM_LO, SURFACE_NUM_FLOOR = -902, -946   # the header's kNumLo and kSurfaceNumFloor (tests/test_pair_div_proof.py holds them to it)


def candidates(Y, p, bound=K_J):
    """The numerator significands the header tries for Y, by its method: Y = 2^c Yo; no candidate for c > MAX_TRAILING; else for
    s in {p, p + 1} and j = j' 2^c, 0 < |j| <= bound: X = j' inv(2^(s - c)) (mod Yo), every representative in [2^(p-1), 2^p)."""
    c = 0
    while c <= MAX_TRAILING and not (Y >> c) & 1:
        c += 1
    if c > MAX_TRAILING:
        return []
    Yo = Y >> c
    out = []
    h = 1
    for _ in range(p - c):
        h = (h + Yo) >> 1 if h & 1 else h >> 1
    for s in (p, p + 1):
        if s == p + 1:
            h = (h + Yo) >> 1 if h & 1 else h >> 1
        acc = 0
        for jp in range(1, bound + 1):
            acc += h
            if acc >= Yo:
                acc -= Yo
            if (jp << c) > bound:
                continue
            for x0 in (acc, (Yo - acc) % Yo):
                X = x0
                while X < (1 << p):
                    if X >= (1 << (p - 1)):
                        out.append(X)
                    X += Yo
    return out


def candidates_by_definition(Y, p, bound=K_J):
    """Every X with 0 < |2^s X - (2Q + 1) Y| <= bound for some Q and s in {p, p + 1}, X >= Y for s = p and X < Y for s = p + 1:
    by looking at every X (reduced precision only)."""
    out = []
    for X in range(1 << (p - 1), 1 << p):
        _, j = j_of(X, Y, p)
        if abs(j) <= bound:
            out.append(X)
    return out


def verdict(Y, p, bound=K_J, min_zl_exp=None):
    """(variant, zh, zl, failing X of the constants as defined or None): the header's verdict for d = Y 2^(1-p).  min_zl_exp: the
    least binary exponent a tried non-zero zl may have (the header's rule for the window's lower edge), None: no such rule."""
    cand = candidates(Y, p, bound)
    consts = [constants(Y, p, k) for k in VARIANT_STEPS]
    ok = [True] * len(consts)
    if min_zl_exp is not None and consts[0][1][0]:
        ok = [abs(zl[0]).bit_length() - 1 + zl[1] >= min_zl_exp for _, zl in consts]
    fail0 = None
    for X in cand:
        ref = ieee(X, Y, p)
        for v, (zh, zl) in enumerate(consts):
            if quotient(X, zh, zl, p) != ref:
                ok[v] = False
                if v == 0 and fail0 is None:
                    fail0 = X
    for v in range(len(consts)):
        if ok[v]:
            return v, consts[v][0], consts[v][1], fail0
    return -1, None, None, fail0


# ------------------------------------------------------------------------------------------------------------------ exhaustive
def exhaustive(p):
    """Every divisor against every numerator at precision p.  Returns
    failures[k] = list of (X, Y, s - p, |j|) for zl moved k ulps, k in VARIANT_STEPS."""
    failures = {k: [] for k in VARIANT_STEPS}
    lo, hi = 1 << (p - 1), 1 << p
    for Y in range(lo, hi):
        refs = [ieee(X, Y, p) for X in range(lo, hi)]
        for k in VARIANT_STEPS:
            zh, zl = constants(Y, p, k)
            if k and zl[0] == 0:
                continue
            for X in range(lo, hi):
                if quotient(X, zh, zl, p) != refs[X - lo]:
                    sp, j = j_of(X, Y, p)
                    failures[k].append((X, Y, sp, abs(j)))
    return failures


def uncovered(failures, k, bounds):
    """The failures of variant k that a candidate list with |j| <= bounds[s - p] would miss."""
    return [f for f in failures[k] if f[3] > bounds[f[2]]]


def superset_holds(p, bound=K_J):
    """The header's enumeration yields every numerator within `bound` of a midpoint, for every divisor of precision p."""
    for Y in range(1 << (p - 1), 1 << p):
        if not set(candidates_by_definition(Y, p, bound)) <= set(candidates(Y, p, bound)):
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------ f64
def significand(d):
    """(Y, exponent) of a positive normal double: d = Y 2^(exponent - 52)."""
    b = struct.unpack("<Q", struct.pack("<d", d))[0]
    return (b & ((1 << 52) - 1)) | (1 << 52), ((b >> 52) & 0x7FF) - 1023


def to_double(v, exponent=0):
    """The double (m, e) 2^exponent."""
    m, e = v
    return float(m) * 2.0 ** (e + exponent) if m else 0.0


def verdict_f64(d, num_lo=NUM_LO):
    """(variant, zh, zl) as doubles for the divisor d and the numerator window's lower edge 2^num_lo, as pair_div_verdict.hpp's
    verdict() states them; variant -1: (-1, 0.0, 0.0)."""
    Y, ex = significand(d)
    v, zh, zl, _ = verdict(Y, 53, min_zl_exp=-1022 - num_lo + ex)
    if v < 0:
        return -1, 0.0, 0.0
    return v, to_double(zh, -ex), to_double(zl, -ex)


def find_unsafe(count, seed=1, ranges=((5.0, 15.0), (50.0, 200.0))):
    """`count` divisors of the benchmark's heat-capacity ranges whose constants as defined fail, with a failing numerator in [1, 2),
    the variant that rescues them (-1: none) and the quotients' bits left to the reader."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        lo, hi = ranges[len(out) % len(ranges)]
        d = rng.uniform(lo, hi)
        Y, _ = significand(d)
        v, _, _, fail = verdict(Y, 53)
        if fail is not None:
            out.append({"divisor": d.hex(), "numerator": (float(fail) * 2.0 ** -52).hex(), "variant": v})
    return out


def main(argv):
    print("J(s, k):  s = p: %d (k = 0), %d (|k| = 1);  s = p + 1: %d, %d;  the header tries |j| <= %d" % (J(0, 0), J(0, 1), J(1, 0), J(1, 1), K_J))
    if "--unsafe" in argv:
        n = int(argv[argv.index("--unsafe") + 1])
        json.dump(find_unsafe(n), sys.stdout, indent=1)
        print()
        return 0
    for p in (8, 9, 10):
        f = exhaustive(p)
        assert superset_holds(p)
        for k in VARIANT_STEPS:
            bounds = {0: J(0, k), 1: J(1, k)}
            worst = {sp: max([x[3] for x in f[k] if x[2] == sp], default=0) for sp in (0, 1)}
            bad = uncovered(f, k, bounds)
            print("p = %2d  k = %+d: %5d failing pairs in %4d divisors; largest |j|: s = p %d (J %d), s = p + 1 %d (J %d); uncovered %d"
                  % (p, k, len(f[k]), len({x[1] for x in f[k]}), worst[0], bounds[0], worst[1], bounds[1], len(bad)))
            assert not bad
        lo, hi = 1 << (p - 1), 1 << p
        unsafe = [Y for Y in range(lo, hi) if verdict(Y, p)[0] < 0]
        print("p = %2d: divisors no variant rescues: %d of %d" % (p, len(unsafe), hi - lo))
    print("pair_div proof ok")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
