"""Reference of the exact moments across members (include/rscm_gpu.h, rscm_ens_moment_sums), in Python integers and fractions.

Every term of every sum is a double (a value, or one IEEE product of two IEEE differences, formed here in numpy float64, which
never fuses), and every double is an integer multiple of 2^-1074, so a weighted sum of them is an exact Python int in units of
2^-1088, the accumulator's unit.  ``float(Fraction)`` rounds correctly, ties to even, so ``finish`` is the definition's RN(S / W).
The block layout is restated too (``term_block``, ``canonical``): device blocks are compared as integers, never limb by limb,
because deferred carries differ with the order of summation."""
import math
from fractions import Fraction

import numpy as np

LIMBS = 68
BLOCK = LIMBS + 1          # RSCM_MOMENT_BLOCK: the limbs, then the count of non-finite terms
UNIT_EXP = -1088           # limb k is in units of 2^(32 k - 1088)
MAX_VECTORS = 8
MAX_TERMS = 1 << 31


def fields(x: float):
    """(sign, mantissa, accumulator bit of the mantissa's lowest bit) of a finite double, from its raw fields."""
    bits = int(np.float64(x).view(np.uint64))
    e, frac = (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1)
    assert e != 0x7FF
    return bits >> 63, (frac if e == 0 else (1 << 52) + frac), max(e, 1) + 13


def term_value(x: float, w: int) -> int:
    """w * x in units of 2^-1088."""
    s, m, pos = fields(x)
    v = (w * m) << pos
    return -v if s else v


def term_block(x: float, w: int):
    """The 68 limb contributions of one term: w * mantissa cut into 32-bit digits at limb boundaries, each with the term's sign."""
    s, m, pos = fields(x)
    v = (w * m) << pos
    limbs = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(LIMBS)]
    assert v >> (32 * LIMBS) == 0
    return [-d for d in limbs] if s else limbs


def canonical(block) -> int:
    """sum limb_k 2^(32 k) of a block of 69 (the count is not part of it)."""
    assert len(block) == BLOCK
    return sum(int(block[k]) << (32 * k) for k in range(LIMBS))


def block_of(terms, w):
    """[69] Python ints of the terms (doubles) with weights w, by the limb scheme, in the order given."""
    out = [0] * BLOCK
    for x, wi in zip(np.asarray(terms, dtype=np.float64).tolist(), w):
        if not math.isfinite(x):
            out[LIMBS] += 1
            continue
        for k, d in enumerate(term_block(x, int(wi))):
            out[k] += d
    return out


def exact_sum(terms, w):
    """(sum of w * term over the finite terms in units of 2^-1088, number of non-finite terms): the canonical value and the count
    the device's block must have."""
    bits = np.asarray(terms, dtype=np.float64).view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    bad = e == 0x7FF
    frac = (bits & np.uint64((1 << 52) - 1)).astype(np.int64)
    mant = np.where(e == 0, frac, frac + (1 << 52))
    pos = np.maximum(e, 1) + 13
    neg = (bits >> np.uint64(63)).astype(bool)
    total = 0
    for m, p, s, b, wi in zip(mant.tolist(), pos.tolist(), neg.tolist(), bad.tolist(), w):
        if b:
            continue
        v = (int(wi) * m) << p
        total += -v if s else v
    return total, int(bad.sum())


def finish(value: int, n_bad: int, W: int) -> float:
    """RN(value * 2^-1088 / W); NaN with a non-finite term or without weight; a zero sum is +0.0."""
    if n_bad or W == 0:
        return math.nan
    if value == 0:
        return 0.0
    try:
        return float(Fraction(value, W << -UNIT_EXP))
    except OverflowError:
        return math.inf if value > 0 else -math.inf


def counted(X, groups=None, n_groups=None):
    """[G] boolean masks of the members counted in each group: listwise finite, and in the group."""
    X = np.asarray(X, dtype=np.float64)
    ok = np.isfinite(X).all(axis=0)
    if groups is None:
        return [ok]
    groups = np.asarray(groups)
    return [ok & (groups == g) for g in range(n_groups)]


def _weights(X, weights):
    n = np.asarray(X).shape[1]
    return [1] * n if weights is None else [int(v) for v in np.asarray(weights).tolist()]


def pair_terms(X, c, a, b):
    """p_i = (x_ia - c_a) * (x_ib - c_b): one IEEE subtraction each, one IEEE multiplication."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (X[a] - np.float64(c[a])) * (X[b] - np.float64(c[b]))


def sums(X, order, center=None, weights=None, groups=None, n_groups=None):
    """Per group (n, W, [(canonical value, count of non-finite terms) per block]) as Python ints, blocks in the order of
    rscm_ens_moment_sums.  A group with a non-finite centre has every term of every block counted as non-finite."""
    X = np.asarray(X, dtype=np.float64)
    K = X.shape[0]
    w = np.array(_weights(X, weights), dtype=object)
    out = []
    for g, ok in enumerate(counted(X, groups, n_groups)):
        idx = np.flatnonzero(ok)
        wg = w[idx].tolist()
        n, W = int(idx.size), int(sum(wg))
        Xg = X[:, idx]
        if order == 1:
            blocks = [exact_sum(Xg[a], wg) for a in range(K)]
        else:
            c = np.asarray(center, dtype=np.float64).reshape(-1, K)[g]
            if not np.isfinite(c).all():
                blocks = [(0, n) for a in range(K) for b in range(a, K)]
            else:
                blocks = [exact_sum(pair_terms(Xg, c, a, b), wg) for a in range(K) for b in range(a, K)]
        out.append((n, W, blocks))
    return out


def sums_array(X, order, center=None, weights=None, groups=None, n_groups=None) -> np.ndarray:
    """What ``Ensemble.moment_sums`` returns, formed by the limb scheme term by term: int64 [G][2 + B * 69]."""
    X = np.asarray(X, dtype=np.float64)
    K = X.shape[0]
    w = np.array(_weights(X, weights), dtype=object)
    rows = []
    for g, ok in enumerate(counted(X, groups, n_groups)):
        idx = np.flatnonzero(ok)
        wg = w[idx].tolist()
        row = [int(idx.size), int(sum(wg))]
        Xg = X[:, idx]
        if order == 1:
            for a in range(K):
                row += block_of(Xg[a], wg)
        else:
            c = np.asarray(center, dtype=np.float64).reshape(-1, K)[g]
            for a in range(K):
                for b in range(a, K):
                    if not np.isfinite(c).all():
                        row += [0] * LIMBS + [int(idx.size)]
                    else:
                        row += block_of(pair_terms(Xg, c, a, b), wg)
        rows.append(row)
    return np.array(rows, dtype=np.int64)


def array_sums(arr, K, order):
    """An int64 array [G][2 + B * 69] (the device's, or a sum of several) in the form of ``sums``: blocks as canonical integers."""
    arr = np.asarray(arr)
    B = K if order == 1 else K * (K + 1) // 2
    assert arr.shape[1] == 2 + B * BLOCK, arr.shape
    out = []
    for row in arr.tolist():
        blocks = [(canonical(row[2 + j * BLOCK:2 + (j + 1) * BLOCK]), row[2 + j * BLOCK + LIMBS]) for j in range(B)]
        out.append((row[0], row[1], blocks))
    return out


def corr_rules(cov):
    """sd and corr of one [K][K] covariance matrix by the rules of ``rscm_amd.ensemble.moments_dict``, element by element."""
    K = cov.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(np.diag(cov))
        corr = np.empty((K, K))
        for a in range(K):
            corr[a, a] = 1.0 if cov[a, a] > 0.0 else np.nan
            for b in range(a + 1, K):
                corr[a, b] = corr[b, a] = cov[a, b] / (sd[a] * sd[b])
    return sd, corr


def moments(X, weights=None, groups=None, n_groups=None, with_sums=False):
    """The reference of ``Ensemble.moments``: {"count", "weight", "mean", "cov", "sd", "corr"} with the group axis leading (of
    length 1 without groups), every mean and covariance the exact sum over W rounded once.  ``with_sums``: also the ``sums`` of
    order 1 and of order 2 about those means, which were formed on the way."""
    X = np.asarray(X, dtype=np.float64)
    K = X.shape[0]
    s1 = sums(X, 1, None, weights, groups, n_groups)
    mean = np.array([[finish(v, nb, W) for v, nb in blocks] for _, W, blocks in s1]).reshape(len(s1), K)
    s2 = sums(X, 2, mean, weights, groups, n_groups)
    cov = np.empty((len(s2), K, K))
    for g, (_, W, blocks) in enumerate(s2):
        it = iter(blocks)
        for a in range(K):
            for b in range(a, K):
                v, nb = next(it)
                cov[g, a, b] = cov[g, b, a] = finish(v, nb, W)
    sd = np.empty((len(s2), K))
    corr = np.empty((len(s2), K, K))
    for g in range(len(s2)):
        sd[g], corr[g] = corr_rules(cov[g])
    out = {"count": np.array([n for n, _, _ in s1], dtype=np.int64), "weight": np.array([W for _, W, _ in s1], dtype=np.int64),
           "mean": mean, "cov": cov, "sd": sd, "corr": corr}
    return (out, s1, s2) if with_sums else out


def same_bits(a, b) -> bool:
    """Doubles bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _block_from_value(v: int, rng=None):
    """A block whose canonical value is v: the plain base-2^32 digits with the sign, or (rng) the same value with carries deferred:
    limb k raised by r 2^32 and limb k + 1 lowered by r, for random r that keep every limb within +-2^62."""
    s, a = (-1 if v < 0 else 1), abs(v)
    limbs = [s * ((a >> (32 * k)) & 0xFFFFFFFF) for k in range(LIMBS)]
    assert a >> (32 * LIMBS) == 0
    if rng is not None:
        for k in range(LIMBS - 1):
            r = int(rng.integers(-(1 << 29), 1 << 29))
            limbs[k] += r << 32
            limbs[k + 1] -= r
    return limbs + [0]


def finish_cases(seed=5):
    """(name, block[69], divisor, expected double) for the finishing step: synthetic blocks with their Fraction results."""
    rng = np.random.default_rng(seed)
    dbl_max = float(np.finfo(np.float64).max)
    cases = []

    def add(name, block, W):
        cases.append((name, [int(x) for x in block], int(W), finish(canonical(block), block[LIMBS], W)))

    M = (1 << 52) + 12345                                                 # an even 53-bit mantissa
    for shift in (0, 14, 15, 700, 2000):
        add(f"tie down to even, shift {shift}", _block_from_value(((M << 1) | 1) << shift), 1)
        add(f"tie up to even, shift {shift}", _block_from_value((((M + 1) << 1) | 1) << shift), 1)
        add(f"just above a tie, shift {shift}", _block_from_value(((((M << 1) | 1) << 40) + 1) << shift), 1)
        add(f"negative tie, shift {shift}", _block_from_value(-(((M + 1) << 1) | 1) << shift), 1)
    add("a tie that the division makes", _block_from_value(3 * ((M << 1) | 1) << 300), 3)
    add("a remainder just above a tie", _block_from_value((3 * ((M << 1) | 1) << 300) + 1), 3)
    add("a remainder just below a tie", _block_from_value((3 * ((M << 1) | 1) << 300) - 1), 3)
    add("carry of the mantissa into 2^53", _block_from_value(((1 << 54) - 1) << 500), 1)
    for v in (1 << 14, 1 << 13, (1 << 13) + 1, 3 << 13, (3 << 13) - 1, 1, (1 << 13) - 1, 5 << 13, ((1 << 52) - 1) << 14, (1 << 66) - 1,
              ((1 << 53) - 1) << 13):
        add(f"subnormal range, {v:#x}", _block_from_value(v), 1)
        add(f"subnormal range, -{v:#x}", _block_from_value(-v), 1)
    add("subnormal by division", _block_from_value(7 << 40), (1 << 30) + 1)
    add("smallest subnormal over a large weight", _block_from_value(term_value(5e-324, 3)), 1 << 62)
    add("largest finite double", _block_from_value(term_value(dbl_max, 1)), 1)
    add("largest finite double times 2^52 over 2^52", _block_from_value(term_value(dbl_max, 1 << 52)), 1 << 52)
    add("largest finite double times 2^63 - 1", _block_from_value(term_value(-dbl_max, (1 << 63) - 1)), (1 << 63) - 1)
    add("half an ulp beyond the largest finite double", _block_from_value(((1 << 54) - 1) << (2046 + 13 - 1)), 1)
    add("just below that", _block_from_value((((1 << 54) - 1) << (2046 + 13 - 1)) - 1), 1)
    add("a zero sum", [0] * BLOCK, 5)
    add("a zero sum behind deferred carries", [1 << 32, -1] + [0] * (BLOCK - 2), 5)
    add("no weight", _block_from_value(12345 << 1000), 0)
    add("no weight, zero sum", [0] * BLOCK, 0)
    add("a flagged block", _block_from_value(12345 << 1000)[:LIMBS] + [3], 7)
    for j in range(12):
        top = int(rng.integers(200, 32 * 60))
        v = int(rng.integers(1, 1 << 62)) << top | int(rng.integers(0, 1 << 62))
        v = -v if j % 2 else v
        W = int(rng.integers(1, 1 << 62)) if j % 3 else (1 << 63) - 1 - j
        add(f"carries deferred through every limb, {j}", _block_from_value(v, rng), W)
    for j in range(6):
        limbs = [int(x) for x in rng.integers(-(1 << 62), 1 << 62, LIMBS)]
        limbs[60:] = [0] * (LIMBS - 60)
        if j == 0:
            limbs = [(1 << 62) - 1] * 60 + [0] * (LIMBS - 60)
        if j == 1:
            limbs = [-(1 << 62)] * 60 + [0] * (LIMBS - 60)
        add(f"limbs near +-2^62, {j}", limbs + [0], int(rng.integers(1, 1 << 40)))
    top = [int(x) for x in rng.integers(-(1 << 62), 1 << 62, LIMBS)]
    add("every limb near +-2^62: beyond the largest double", top + [0], 1)
    return cases
