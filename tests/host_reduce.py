"""References for the kernels that reduce ACROSS the members of an ensemble (the plume summary of csrc/ensemble_ops.hip, the
likelihood-to-weights kernels of csrc/weights.hip), in numpy and Python floats: rows whose sum has one right answer whatever the
reduction tree, rows on which only an error bound can hold, that bound derived from the kernels' addition tree, and a plain
restatement of the tree itself, which the CPU tier uses to show that the bound holds for the tree and fails for a tree that loses
members."""
import math

import numpy as np

BLOCK = 256          # kBlock: threads of a workgroup
WAVE = 64            # lanes of a wavefront
SUMMARY_CAP = 1024   # the cap of summary_blocks (grid_for(n, 1024)); exceedance, loglik_max and the weight check share it
ONE_GRID = SUMMARY_CAP * BLOCK   # 262 144: members beyond this are reached by a thread's second pass of its grid-stride loop
U = 2.0 ** -53       # unit round-off of binary64


def summary_blocks(n: int) -> int:
    """Blocks along x of the partial kernel: ceil(n / 256), at least 1, at most 1024."""
    return max(1, min(SUMMARY_CAP, -(-int(n) // BLOCK)))


# ---- rows ---------------------------------------------------------------------------------------------------------------

def exact_row(rng, n: int) -> np.ndarray:
    """n members k * 2^-20 with integer |k| < 2^20.  Every sum of any subset of at most 2^21 of them is an integer multiple of
    2^-20 below 2^21 * 2^20 * 2^-20 = 2^21 in magnitude, i.e. an integer below 2^41 in units of 2^-20: representable, so every
    partial sum in every order is exact in binary64 and every reduction tree gives math.fsum's bits."""
    assert n <= 1 << 21
    k = rng.integers(-(1 << 20) + 1, 1 << 20, size=n, dtype=np.int64)
    return k.astype(np.float64) * 2.0 ** -20


def ill_conditioned_row(rng, n: int) -> np.ndarray:
    """n members whose sum is tiny next to the sum of their magnitudes: pairs +m, -m with m from 1e-300 to 1e300 (log-uniform), and
    a remainder of one (n odd) or two (n even) members in +-[1, 2), which is the exact sum.  Pair j sits at members j and n - 1 - j,
    and pair 0 has the largest magnitude, 1e300: the partner of the LAST member is the first, so a reduction that loses any tail of
    the row is off by 1e300, far outside any rounding bound."""
    n = int(n)
    n_rem = min(n, 2 - n % 2)
    pairs = (n - n_rem) // 2
    x = np.empty(n)
    m = 10.0 ** rng.uniform(-300.0, 300.0, pairs)
    if pairs:
        m[0] = 1e300
    m *= rng.choice([-1.0, 1.0], pairs)
    x[:pairs] = m
    x[n - pairs:] = -m[::-1]
    x[pairs:pairs + n_rem] = rng.uniform(1.0, 2.0, n_rem) * rng.choice([-1.0, 1.0], n_rem)
    return x


# ---- the reference of a summary ------------------------------------------------------------------------------------------

def summary(x):
    """(count, sum, min, max) over the finite members as rscm_ens_summary defines them: the count as an int, the sum correctly
    rounded (math.fsum), min = +inf and max = -inf without a finite member."""
    x = np.asarray(x, dtype=np.float64)
    f = x[np.isfinite(x)]
    if f.size == 0:
        return 0, 0.0, math.inf, -math.inf
    return int(f.size), math.fsum(f), float(f.min()), float(f.max())


def additions_depth(n: int) -> int:
    """D: the greatest number of floating-point additions the value of one member passes through on its way into the sum that
    summary_rows_partial_kernel and summary_rows_final_kernel (csrc/ensemble_ops.hip) write, read from their code.

    Partial kernel, nb = summary_blocks(n) blocks of 256 threads.  A thread adds the members i, i + 256 nb, i + 2 * 256 nb, ... to
    its running sum one after the other: s_p = ceil(n / (256 nb)) serial additions, and the member taken first passes through all
    of them.  wave_reduce folds the 64 lanes in six __shfl_down steps (offsets 32 .. 1), one addition each, and what ends in
    lane 0 has passed through at most six.  block_reduce's thread 0 then adds the three other wave partials to its own, one after
    the other: three more for the value of wave 0.  Final kernel, one block per row: a thread adds the partials b, b + 256, ...
    serially, s_f = ceil(nb / 256) additions (four at the cap), then the same six wave steps and three wave partials.

        D = (s_p + 6 + 3) + (s_f + 6 + 3)

    (The first serial addition of either kernel is 0.0 + x and exact; counting it leaves two units of slack, which more than pay
    for math.fsum's own rounding of the reference, at most 2^-53 |sum x|, and of sum |x|.)"""
    nb = summary_blocks(n)
    s_p = max(1, -(-int(n) // (BLOCK * nb)))
    s_f = -(-nb // BLOCK)
    return (s_p + 6 + 3) + (s_f + 6 + 3)


def sum_bound(x) -> float:
    """The bound on |device sum - math.fsum| over the finite members of x: D u sum|x| / (1 - D u), u = 2^-53, D = additions_depth.
    This is the standard bound of any summation tree in which no operand passes through more than D additions (each addition
    contributes a relative error of at most u to everything below it): derived from the code, not measured."""
    x = np.asarray(x, dtype=np.float64)
    f = x[np.isfinite(x)]
    d = additions_depth(x.size) * U
    return d * math.fsum(np.abs(f)) / (1.0 - d)


# ---- the kernels' addition tree, restated ---------------------------------------------------------------------------------

def _block_sums(v: np.ndarray) -> np.ndarray:
    """[B][256] thread values -> [B] block sums in block_reduce's order: per wave the six steps lane += lane + off for off = 32 ..
    1 (only the lanes below off matter for lane 0), then ((w0 + w1) + w2) + w3."""
    w = v.reshape(v.shape[0], BLOCK // WAVE, WAVE).copy()
    off = WAVE // 2
    while off:
        w[..., :off] = w[..., :off] + w[..., off:2 * off]
        off //= 2
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def device_tree_sum(x, passes=None) -> float:
    """The sum field of the two summary kernels, addition by addition, in numpy float64.  A non-finite member adds 0.0 where the
    kernel skips it: the same value.  ``passes`` limits a thread's grid-stride loop to that many members: passes=1 is the tree of
    a kernel that loses everything beyond the first 262 144 members."""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(np.isfinite(x), x, 0.0)
    nb = summary_blocks(x.size)
    stride = nb * BLOCK
    n_pass = -(-x.size // stride)
    if passes is not None:
        n_pass = min(n_pass, passes)
    acc = np.zeros(stride)
    for p in range(n_pass):
        chunk = x[p * stride:(p + 1) * stride]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    part = _block_sums(acc.reshape(nb, BLOCK))
    facc = np.zeros(BLOCK)
    for p in range(-(-nb // BLOCK)):
        chunk = part[p * BLOCK:(p + 1) * BLOCK]
        facc[:chunk.size] = facc[:chunk.size] + chunk
    return float(_block_sums(facc.reshape(1, BLOCK))[0])


def pairwise_sum(x) -> float:
    """Recursive halving down to single members: another tree altogether."""
    x = np.asarray(x, dtype=np.float64)
    while x.size > 1:
        if x.size % 2:
            x = np.append(x, 0.0)
        x = x[0::2] + x[1::2]
    return float(x[0]) if x.size else 0.0


# ---- likelihood to weights --------------------------------------------------------------------------------------------------

def loglik_ok(ll, status) -> np.ndarray:
    """The members whose log-likelihood counts: status 0 and a finite value."""
    return (np.asarray(status) == 0) & np.isfinite(np.asarray(ll, dtype=np.float64))


def loglik_max(ll, status) -> float:
    """max ll over the members that count, -inf without one (rscm_ens_loglik_max)."""
    ok = loglik_ok(ll, status)
    return float(np.asarray(ll, dtype=np.float64)[ok].max()) if ok.any() else -math.inf


def weights_from_loglik(ll, status, ll_max: float, bits: int) -> np.ndarray:
    """rint(exp(min(ll - ll_max, 0)) * 2^bits) as float64 for the members that count, 0 for the others.  The device's integer is
    within one unit of it (its exp and numpy's are each within an ulp of the true value, below 2^-18 at bits <= 34, and the two
    roundings to an integer can fall either side of a half)."""
    ok = loglik_ok(ll, status)
    d = np.minimum(np.where(ok, np.asarray(ll, dtype=np.float64) - ll_max, 0.0), 0.0)
    return np.where(ok, np.rint(np.exp(d) * 2.0 ** bits), 0.0)
