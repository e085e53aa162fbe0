"""The counter-based random streams of the device restated in numpy: Philox4x32-10 (rscm_amd/csrc/philox.hpp), the keyed
Feistel permutation and Latin hypercube of rscm_amd/csrc/ensemble_ops.hip (lhs_kernel, launch_lhs), and the stretch move of
rscm_amd/csrc/sampler.hip (propose_kernel, accept_kernel) driven as rscm_sampler_set_positions / rscm_sampler_iterate drive
it.  Every draw is keyed and countered by values the host knows and the rest is plain f64 arithmetic in the kernels' order,
so these predict the device bit for bit.  tests/test_host_sampler.py checks them against published answers and analytic
targets; the GPU tests pin the device to them."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of Salmon et al. (2011), vectorised: the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u32(v) for v in (c0, c1, c2, c3, k0, k1)))
    c0, c1, c2, c3, k0, k1 = (np.array(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = _PHILOX_M0 * c0
        p1 = _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(_PHILOX_W0)) & M32
        k1 = (k1 + np.uint64(_PHILOX_W1)) & M32
    return c0, c1, c2, c3


def u01_from_bits(lo, hi):
    """The 53-bit uniform in [0, 1) of two 32-bit words: ((hi << 32 | lo) >> 11) * 2**-53."""
    bits = ((_u32(hi) << np.uint64(32)) | _u32(lo)) >> np.uint64(11)
    return bits.astype(np.float64) * (1.0 / 9007199254740992.0)


# ---------------------------------------------------------------------------------------------- Latin hypercube
def lhs_half_bits(n_total: int) -> int:
    """launch_lhs: the smallest even bit count >= 2 with 2**bits >= n_total, halved."""
    bits = 2
    while (1 << bits) < n_total:
        bits += 1
    bits += bits & 1
    return bits // 2


def feistel_perm(x, n: int, half_bits: int, k0: int, k1: int) -> np.ndarray:
    """The keyed bijection of [0, n): a 4-round Feistel network on [0, 4**half_bits), cycle-walked back into range."""
    x = np.array(x, dtype=np.uint64, copy=True)
    mask = np.uint64((1 << half_bits) - 1)
    hb = np.uint64(half_bits)
    todo = np.arange(x.size)
    while todo.size:   # the device walks every lane at least once, then again while the value lies outside [0, n)
        v = x[todo]
        l, r = v >> hb, v & mask
        for rnd in range(4):
            c0, c1, _, _ = philox4x32_10(r & M32, r >> np.uint64(32), rnd, 0x5EED, k0, k1)
            f = ((c1 << np.uint64(32)) | c0) & mask
            l, r = r, l ^ f
        x[todo] = (l << hb) | r
        todo = todo[x[todo] >= np.uint64(n)]
    return x


def lhs_keys(seed: int, j: int):
    """(k0, k1) of dimension j: the Feistel key; the uniform inside the stratum is keyed by (k0, ~k1)."""
    seed &= (1 << 64) - 1
    k0 = (seed & 0xFFFFFFFF) ^ ((0x9E3779B9 * (j + 1)) & 0xFFFFFFFF)
    k1 = ((seed >> 32) + j) & 0xFFFFFFFF
    return k0, k1


def lhs_matrix(seed: int, low, high, member_offset: int, n_local: int, n_total: int) -> np.ndarray:
    """[P][n_local] float64: what rscm_ens_sample_lhs writes for members [member_offset, member_offset + n_local) of an
    ensemble of n_total, in the kernel's expression order."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    g = np.arange(member_offset, member_offset + n_local, dtype=np.uint64)
    hb = lhs_half_bits(n_total)
    interval = 1.0 / float(n_total)
    out = np.empty((len(low), n_local))
    for j in range(len(low)):
        k0, k1 = lhs_keys(seed, j)
        stratum = feistel_perm(g, n_total, hb, k0, k1)
        c0, c1, _, _ = philox4x32_10(g & M32, g >> np.uint64(32), 0xA5A5, j, k0, ~np.uint64(k1) & M32)
        u = stratum.astype(np.float64) * interval + u01_from_bits(c0, c1) * interval
        out[j] = low[j] + u * (high[j] - low[j])
    return out


# ---------------------------------------------------------------------------------------------- stretch move
STREAM_PROPOSE, STREAM_ACCEPT = 0x57A7, 0xACCE


def walker_of(k, half: int, n_walkers: int, n_groups: int):
    """Walker index of half-walker k of half ``half``: groups of Wg walkers one after the other, each split in two."""
    Wg = n_walkers // n_groups
    Hg = Wg // 2
    k = np.asarray(k, dtype=np.int64)
    return (k // Hg) * Wg + half * Hg + (k % Hg)


def stretch_draws(seed: int, iteration: int, half: int, n_half: int, stretch_a: float, Hg: int):
    """(z, j) of every half-walker k < n_half: the stretch factor and the partner's index in the complementary half."""
    seed &= (1 << 64) - 1
    k = np.arange(n_half, dtype=np.uint64)
    c0, c1, c2, c3 = philox4x32_10(k, iteration, half, STREAM_PROPOSE, seed & 0xFFFFFFFF, seed >> 32)
    u = u01_from_bits(c0, c1)
    s = (stretch_a - 1.0) * u + 1.0
    z = s * s / stretch_a
    j = ((c2 << np.uint64(32)) | c3) % np.uint64(Hg)
    return z, j.astype(np.int64)


def accept_uniform(seed: int, iteration: int, half: int, n_half: int):
    seed &= (1 << 64) - 1
    k = np.arange(n_half, dtype=np.uint64)
    c0, c1, _, _ = philox4x32_10(k, iteration, half, STREAM_ACCEPT, seed & 0xFFFFFFFF, seed >> 32)
    return u01_from_bits(c0, c1)


def log_ratio(z, new_logp, old_logp, n_dims: int, z_power=None):
    """(D - 1) log z + (new - old); ``z_power`` replaces D - 1 (tests only: a deliberately wrong exponent)."""
    p = float(n_dims - 1 if z_power is None else z_power)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return p * np.log(z) + (new_logp - old_logp)


def accept_rule(u, lr, new_logp):
    """accept iff the proposal's score is finite and u < exp(log_ratio)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(new_logp) & (u < np.exp(lr))


def marginal(u, lr, new_logp, score_tol=0.0, rel=1e-13):
    """Decisions that a rounding difference in exp / log (a few ulp: ``rel``), or a score known to ``score_tol`` only,
    could flip: the comparison u < exp(log_ratio) lies inside that band."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(lr)   # an overflow to +inf accepts whatever the rounding: not marginal
        near = np.isfinite(e) & (np.abs(u - e) <= rel * np.maximum(u, e))
        if np.any(np.asarray(score_tol) > 0):
            near |= np.abs(np.log(u) - lr) <= score_tol + rel * (1.0 + np.abs(lr))
    return np.isfinite(new_logp) & np.isfinite(lr) & near


class HalfStep:
    """What one half-step proposes from a state, before anything is scored."""

    def __init__(self, iteration, half, active, comp, z, proposal, u):
        self.iteration, self.half = iteration, half
        self.active, self.comp, self.z, self.proposal, self.u = active, comp, z, proposal, u


class HostStretchMove:
    """The device sampler's chain on the host.  ``score`` maps positions [n][D] to log posteriors, -inf outside the prior's
    support (the device never asks the model about those) and for anything that fails.  ``z_power`` is for tests only."""

    def __init__(self, n_walkers: int, n_dims: int, score, stretch_a: float = 2.0, seed: int = 0, n_groups: int = 1,
                 z_power=None):
        if n_walkers % n_groups or (n_walkers // n_groups) % 2 or n_walkers // n_groups < 2:
            raise ValueError("n_walkers must split into n_groups groups of an even number (>= 2) of walkers")
        self.W, self.D, self.score = int(n_walkers), int(n_dims), score
        self.a, self.seed, self.groups, self.z_power = float(stretch_a), int(seed) & ((1 << 64) - 1), int(n_groups), z_power
        self.Wg = self.W // self.groups
        self.Hg = self.Wg // 2
        self.iteration = 0
        self.records = []   # per half-step: (iteration, half, active, new_logp, accept) when ``keep_records``
        self.keep_records = False
        self.n_decisions = 0
        self.n_marginal = 0   # decisions inside marginal()'s band: a rounding difference of log / exp could flip them

    def set_positions(self, positions, logp=None):
        """rscm_sampler_set_positions: scores the walkers where they stand, resets the counters and the iteration."""
        self.pos = np.array(positions, dtype=np.float64).reshape(self.W, self.D)
        self.logp = np.array(self.score(self.pos) if logp is None else logp, dtype=np.float64)
        self.n_accepted = np.zeros(self.W, dtype=np.int64)
        self.n_proposed = np.zeros(self.W, dtype=np.int64)
        self.iteration = 0

    def propose(self, half: int, iteration=None, pos=None) -> HalfStep:
        it = self.iteration if iteration is None else iteration
        pos = self.pos if pos is None else pos
        n_half = self.W // 2
        k = np.arange(n_half)
        z, j = stretch_draws(self.seed, it, half, n_half, self.a, self.Hg)
        active = walker_of(k, half, self.W, self.groups)
        comp = (k // self.Hg) * self.Wg + (1 - half) * self.Hg + j
        x, c = pos[active], pos[comp]
        y = c + z[:, None] * (x - c)
        return HalfStep(it, half, active, comp, z, y, accept_uniform(self.seed, it, half, n_half))

    def decide(self, step: HalfStep, new_logp, old_logp):
        lr = log_ratio(step.z, new_logp, old_logp, self.D, self.z_power)
        return accept_rule(step.u, lr, new_logp), lr

    def half_step(self, half: int):
        step = self.propose(half)
        new_logp = np.asarray(self.score(step.proposal), dtype=np.float64)
        accept, lr = self.decide(step, new_logp, self.logp[step.active])
        self.n_decisions += len(accept)
        self.n_marginal += int(marginal(step.u, lr, new_logp).sum())
        a = step.active
        self.n_proposed[a] += 1
        self.n_accepted[a[accept]] += 1
        self.pos[a[accept]] = step.proposal[accept]
        self.logp[a[accept]] = new_logp[accept]
        if self.keep_records:
            self.records.append((step.iteration, half, a, new_logp, accept))
        return step, new_logp, accept

    def sweep(self):
        """rscm_sampler_iterate(1): half 0 against half 1, then half 1 against the updated half 0."""
        self.iteration += 1
        self.half_step(0)
        self.half_step(1)

    def run(self, n_iterations: int, thin: int = 1):
        """The sweeps ``Chain`` keeps (1, 1 + thin, ...): lists of positions and log probabilities."""
        samples, log_probs = [], []
        for it in range(1, n_iterations + 1):
            self.sweep()
            if (it - 1) % max(1, thin) == 0:
                samples.append(self.pos.copy())
                log_probs.append(self.logp.copy())
        return samples, log_probs
