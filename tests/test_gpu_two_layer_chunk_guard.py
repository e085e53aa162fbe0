"""GPU tier (-m gpu): the EXACT two-layer kernel's chunk guard -- the state checked at every third sub-step against the boxes of
csrc/two_layer_chunk_box.hpp, the numerators in spec_div's wide window -- against the numerator guard and the CPU oracle, bit for bit,
on parameters, forcings and states on both sides of every chunk-box edge; and the wide window itself on the device."""
import numpy as np
import pytest

from scripts import two_layer_box_proof as proof
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import SEED, assert_bit_equal, axis_values, f_syn, two_layer_params
from tests.test_gpu_two_layer_guard import BASE, _edge_values, _guard, _run, _three_ways

pytestmark = pytest.mark.gpu

CHUNK = proof.read_boxes(proof.CHUNK_HEADER)
# parameter rows and their chunk boxes (efficacy * eta is boxed as a product: row 2 is efficacy, set apart below)
ROWS = {0: CHUNK["Lambda0"], 1: CHUNK["A"], 3: CHUNK["Eta"], 4: CHUNK["Cs"], 5: CHUNK["Cd"]}


@pytest.fixture(scope="module")
def orc():
    from oracle import cbind
    return cbind


def _counts(enable):
    """wavefronts per guard (numerators, states, chunks) of this thread's counting launches since the last call; counting on / off"""
    import ctypes as C
    from rscm_amd import _lib as L
    out = (C.c_int64 * 3)()
    L.check(L.load().rscm_gpu_two_layer_guard_counts(0, enable, out))
    return list(out)


def test_the_guard_counts_name_the_path_taken(ra):
    """Two wavefronts inside the chunk boxes take the chunk guard; one member with Cs = 3 (outside the chunk's Cs box, inside the state
    guard's) sends its wavefront to the state guard; the numerator switch sends both to the numerator guard; FAST counts nothing."""
    t = axis_values(1750, 1760)
    P = np.repeat(BASE[:, None], 128, axis=1)
    F = f_syn(t)
    _counts(1)
    try:
        _run(ra, t, P, F, 0.1, 0.0)
        assert _counts(1) == [0, 0, 2]
        P[4, 70] = 3.0
        _run(ra, t, P, F, 0.1, 0.0)
        assert _counts(1) == [0, 1, 1]
        try:
            _guard(1)
            _run(ra, t, P, F, 0.1, 0.0)
        finally:
            _guard(0)
        assert _counts(1) == [2, 0, 0]
    finally:
        _counts(0)


def test_step_sizes_on_both_sides_of_the_chunk_step_boxes(ra, orc):
    """h = 15/128 below 2^-3 and h = 2^-3 at it, h = 0.09375 (h / 6 = 2^-6 exactly) and 2^-10 below it, on axes of ten sub-steps per
    step (binary fractions, so that the sub-steps land on the axis): the chunk guard where h, h / 2 and h / 6 are inside their boxes,
    the state guard elsewhere; bits as the oracle's either way."""
    P = two_layer_params(256, seed=SEED + 19)
    for h, inside in ((15.0 / 128.0, True), (0.125, False), (0.09375, True), (0.09375 - 2.0 ** -10, False)):
        tt = 1750.0 + 10.0 * h * np.arange(40)
        _counts(1)
        try:
            _three_ways(ra, orc, tt, P, f_syn(tt), 0.1, 0.05, h=h, what=f"h={h!r}")
            c = _counts(1)
        finally:
            _counts(0)
        assert (c[2] > 0) == inside and c[1] + c[2] > 0, (h, c)


def test_wide_window_division_is_ieee(ra):
    """spec_div == IEEE division for |n| in the wide window and d in the wide divisor box, with operands on both sides of the edges."""
    from rscm_amd.ensemble import selftest_div
    rng = np.random.default_rng(11)
    dlo, dhi = CHUNK["WideDiv"]
    nlo, nhi = CHUNK["WideNum"]
    k = 1 << 17
    ne = rng.choice([nlo - 2, nlo - 1, nlo, nlo + 1, nhi - 2, nhi - 1, nhi, nhi + 1], k)
    de = rng.choice([dlo, dlo + 1, (dlo + dhi) // 2, dhi - 2, dhi - 1], k)
    num = np.ldexp(rng.uniform(1, 2, k), ne) * rng.choice([-1.0, 1.0], k)
    den = np.ldexp(rng.uniform(1, 2, k), de)
    # the exact edges and their neighbours, against divisors at and next to the box's edges
    en = np.array([2.0 ** nlo, np.nextafter(2.0 ** nlo, 0.0), np.nextafter(2.0 ** nhi, 0.0), 2.0 ** nhi, 2.0 ** (nlo + 1) * 1.5])
    ed = np.array([2.0 ** dlo, np.nextafter(2.0 ** dlo, np.inf), np.nextafter(2.0 ** dhi, 0.0), 5.0, 15.0, 50.0, 200.0, 3.0])
    gn, gd = np.meshgrid(np.concatenate([en, -en]), ed)
    # wide-exponent numerators over the whole window against heat capacities spread over the box
    w = 1 << 16
    wn = np.ldexp(rng.uniform(1, 2, w), rng.integers(nlo, nhi, w))
    wd = np.ldexp(rng.uniform(1, 2, w), rng.integers(dlo, dhi, w))
    num = np.concatenate([num, gn.ravel(), wn])
    den = np.concatenate([den, gd.ravel(), wd])
    ref, fast, _ = selftest_div(num, den)
    with np.errstate(all="ignore"):
        assert_bit_equal(ref, num / den, "device IEEE division vs host IEEE division")
    inside = (np.abs(num) >= 2.0 ** nlo) & (np.abs(num) < 2.0 ** nhi) & (den >= 2.0 ** dlo) & (den < 2.0 ** dhi)
    assert_bit_equal(fast[inside], ref[inside], "hoisted-reciprocal quotient vs IEEE division in the wide window")
    assert 0.3 < inside[:k].mean() < 0.9          # both sides of the numerator edges are exercised
    assert inside[-w:].all()


def test_parameters_on_both_sides_of_every_chunk_box_edge(ra, orc):
    """Per parameter and edge, one wavefront just inside the chunk box at that edge (chunk guard) next to one whose 64 members are the
    same but for one just outside (the whole wavefront takes the per-sub-step state guard); efficacy*eta at its own edges."""
    t = axis_values(1750, 1800)
    rows = []
    rng = np.random.default_rng(5)
    for j, (lo, hi) in ROWS.items():
        below_lo, at_lo, below_hi, at_hi = _edge_values(lo, hi)
        for inside, outside in ((at_lo, below_lo), (below_hi, at_hi)):
            wave = np.repeat(BASE[:, None], 64, axis=1) * rng.uniform(0.9, 1.1, (6, 64))
            wave[1] = rng.uniform(0.0, 0.1, 64)
            wave[j, ::2] = inside
            rows.append(wave.copy())
            wave[j, 5] = outside
            rows.append(wave)
    for target in _edge_values(*CHUNK["EffEta"]):
        wave = np.repeat(BASE[:, None], 64, axis=1)
        wave[3] = 0.5
        wave[2] = target / 0.5
        rows.append(wave)
    P = np.concatenate(rows, axis=1)
    F = f_syn(t)
    _counts(1)
    try:
        _three_ways(ra, orc, t, P, F, 0.0, 0.0, what="chunk parameter edges")
        c = _counts(1)
        _three_ways(ra, orc, t, P, F, 0.3, -0.1, what="chunk parameter edges, warm start")
    finally:
        _counts(0)
    assert c[1] > 0 and c[2] > 0, c           # both sides of the chunk boxes' edges ran


def test_forcings_on_both_sides_of_the_chunk_forcing_box(ra, orc):
    """|F| just below, at and above 2^3 and 2^-128, +0 and -0, per scenario."""
    t = axis_values(1750, 1850)
    P = two_layer_params(640, seed=SEED + 13)
    lo, hi = CHUNK["Forcing"]
    sign = np.where(np.arange(len(t)) % 2 == 0, 1.0, -1.0)
    F = np.stack([sign * np.nextafter(2.0 ** hi, 0.0), sign * 2.0 ** hi, -(2.0 ** hi) * np.ones_like(t), sign * 2.0 ** lo,
                  sign * np.nextafter(2.0 ** lo, 0.0), np.where(np.arange(len(t)) % 4 == 0, 0.0, f_syn(t)),
                  np.where(np.arange(len(t)) % 4 == 1, -0.0, f_syn(t)), f_syn(t) * 1.6])
    scen = (np.arange(P.shape[1]) % F.shape[0]).astype(np.int32)
    _three_ways(ra, orc, t, P, F, 0.0, 0.0, scen=scen, what="chunk forcing edges")
    _three_ways(ra, orc, t, P, F, 0.4, 0.1, scen=scen, what="chunk forcing edges, warm start")


def test_states_across_the_chunk_state_box_edges(ra, orc):
    """Initial states below, at and above 2^-128 and 2^7, zeros: relaxing members leave the box upwards, tiny ones enter it, hot ones
    cool through 2^7 within a few years; the default heat capacities keep every member in the chunk's parameter boxes."""
    t = axis_values(1750, 1850)
    lo, hi = CHUNK["State"]
    vals = [2.0 ** (lo - 1), np.nextafter(2.0 ** lo, 0.0), 2.0 ** lo, -2.0 ** lo, 1e-30, np.nextafter(2.0 ** hi, 0.0), 2.0 ** hi,
            -2.0 ** hi, 3.0 * 2.0 ** (hi - 1), 2.0 ** (hi + 3), 0.0, -0.0, 5e-324]
    n = 64 * len(vals)
    P = np.repeat(BASE[:, None], n, axis=1)
    P[0] = 1.9                                       # strong relaxation inside the chunk's lambda0 box
    P[4] = 4.0
    ts0 = np.repeat(np.array(vals), 64)
    td0 = np.roll(ts0, 64)
    for F in (np.zeros_like(t), f_syn(t) * 1e-36, f_syn(t)):
        want = _three_ways(ra, orc, t, P, F, ts0, td0, what="chunk state edges")
    big = np.abs(ts0) >= 2.0 ** hi
    with np.errstate(invalid="ignore"):
        assert (np.abs(want[0][-1][big & np.isfinite(ts0)]) < 2.0 ** hi).any()   # some members come down into the box


def test_members_that_run_away_mid_run(ra, orc):
    """Large a and small heat capacities inside the chunk boxes: members leave the state box upwards, overflow and turn NaN."""
    t = axis_values(1750, 2000)
    P = two_layer_params(512, seed=SEED + 17)
    P[1] = np.linspace(0.05, 0.12, P.shape[1])
    P[4] = 4.5
    P[0] = 0.3
    want = _three_ways(ra, orc, t, P, f_syn(t) * 1.5, 0.0, 0.0, what="runaway")
    with np.errstate(invalid="ignore"):
        assert not np.isfinite(want[0][-1]).all()
