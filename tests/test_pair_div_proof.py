"""The argument behind the two-instruction quotient by a constant (rscm_amd/csrc/pair_div_verdict.hpp, rk4_device.hpp pair_div), run:
scripts/pair_div_proof.py derives the bound J(s, k) on how close, in units j of the congruence, a quotient must lie to a rounding
boundary for pair_div to miss the IEEE quotient, and tries EVERY divisor against EVERY numerator at 8, 9 and 10 bits of precision.
Every failure must lie within J; the header's way of listing the candidates must yield every numerator within its bound; and the
numerators the chunk guard admits must lie inside the windows the header states (scripts/two_layer_box_proof.py, check_pair_window)."""
import pytest

from tests.helpers import load_script

P = load_script("pair_div_proof")
B = load_script("two_layer_box_proof")


@pytest.fixture(scope="module", params=[8, 9, 10])
def run(request):
    p = request.param
    return p, P.exhaustive(p)


def test_bounds_are_the_ones_derived():
    """2^(s - p + 1) (1 + k) - 1, and the header's one bound covers all of them."""
    assert [P.J(0, 0), P.J(1, 0), P.J(0, 1), P.J(1, -1)] == [1, 3, 3, 7]
    assert max(P.J(sp, k) for sp in (0, 1) for k in P.VARIANT_STEPS) <= P.K_J
    assert P.VARIANT_STEPS == (0, 1, -1) and (1 << P.MAX_TRAILING) <= P.K_J < (2 << P.MAX_TRAILING)


def test_every_failure_lies_within_the_bound_and_not_within_one_less(run):
    p, failures = run
    assert failures[0], "the constants as defined fail for no pair at all: the run has no teeth"
    for k in P.VARIANT_STEPS:
        bounds = {0: P.J(0, k), 1: P.J(1, k)}
        for X, Y, sp, j in failures[k]:
            print(f"p = {p}  k = {k:+d}: X = {X} Y = {Y} s = p + {sp} |j| = {j} (J = {bounds[sp]})")
        assert not P.uncovered(failures, k, bounds)
        # a bound lowered to one below the largest |j| seen misses that failure
        for sp in (0, 1):
            worst = max([f[3] for f in failures[k] if f[2] == sp], default=0)
            if worst:
                lowered = dict(bounds)
                lowered[sp] = worst - 1
                assert P.uncovered(failures, k, lowered)


def test_the_headers_enumeration_yields_every_numerator_near_a_boundary(run):
    p, failures = run
    assert P.superset_holds(p)
    # ... and with it every failing pair, for the constants as defined and for both neighbours
    for k in P.VARIANT_STEPS:
        by_divisor = {}
        for X, Y, _, _ in failures[k]:
            by_divisor.setdefault(Y, []).append(X)
        for Y, xs in by_divisor.items():
            assert set(xs) <= set(P.candidates(Y, p))


def test_the_verdict_calls_no_failing_divisor_safe(run):
    p, failures = run
    failing = {k: {f[1] for f in failures[k]} for k in P.VARIANT_STEPS}
    for Y in range(1 << (p - 1), 1 << p):
        v = P.verdict(Y, p)[0]
        if v >= 0:
            assert Y not in failing[P.VARIANT_STEPS[v]]
        else:
            assert all(Y in failing[k] for k in P.VARIANT_STEPS)


def test_the_chunk_guards_numerators_lie_in_the_pair_windows():
    lo, hi, surface_lo = B.check_pair_window()
    consts = B.read_constants(B.PAIR_HEADER)
    assert (lo, hi, surface_lo) == (consts["NumLo"], consts["NumHi"], consts["SurfaceNumFloor"])
    assert (P.NUM_LO, P.SURFACE_NUM_FLOOR) == (lo, surface_lo)
    # either lower edge moved up by one binade, or the upper edge down, leaves a numerator outside: the edges are what the guard needs
    chunk = B.read_boxes(B.CHUNK_HEADER)
    numerators = B.prove_chunk(chunk)
    assert min(v.lo for n, v in numerators.items() if n.startswith("num_s")) == surface_lo
    with pytest.raises(B.ProofError):
        B.check_pair_window(surface_lo=surface_lo + 1)
    with pytest.raises(B.ProofError):
        B.check_pair_window(pair=(min(v.lo for n, v in numerators.items() if n.startswith("num_d")) + 1, hi))
    # ... and an edge moved past what the arithmetic allows is refused whatever the guard admits
    with pytest.raises(B.ProofError):
        B.check_pair_window(pair=(lo - 1, hi))
    with pytest.raises(B.ProofError):
        B.check_pair_window(pair=(lo, 1023 + chunk["WideDiv"][0]))
