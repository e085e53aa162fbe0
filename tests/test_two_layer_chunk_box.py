"""CPU tier: the proof behind the EXACT two-layer kernel's chunk guard (scripts/two_layer_box_proof.py, prove_chunk) holds for the
constants the kernel is compiled with (rscm_amd/csrc/two_layer_chunk_box.hpp), and fails when a box, the chunk length or the wide
numerator window is moved past what it covers."""
import math

import pytest

from scripts import two_layer_box_proof as proof

EDGES = ("Lambda0", "A", "EffEta", "Eta", "Cs", "Cd", "H", "Half", "Sixth", "Forcing", "State", "WideDiv", "WideNum")


def _boxes():
    return proof.read_boxes(proof.CHUNK_HEADER)


def test_the_kernels_chunk_boxes_are_proven():
    boxes = _boxes()
    assert set(boxes) == set(EDGES)
    n_sub = proof.read_constants(proof.CHUNK_HEADER)["ChunkSubSteps"]
    assert n_sub >= 2
    out = proof.prove_chunk(boxes)
    assert len(out) == 8 * n_sub
    lo, hi = boxes["WideNum"]
    for name, v in out.items():
        assert "-0" not in v.kinds, name
        assert v.lo >= lo and v.hi < math.ldexp(1.0, hi), name


def test_one_more_sub_step_is_not_covered():
    n_sub = proof.read_constants(proof.CHUNK_HEADER)["ChunkSubSteps"]
    with pytest.raises(proof.ProofError):
        proof.prove_chunk(_boxes(), n_sub + 1)


def test_the_chunk_state_box_is_the_widest_the_proof_allows_upwards():
    boxes = _boxes()
    lo, hi = boxes["State"]
    with pytest.raises(proof.ProofError):
        proof.prove_chunk(dict(boxes, State=(lo, hi + 1)))


def test_the_chunk_boxes_hold_the_benchmark_draw_with_margin():
    """bench.py's draw: lambda0 0.8-1.5, a 0-0.1, efficacy 1-1.8, eta 0.5-1, Cs 5-15, Cd 50-200, |F| <= 5, h = 0.1."""
    b = _boxes()
    inside = lambda name, lo, hi: 2.0 ** b[name][0] <= lo and hi < 2.0 ** b[name][1]  # noqa: E731
    assert inside("Lambda0", 0.8, 1.5) and inside("A", 1e-12, 0.1) and inside("EffEta", 0.5, 1.8) and inside("Eta", 0.5, 1.0)
    assert inside("Cs", 5.0, 15.0) and inside("Cd", 50.0, 200.0) and inside("Forcing", 1e-30, 5.0)
    assert inside("H", 0.1, 0.1) and inside("Half", 0.1 / 2.0, 0.1 / 2.0) and inside("Sixth", 0.1 / 6.0, 0.1 / 6.0)


@pytest.mark.parametrize("name", [n for n in EDGES if not n.startswith("Wide")])
def test_every_edge_is_where_the_checker_puts_it(name):
    """One binary order further out on either side is refused by the checker -- unless the edge is the state guard's (a wavefront
    takes the chunk guard only inside the state guard's parameter boxes; the forcing box's lower edge is held there on purpose) or the
    wide divisor box's."""
    boxes, state = _boxes(), proof.read_boxes()
    dlo, dhi = boxes["WideDiv"]
    for side, step in ((0, -1), (1, 1)):
        b = list(boxes[name])
        if name in state and name != "State" and b[side] == state[name][side]:
            continue
        if name in ("Cs", "Cd") and b[side] == (dlo, dhi)[side]:
            continue
        b[side] += step
        with pytest.raises(proof.ProofError):
            proof.prove_chunk(dict(boxes, **{name: tuple(b)}))


def test_the_chunk_forcing_box_contains_the_state_guards():
    """A forcing the state guard accepts never makes the chunk guard replay a year: the chunk forcing box contains the state guard's
    (two_layer_box.hpp), both with +0."""
    mine, theirs = _boxes()["Forcing"], proof.read_boxes()["Forcing"]
    assert mine[0] <= theirs[0] and mine[1] >= theirs[1]


def test_the_chunk_parameter_boxes_lie_inside_the_state_guards():
    mine, theirs = _boxes(), proof.read_boxes()
    for name in ("Lambda0", "A", "EffEta", "Eta", "Cs", "Cd"):
        assert theirs[name][0] <= mine[name][0] and mine[name][1] <= theirs[name][1], name
    for name in ("H", "Half"):
        assert theirs["H"][0] <= mine[name][0] and mine[name][1] <= theirs["H"][1], name


@pytest.mark.parametrize("name,value", [("WideNum", (-970, 760)), ("WideNum", (-960, 767)), ("WideDiv", (-10, 14)),
                                        ("WideDiv", (-2, 130)), ("Cd", (5, 15))])
def test_the_wide_window_is_held_to_the_division_hardware(name, value):
    """numerators whose biased exponent is 53 or less, or 768 binary orders above the smallest divisor, are scaled by
    v_div_scale_f64; the heat-capacity boxes must lie in the wide window's divisor box."""
    with pytest.raises(proof.ProofError):
        proof.check_wide_window(dict(_boxes(), **{name: value}))
