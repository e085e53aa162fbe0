"""CPU tier: the proof behind the EXACT two-layer kernel's state guard (scripts/two_layer_box_proof.py) holds for the boxes the
kernel is compiled with (rscm_amd/csrc/two_layer_box.hpp), and fails when a box is widened past what it covers."""
import math

import pytest

from scripts import two_layer_box_proof as proof

EDGES = ("Lambda0", "A", "EffEta", "Eta", "Cs", "Cd", "H", "Forcing", "State")


def test_the_kernels_boxes_are_proven():
    boxes = proof.read_boxes()
    assert set(boxes) == set(EDGES)
    out = proof.prove(boxes)
    assert len(out) == 8
    for name, v in out.items():
        assert "-0" not in v.kinds, name
        assert v.lo >= proof.WINDOW_LO and v.hi < math.ldexp(1.0, proof.WINDOW_HI), name


def test_the_kernels_state_box_is_the_widest_the_proof_allows_upwards():
    boxes = proof.read_boxes()
    lo, hi = boxes["State"]
    with pytest.raises(proof.ProofError, match="513"):
        proof.prove(dict(boxes, State=(lo, hi + 1)))


@pytest.mark.parametrize("name,side,step", [("State", 0, -300), ("Forcing", 0, -400), ("A", 1, 16), ("Cs", 0, -16), ("H", 1, 16),
                                            ("Lambda0", 1, 40), ("Eta", 0, -300), ("EffEta", 0, -300), ("Cd", 1, 200)])
def test_a_widened_box_is_refused(name, side, step):
    boxes = proof.read_boxes()
    b = list(boxes[name])
    b[side] += step
    with pytest.raises(proof.ProofError):
        proof.prove(dict(boxes, **{name: tuple(b)}))


def test_sign_rules():
    """-0 forcing or a zero state would let a numerator be -0; a negative eta would too."""
    boxes = proof.read_boxes()
    zero_state = proof.V({"+", "-", "+0", "-0"}, -10, 1.0)
    diff = proof.sub(zero_state, zero_state)
    assert "-0" in diff.kinds
    assert "-0" in proof.mul(proof.V({"-"}, -1, 1.0), proof.V({"+0"}, 0, 0.0)).kinds
    assert proof.add(proof.V({"+"}, -3, 1.0), proof.V({"-"}, -5, 1.0)).lo == -3 - 53
    with pytest.raises(proof.ProofError, match="divisor"):
        proof.prove(dict(boxes, Cd=(0, 130)))
