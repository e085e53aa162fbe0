"""The two comparisons every test file shares (tests/helpers.py), pinned by their truth tables -- same_values: +0 equals -0; same_bits:
the sign of a zero counts; under both any NaN equals any NaN and shapes must agree -- and the noisy two-layer case that the series,
diagnostic and energy-budget files draw their members from."""
import numpy as np
import pytest

from tests.helpers import assert_bit_equal, same_bits, same_values, two_layer_noise_case, two_layer_params

NAN_A = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]     # the quiet NaN
NAN_B = np.array([0xFFF0000000000ABC], dtype=np.uint64).view(np.float64)[0]     # another payload, sign set
ONE_UP = np.nextafter(1.0, 2.0)

# (what, a, b, same_values, same_bits)
TABLE = [
    ("+0 and -0", [0.0], [-0.0], True, False),
    ("+0 and +0", [0.0], [0.0], True, True),
    ("-0 and -0", [-0.0], [-0.0], True, True),
    ("two NaN payloads", [NAN_A], [NAN_B], True, True),
    ("NaN and a number", [np.nan], [1.0], False, False),
    ("a number and NaN", [0.0], [np.nan], False, False),
    ("+Inf and +Inf", [np.inf], [np.inf], True, True),
    ("-Inf and -Inf", [-np.inf], [-np.inf], True, True),
    ("+Inf and -Inf", [np.inf], [-np.inf], False, False),
    ("+Inf and NaN", [np.inf], [np.nan], False, False),
    ("+Inf and the largest double", [np.inf], [np.finfo(np.float64).max], False, False),
    ("the least denormal and 0", [5e-324], [0.0], False, False),
    ("the least denormals of both signs", [5e-324], [-5e-324], False, False),
    ("1 and its neighbour", [1.0], [ONE_UP], False, False),
    ("1 and 1", [1.0], [1.0], True, True),
    ("1 and -1", [1.0], [-1.0], False, False),
    ("one differing element among equal ones", [1.0, -0.0, NAN_A, 2.0], [1.0, 0.0, NAN_B, 2.0], True, False),
    ("all of them at once, equal", [[1.0, -0.0], [NAN_A, -np.inf]], [[1.0, -0.0], [NAN_B, -np.inf]], True, True),
    ("a shape mismatch", [1.0, 2.0], [[1.0, 2.0]], False, False),
    ("a length mismatch", [1.0, 2.0], [1.0], False, False),
    ("a scalar and a one-element array", 1.0, [1.0], False, False),
    ("empty arrays", [], [], True, True),
    ("two equal scalars", 2.5, 2.5, True, True),
    ("scalar zeros of both signs", 0.0, -0.0, True, False),
    ("an int array and its float image", np.array([-3, 0, 7]), np.array([-3.0, 0.0, 7.0]), True, True),
    ("an int zero and -0.0", np.array([0]), np.array([-0.0]), True, False),
    ("a float32 array and its float64 image", np.array([0.1, -2.5], dtype=np.float32),
     np.array([0.1, -2.5], dtype=np.float32).astype(np.float64), True, True),
]


@pytest.mark.parametrize("what,a,b,values,bits", TABLE, ids=[row[0] for row in TABLE])
def test_truth_table(what, a, b, values, bits):
    for x, y in ((a, b), (b, a)):                                # both predicates are symmetric
        got = same_values(x, y), same_bits(x, y)
        assert got == (values, bits) and all(type(g) is bool for g in got), (what, got)
    assert not bits or values                                   # bit equality implies value equality


@pytest.mark.parametrize("what,a,b,values,bits", TABLE, ids=[row[0] for row in TABLE])
def test_assert_bit_equal_raises_exactly_where_same_bits_is_false(what, a, b, values, bits):
    if bits:
        assert_bit_equal(a, b, what)
    else:
        with pytest.raises(AssertionError):
            assert_bit_equal(a, b, what)


def test_assert_bit_equal_names_the_first_difference():
    with pytest.raises(AssertionError, match=r"rows: 2 of 4 differ; first at \(.*\b0\b.*, .*\b1\b.*\): .*\b0\.0\b.* vs .*-0\.0\b"):
        assert_bit_equal([[1.0, 0.0], [NAN_A, 3.0]], [[1.0, -0.0], [NAN_B, 4.0]], "rows")


def test_noise_case_is_a_block_of_one_draw():
    """A shard's case is the slice of the whole draw, so sharded runs see the members of the one-handle run."""
    P, scen = two_layer_noise_case(1000)
    assert P.shape == (8, 1000) and scen.shape == (1000,) and scen.dtype == np.int32
    Pb, sb = two_layer_noise_case(257, 64, 1000)
    assert same_bits(Pb, P[:, 64:321]) and np.array_equal(sb, scen[64:321])
    assert Pb.flags.c_contiguous and sb.flags.c_contiguous
    assert same_bits(two_layer_noise_case(1000, 0, 1000)[0], P)
    assert same_bits(P[:6, :997], two_layer_params(1000)[:, :997])          # the six two-layer rows are the shared draw's


@pytest.mark.parametrize("n", [62, 63])
def test_noise_case_special_members(n):
    """From 63 members on: member n - 3 silent under zero forcing, member n - 2 with the amplitude 1.7e308, member n - 1 with a NaN
    in row 0; below 63 none, and everywhere else amplitudes in [0.1, 0.6), persistences in [0, 0.9), scenarios alternating."""
    P, scen = two_layer_noise_case(n)
    plain = n - 3 if n >= 63 else n
    assert np.isfinite(P[:, :plain]).all() and np.array_equal(scen[:plain], np.arange(plain) % 2)
    assert ((P[6, :plain] >= 0.1) & (P[6, :plain] < 0.6)).all() and ((P[7] >= 0.0) & (P[7] < 0.9)).all()
    if n < 63:
        return
    assert P[6, n - 3] == 0.0 and not np.signbit(P[6, n - 3]) and scen[n - 3] == 0
    assert P[6, n - 2] == 1.7e308 and scen[n - 2] == (n - 2) % 2
    assert np.isnan(P[0, n - 1]) and np.isfinite(P[1:, n - 1]).all() and scen[n - 1] == (n - 1) % 2
    assert np.isfinite(P[:, n - 3]).all() and np.isfinite(P[:, n - 2]).all()
