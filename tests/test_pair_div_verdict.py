"""The verdict per divisor of the two-instruction quotient (rscm_amd/csrc/pair_div_verdict.hpp) as host code:
tests/c_abi/pair_div_host.cpp compiles the header on its own -- once plainly, once with AddressSanitizer and
UndefinedBehaviorSanitizer -- and prints constants and verdicts, which must be those of the integer restatement in
scripts/pair_div_proof.py, bit for bit, on about 1e4 divisors: both heat-capacity ranges of the benchmark, powers of two, even
significands with one to five trailing zeros, 1 +- ulp and the edges of the divisor box.  tests/golden/pair_div_unsafe.json lists
divisors of those ranges whose constants as defined fail, each with a failing numerator.  The last test is the cap on what the pair
lane can give: the share of 64-member blocks of the benchmark's Latin hypercube in which every heat capacity has safe constants."""
import json
import math
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_sampler  # noqa: E402

from tests.helpers import load_script  # noqa: E402

P = load_script("pair_div_proof")

GOLDEN = os.path.join(ROOT, "tests", "golden", "pair_div_unsafe.json")
# bench.py's headline draw, from bench.py itself: the parameter ranges, the seed and the default size
_bench = load_script("bench", folder="")
BENCH_LOW, BENCH_HIGH, BENCH_SEED = list(_bench.TL_LOW), list(_bench.TL_HIGH), _bench.SEED


def _bench_members():
    """--members as bench.py's own parser defaults it"""
    with open(os.path.join(ROOT, "bench.py")) as f:
        m = re.search(r'add_argument\("--members", type=int, default=([0-9_]+)', f.read())
    assert m, "bench.py no longer states the headline's member count where this test reads it"
    return int(m.group(1).replace("_", ""))


BENCH_MEMBERS = _bench_members()


def _build(tmp, name, extra):
    out = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "rscm_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_abi", "pair_div_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("pair_div")


@pytest.fixture(scope="module")
def exe(tmp):
    return _build(tmp, "pair_div_host", ["-O2"])


@pytest.fixture(scope="module")
def exe_sanitized(tmp):
    return _build(tmp, "pair_div_host_san", ["-O1", "-fsanitize=address,undefined"])


def _run(exe, tmp, divisors, *args):
    path = str(tmp / "divisors.bin")
    np.asarray(divisors, dtype="<f8").tofile(path)
    r = subprocess.run([exe, path, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def _f(hexbits):
    return struct.unpack("<d", struct.pack("<Q", int(hexbits, 16)))[0]


def _divisors():
    rng = random.Random(20260327)
    d = [rng.uniform(5.0, 15.0) for _ in range(4500)] + [rng.uniform(50.0, 200.0) for _ in range(4500)]
    d += [2.0 ** k for k in range(-4, 17)]                                       # powers of two, past both edges of the box
    for z in range(1, 6):                                                        # even significands: z trailing zero bits
        for _ in range(100):
            y = (1 << 52) | (rng.getrandbits(52) & ~((2 << z) - 1)) | (1 << z)
            d.append(math.ldexp(float(y), rng.randrange(-2, 14) - 52))
    d += [math.nextafter(1.0, 2.0), math.nextafter(1.0, 0.0), 1.0, 3.0, 5.0, 7.0, 10.0, 0.1, 1.0 / 3.0]
    d += [0.25, math.nextafter(0.25, 0.0), math.nextafter(0.25, 1.0), 16384.0, math.nextafter(16384.0, 0.0), math.nextafter(16384.0, 1e9)]
    d += [rng.uniform(0.25, 16384.0) for _ in range(400)]
    d += [float.fromhex(g["divisor"]) for g in json.load(open(GOLDEN))]
    return d


def test_constants_and_verdicts_equal_the_integer_restatement(exe, exe_sanitized, tmp):
    divisors = _divisors()
    assert len(divisors) >= 10_000
    out = _run(exe, tmp, divisors)
    assert out == _run(exe_sanitized, tmp, divisors)   # the sanitized build: the same output and no report
    rows = out.split("\n")[:-1]
    assert len(rows) == len(divisors)
    seen = {}
    for d, row in zip(divisors, rows):
        bits, zh, zl, variant = row.split()
        variant = int(variant)
        seen[variant] = seen.get(variant, 0) + 1
        assert _f(bits) == d
        if not 0.25 <= d < 16384.0:
            assert (variant, _f(zh), _f(zl)) == (-2, 0.0, 0.0), d.hex()
            continue
        assert (variant, _f(zh), _f(zl)) == P.verdict_f64(d), d.hex()
    assert all(seen.get(v, 0) > 0 for v in (-2, -1, 0, 1, 2)), seen   # every outcome occurs
    # the surface equation's deeper window, asked for by name: the same constants, or a refusal where zl is too small for it
    deep = P.SURFACE_NUM_FLOOR
    sample = [d for d in divisors if 0.25 <= d < 16384.0][::10] + [math.ldexp(float((1 << 52) + 1), -50), math.ldexp(float((1 << 52) + 3), -44)]
    refused = 0
    for d, row in zip(sample, _run(exe, tmp, sample, "rows", str(deep)).split("\n")):
        _, zh, zl, variant = row.split()
        assert (int(variant), _f(zh), _f(zl)) == P.verdict_f64(d, num_lo=deep), d.hex()
        refused += int(variant) == -1 and P.verdict_f64(d)[0] >= 0
    assert refused >= 2


def test_a_small_zl_limits_how_far_down_the_window_reaches():
    """The header's rule for the window's lower edge: n zl normal there.  A divisor whose zl is tiny is refused for a deeper window
    than the one that holds for every divisor, a typical one is not (the restatement; the header equals it above)."""
    Y = (1 << 52) + 1   # 1/d = 1 - 2^-52 + 2^-104 - ...: zh = 1 - 2^-52, zl just below 2^-104
    zh, zl = P.constants(Y, 53)
    ez = abs(zl[0]).bit_length() - 1 + zl[1]
    assert ez == -105
    assert P.verdict(Y, 53, min_zl_exp=ez - 1)[0] == P.verdict(Y, 53)[0] >= 0   # (its neighbour below keeps the exponent)
    assert P.verdict(Y, 53, min_zl_exp=ez + 1)[0] == -1
    assert P.verdict_f64(10.0, num_lo=-946)[0] == 0


def test_golden_divisors_fail_with_the_constants_as_defined():
    golden = json.load(open(GOLDEN))
    assert len(golden) >= 50
    rescued = stay = 0
    for g in golden:
        d, n = float.fromhex(g["divisor"]), float.fromhex(g["numerator"])
        assert 5.0 <= d <= 15.0 or 50.0 <= d <= 200.0
        Y, _ = P.significand(d)
        X, _ = P.significand(n)
        zh, zl = P.constants(Y, 53)
        assert P.quotient(X, zh, zl, 53) != P.ieee(X, Y, 53)
        # ... which the host's own arithmetic confirms: zh, zl and the quotient in f64
        fzh = 1.0 / d
        fzl = P.to_double(zl, -P.significand(d)[1])
        assert P.to_double(zh, -P.significand(d)[1]) == fzh
        v = P.verdict_f64(d)
        assert v[0] == g["variant"] and v[0] != 0
        if v[0] > 0:
            rescued += 1
            Xs = (X, 1 - 53)
            zhv, zlv = P.constants(Y, 53, P.VARIANT_STEPS[v[0]])
            assert P.fma(Xs, zhv, P.mul(Xs, zlv, 53), 53) == P.ieee(X, Y, 53)
            assert fzl != v[2]
        else:
            stay += 1
    assert rescued > 0 and stay > 0


def test_share_of_wholly_safe_wavefronts_in_the_benchmarks_draw(exe, tmp):
    """At least 0.85 of the 64-member blocks of the benchmark's 1e5-member Latin hypercube have safe constants for all 128 divisors:
    below that the pair lane is not worth its code."""
    m = host_sampler.lhs_matrix(BENCH_SEED, BENCH_LOW, BENCH_HIGH, 0, BENCH_MEMBERS, BENCH_MEMBERS)
    # as the device forms them: Cs vouched for down to the surface equation's numerators, Cd for the window that holds for every divisor
    flags = _run(exe, tmp, m[4], "flags", str(P.SURFACE_NUM_FLOOR)).strip() + _run(exe, tmp, m[5], "flags").strip()
    safe = np.frombuffer(flags.encode(), dtype=np.uint8) == ord("1")
    assert safe.size == 2 * BENCH_MEMBERS
    member = safe[:BENCH_MEMBERS] & safe[BENCH_MEMBERS:]
    n_blocks = (BENCH_MEMBERS + 63) // 64
    padded = np.ones(n_blocks * 64, dtype=bool)
    padded[:BENCH_MEMBERS] = member
    share = padded.reshape(n_blocks, 64).all(axis=1).mean()
    print(f"members without safe constants: {int((~member).sum())} of {BENCH_MEMBERS}; wholly safe blocks: {share:.4f} of {n_blocks}")
    assert share >= 0.85
