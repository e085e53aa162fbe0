"""The finishing step of the cross-member moments, rscm::moment_finish (rscm_amd/csrc/moments_finish.hpp), on the host:
tests/c_abi/moments_finish_host.cpp includes that header alone and links nothing of the project.  Built with AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program and run over the synthetic blocks of tests/host_moments.finish_cases (ties in
both directions, the subnormal range, the largest finite double, negative sums, limbs near +-2^62 with carries deferred through
every limb, a zero sum, no weight, a flagged block) and the refusals (n_terms = 2^31, a negative divisor): every result bit for bit
the Fraction's, and no shift, overflow or out-of-bounds read the sanitizers object to."""
import os
import subprocess

import numpy as np
import pytest

from tests import host_moments as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("moments_finish") / "moments_finish_host")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall",
           "-I", os.path.join(ROOT, "rscm_amd", "csrc"), os.path.join(ROOT, "tests", "c_abi", "moments_finish_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_every_synthetic_block_finishes_as_its_fraction(exe, tmp_path):
    cases = hm.finish_cases()
    lines = []
    for _, block, W, want in cases:
        lines.append(" ".join([str(W), "1000", "0", f"{int(np.float64(want).view(np.uint64)):016x}"] + [str(x) for x in block]))
    zero = ["0"] * hm.BLOCK
    lines.append(" ".join(["1", str(hm.MAX_TERMS), "1", "0"] + zero))          # n_terms = 2^31 is refused
    lines.append(" ".join(["1", str(hm.MAX_TERMS - 1), "0", "0"] + zero))      # one fewer is taken
    lines.append(" ".join(["1", "-1", "1", "0"] + zero))
    lines.append(" ".join(["-1", "5", "1", "0"] + zero))                       # a negative divisor
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert f"moments_finish ok ({len(lines)} cases)" in r.stdout


def test_the_header_needs_nothing_of_the_project():
    """moments_finish.hpp includes the standard library only: no HIP."""
    with open(os.path.join(ROOT, "rscm_amd", "csrc", "moments_finish.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
