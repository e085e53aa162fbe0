"""The integer pieces of the moments of stored rows (rscm_amd/csrc/moment_window.hpp: a term as five digits, a digit into a lane's
window register, the fold of the windows into the 68 limbs) on the host: tests/c_abi/moment_window_host.cpp includes that header
alone and links nothing of the project.  Built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program that
plays a wave of 64 lanes: for single edge terms (2^-1074, subnormals, the largest finite double, w = 2^53 - 1, both signs), terms at
both edges of the window and just outside, random terms over the whole range of doubles and a sequence that moves the window up
and down, window-add plus fold equals the direct placement into the limbs as canonical integers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "rscm_amd", "csrc", "moment_window.hpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("moment_window") / "moment_window_host")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall",
           "-I", os.path.join(ROOT, "rscm_amd", "csrc"), os.path.join(ROOT, "tests", "c_abi", "moment_window_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_window_add_and_fold_equal_the_direct_placement(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "moment_window ok (" in r.stdout


def test_the_header_needs_nothing_of_the_project():
    """moment_window.hpp includes the standard library only: no HIP."""
    with open(HEADER) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
