"""The facts the host proves once per launch about the years of an EXACT two-layer run, rscm::tl::YearFacts
(rscm_amd/csrc/two_layer_year_facts.hpp): the common RK4 sub-step count of a step range and whether every forcing value the range can
read -- all scenarios, the look-ahead's clamp included -- is +0 or a magnitude in the chunk guard's forcing box.  The kernel skips its
per-year checks on their word, so tests/c_abi/year_facts_host.cpp walks them over empty and one-step ranges, a differing count at the
first, the last and the position past a range, every edge value of the box at every index with both source offsets, several
scenarios, and a table replaced.  Built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "rscm_amd", "csrc", "two_layer_year_facts.hpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("year_facts") / "year_facts_host")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-g", "-O1", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "rscm_amd", "csrc"), os.path.join(ROOT, "tests", "c_abi", "year_facts_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_every_fact_holds_exactly_where_the_range_allows_it(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "year_facts ok" in r.stdout


def test_the_header_is_host_only_and_takes_the_box_from_its_header():
    """No HIP include, and the forcing box's edges come from two_layer_chunk_box.hpp: no exponent of it is restated."""
    with open(HEADER) as f:
        text = f.read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert '"two_layer_chunk_box.hpp"' in includes
    assert not [i for i in includes if "hip" in i], includes
    assert [i for i in includes if i.startswith('"')] == ['"two_layer_chunk_box.hpp"']
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "chunk::kForcingLo" in code and "chunk::kForcingHi" in code
    assert "-128" not in code and "ldexp(1.0, 13)" not in code
