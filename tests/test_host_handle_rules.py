"""The two host-only descriptions behind a handle's rules (rscm_amd/csrc): the one table of structural parameter rows
(structural_rows.hpp) -- what the samplers and the Latin hypercube refuse and what the configuration checks for uniformity -- and the
internal component state as runs of rows (internal_state.hpp) -- what the checkpoint and the branch copy.  tests/c_abi/handle_rules_host.cpp
walks them: every table entry inside its kind's rows and listed once; ClimateUDEB's three runs at 2, 50 and 65 layers and the first, the
second and the last time index; OceanCarbon's ring empty, partly filled, exactly full, at its first wrap and after many rounds, against a
loop that walks the ring one row at a time; no runs for the other kinds.  Built with AddressSanitizer and UndefinedBehaviorSanitizer as
a stand-alone program.  The printed table is compared here with the rows tests/param_rows.py calls structural."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rscm_amd", "csrc")
HEADERS = ("structural_rows.hpp", "internal_state.hpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("handle_rules") / "handle_rules_host")
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined", "-g", "-O1", "-Wall", "-Werror",
           "-I", CSRC, os.path.join(ROOT, "tests", "c_abi", "handle_rules_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def output(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def test_the_table_and_the_state_runs_hold_their_checks(output):
    assert "handle_rules ok" in output


def test_the_table_lists_the_rows_the_parameter_catalogue_calls_structural(output):
    """(kind, row, name) for every structural row of tests/param_rows.py -- the 15 rows tests/test_param_rows_cpu.py counts -- and
    the N2O delay as the one further entry."""
    from rscm_amd import _lib as L
    from tests import param_rows as R
    table = set()
    for line in output.splitlines():
        if line[:1].isdigit():
            kind, row, name = line.split(" ", 2)
            table.add((int(kind), int(row), name))
    want = {(k, R.spec(k).names.index(name), name) for k in R.KINDS for name in R.spec(k).structural}
    assert len(want) == 15
    extra = table - want
    assert want <= table and len(extra) == 1, (sorted(want - table), sorted(extra))
    kind, row, _ = next(iter(extra))
    assert kind == L.KIND_N2O_CHEMISTRY and R.spec(kind).names[row] == "strat_delay"


def test_the_headers_are_host_only():
    """No HIP include in either; the table includes nothing but the boundary header."""
    includes = {}
    for h in HEADERS:
        with open(os.path.join(CSRC, h)) as f:
            includes[h] = [line.split()[1] for line in f.read().splitlines() if line.startswith("#include")]
        assert not [i for i in includes[h] if "hip" in i], (h, includes[h])
    assert includes["structural_rows.hpp"] == ['"../../include/rscm_gpu.h"']
    assert includes["internal_state.hpp"] == ['"kinds.hpp"']
    with open(os.path.join(CSRC, "kinds.hpp")) as f:
        assert not [line for line in f.read().splitlines() if line.startswith("#include") and "hip" in line]
    with open(os.path.join(ROOT, "tests", "c_abi", "handle_rules_host.cpp")) as f:
        own = [line.split()[1] for line in f.read().splitlines() if line.startswith("#include") and '"' in line]
    assert sorted(own) == ['"internal_state.hpp"', '"structural_rows.hpp"']
