"""The owner of the host layer's device buffers, rscm::DevBuf -- a call's temporaries and the d_* members of the handle, the sampler and
the lock-step plan -- and rscm::dev_malloc (rscm_amd/csrc/dev_buf.hpp), on the host: tests/c_abi/dev_buf_host.cpp includes that header
alone, defines hipMalloc, hipFree, hipMemset and hipDeviceSynchronize as counting stubs over malloc / free (one of them can fail the
k-th allocation) and links no HIP library.  Built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, so a
double free, a use after free or a leak past any of its scenarios ends the run: scope exit, early return, a failed allocation, a
second alloc, moves, an exception; size() and the read as a pointer; reserve() below, at and above size() and with a failing
allocation; reset(); move-assignment of a local into a full and into an empty member; a struct of owners with an array of four
destroyed half full; "build aside, fail before the move"; a half-built object in a unique_ptr whose third allocation fails."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dev_buf") / "dev_buf_host")
    cmd = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined", "-g", "-O1", "-Wall",
           "-I", os.path.join(ROOT, "rscm_amd", "csrc"), os.path.join(ROOT, "tests", "c_abi", "dev_buf_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, poison):
    env = {k: v for k, v in os.environ.items() if k != "RSCM_POISON_ALLOC"}
    if poison:
        env["RSCM_POISON_ALLOC"] = "1"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def test_no_scenario_leaves_an_allocation_or_frees_one_twice(exe):
    assert "dev_buf ok (poison off)" in _run(exe, False)


def test_poisoned_allocations_are_filled_once_and_empty_ones_not_at_all(exe):
    assert "dev_buf ok (poison on)" in _run(exe, True)


def test_the_header_needs_nothing_of_the_project():
    """dev_buf.hpp includes the HIP runtime API and the standard library only."""
    with open(os.path.join(ROOT, "rscm_amd", "csrc", "dev_buf.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    assert [i for i in includes if "hip" in i] == ["<hip/hip_runtime_api.h>"]
