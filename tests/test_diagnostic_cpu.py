"""CPU tier of the diagnostic variables (ABI minor 18): the boundary declares and binds the new entry points, and the data the GPU
tier (tests/test_gpu_diagnostic.py) compares on can tell the definition -- multiply, round, add, round, left to right -- from a
fused multiply-add and from another order of summation.  No device call is made."""
import os
import re
from fractions import Fraction

import numpy as np

from rscm_amd import _lib
from tests import host_diagnostic as hd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rscm_ens_define_diagnostic", "rscm_ens_diagnostic", "rscm_ens_compute_diagnostic", "rscm_ens_clear_diagnostics",
         "rscm_ens_n_diagnostics")


def test_abi_minor_18_declares_and_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", header).group(1)) >= 18
    assert int(re.search(r"#define\s+RSCM_DIAG_MAX_TERMS\s+(\d+)", header).group(1)) == _lib.DIAG_MAX_TERMS == 4
    assert int(re.search(r"#define\s+RSCM_DIAG_MAX\s+(\d+)", header).group(1)) == _lib.DIAG_MAX == 4
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 18
    for name in NAMES:
        assert re.search(r"RSCM_API\s+int\s+" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_python_surface_exists():
    import rscm_amd
    from rscm_amd.core import GraphModel, ModelBuilder
    from rscm_amd.distributed import ShardedEnsemble
    for cls, names in ((rscm_amd.Ensemble, ("define_diagnostic", "compute_diagnostic", "diagnostics", "clear_diagnostics", "define_heat_content")),
                       (GraphModel, ("define_diagnostic", "compute_diagnostic")), (ModelBuilder, ("with_diagnostic",)),
                       (ShardedEnsemble, ("define_diagnostic", "compute_diagnostic"))):
        for name in names:
            assert hasattr(cls, name), (cls.__name__, name)


def test_the_gpu_data_can_tell_a_fused_multiply_add_from_the_definition():
    """The first 64 members of the GPU file's two-term case on its random rows: w0 x0 + w1 x1 with the last product exact and
    ONE rounding (what v_fma_f64 would give) differs from the restatement for at least one member."""
    n, first = 257, 64
    P, _ = hd.two_layer_case(n)
    x = hd.random_rows(n)
    want = hd.diagnostic(hd.HEAT_CONTENT, [x[0], x[1]], P)
    w = hd.weights(hd.HEAT_CONTENT, P)
    differ = 0
    for r in range(x.shape[1]):
        for i in range(first):
            head = float(w[0][i]) * float(x[0, r, i])                                  # rounded
            fused = float(Fraction(head) + Fraction(float(w[1][i])) * Fraction(float(x[1, r, i])))   # exact product and sum, one rounding
            assert np.isfinite(want[r, i]) and abs(fused - want[r, i]) <= 2.0 * np.spacing(abs(want[r, i]))
            differ += fused != want[r, i]
    assert differ >= 1, "no member of the GPU test's data distinguishes fma from multiply-then-add"


def test_the_order_of_summation_matters_on_the_restatements_own_data():
    terms, sources, P = hd.random_case(4, 64)
    left, right = hd.diagnostic(terms, sources, P), hd.diagnostic_right_to_left(terms, sources, P)
    assert np.isfinite(left).all() and (left != right).any()
    # ... and a one-term diagnostic with scale 1.0 and no parameter row is the row itself, bit for bit
    assert np.array_equal(hd.diagnostic([(1, None, 1.0)], sources[:1], P), sources[0])


def test_restatement_propagates_specials_by_ieee_arithmetic():
    P = np.array([[2.0, np.nan, 0.0, 1.0]])
    x = np.array([[[np.inf, 1.0, 3.0, 5e-324]], [[1.0, 1.0, -np.inf, 0.0]]])
    y = hd.diagnostic([(1, 0, -2.5), (2, None, 1.0)], x, P)[0]
    assert np.isneginf(y[0]) and np.isnan(y[1]) and np.isneginf(y[2]) and y[3] == -2.5 * 5e-324
    assert np.signbit(hd.weights([(1, 0, -2.5)], P)[0][2])                              # -2.5 * 0.0 is -0.0
