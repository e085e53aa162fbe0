"""CPU tier of the energy-budget diagnostics (ABI minor 22): the boundary declares and binds the new entry points, the data the GPU
tier (tests/test_gpu_energy_budget.py) compares on can tell the definition's association ((F - R) - X) + H from another one, the
restatement agrees with itself, and the Python front end refuses what it can refuse without a device.  No device call is made."""
import os
import re

import numpy as np
import pytest

from rscm_amd import _lib
from tests import host_diagnostic as hd
from tests import host_energy_budget as hb
from tests.helpers import same_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rscm_ens_define_energy_budget", "rscm_ens_diagnostic_quantity")


def test_abi_minor_22_declares_and_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", header).group(1)) >= 22
    for name, value in (("FORCING", _lib.BUDGET_FORCING), ("RESPONSE", _lib.BUDGET_RESPONSE), ("DEEP_UPTAKE", _lib.BUDGET_DEEP_UPTAKE),
                        ("IMBALANCE", _lib.BUDGET_IMBALANCE)):
        assert int(re.search(r"#define\s+RSCM_BUDGET_" + name + r"\s+(\d+)", header).group(1)) == value
    assert set(_lib.BUDGET_QUANTITIES) == set(hb.QUANTITIES) == set(_lib.BUDGET_DEFAULT_NAMES)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 22
    for name in NAMES:
        assert re.search(r"RSCM_API\s+int\s+" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_python_surface_exists():
    import rscm_amd
    from rscm_amd.core import GraphModel, ModelBuilder
    from rscm_amd.distributed import ShardedEnsemble
    for cls, names in ((rscm_amd.Ensemble, ("define_energy_budget", "define_toa_imbalance")), (GraphModel, ("define_energy_budget",)),
                       (ModelBuilder, ("with_energy_budget",)), (ShardedEnsemble, ("define_energy_budget",))):
        for name in names:
            assert hasattr(cls, name), (cls.__name__, name)


def _random_case(n):
    """The GPU file's parameters for n members with its random rows as Ts and Td, and a full-mantissa forcing."""
    P, _ = hd.two_layer_case(n)
    x = hd.random_rows(n)
    rng = np.random.default_rng(n + 22)
    F = np.where(rng.random(x[0].shape) < 0.5, -1.0, 1.0) * rng.uniform(0.01, 5.0, x[0].shape)
    return P, x[0], x[1], F


def test_the_gpu_data_can_tell_the_wrong_association_from_the_definition():
    P, Ts, Td, F = _random_case(257)
    want = hb.budget("imbalance", Ts, Td, P, F)
    wrong = hb.imbalance_wrong_association(Ts, Td, P, F)
    fin = np.isfinite(want) & np.isfinite(wrong)
    assert fin.sum() > want.size // 2 and (want[fin] != wrong[fin]).any()
    # ... and the two stay within a few ulp of the largest term: they are the same sum in real arithmetic
    big = np.maximum.reduce([np.abs(F), np.abs(hb.budget("response", Ts, Td, P, F)), np.abs(want)])
    assert (np.abs(want[fin] - wrong[fin]) <= 8.0 * np.spacing(big[fin]) + 8.0 * np.spacing(np.abs(P[2] * P[3] * (Ts - Td))[fin])).all()


def test_the_identity_holds_in_the_restatements_own_terms():
    P, Ts, Td, F = _random_case(64)
    t = hb.terms(Ts, Td, P, F)
    with np.errstate(all="ignore"):
        X = (P[2] * P[3]) * (Ts - Td)
        N = ((t["forcing"] - t["response"]) - X) + t["deep_uptake"]
    assert same_values(N, t["imbalance"]) and np.isfinite(N).any()
    assert same_values(t["deep_uptake"], P[3] * (Ts - Td))
    # scale: multiplied even by 1.0 (the same bits), and -2.5 is one more rounding of the quantity
    assert same_values(hb.budget("imbalance", Ts, Td, P, F, 1.0), N)
    assert same_values(hb.budget("response", Ts, Td, P, F, -2.5), -2.5 * t["response"])
    # with a = 0 the response is lambda0 Ts, the linear diagnostic [(Ts, row 0, 1.0)]
    P0 = P.copy()
    P0[1] = 0.0
    assert same_values(hb.budget("response", Ts, Td, P0, F), hd.diagnostic([(1, 0, 1.0)], [Ts], P0))


def test_member_forcing_is_the_existing_restatements():
    from tests import host_forcing_mix as hm
    from tests import host_forcing_noise_members as hnm
    n, T = 5, 9
    P, scen = hd.two_layer_case(n)
    table = np.stack([np.zeros(T), 0.05 * np.arange(T)])
    plain = hb.member_forcing(table, P, scen)
    assert plain.shape == (n, T) and np.array_equal(plain, table[scen])
    got = hb.member_forcing(table, P, scen, noise=("members", 3), member_offset=2)
    assert np.array_equal(got, hnm.noisy_forcing_members(table[scen], P[6], P[7], 3, 2))
    S = np.arange(2 * 2 * T, dtype=np.float64).reshape(2, 2, T)
    assert np.array_equal(hb.member_forcing(S, P, scen, n_comp=2), hm.mix_forcing(S, P[6:8], scen))
    assert np.array_equal(hb.rows_forcing(plain, 1, 8, 3, 1), plain[:, [2, 5, 8]].T)


def test_the_front_end_refuses_without_a_device():
    import rscm_amd
    e = object.__new__(rscm_amd.Ensemble)                                   # no handle: nothing below may reach the library
    e.var_ids = {"Effective Radiative Forcing": 0, "Surface Temperature": 1, "Deep Ocean Temperature": 2}
    e._diagnostic_names = {}
    with pytest.raises(ValueError, match="unknown energy-budget quantity"):
        e.define_energy_budget("albedo")
    with pytest.raises(ValueError, match="is taken"):
        e.define_energy_budget("imbalance", "Surface Temperature")
    e.var_ids["Top of Atmosphere Imbalance"] = 3
    with pytest.raises(ValueError, match="is taken"):
        e.define_toa_imbalance()
    with pytest.raises(ValueError, match="needs a name"):
        e.define_energy_budget("forcing", "")
    from rscm_amd.core import GraphModel, ModelBuilder

    class Home:                                                             # stands in for an ensemble of the graph
        def __init__(self, kind):
            self.kind, self.calls = kind, []

        def define_energy_budget(self, quantity, name, scale):
            self.calls.append((quantity, name, scale))
            return 3

    g = object.__new__(GraphModel)
    g._diagnostics, g._var_home = {}, {"Surface Temperature": ("tl", 1)}
    g.ensembles = {"erf": Home(_lib.KIND_CO2_ERF)}
    with pytest.raises(ValueError, match="exactly one two-layer ensemble"):
        g.define_energy_budget("response")                                  # none
    g.ensembles = {"tl": Home(_lib.KIND_TWO_LAYER), "tl2": Home(_lib.KIND_TWO_LAYER)}
    with pytest.raises(ValueError, match="exactly one two-layer ensemble"):
        g.define_energy_budget("response")                                  # several
    g.ensembles = {"erf": Home(_lib.KIND_CO2_ERF), "tl": Home(_lib.KIND_TWO_LAYER)}
    with pytest.raises(ValueError, match="unknown energy-budget quantity"):
        g.define_energy_budget("albedo")
    with pytest.raises(ValueError, match="is taken"):
        g.define_energy_budget("response", "Surface Temperature")
    assert g.define_energy_budget("deep_uptake", scale=2.0) == 3
    assert g.ensembles["tl"].calls == [("deep_uptake", "Deep Ocean Heat Uptake", 2.0)] and g.ensembles["erf"].calls == []
    assert g._diagnostics == {"Deep Ocean Heat Uptake": ("tl", 3)}
    with pytest.raises(ValueError, match="is taken"):
        g.define_energy_budget("deep_uptake")
    b = ModelBuilder().with_energy_budget("imbalance")
    with pytest.raises(ValueError, match="unknown energy-budget quantity"):
        b.with_energy_budget("albedo")
    with pytest.raises(ValueError, match="defined already"):
        b.with_energy_budget("imbalance")
