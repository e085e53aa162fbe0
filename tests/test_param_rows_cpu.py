"""The condition that keeps tests/test_gpu_param_rows.py from being vacuous, on the CPU oracles alone: every parameter row of every
kind has a class, and every non-structural row, varied alone over the members, changes the oracle's output in at least one of the
kind's configurations (tests/param_rows.py).  The rows that change nothing anywhere are the frozen sets DEAD_ROWS: rows the block
carries and no solve reads."""
import numpy as np
import pytest

from rscm_amd import _lib as L
from tests import param_rows as R

_LIVE = {}


def _live(kind):
    if kind not in _LIVE:
        sp = R.spec(kind)
        _LIVE[kind] = R.liveness(sp, [R.varied_block(sp, R.N_MEMBERS, c) for c in range(len(sp.configs))])
    return _LIVE[kind]


def test_every_row_of_every_kind_has_a_class():
    assert set(R.KINDS) == set(L.KIND_TABLE) and len(R.KINDS) == 18
    total = 0
    for kind in R.KINDS:
        sp = R.spec(kind)
        assert sp.P == L.KIND_TABLE[kind][1] == len(sp.names) and len(set(sp.names)) == sp.P, sp.name
        assert set(sp.switch) <= set(sp.names) and set(sp.structural) <= set(sp.names) and not set(sp.switch) & set(sp.structural), sp.name
        assert all(sp.row_class(j) in ("continuous", "switch", "structural") for j in range(sp.P))
        assert len(sp.tol) == sp.n_vars and (sp.fast_tol is None or len(sp.fast_tol) == sp.n_vars), sp.name
        for _, d in sp.configs:
            assert d.shape == (sp.P,)
            for nm, legal in sp.switch.items():
                assert d[sp.names.index(nm)] in legal, (sp.name, nm)
        total += sp.P
    assert total == 517


def test_structural_rows_are_the_ones_the_header_marks():
    """include/rscm_gpu.h marks the ensemble-wide rows [u]: nine of ClimateUDEB, five of OceanCarbon, GhgForcing's method."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rscm_gpu.h")).read()
    ud = set(re.findall(r"#define RSCM_UD_P_(\w+) +\d+ +/\* \[u\]", text))
    alias = {"LAND_HC_ENABLED": "land_heat_capacity_enabled"}
    assert {alias.get(x, x.lower()) for x in ud} == set(R.spec(L.KIND_UDEB).structural) and len(ud) == 9
    oc = text[text.index("params  model [u]"):text.index("[u] rows are uniform")]
    assert set(re.findall(r"(\w+) \[u\]", oc)) == set(R.spec(L.KIND_OCEAN_CARBON).structural)
    assert re.search(r"#define RSCM_GH_P_METHOD 0 +/\* \[u\]", text) and R.spec(L.KIND_GHG_FORCING).structural == ("method",)
    assert sum(len(R.spec(k).structural) for k in R.KINDS) == 15


@pytest.mark.parametrize("kind", R.KINDS, ids=[R.KIND_NAMES[k] for k in R.KINDS])
def test_every_free_row_changes_the_oracle_output_somewhere(kind):
    sp = R.spec(kind)
    V = R.varied_block(sp, R.N_MEMBERS)
    for j in sp.free_rows():   # the draw itself varies: member 1 differs from member 0
        assert V[j, 0] != V[j, 1] and len(np.unique(V[j])) > 1, (sp.name, sp.names[j])
    for j in range(sp.P):
        if sp.row_class(j) == "structural":
            assert len(np.unique(V[j])) == 1
    live = _live(kind)
    dead = frozenset(sp.names[j] for j in sp.free_rows() if not live[:, j].any())
    print(f"{sp.name}: {sp.P} rows, {len(sp.free_rows())} free; live per configuration "
          f"{[int(live[c].sum()) for c in range(len(sp.configs))]}; dead everywhere {sorted(dead)}")
    assert dead == R.DEAD_ROWS.get(kind, frozenset())
    assert frozenset(nm for nm in dead if sp.row_class(sp.names.index(nm)) == "continuous") == R.DEAD_CONTINUOUS.get(kind, frozenset())
    base = sp.run(R.block(sp, V, [], 0), R.scen_map(R.N_MEMBERS))
    assert not np.isnan(base[:, 1:]).any()   # the default run is a real trajectory, not NaN against NaN


def test_dead_rows_under_the_defaults():
    """Rows that never change the output under one configuration, method by method (structural rows counted as dead, as a caller
    who may not vary them sees it): what the second configurations are for."""
    def dead(kind, config):
        sp = R.spec(kind)
        return {sp.names[j] for j in range(sp.P) if not _live(kind)[config, j]}
    harm = {"harmonize", "harmonize_year", "harmonize_target"}
    assert dead(L.KIND_AEROSOL_DIRECT, 0) == harm and dead(L.KIND_AEROSOL_INDIRECT, 0) == harm
    olbl, tar = dead(L.KIND_GHG_FORCING, 0), dead(L.KIND_GHG_FORCING, 1)
    assert olbl == {"method", "delq2xco2", "ch4_radeff", "n2o_radeff"}
    assert tar == {"method"} | {nm for nm in R.spec(L.KIND_GHG_FORCING).names if nm.startswith("olbl_")} and len(tar) == 12
    hc = dead(L.KIND_HALOCARBON, 0)
    assert len(hc) == 74 and "eesc_delay" in hc
    assert all(nm == "eesc_delay" or nm.rsplit(".", 1)[1] in ("n_cl", "n_br", "fractional_release") for nm in hc)
    assert dead(L.KIND_HALOCARBON, 1) == {"eesc_delay"}
