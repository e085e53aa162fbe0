"""Every parameter row of every kind read per member and through the uniform path (tests/param_rows.py): the host picks the path
from the bits it is handed (rscm_ens_set_params: uniform_rows; param_at / param_at_scalar / params_block; derived_uniform of the
member constants; LdsCache parameter slots of the fused launch), so the masks below are what selects the code under test.

One handle per kind stays open and takes one set_params + rewind + run per mask, as in a calibration; every stored variable at every
row is compared with the oracle run of exactly the block that was set, at the tolerance of the kind's own GPU test (bit equality
where that test asserts it).  130 members: two wavefronts and two lanes.  Masks (True: the row varies over the members), each in
EVERY configuration of the kind -- GhgForcing under both methods (ghg_kernel<0> / <1>, ghg_derive_sources(0) / (1)), ClimateUDEB
with and without efficacy, HalocarbonChemistry with and without chlorine and bromine in every species, Aggregate as Sum and Weighted:
  (a) all rows varied; all rows uniform (the all-scalar path of params_block at n > 1)
  (b) every non-structural row alone varied; the oracle must show the row acting in at least one configuration
  (c) every non-structural row below 64 alone uniform, the rest varied
  (d) eight seeded random masks and their complements
The kinds with a FAST mode repeat (a) and (d) in it.

The light kinds repeat every mask of (a), (c) and (d) through rscm_ens_run_lockstep: the same bits as run().  A call on one handle
alone is never fused (csrc/lockstep.cpp: a fused launch takes a segment of more than one handle), so the handle goes
  - next to a CO2ERF handle: one fused multi-step launch (csrc/group.hip).  The small kinds (group_kind_is_small) get LDS slots for their
    series and, where a row varies, for their parameters; OzoneForcing, AerosolDirect, CH4Chemistry, N2OChemistry and
    TerrestrialCarbon are not small and run the fused launch without any slot; GhgForcing without linked inputs is not fusable at
    all, its call is one-step launches of its own kernel;
  - (small kinds, masks (a) and (d)) in front of six more small handles whose series spend the 20-slot budget: the launch keeps LDS
    slots but none is left for the parameters of the handle under test (assign_cache_slots);
  - (masks (a)) alone: one-step launches.
tests/host_lockstep.cache_plan restates which of these a graph gets; the test asserts it reached them.
Structural rows varied over the members are refused and leave the handle as it was."""
import ctypes as C

import numpy as np
import pytest

from rscm_amd import _lib as L
from tests import host_lockstep as H
from tests import param_rows as R
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import assert_bit_equal, same_values

pytestmark = pytest.mark.gpu
N = R.N_MEMBERS
FAST_KINDS = (L.KIND_TWO_LAYER, L.KIND_COUPLED, L.KIND_UDEB, L.KIND_OCEAN_CARBON, L.KIND_CARBON_CYCLE)
# six small handles with 18 series: with the one to four series of the handle in front of them the 20 slots are spent
CROWD = (L.KIND_FOURBOX_OHU,) * 4 + (L.KIND_AEROSOL_INDIRECT, L.KIND_CO2_ERF)


@pytest.fixture(scope="module")
def stream(ra):
    s = C.c_void_p()
    L.check(L.load().rscm_gpu_stream_create(0, C.byref(s)))
    yield s.value
    L.check(L.load().rscm_gpu_stream_destroy(0, s))


def _slot_plan(kind, P, others, T):
    """assign_cache_slots restated (tests/host_lockstep.cache_plan) for the handle under test with parameters P in front of `others`
    (all with uniform parameters)."""
    g = H.hand_graph((kind,) + tuple(others), N=P.shape[1], T=T, uniform=True)
    g.nodes[0].params = P
    return H.cache_plan(g)


class Live:
    """One handle of the spec's kind with forcing and initial values set, and (light kinds) the handles it is fused with: a CO2ERF
    handle, and for the small kinds the CROWD."""

    def __init__(self, ra, sp, n, stream, mode=L.MODE_EXACT, companions=False):
        self.sp, self.n = sp, n
        self.scen = R.scen_map(n)
        self.e = ra.Ensemble(sp.kind, n, sp.bounds)
        self.other, self.crowd = None, []
        try:
            self.e.set_stream(stream)
            self.e.set_mode(mode)
            self.e.set_params(np.repeat(sp.default().reshape(-1, 1), n, axis=1))
            self.e.set_forcing(sp.inputs, self.scen)
            for v, x in sp.init.items():
                self.e.set_initial(v, x)
            if companions:
                self.other = self._companion(ra, L.KIND_CO2_ERF, stream)
                if sp.kind in H.SMALL_KINDS:
                    for k in CROWD:
                        self.crowd.append(self._companion(ra, k, stream))
        except Exception:
            self.close()
            raise

    def _companion(self, ra, kind, stream):
        """A handle of a stateless kind with its defaults for every member and the first scenario of its own description."""
        cs = R.spec(kind)
        assert cs.T == self.sp.T and not cs.init
        c = ra.Ensemble(kind, self.n, self.sp.bounds)
        try:
            c.set_stream(stream)
            c.set_params(np.repeat(cs.default().reshape(-1, 1), self.n, axis=1))
            c.set_forcing(cs.inputs[:1])
        except Exception:
            c.close()
            raise
        return c

    def series(self):
        return np.stack([self.e.get_series(v) for v in range(1, self.sp.n_vars + 1)])

    def run(self, P):
        self.e.set_params(P)
        self.e.rewind()
        self.e.run()
        return self.series()

    def lockstep(self, others=()):
        """The parameters of the last run() again, through rscm_ens_run_lockstep with `others` behind the handle."""
        from rscm_amd.ensemble import run_lockstep
        for h in (self.e,) + tuple(others):
            h.rewind()
        run_lockstep((self.e,) + tuple(others), self.sp.T - 1)
        return self.series()

    def close(self):
        for h in [self.e, self.other] + self.crowd:
            if h is not None:
                h.close()


def _all(sp, value):
    m = np.zeros(sp.P, dtype=bool)
    m[sp.free_rows()] = value
    return m


def _one(sp, j, value):
    m = _all(sp, not value)
    m[j] = value
    return m


@pytest.mark.parametrize("kind", R.KINDS, ids=[R.KIND_NAMES[k] for k in R.KINDS])
def test_every_row_on_the_uniform_and_the_per_member_path(ra, stream, kind):
    sp = R.spec(kind)
    configs = range(len(sp.configs))
    V = [R.varied_block(sp, N, c) for c in configs]
    scen = R.scen_map(N)
    free = sp.free_rows()
    small = kind in H.SMALL_KINDS
    count = dict(a=0, b=0, c=0, d=0, fast=0, lockstep=0, crowded=0)
    worst = dict(exact=0.0, fast=0.0)
    h = Live(ra, sp, N, stream, companions=sp.light)

    def check(mask, config, what, group, lockstep=False, crowd=False, alone=False):
        P = R.block(sp, V[config], mask, config)
        want = sp.run(P, scen)
        got = h.run(P)
        what = f"{sp.name} {what}, configuration {sp.configs[config][0]!r}"
        worst["exact"] = max(worst["exact"], R.deviation(sp, got, want, what))
        count[group] += 1
        if lockstep and sp.light:
            assert_bit_equal(h.lockstep((h.other,)), got, f"{what}: lock-step call next to a CO2ERF handle against run()")
            count["lockstep"] += 1
            if crowd and small:
                assert_bit_equal(h.lockstep(h.crowd), got, f"{what}: lock-step call with the slot budget spent against run()")
                count["crowded"] += 1
            if alone:
                assert_bit_equal(h.lockstep(), got, f"{what}: lock-step call on the handle alone against run()")
        return want

    try:
        if sp.light:   # what the two fused launches are, by the restated slot plan: parameter slots next to CO2ERF, none in the crowd
            P = R.block(sp, V[0], _all(sp, True))
            pair = _slot_plan(kind, P, (L.KIND_CO2_ERF,), sp.T)
            assert (pair is None) == (kind == L.KIND_GHG_FORCING)   # unlinked: not fusable, no fused launch to plan
            if pair is not None:
                assert (pair.slots > 0) == small and not pair.own_kernel
                assert (pair.param_slot[0] >= 0) == (small and kind != L.KIND_AGGREGATE)
            if small:
                crowded = _slot_plan(kind, P, CROWD, sp.T)
                assert crowded.slots > 0 and crowded.series_slot[0] == 0 and crowded.param_slot == [-1] * (1 + len(CROWD))
                assert not crowded.own_kernel and crowded.slots + sp.P > H.CACHE_SLOT_BUDGET
        base = []
        for c in configs:                  # (a)
            check(_all(sp, True), c, "(a) all rows varied", "a", lockstep=True, crowd=True, alone=True)
            base.append(check(_all(sp, False), c, "(a) all rows uniform", "a", lockstep=True, crowd=True, alone=True))
        for j in free:                     # (b)
            acts = False
            for c in configs:
                want = check(_one(sp, j, True), c, f"(b) row {j} ({sp.names[j]}) alone varied", "b")
                acts = acts or not same_values(want, base[c])
            # the comparisons were not vacuous: the row acts somewhere, or it is one of the rows no solve reads
            assert acts != (sp.names[j] in R.DEAD_ROWS.get(kind, ())), f"{sp.name}: row {j} ({sp.names[j]}): acts {acts}"
        masks = R.random_masks(sp)
        for c in configs:
            for j in free:                 # (c)
                if j < 64:
                    check(_one(sp, j, False), c, f"(c) row {j} ({sp.names[j]}) alone uniform", "c", lockstep=True)
            for k, m in enumerate(masks):  # (d)
                check(m, c, f"(d) random mask {k // 2}{' complement' if k % 2 else ''} {np.flatnonzero(m).tolist()}", "d", lockstep=True,
                      crowd=True)
    finally:
        h.close()
    if kind in FAST_KINDS:
        assert sp.fast_tol is not None
        h = Live(ra, sp, N, stream, mode=L.MODE_FAST)
        try:
            for k, m in enumerate([_all(sp, True), _all(sp, False)] + masks):
                P = R.block(sp, V[0], m, 0)
                what = f"{sp.name} FAST mask {k} {np.flatnonzero(m).tolist()}"
                worst["fast"] = max(worst["fast"], R.deviation(sp, h.run(P), sp.run(P, scen), what, fast=True))
                count["fast"] += 1
        finally:
            h.close()
    else:
        assert sp.fast_tol is None
    tols = sorted({t for t in sp.tol if t != R.BIT})
    print(f"{sp.name}: {sum(count[g] for g in 'abcd')} masks in EXACT mode over {len(sp.configs)} configuration(s) {dict(count)}; "
          f"largest deviation from the oracle {worst['exact']:.2e} (tolerance {tols if tols else 'bit equality'}"
          f"{', bit equality on ' + str(sum(t == R.BIT for t in sp.tol)) + ' variables' if tols and R.BIT in sp.tol else ''})"
          + (f"; FAST {worst['fast']:.2e} (tolerance {sorted(set(sp.fast_tol))})" if count["fast"] else ""))
    nc = len(sp.configs)
    assert count["a"] == 2 * nc and count["b"] == nc * len(free) and count["c"] == nc * sum(j < 64 for j in free) and count["d"] == 16 * nc
    assert count["lockstep"] == (count["a"] + count["c"] + count["d"] if sp.light else 0)
    assert count["crowded"] == (count["a"] + count["d"] if small else 0)


def test_udeb_one_thread_kernel_reads_every_row_both_ways(ra, stream):
    """More than 32 768 members take ClimateUDEB's one-thread-per-member kernel: (a) and four masks of (d) with their complements at
    33 000 members x 6 years, the oracle on 128 members from both ends and the middle."""
    n = 33_000
    sp = R.udeb_spec(T=7)
    V = R.varied_block(sp, n)
    scen = R.scen_map(n)
    pick = np.concatenate([np.arange(43), n // 2 - 21 + np.arange(42), n - 43 + np.arange(43)])
    assert len(pick) == 128
    worst = 0.0
    h = Live(ra, sp, n, stream)
    try:
        for k, m in enumerate([_all(sp, True), _all(sp, False)] + R.random_masks(sp, 4)):
            P = R.block(sp, V, m)
            got = h.run(P)
            want = sp.run(np.ascontiguousarray(P[:, pick]), scen[pick].copy())
            worst = max(worst, R.deviation(sp, got[:, :, pick], want, f"ClimateUDEB one-thread kernel mask {k} {np.flatnonzero(m).tolist()}"))
    finally:
        h.close()
    print(f"ClimateUDEB one-thread kernel, {n} members: 10 masks, largest deviation from the oracle {worst:.2e} (tolerance {sp.tol[0]:g})")


# ------------------------------------------------------------------------------------------------ structural rows
# a second legal value per structural row (what a member would hold if the row were allowed to vary)
OTHER_VALUE = {
    (L.KIND_UDEB, "n_layers"): 40.0, (L.KIND_UDEB, "mixed_layer_depth"): 66.0, (L.KIND_UDEB, "layer_thickness"): 110.0,
    (L.KIND_UDEB, "feedback_cumt_period"): 250.0, (L.KIND_UDEB, "depth_dependent_area"): 0.0,
    (L.KIND_UDEB, "land_heat_capacity_enabled"): 0.0, (L.KIND_UDEB, "efficacy_apply"): 1.0, (L.KIND_UDEB, "ocean_temp_profile"): 1.0,
    (L.KIND_UDEB, "steps_per_year"): 6.0,
    (L.KIND_OCEAN_CARBON, "model"): 1.0, (L.KIND_OCEAN_CARBON, "irf_scale"): 1.0, (L.KIND_OCEAN_CARBON, "steps_per_year"): 6.0,
    (L.KIND_OCEAN_CARBON, "max_history_months"): 5000.0, (L.KIND_OCEAN_CARBON, "irf_switch_time"): 2.0,
    (L.KIND_GHG_FORCING, "method"): 0.0,
}


def test_every_structural_row_has_a_case():
    assert sorted((k, nm) for k in R.KINDS for nm in R.spec(k).structural) == sorted(OTHER_VALUE) and len(OTHER_VALUE) == 15


@pytest.mark.parametrize("kind", sorted({k for k, _ in OTHER_VALUE}), ids=lambda k: R.KIND_NAMES[k])
def test_structural_rows_varied_over_the_members_are_refused(ra, stream, kind):
    """set_params with a structural row that differs between members returns RSCM_ERR_INVALID and leaves the handle as it was: a
    following run() gives the earlier bits, the parameter block is the earlier one.  sample_lhs with low != high on such a row
    likewise."""
    sp = R.spec(kind)
    V = R.varied_block(sp, N)
    P = R.block(sp, V, _all(sp, True))
    h = Live(ra, sp, N, stream)
    try:
        first = h.run(P)
        assert not np.isnan(first[:, 1:]).all()
        for nm in sp.structural:
            j = sp.names.index(nm)
            other = OTHER_VALUE[(kind, nm)]
            assert other != sp.default()[j]
            for where in (1, N - 1, slice(64, None)):   # one member of the first wavefront, the last member, the whole tail
                bad = P.copy()
                bad[j, where] = other
                with pytest.raises(ra.RscmGpuError) as err:
                    h.e.set_params(bad)
                assert err.value.code == L.ERR_INVALID, (nm, str(err.value))
                assert_bit_equal(h.e.get_params(), P, f"{sp.name} {nm}: parameter block after the refused call")
                h.e.rewind()
                h.e.run()
                assert_bit_equal(h.series(), first, f"{sp.name} {nm}: run() after the refused call")
            lo, hi = sp.default().copy(), sp.default().copy()
            lo[j], hi[j] = min(other, lo[j]), max(other, hi[j])
            with pytest.raises(ra.RscmGpuError) as err:
                h.e.sample_lhs(7, lo, hi)
            assert err.value.code == L.ERR_INVALID, (nm, str(err.value))
            assert_bit_equal(h.e.get_params(), P, f"{sp.name} {nm}: parameter block after the refused sample_lhs")
            h.e.rewind()
            h.e.run()
            assert_bit_equal(h.series(), first, f"{sp.name} {nm}: run() after the refused sample_lhs")
    finally:
        h.close()
