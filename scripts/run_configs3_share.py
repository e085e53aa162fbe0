"""BASELINE.json configs[3], one GPU's share at full size (run on the GPU box): the emissions-driven MAGICC
graph (ten rscm-magicc components, Sum of eight forcings, FourBox transforms), 125 000 members (1e6 / 8 GPUs),
MONTHLY model steps 1750-2500 (9001 points, 9000 steps), ClimateUDEB and OceanCarbon at their 12 sub-steps per
model step, series in a window of --window rows (default 96: 3.5 GB of the 288; the window slides once every ~80 steps) with annual
(every 12th) rows of every variable kept.

    python scripts/run_configs3_share.py [--members 125000] [--years 750] [--exact] [--plume [--weighted]]

Prints one JSON line: build / run wall time, HBM allocated, launches, member-years/s (a member-year = 12 model
steps here), ensemble statistics at the end, and -- the parity anchor at this size -- whether the first 64
members equal a 64-member run of the same graph, bit for bit, on every kept row of five variables."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rscm_amd import _lib as L  # noqa: E402
from scripts.bench_magicc_chain import build_chain  # noqa: E402

NAMES = ["Sea Surface Temperature", "Atmospheric Concentration|CO2", "Effective Radiative Forcing", "Atmospheric Concentration|CH4",
         "Carbon Flux|Ocean"]


def build(members, years, exact, window=16, device=0, member_offset=0, members_total=None):
    """The share's graph, built and in its arithmetic mode, ready to run (bench.py's N > 1 leg times `model.run()` itself)."""
    model = build_chain(members, years, "topological", steps_per_year=12, device=device, member_offset=member_offset,
                        members_total=members_total, series_window=window, output_stride=12)
    if not exact:
        model.set_mode(L.MODE_FAST)
    return model


PLUME_Q = [0.05, 0.17, 0.5, 0.83, 0.95]


def plume(model):
    """The annual plume of surface temperature on the device (GraphModel.quantile_rows over the output store, a radix select),
    timed after one warm-up call, against copying the same rows to the host and calling numpy.nanquantile."""
    model.quantile_rows("Surface Temperature", PLUME_Q, t_stride=12)
    t0 = time.perf_counter()
    got = model.quantile_rows("Surface Temperature", PLUME_Q, t_stride=12)
    dev_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ser = model.get_series("Surface Temperature", t_stride=12)
    copy_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        want = np.nanquantile(ser, PLUME_Q, axis=1).T
    np_s = time.perf_counter() - t0
    return {"rows": int(ser.shape[0]), "quantiles": PLUME_Q, "quantile_rows_ms": dev_s * 1e3, "host_copy_ms": copy_s * 1e3,
            "host_copy_mb": ser.nbytes / 1e6, "numpy_nanquantile_ms": np_s * 1e3,
            "equals_numpy": bool(np.array_equal(got["quantiles"], want, equal_nan=True)),
            "median_warming_end_K": float(got["quantiles"][-1][2]), "band_5_95_end_K": [float(got["quantiles"][-1][0]),
                                                                                           float(got["quantiles"][-1][4])]}


HIST_YEARS = (1850, 2014)   # the "historical" annual rows the weighted plume is constrained on
OBS_SIGMA = 0.1             # K


def weighted_plume(model):
    """The constrained plume: member weights from each member's fit to a historical record of annual surface temperature, then
    the weighted annual plume on the device (GraphModel.quantile_rows(weighted=True), numpy's "inverted_cdf"), against numpy's
    weighted nanquantile of the rows copied to the host.  The repository holds no observed record, so the record is a synthetic
    stand-in: member 0's own run (as scripts/calibrate_magicc_chain.py does).  The log-likelihood is formed on the host from
    the rows of the output store -- glue, not a device path."""
    ser = model.get_series("Surface Temperature", t_stride=12)
    lo, hi = HIST_YEARS[0] - 1750, min(HIST_YEARS[1] - 1750, ser.shape[0] - 1)
    hist = ser[lo:hi + 1]
    obs = hist[:, 0].copy()
    with np.errstate(all="ignore"):
        ll = -0.5 * (((hist - obs[:, None]) / OBS_SIGMA) ** 2).sum(axis=0)
    ll_max, bits = model.set_weights_from_loglik(ll)
    w = model.ensembles["ClimateUDEB"].member_weights()
    model.quantile_rows("Surface Temperature", PLUME_Q, t_stride=12, weighted=True)
    t0 = time.perf_counter()
    got = model.quantile_rows("Surface Temperature", PLUME_Q, t_stride=12, weighted=True)
    dev_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    live = got["weight"] > 0
    with np.errstate(all="ignore"):
        want = np.full_like(got["quantiles"], np.nan)
        want[live] = np.nanquantile(ser[live], PLUME_Q, axis=1, weights=np.broadcast_to(w, ser[live].shape), method="inverted_cdf").T
    np_s = time.perf_counter() - t0
    same = np.array_equal(np.where(got["quantiles"] == 0, 0.0, got["quantiles"]), np.where(want == 0, 0.0, want), equal_nan=True)
    return {"constrained_on": f"annual surface temperature {HIST_YEARS[0]}-{lo + 1750 + hist.shape[0] - 1}, member 0's run as "
                              f"the record, sigma {OBS_SIGMA} K", "ll_max": ll_max, "bits": bits,
            "ess": model.ensembles["ClimateUDEB"].weights_ess(), "weighted_quantile_rows_ms": dev_s * 1e3,
            "numpy_weighted_nanquantile_ms": np_s * 1e3, "equals_numpy": bool(same),
            "median_warming_end_K": float(got["quantiles"][-1][2]),
            "band_5_95_end_K": [float(got["quantiles"][-1][0]), float(got["quantiles"][-1][4])]}


def run(members, years, exact, window=16, device=0, member_offset=0, members_total=None, with_plume=False, weighted=False):
    free0, total = L.mem_info(device)
    t0 = time.perf_counter()
    model = build_chain(members, years, "topological", steps_per_year=12, device=device, member_offset=member_offset,
                        members_total=members_total, series_window=window, output_stride=12)
    if not exact:
        model.set_mode(L.MODE_FAST)
    build_s = time.perf_counter() - t0
    free1, _ = L.mem_info(device)
    L.check(L.load().rscm_gpu_lockstep_stats(None, None))
    t0 = time.perf_counter()
    model.run()
    run_s = time.perf_counter() - t0
    nl, ns = C.c_int64(), C.c_int64()
    L.check(L.load().rscm_gpu_lockstep_stats(C.byref(nl), C.byref(ns)))
    rows = {n: model.get_series(n, t_stride=12) for n in NAMES}
    plume_out = plume(model) if with_plume else None
    if with_plume and weighted:
        plume_out["weighted"] = weighted_plume(model)
    T = years * 12 + 1
    warm = model.ensembles["Transform:Surface Temperature"].summary(1, T - 1)
    co2 = model.ensembles["CO2Budget"].summary(1, T - 1)
    status = int(model.ensembles["ClimateUDEB"].status().sum())
    model.close()
    return dict(build_s=build_s, run_s=run_s, hbm_gib=(free0 - free1) / 2**30, hbm_total_gib=total / 2**30, launches=int(nl.value),
                component_steps=int(ns.value), warm=warm, co2=co2, failed=status, plume=plume_out), rows


def first_64(members, years, exact, window=16, device=0, member_offset=0, members_total=None):
    """Parity anchor at this size: a 64-member ensemble that is GIVEN the first 64 members' parameters of the
    `members`-member one (build_chain draws whole vectors from one seeded generator: replayed here for the big
    ensemble's draws).  Returns the kept (annual) rows of NAMES."""
    import scripts.bench_magicc_chain as mod
    small = build_chain(64, years, "topological", steps_per_year=12, device=device, series_window=window, output_stride=12)
    rng = np.random.default_rng(20260327)
    total = members if members_total is None else members_total
    first = slice(member_offset, member_offset + 64)
    ecs = rng.uniform(2.0, 4.5, total)
    kappa = rng.uniform(0.5, 1.2, total)
    beta_f = rng.uniform(0.7, 1.3, total)
    ud = small.ensembles["ClimateUDEB"]
    P = ud.get_params()
    P[L.UD_PARAM_NAMES.index("ecs")] = ecs[first]
    P[L.UD_PARAM_NAMES.index("kappa")] = kappa[first]
    ud.set_params(P)
    tc = small.ensembles["TerrestrialCarbon"]
    Q = tc.get_params()
    base_beta = mod.chain_components()[7].param_vector()[L.TC_PARAM_NAMES.index("beta")]
    Q[L.TC_PARAM_NAMES.index("beta")] = base_beta * beta_f[first]
    tc.set_params(Q)
    if not exact:
        small.set_mode(L.MODE_FAST)
    small.run()
    rows = {n: small.get_series(n, t_stride=12) for n in NAMES}
    small.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=125_000)
    ap.add_argument("--years", type=int, default=750)
    ap.add_argument("--exact", action="store_true", help="RSCM_MODE_EXACT: OceanCarbon's literal O(T^2) convolution")
    ap.add_argument("--window", type=int, default=96, help="rows of every series kept on the device (36 MB per row at 125 000 members)")
    ap.add_argument("--fusion", type=int, default=1, help="rscm_gpu_set_lockstep_fusion mode 0..3 (include/rscm_gpu_internal.h)")
    ap.add_argument("--no-anchor", action="store_true",
                    help="skip the 64-member parity anchor (profiling passes: half the dispatches; the anchor is checked by every un-profiled run)")
    ap.add_argument("--plume", action="store_true",
                    help="also time the annual 5/17/50/83/95 %% plume of surface temperature on the device (quantile_rows) against numpy")
    ap.add_argument("--weighted", action="store_true",
                    help="with --plume: also the plume weighted by each member's fit to a historical record (see weighted_plume)")
    args = ap.parse_args()
    L.check(L.load().rscm_gpu_set_lockstep_fusion(args.fusion))
    big, rows = run(args.members, args.years, args.exact, args.window, with_plume=args.plume, weighted=args.weighted)
    small_rows = {n: rows[n][:, :64] for n in NAMES} if args.no_anchor else first_64(args.members, args.years, args.exact, args.window)
    same = {}
    for n in NAMES:
        a, b = rows[n][:, :64], small_rows[n]
        same[n] = bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)) or np.array_equal(a, b, equal_nan=True))
    steps = args.years * 12
    out = {"workload": f"BASELINE configs[3], one GPU's share: MAGICC graph, {args.members} members x {steps} monthly steps "
                       f"({args.years} years), window {args.window} rows + annual outputs of all 36 series, mode {'EXACT' if args.exact else 'FAST'}",
           "run_s": big["run_s"], "build_s": big["build_s"], "member_years_per_s": args.members * args.years / big["run_s"],
           "member_model_steps_per_s": args.members * steps / big["run_s"], "ms_per_model_step": big["run_s"] / steps * 1e3,
           "launches": big["launches"], "launches_per_step": big["launches"] / steps, "hbm_allocated_gib": big["hbm_gib"],
           "hbm_total_gib": big["hbm_total_gib"], "failed_members": big["failed"],
           "warming_end_K": big["warm"], "co2_end_ppm": big["co2"],
           "first_64_members_equal_a_64_member_run": same}
    if args.plume:
        out["plume"] = big["plume"]
    print(json.dumps(out))
    sys.exit(0 if all(same.values()) and big["failed"] == 0 and (not args.plume or big["plume"]["equals_numpy"])
             and (not (args.plume and args.weighted) or big["plume"]["weighted"]["equals_numpy"]) else 1)


if __name__ == "__main__":
    main()
