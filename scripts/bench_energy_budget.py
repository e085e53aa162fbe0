"""Cost of the energy-budget diagnostics (Ensemble.define_energy_budget, csrc/energy_budget.hip) on the GPU, against the ocean heat
content (Ensemble.define_heat_content, csrc/diagnostic.hip) over the same rows as the yardstick: both read Ts and Td and write one
row per row and member, 24 B per element.  Two-layer ensembles after a run, 171 annual rows (the forcing-reading quantities over
the same 171: the source is exogenous, so the last row has its forcing index), three configurations -- a plain table, a mix handle
with K = 3 components, per-member red noise -- and for each the four quantities and the heat content, the calls in alternation in
one process.  Each call is timed by the host clock around it; a call returns after its kernel has finished (the entry point
synchronises the handle's stream), so the time is the row-pointer upload, the launch and the kernel.  Two warm-up rounds, then
--runs timed rounds; median, minimum and maximum are printed, the bytes by count (3 x 8 x R x N) over the median, and the ratio of
the medians to the heat content's.  The noise kinds pay one draw per forcing index from 0 on: for them the yardstick is
Ensemble.forcing_noise_rows over the same indices into device memory, timed the same way, and that ratio is printed too.
profiles/energy_budget_bench.txt holds one output of this script.

    python scripts/bench_energy_budget.py [--runs 20] [--sizes 100000 1000000]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd import _lib as L  # noqa: E402

R = 171
YEARS = np.arange(1850.0, 1850.0 + R)
BOUNDS = np.append(YEARS, YEARS[-1] + 1.0)
LO = [0.8, 0.0, 1.0, 0.5, 5.0, 50.0]
HI = [1.5, 0.1, 1.8, 1.0, 15.0, 200.0]
QUANTITIES = ("forcing", "response", "deep_uptake", "imbalance")
CONFIGS = ("plain", "mix K=3", "per-member noise")


def ensemble(config, n):
    t = YEARS - 1850.0
    F = 0.035 * t + 0.25 * np.sin(2.0 * np.pi * t / 11.0)
    if config == "mix K=3":
        e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS, forcing_components=3)
        e.sample_lhs(20260422, LO + [0.5, 0.5, 0.5], HI + [1.5, 1.5, 1.5])
        e.set_forcing(np.stack([0.6 * F, 0.3 * F, 0.1 * np.cos(2.0 * np.pi * t / 11.0)]))
    elif config == "per-member noise":
        e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS, noise_params=True)
        e.sample_lhs(20260422, LO + [0.1, 0.0], HI + [0.6, 0.9])
        e.set_forcing(F)
        e.set_forcing_noise_members(1)
    else:
        e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS)
        e.sample_lhs(20260422, LO, HI)
        e.set_forcing(F)
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run()
    return e


def timed(calls, sync, runs):
    out = {name: [] for name in calls}
    for r in range(runs + 2):
        for name, call in calls.items():
            sync()
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if r >= 2:
                out[name].append(1e3 * dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs must be at least 1")
    if rscm_amd._lib.device_count() < 1:
        raise SystemExit("bench_energy_budget.py needs a HIP device")
    for n in a.sizes:
        for config in CONFIGS:
            with ensemble(config, n) as e:
                # three of the four slots at a time: the heat content keeps one
                heat = e.define_heat_content()
                ms = {}
                for group in (QUANTITIES[:3], QUANTITIES[3:]):
                    ids = {q: e.define_energy_budget(q) for q in group}
                    calls = {"heat content": lambda: e.compute_diagnostic(heat, 0, R)}
                    calls.update({q: (lambda v=v: e.compute_diagnostic(v, 0, R)) for q, v in ids.items()})
                    if config == "per-member noise" and "imbalance" in ids:
                        with rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS) as scratch:   # R x N doubles on the device
                            out = C.c_void_p()
                            L.check(scratch._lib.rscm_ens_series_devptr(scratch._h, 1, C.byref(out)))
                            ptr = C.cast(out, C.POINTER(C.c_double))
                            calls["forcing_noise_rows"] = lambda: (L.check(e._lib.rscm_ens_forcing_noise_rows(e._h, 0, R, ptr, 1)), e.sync())
                            got = timed(calls, e.sync, a.runs)
                    else:
                        got = timed(calls, e.sync, a.runs)
                    for k, v in got.items():
                        ms.setdefault(k, []).extend(v)
                    e.clear_diagnostics()
                    heat = e.define_heat_content()
            base = statistics.median(ms["heat content"])
            noise = statistics.median(ms["forcing_noise_rows"]) if "forcing_noise_rows" in ms else None
            print(f"N = {n}, {config}, {R} rows, {a.runs} rounds (wall ms per call, synchronised)")
            for name, x in ms.items():
                med = statistics.median(x)
                rows = 1 if name == "forcing_noise_rows" else 3             # it writes its rows and reads none
                gbs = rows * 8.0 * R * n / (med * 1e-3) / 1e9
                line = (f"  {name:<18} median {med:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}   {rows} x 8 B x R x N over the median: {gbs:7.0f} GB/s"
                        f"   ratio to heat content {med / base:5.2f}")
                if noise is not None and name in ("forcing", "imbalance"):
                    line += f"   to forcing_noise_rows {med / noise:5.2f}"
                print(line)
            sys.stdout.flush()


if __name__ == "__main__":
    main()
