"""Cost of the seeded forcing noise of a two-layer ensemble (rscm_ens_set_forcing_noise) on the GPU: the same handle run with the
noise on and off, in alternation.  Device-event times (rscm_ens_last_run_ms), two warm-up rounds, then --runs timed rounds; the
median and the minimum are printed, and the ratio of the medians.  The draw is a Philox block every other year and an AS241
deviate every year, on top of a year of ten RK4 sub-steps.  profiles/forcing_noise_bench.txt holds one output of this script.

With --phi the red (AR(1)) noise joins: off, white and red on the same handle in alternation, red against white as the ratio of the
medians beside the white runs' own min-max spread, and one spin-up -- the second half of the axis run from index 375 with the
red noise's cache in place and with it dropped (the launch then forms e_0 .. e_374 from the draws first).
profiles/forcing_noise_red_bench.txt holds one such output.

With --per-member (and --phi) the per-member noise (rscm_ens_set_forcing_noise_members) is timed instead: a handle with the two noise
parameter rows run under the handle-wide red setting, under per-member noise with both rows uniform (the same sigma and phi: one
element read for the wavefront) and under per-member noise with rows that vary, in alternation; each against the handle-wide red
runs' median and min-max spread.  profiles/forcing_noise_members_bench.txt holds one such output.

    python scripts/bench_forcing_noise.py [--runs 10] [--sizes 100000 1000000] [--phi 0.7] [--per-member]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402

T = 751
BOUNDS = np.arange(T + 1, dtype=np.float64) + 1750.0
LO = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HI = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
SIGMA, SEED = 0.3, 20260327


def ensemble(n, K, mode, noise_params=False):
    """K == 0: the plain two-layer handle; K > 0: a mix handle.  noise_params: with the two noise rows, sigma in [0.1, 0.5] and phi in
    [0.4, 0.9]."""
    e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS, forcing_components=K if K else None, noise_params=noise_params)
    e.set_mode(mode)
    lo, hi = (np.r_[LO, np.full(K, 0.7)], np.r_[HI, np.full(K, 1.3)]) if K else (LO, HI)
    if noise_params:
        lo, hi = np.r_[lo, 0.1, 0.4], np.r_[hi, 0.5, 0.9]
    e.sample_lhs(SEED, lo, hi)
    t = np.arange(T, dtype=np.float64)
    base = 4.0 * (1.0 - np.exp(-t / 120.0)) + 0.3 * np.sin(2.0 * np.pi * t / 11.0)
    e.set_forcing(np.stack([base / K * (1.0 + 0.1 * np.cos(0.05 * t * (k + 1))) for k in range(K)])[None] if K else base)
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    return e


def timed(e, runs, phi=0.0):
    """{"off": [ms], "on": [ms][, "red": [ms]]} of one handle: two warm-up rounds, then `runs` rounds of off, on[, red]."""
    names = ("off", "on", "red") if phi else ("off", "on")
    out = {name: [] for name in names}
    for r in range(runs + 2):
        for name in names:
            if name == "off":
                e.clear_forcing_noise()
            else:
                e.set_forcing_noise(SIGMA, SEED, 0, phi if name == "red" else 0.0)
            e.rewind()
            e.run()
            if r >= 2:
                out[name].append(e.last_run_ms())
    return out


def timed_members(e, runs, phi):
    """{"red": [ms], "uniform": [ms], "varying": [ms]} of one handle with the noise rows: two warm-up rounds, then `runs` rounds of
    the handle-wide red setting, per-member noise with uniform rows (sigma and phi the red setting's) and with the sampled rows.
    Every run follows a set_params of its own, the red one too (the rows are inert there): the 64 MB copy and the host's comparison
    of the rows at 1e6 members leave the GPU idle for tens of milliseconds, and a run that follows such a pause is slower than one
    that follows a run."""
    varying = e.get_params()
    uniform = varying.copy()
    uniform[-2], uniform[-1] = SIGMA, phi
    out = {"red": [], "uniform": [], "varying": []}
    for r in range(runs + 2):
        for name in out:
            e.set_params(varying if name == "varying" else uniform)
            if name == "red":
                e.set_forcing_noise(SIGMA, SEED, 0, phi)
            else:
                e.set_forcing_noise_members(SEED)
            e.rewind()
            e.run()
            if r >= 2:
                out[name].append(e.last_run_ms())
    return out


def main_members(a):
    for n in a.sizes:
        for mode, mode_name in ((rscm_amd.MODE_EXACT, "EXACT"), (rscm_amd.MODE_FAST, "FAST")):
            for K, what in ((0, "plain two-layer"), (4, "mix K=4")):
                e = ensemble(n, K, mode, noise_params=True)
                ms = {name: np.asarray(v) for name, v in timed_members(e, a.runs, a.phi).items()}
                blocks, chunks = e.last_run_plan()
                e.close()
                red = ms["red"]
                print(f"{n} members x {T - 1} steps, {mode_name}, {what} (noise run cut into {blocks} block(s) x {chunks} chunk(s))")
                print(f"  handle-wide red {a.phi:+.2f}  median {np.median(red):9.3f} ms   min {red.min():9.3f} ms   max {red.max():9.3f} ms   "
                      f"({red.size} runs)   {n * (T - 1) / np.median(red) * 1e3:.3e} member-years/s")
                for name in ("uniform", "varying"):
                    x = ms[name]
                    inside = "inside" if red.min() <= np.median(x) <= red.max() else "OUTSIDE"
                    print(f"  per-member, {name} rows  median {np.median(x):9.3f} ms   min {x.min():9.3f} ms   max {x.max():9.3f} ms   "
                          f"x{np.median(x) / np.median(red):.3f} of red, {inside} the red runs' spread   "
                          f"{n * (T - 1) / np.median(x) * 1e3:.3e} member-years/s", flush=True)


def spin_up(e, runs, phi, at=375):
    """{"cached": [ms], "spun up": [ms]}: run() from index `at` after run(at), the red noise's cache left in place or dropped."""
    out = {"cached": [], "spun up": []}
    e.set_forcing_noise(SIGMA, SEED, 0, phi)
    for r in range(runs + 2):
        for name in out:
            e.rewind()
            e.run(at)
            if name == "spun up":
                e.set_forcing_noise(SIGMA, SEED, 0, phi)   # any setter of the noise drops the cache
            assert e.forcing_noise_cached_index == (at - 1 if name == "cached" else -1)
            e.run()
            if r >= 2:
                out[name].append(e.last_run_ms())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--phi", type=float, default=0.0, help="also time the red noise with this lag-one correlation, and one spin-up")
    ap.add_argument("--per-member", action="store_true", help="time the per-member noise against the handle-wide red setting (needs --phi)")
    a = ap.parse_args()
    if a.per_member:
        if not a.phi:
            ap.error("--per-member needs --phi")
        return main_members(a)
    for n in a.sizes:
        for mode, mode_name in ((rscm_amd.MODE_EXACT, "EXACT"), (rscm_amd.MODE_FAST, "FAST")):
            for K, what in ((0, "plain two-layer"), (4, "mix K=4")):
                e = ensemble(n, K, mode)
                ms = timed(e, a.runs, a.phi)
                blocks, chunks = e.last_run_plan()
                spin = spin_up(e, a.runs, a.phi) if a.phi else None
                e.close()
                off, on = np.asarray(ms["off"]), np.asarray(ms["on"])
                print(f"{n} members x {T - 1} steps, {mode_name}, {what} (noise run cut into {blocks} block(s) x {chunks} chunk(s))")
                print(f"  noise off  median {np.median(off):9.3f} ms   min {off.min():9.3f} ms   ({off.size} runs)")
                print(f"  noise on   median {np.median(on):9.3f} ms   min {on.min():9.3f} ms   ({on.size} runs)   "
                      f"x{np.median(on) / np.median(off):.3f} of off   {n * (T - 1) / np.median(on) * 1e3:.3e} member-years/s", flush=True)
                if a.phi:
                    red = np.asarray(ms["red"])
                    print(f"  red {a.phi:+.2f}  median {np.median(red):9.3f} ms   min {red.min():9.3f} ms   ({red.size} runs)   "
                          f"x{np.median(red) / np.median(on):.3f} of white (white runs {on.min():.3f} .. {on.max():.3f} ms)   "
                          f"{n * (T - 1) / np.median(red) * 1e3:.3e} member-years/s")
                    c, u = np.asarray(spin["cached"]), np.asarray(spin["spun up"])
                    print(f"  steps 375..749: cache in place median {np.median(c):9.3f} ms, dropped {np.median(u):9.3f} ms "
                          f"(+{np.median(u) - np.median(c):.3f} ms for 375 deviates per member)", flush=True)


if __name__ == "__main__":
    main()
