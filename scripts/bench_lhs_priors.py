"""Times Ensemble.sample_lhs_priors (the device Latin hypercube through Normal, LogNormal and truncated priors, lhs_priors_kernel in
csrc/ensemble_ops.hip) against Ensemble.sample_lhs of the same build and against the host route it replaces.

Cases, on a two-layer ensemble (6 parameter rows) of 1e5 and 1e6 members, all in one process:

  uniform     sample_lhs_priors with six Uniform rows        -- to be compared with sample_lhs: the same bits, the uniform branch
  normal      sample_lhs_priors with six Normal rows
  mix         Uniform, Uniform, Normal, Bound(Normal), LogNormal, Bound(LogNormal)
  sample_lhs  Ensemble.sample_lhs on the same box
  host        ParameterSet.sample_lhs on the host (numpy, scipy.special.ndtri) for the six Normal rows, then set_params: the upload

The four device cases are taken in alternation (uniform, normal, mix, sample_lhs, uniform, ...) after a warm-up round, --repeats
times.  Each call is bracketed by two device events on the handle's stream, so "event_ms" is the time between them on the device: the
upload of the 56-byte-per-row table, the kernel, and the wait for whatever the host does between recording the first event and the
launch (building the table in Python among it); "host_ms" is the host clock around the same synchronous call.  Medians with minimum
and maximum.  The host route is timed by the host clock alone, --host-repeats times.  One JSON line per size.  The kernels' own
durations come from a kernel trace of a run with --cases uniform normal sample_lhs, which are three kernels by name."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd.calibrate import Bound, LogNormal, Normal, ParameterSet, Uniform  # noqa: E402

LOW = [0.8, 0.0, 1.0, 0.5, 5.0, 50.0]
HIGH = [1.5, 0.1, 1.8, 1.0, 15.0, 200.0]
CASES = {
    "uniform": {j: Uniform(lo, hi) for j, (lo, hi) in enumerate(zip(LOW, HIGH))},
    "normal": {j: Normal(0.5 * (lo + hi), 0.1 * (hi - lo)) for j, (lo, hi) in enumerate(zip(LOW, HIGH))},
    "mix": {0: Uniform(0.8, 1.5), 1: Uniform(0.0, 0.1), 2: Normal(1.3, 0.1), 3: Bound(Normal(0.7, 0.2), 0.5, 1.0),
            4: LogNormal(math.log(8.0), 0.2), 5: Bound(LogNormal(math.log(100.0), 0.4), 50.0, 200.0)},
}


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=list(CASES) + ["sample_lhs"], help="the device cases to time (a kernel trace tells "
                    "lhs_kernel and the two instances of lhs_priors_kernel apart by name: uniform, normal, sample_lhs)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lhs_priors: no GPU; nothing is timed without one")
    stream = torch.cuda.current_stream().cuda_stream
    for n in args.members:
        with rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, np.arange(1750.0, 1754.0)) as e:
            e.set_stream(stream or None)
            calls = {name: (lambda p=priors: e.sample_lhs_priors(7, p)) for name, priors in CASES.items()}
            calls["sample_lhs"] = lambda: e.sample_lhs(7, LOW, HIGH)
            calls = {name: fn for name, fn in calls.items() if name in args.cases}
            for fn in calls.values():   # warm-up: code objects, first allocations
                fn()
            ev = {name: [] for name in calls}
            host = {name: [] for name in calls}
            for _ in range(args.repeats):
                for name, fn in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    host[name].append((time.perf_counter() - t0) * 1e3)
                    ev[name].append(a.elapsed_time(b))
            e.sample_lhs_priors(7, CASES["uniform"])
            drawn = e.get_params()
            e.sample_lhs(7, LOW, HIGH)
            same = bool(np.array_equal(drawn, e.get_params()))
            ps = ParameterSet()
            for j, d in CASES["normal"].items():
                ps.add(f"p{j}", d)
            draw_ms, upload_ms = [], []
            for k in range(args.host_repeats):
                t0 = time.perf_counter()
                P = np.ascontiguousarray(ps.sample_lhs(n, np.random.default_rng(k)).T)
                t1 = time.perf_counter()
                e.set_params(P)
                t2 = time.perf_counter()
                draw_ms.append((t1 - t0) * 1e3)
                upload_ms.append((t2 - t1) * 1e3)
        res = {"members": n, "rows": 6, "repeats": args.repeats,
               "event_ms": {k: stats(v) for k, v in ev.items()}, "host_ms": {k: stats(v) for k, v in host.items()},
               "uniform_over_sample_lhs_event": (round(statistics.median(ev["uniform"]) / statistics.median(ev["sample_lhs"]), 3)
                                                 if "uniform" in ev and "sample_lhs" in ev else None),
               "uniform_equals_sample_lhs_bits": same,
               "host_route_ms": {"draw": stats(draw_ms), "set_params": stats(upload_ms), "upload_bytes": 6 * 8 * n},
               "host_route_over_normal": (round((statistics.median(draw_ms) + statistics.median(upload_ms)) / statistics.median(host["normal"]), 1)
                                          if "normal" in host else None)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
