"""Times the posterior step of an assessment on the device against the host route it replaces.

For each configuration (two-layer at 1e6 members, ClimateUDEB at 65 536 members, with --graph the configs[3]-share MAGICC graph
at 125 000 members) an ensemble is run to a branch point, weighted, and then, as the median of --repeats runs after a warm-up:

  1. resample:   Ensemble.resample -- the inclusive scan of the weights plus the ancestor search (rscm_ens_resample);
  2. gather:     Ensemble.branch -- rscm_ens_gather_members into a destination of the same size, with the bytes it moves
                 (every row read once and written once, the ancestors read once) and the rate against HBM;
  3. host route: checkpoint() -> numpy take along the member axis -> restore(), the existing code the gather replaces.

Times are host clocks around calls that return after the device has finished.  One JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd import _lib as L  # noqa: E402

HBM_SPEC_TBS = 8.0        # HBM3E peak of the MI355X (datasheet)
HBM_COPY_TBS = 6.29       # what a plain float4 copy kernel reaches on it


def median_ms(fn, repeats):
    fn()                                                    # warm-up: code objects, first allocations
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def rows_moved(e, k):
    """Rows of doubles one member's copy consists of (rscm_ens_gather_members): parameters, the current and look-back rows of
    every stored variable, the internal component state."""
    n_vars = max(e.var_ids.values())
    rows = e.n_params + n_vars * (min(e._history_depth(), k) + 1)
    if e.kind == L.KIND_UDEB:
        rows += 2 * int(e.get_params()[0, 0]) + 11 + (k + 1)
    if e.kind == L.KIND_OCEAN_CARBON:
        rows += min(k * 12, 6060, (e.n_times - 1) * 12)
    return rows


def host_route(src, dst, anc):
    ck = src.checkpoint(all_variables=True)
    n = src.n_members
    ck["n_members"] = dst.n_members
    ck["params"] = np.ascontiguousarray(ck["params"][:, anc])
    ck["state"] = {k: np.ascontiguousarray(v[anc]) for k, v in ck["state"].items()}
    ck["history"] = {k: np.ascontiguousarray(v[:, anc]) for k, v in ck["history"].items()}
    if ck["internal"] is not None:
        ck["internal"] = np.ascontiguousarray(ck["internal"].reshape(-1, n)[:, anc]).ravel()
    dst.restore(ck)


def weights_for(n, rng):
    ll = -0.5 * rng.standard_normal(n) ** 2 * 8.0
    w = np.floor(np.exp(ll - ll.max()) * 2.0 ** 33).astype(np.int64)
    return w


def measure(name, src, dst, k, repeats, rng):
    n = src.n_members
    src.run(k)
    src.set_member_weights(weights_for(n, rng))
    stats = src.weights_stats()
    t_res = median_ms(lambda: src.resample(n, seed=1), repeats)
    anc_dev = src.resample(n, seed=1)
    t_gat = median_ms(lambda: src.branch(dst, anc_dev), repeats)
    anc = anc_dev.to_host()
    t_host = median_ms(lambda: host_route(src, dst, anc), max(2, repeats // 3))
    moved = n * (rows_moved(src, k) * 16 + 2 + 8)
    rate = moved / (t_gat[0] * 1e-3) / 1e12
    line = {"config": name, "members": n, "draws": n, "time_index": k, "ess": stats["ess"], "n_nonzero": stats["n_nonzero"],
            "resample_ms_median": round(t_res[0], 4), "resample_ms_min": round(t_res[1], 4),
            "gather_ms_median": round(t_gat[0], 4), "gather_ms_min": round(t_gat[1], 4), "gather_bytes": moved,
            "gather_tb_per_s": round(rate, 3), "gather_share_of_hbm_spec": round(rate / HBM_SPEC_TBS, 3),
            "gather_share_of_copy_kernel": round(rate / HBM_COPY_TBS, 3),
            "host_route_ms_median": round(t_host[0], 2), "host_route_over_gather": round(t_host[0] / t_gat[0], 1)}
    print(json.dumps(line), flush=True)


def two_layer(n, T):
    b = np.arange(T + 1, dtype=float) + 1750.0
    rng = np.random.default_rng(1)
    lo = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
    hi = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
    F = 4.0 * (1.0 - np.exp(-np.arange(T) / 120.0))
    src = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, b)
    src.set_params(lo[:, None] + rng.random((6, n)) * (hi - lo)[:, None])
    src.set_forcing(F)
    src.set_initial(1, 0.0)
    src.set_initial(2, 0.0)
    dst = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, b)
    dst.set_forcing(F)
    return src, dst


def udeb(n, T):
    b = np.arange(T + 1, dtype=float) + 1750.0
    rng = np.random.default_rng(2)
    P = np.repeat(np.asarray(L.UD_DEFAULTS, dtype=np.float64).reshape(-1, 1), n, axis=1)
    P[L.UD_PARAM_NAMES.index("ecs")] = rng.uniform(2.0, 4.5, n)
    P[L.UD_PARAM_NAMES.index("kappa")] = rng.uniform(0.5, 1.2, n)
    F = 0.04 * np.arange(T, dtype=float)
    src = rscm_amd.Ensemble(rscm_amd.KIND_UDEB, n, b)
    src.set_params(P)
    src.set_forcing(F)
    for v in range(1, 5):
        src.set_initial(v, 0.0)
    dst = rscm_amd.Ensemble(rscm_amd.KIND_UDEB, n, b)
    dst.set_forcing(F)
    return src, dst


def graph(n, years, k, repeats, rng):
    """The MAGICC graph: the same three measurements over all of its linked ensembles (GraphModel.branch / checkpoint / restore)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_magicc_chain", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                     "bench_magicc_chain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src, dst = mod.build_chain(n, years, "topological"), mod.build_chain(n, years, "topological")
    for _ in range(k):
        src.step()
    src.set_member_weights(weights_for(n, rng))
    t_res = median_ms(lambda: src.resample(n, seed=1), repeats)
    anc_dev = src.resample(n, seed=1)
    t_gat = median_ms(lambda: src.branch(dst, anc_dev), repeats)
    anc = anc_dev.to_host()

    def route():
        ck = src.checkpoint()
        for c in ck["ensembles"].values():
            c["params"] = np.ascontiguousarray(c["params"][:, anc])
            c["state"] = {key: np.ascontiguousarray(v[anc]) for key, v in c["state"].items()}
            c["history"] = {key: np.ascontiguousarray(v[:, anc]) for key, v in c["history"].items()}
            if c["internal"] is not None:
                c["internal"] = np.ascontiguousarray(c["internal"].reshape(-1, n)[:, anc]).ravel()
        dst.restore(ck)
    t_host = median_ms(route, 2)
    moved = sum(n * (rows_moved(e, k) * 16 + 2 + 8) for e in src.ensembles.values())
    rate = moved / (t_gat[0] * 1e-3) / 1e12
    print(json.dumps({"config": f"MAGICC graph, {len(src.ensembles)} linked ensembles", "members": n, "draws": n, "time_index": k,
                      "resample_ms_median": round(t_res[0], 4), "gather_ms_median": round(t_gat[0], 4), "gather_ms_min": round(t_gat[1], 4),
                      "gather_bytes": moved, "gather_tb_per_s": round(rate, 3), "gather_share_of_hbm_spec": round(rate / HBM_SPEC_TBS, 3),
                      "host_route_ms_median": round(t_host[0], 2), "host_route_over_gather": round(t_host[0] / t_gat[0], 1)}), flush=True)
    for m in (src, dst):
        m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--two-layer-members", type=int, default=1_000_000)
    ap.add_argument("--udeb-members", type=int, default=65_536)
    ap.add_argument("--graph", action="store_true", help="also the configs[3]-share graph (125 000 members; minutes)")
    ap.add_argument("--graph-members", type=int, default=125_000)
    args = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("bench_resample.py needs a HIP device: nothing is measured without one")
    rng = np.random.default_rng(0)
    if args.two_layer_members:
        s, d = two_layer(args.two_layer_members, 101)
        with s, d:
            measure("two-layer", s, d, 50, args.repeats, rng)
    if args.udeb_members:
        s, d = udeb(args.udeb_members, 101)
        with s, d:
            measure("ClimateUDEB, 50 layers", s, d, 50, args.repeats, rng)
    if args.graph:
        graph(args.graph_members, 100, 50, args.repeats, rng)
