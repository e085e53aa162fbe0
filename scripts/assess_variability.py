"""Internal variability with unknown amplitude and persistence, on the device: a two-layer ensemble whose noise amplitude sigma and
lag-one correlation phi are parameter rows (``Ensemble(..., noise_params=True)``, ``set_forcing_noise_members``).

  * a Latin hypercube over the six model parameters AND sigma, phi;
  * the history 1850-2020 run under each member's own AR(1) noise, scored against a record (here: one run of a member with known
    sigma and phi and its own seed, every fifth year), weighted (``loglik`` then ``set_weights_from_loglik``);
  * the prior and the weighted quantiles of ``params_vector(sigma_row)`` and ``params_vector(phi_row)``, the weighted ones compared
    with numpy;
  * a posterior ensemble (``posterior()``) made with ``noise_params=True``: every draw inherits its ancestor's sigma and phi, realises
    its own noise under its own seed, and is projected to 2100 -- the plume then carries the variability the record supports.

A point likelihood of one realisation constrains sigma and phi only weakly (members with less noise fit a record's slow part
better), so the script then weights by the record's variability itself:

  * the targets are the standard deviation and the lag-one autocorrelation of the first differences of the record's 171 annual
    values, ``rscm_amd.variability.series_variability(record, "difference")`` -- the estimator ``Ensemble.variability`` applies to
    every member on the device;
  * their sigmas are the sampling errors of the two statistics over n differences, ``sd / sqrt(2 n)`` and ``sqrt((1 - r1^2) / n)``,
    times ``sqrt(2)``: the record and a member are one realisation each, so the difference of their statistics carries both errors;
  * ``loglik_vectors`` scores the members by the statistics alone and added onto the point likelihood; the sigma / phi quantiles and
    the effective sample size of all three weightings are printed beside the prior.  The statistics constrain a ridge, not a point:
    the temperature's variability depends on sigma, phi, the feedback and the heat capacities jointly.

With ``--spectrum`` the record's power spectrum is the target as well: the band powers of the differences'
periodogram, ``rscm_amd.variability.series_spectrum(record, "difference")`` against ``Ensemble.spectrum`` of every member, scored by
``loglik_spectrum`` -- alone ("spectrum") and with the (sd, r1) likelihood added onto it ("spectrum_and_statistics").  One lag cannot
tell strong short-lived noise from weak persistent noise once the ocean has filtered it; the spectrum's shape can.

With ``--heat-content`` the record is the truth member's ocean heat content as well as its temperature:
``H = C Ts + Cd Td`` as a diagnostic variable of the ensemble (``define_heat_content``, ``compute_diagnostic``), whose first
differences are the year-to-year heat uptake.  Their (sd, r1) -- and with ``--spectrum`` their band powers -- are scored like the
temperature's and added onto the temperature's likelihoods; the effective sample size and the 5-50-95 % ranges of sigma, phi,
lambda0 and the two heat capacities are printed for temperature alone and for temperature plus heat content.

With ``--covariability`` (it requires ``--heat-content``) the RELATION between the two series is a target too (DESIGN.md section
8s): the correlation, the regression slope and the cross-correlations one year either way of the heat content's differences against
the temperature at the midpoints, linearly detrended -- ``rscm_amd.variability.series_covariability(temperature, heat, "linear",
"difference", 1)`` of the record against ``Ensemble.covariability`` of every member, scored by ``loglik_vectors`` alone
("covariability") and added onto the temperature-plus-heat-content likelihood ("all").  The sigmas are the sampling errors over n
terms times ``sqrt(2)``: ``(1 - r^2) / sqrt(n)`` for the correlations, ``sqrt((var_y - slope cov) / (n var_x))`` for the slope.  The
effective sample size and the 5-50-95 % ranges of sigma, phi, lambda0, the efficacy and the two heat capacities are printed.

With ``--cross-spectrum`` (it requires ``--heat-content`` too) the relation is scored per frequency band: the
squared coherence, the gain and the quadrature gain of the heat content's differences on the temperature at the midpoints, linearly
detrended, in three bands -- ``rscm_amd.variability.series_cross_spectrum(temperature, heat, "linear", "difference")`` of the record
against ``Ensemble.cross_spectrum`` of every member, scored by ``loglik_vectors`` alone ("cross_spectrum") and added onto the
likelihoods before it ("all").  The sigmas are the usual large-sample ones for a band of m ordinates,
``sqrt((1 - coh2) / (2 m coh2)) |gain|`` for both gains (``|gain|`` the magnitude of the complex gain, ``hypot(gain, gain_quad)``) and ``sqrt(2 / m) (1 - coh2) sqrt(coh2)`` for coh2, at the record's values,
times ``sqrt(2)`` as for every other target here (record and member are one realisation each).

With ``--toa-imbalance`` (it requires ``--heat-content`` too) the record's top-of-atmosphere imbalance is a target (DESIGN.md
section 8u): N as an energy-budget diagnostic (``define_toa_imbalance``) of the truth member and of every member, the correlation
and the regression slope of N on the temperature, both linearly detrended, lag 0 -- the record's Gregory slope --
``series_covariability(temperature, N, "linear", "linear", 0)`` against ``Ensemble.covariability``, scored alone ("toa_imbalance")
and added onto the temperature-plus-heat-content likelihood ("all"); the 5-95 % range of lambda0 with and without it goes to stderr.

With ``--running-mean W`` the 1.5 K crossing of the history is read twice: the first YEAR at or above 1.5 K
(``indicators`` on the annual values, which carry each member's own variability) and the first W-year centred mean at or above it
(``define_running_mean``, ``compute_diagnostic``, then ``indicators`` on the diagnostic); the 5 %, 50 % and 95 % points of the two
crossing times under the point likelihood's weights go to stderr side by side and into the JSON line (a member that never crosses
counts as +inf).

    python scripts/assess_variability.py [--members 100000] [--draws 20000] [--fast] [--spectrum] [--heat-content] [--covariability] [--toa-imbalance]
                                         [--cross-spectrum]

Prints one JSON line; exit code 0 iff every comparison holds."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd.variability import series_covariability, series_cross_spectrum, series_spectrum, series_variability  # noqa: E402

Q = [0.05, 0.17, 0.5, 0.83, 0.95]
YEARS = np.arange(1850.0, 2101.0)
BOUNDS = np.append(YEARS, YEARS[-1] + 1.0)
NOW = 2020 - 1850   # the time index the record ends at
LO = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0, 0.05, 0.0])
HI = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0, 1.0, 0.95])
TRUTH = np.array([1.1, 0.05, 1.3, 0.7, 8.0, 100.0, 0.4, 0.6])
OBS_SIGMA = 0.12
TS = "Surface Temperature"


def forcing():
    t = YEARS - 1850.0
    return 0.035 * t + 0.25 * np.sin(2.0 * np.pi * t / 11.0)


def make(n, mode, seed, offset=0):
    e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS, noise_params=True)
    e.set_mode(mode)
    e.set_forcing(forcing())
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.set_forcing_noise_members(seed, offset)
    return e


def np_weighted(row, w):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(row, Q, weights=w, method="inverted_cdf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000)
    ap.add_argument("--draws", type=int, default=20_000)
    ap.add_argument("--fast", action="store_true")
    ap.add_argument("--spectrum", action="store_true", help="also weight by the record's band powers (loglik_spectrum)")
    ap.add_argument("--heat-content", action="store_true", help="also weight by the variability of the record's ocean heat content")
    ap.add_argument("--covariability", action="store_true",
                    help="also weight by the covariability of the record's heat uptake and temperature (requires --heat-content)")
    ap.add_argument("--cross-spectrum", action="store_true",
                    help="also weight by the band coherence and gains of the record's heat uptake on its temperature (requires --heat-content)")
    ap.add_argument("--toa-imbalance", action="store_true",
                    help="also weight by the covariability of the record's temperature and top-of-atmosphere imbalance (requires --heat-content)")
    ap.add_argument("--running-mean", type=int, default=0, metavar="W",
                    help="also print the weighted 1.5 K crossing time from annual values beside that of the W-year centred mean (2 .. 64)")
    ap.add_argument("--correlations", action="store_true",
                    help="also print the posterior correlation matrix of the parameters (Ensemble.moments) under the last weights formed")
    a = ap.parse_args()
    if a.toa_imbalance and not a.heat_content:
        ap.error("--toa-imbalance requires --heat-content")
    if a.covariability and not a.heat_content:
        ap.error("--covariability requires --heat-content")
    if a.cross_spectrum and not a.heat_content:
        ap.error("--cross-spectrum requires --heat-content")
    if a.running_mean and not 2 <= a.running_mean <= 64:
        ap.error("--running-mean takes a window of 2 .. 64 years")
    mode = rscm_amd.MODE_FAST if a.fast else rscm_amd.MODE_EXACT

    # the record: one member with known amplitude and persistence, a seed of its own
    with make(1, mode, seed=99) as truth:
        truth.set_params(TRUTH[:, None])
        truth.run(NOW)
        rows = np.arange(5, NOW + 1, 5)
        annual = truth.get_series(TS, 0, NOW + 1)[:, 0]
        record = annual[rows]
        annual_heat = TRUTH[4] * annual + TRUTH[5] * truth.get_series("Deep Ocean Temperature", 0, NOW + 1)[:, 0]
        annual_toa = None
        if a.toa_imbalance:
            nid = truth.define_toa_imbalance()
            truth.compute_diagnostic(nid, 0, NOW + 1)
            annual_toa = truth.get_series(nid, 0, NOW + 1)[:, 0]

    with make(a.members, mode, seed=1) as ens:
        sigma_row, phi_row = ens.noise_param_rows
        ens.sample_lhs(20260327, LO, HI)
        ens.run(NOW)
        ll = ens.loglik([TS] * rows.size, rows, record, np.full(rows.size, OBS_SIGMA), on_device=True)
        ens.set_weights_from_loglik(ll)
        vectors = [ens.params_vector(sigma_row), ens.params_vector(phi_row)]
        prior = ens.quantile_vectors(vectors, Q)["quantiles"]
        post = ens.quantile_vectors(vectors, Q, weighted=True)["quantiles"]
        P, w = ens.get_params(), ens.member_weights()
        checks = {"weighted_quantiles_equal_numpy": bool(np.array_equal(post, np.stack([np_weighted(P[sigma_row], w), np_weighted(P[phi_row], w)])))}
        ess = ens.weights_stats()["ess"]

        crossing = None
        if a.running_mean:
            # the first year at or above 1.5 K, and the first W-year centred mean at or above it, over the history under the point
            # likelihood's weights: lower empirical quantiles, +inf for a member that never crosses
            level, q3c = 1.5, [0.05, 0.5, 0.95]
            mid = ens.define_running_mean(f"{TS}|{a.running_mean}-year mean", TS, a.running_mean, "centre")
            ens.compute_diagnostic(mid)
            lo, hi = ens.running_mean_range(mid)
            annual_x = ens.indicators(TS, 0, NOW + 1, thresholds=[level], slot=2)["crossing"][0].to_host()
            mean_x = ens.indicators(mid, lo, hi, thresholds=[level], slot=3)["crossing"][0].to_host()
            ok = ~(np.isnan(annual_x) | np.isnan(mean_x)) & (w > 0)
            crossing = {"level_K": level, "window": a.running_mean, "quantiles": q3c, "members": int(ok.sum()),
                        "annual": np.quantile(annual_x[ok], q3c, weights=w[ok], method="inverted_cdf").tolist(),
                        "running_mean": np.quantile(mean_x[ok], q3c, weights=w[ok], method="inverted_cdf").tolist(),
                        "mean_rows": [float(YEARS[lo]), float(YEARS[hi - 1])]}
            print(f"1.5 K crossing in 1850-2020, {crossing['members']} weighted members, 5 / 50 / 95 %:", file=sys.stderr)
            print("  first year at or above it            " + "  ".join(f"{v:7.1f}" for v in crossing["annual"]), file=sys.stderr)
            print(f"  first {a.running_mean:2d}-year centred mean at or above " + "  ".join(f"{v:7.1f}" for v in crossing["running_mean"]),
                  file=sys.stderr)

        # the posterior: the draws inherit sigma and phi with the other rows and realise their own noise to 2100
        anc = ens.resample(a.draws, seed=7).to_host()
        dst, _ = ens.posterior(lambda n: make(n, mode, seed=2), a.draws, seed=7)
        with dst:
            got = dst.get_params()
            checks["draws_inherit_their_ancestors_rows"] = bool(np.array_equal(got, P[:, anc]))
            dst.run()
            plume = dst.quantile_rows(TS, Q, len(YEARS) - 1, len(YEARS))["quantiles"][0]
            twins = np.flatnonzero(anc[1:] == anc[:-1])
            last = dst.get_series(TS, len(YEARS) - 1)[0]
            checks["draws_of_one_ancestor_diverge"] = bool(twins.size == 0 or (last[twins] != last[twins + 1]).any())

        # the record's variability as the target: by the statistics alone, and added onto the point likelihood (ll, in place)
        target = series_variability(annual, "difference")
        n_diff = annual.size - 1
        values = [target["sd"], target["r1"]]
        sigmas = [np.sqrt(2.0) * target["sd"] / np.sqrt(2.0 * n_diff), np.sqrt(2.0) * np.sqrt((1.0 - target["r1"] ** 2) / n_diff)]
        var = ens.variability(TS, 0, NOW + 1, detrend="difference")
        stats = [var["sd"], var["r1"]]
        constraint = {}
        for name, add_to in (("both", ll), ("statistics", None)):
            ens.set_weights_from_loglik(ens.loglik_vectors(stats, values, sigmas, add_to=add_to))
            q = ens.quantile_vectors(vectors, Q, weighted=True)["quantiles"]
            constraint[name] = {"sigma": q[0].tolist(), "phi": q[1].tolist(), "ess": ens.weights_stats()["ess"]}
        w = ens.member_weights()
        checks["statistics_weighted_quantiles_equal_numpy"] = bool(np.array_equal(
            [constraint["statistics"]["sigma"], constraint["statistics"]["phi"]], np.stack([np_weighted(P[sigma_row], w), np_weighted(P[phi_row], w)])))

        spectral = None
        if a.spectrum:
            rec = series_spectrum(annual, "difference")
            spec = ens.spectrum(TS, 0, NOW + 1, detrend="difference", bands=rec["edges"], slot=1)
            spectral = {"edges": rec["edges"].tolist(), "counts": rec["counts"].tolist(), "record_power": rec["power"]}
            for name, with_stats in (("spectrum", False), ("spectrum_and_statistics", True)):
                lls = ens.loglik_spectrum(spec["power"], rec["power"], rec["counts"])
                if with_stats:
                    lls = ens.loglik_vectors(stats, values, sigmas, add_to=lls)
                ens.set_weights_from_loglik(lls)
                q = ens.quantile_vectors(vectors, Q, weighted=True)["quantiles"]
                constraint[name] = {"sigma": q[0].tolist(), "phi": q[1].tolist(), "ess": ens.weights_stats()["ess"]}
            w = ens.member_weights()
            checks["spectrum_weighted_quantiles_equal_numpy"] = bool(np.array_equal(
                [constraint["spectrum_and_statistics"]["sigma"], constraint["spectrum_and_statistics"]["phi"]],
                np.stack([np_weighted(P[sigma_row], w), np_weighted(P[phi_row], w)])))

        heat = None
        if a.heat_content:
            # temperature alone: the (sd, r1) likelihood, with --spectrum the spectral one added; then the same estimators on the heat
            # content's differences added onto it (the handle has one likelihood vector: every step continues it in place)
            q3 = [0.05, 0.5, 0.95]
            named = {"sigma": sigma_row, "phi": phi_row, "lambda0": 0, "heat_capacity_surface": 4, "heat_capacity_deep": 5}
            pvec = [ens.params_vector(r) for r in named.values()]

            def weigh(lls):
                ens.set_weights_from_loglik(lls)
                q = ens.quantile_vectors(pvec, q3, weighted=True)["quantiles"]
                return {"ess": ens.weights_stats()["ess"], **{k: q[j].tolist() for j, k in enumerate(named)}}

            hid = ens.define_heat_content()
            ens.compute_diagnostic(hid, 0, NOW + 1)
            htarget = series_variability(annual_heat, "difference")
            hvalues = [htarget["sd"], htarget["r1"]]
            hsigmas = [np.sqrt(2.0) * htarget["sd"] / np.sqrt(2.0 * n_diff), np.sqrt(2.0) * np.sqrt((1.0 - htarget["r1"] ** 2) / n_diff)]
            lls = ens.loglik_vectors(stats, values, sigmas)
            if a.spectrum:
                lls = ens.loglik_spectrum(spec["power"], rec["power"], rec["counts"], add_to=lls)
            heat = {"quantiles": q3, "target": {"sd": hvalues[0], "r1": hvalues[1], "sd_sigma": float(hsigmas[0]), "r1_sigma": float(hsigmas[1])},
                    "prior": {k: q.tolist() for k, q in zip(named, ens.quantile_vectors(pvec, q3)["quantiles"])},
                    "temperature": weigh(lls)}
            hvar = ens.variability(hid, 0, NOW + 1, detrend="difference", slot=2)
            lls = ens.loglik_vectors([hvar["sd"], hvar["r1"]], hvalues, hsigmas, add_to=lls)
            if a.spectrum:
                hrec = series_spectrum(annual_heat, "difference")
                hspec = ens.spectrum(hid, 0, NOW + 1, detrend="difference", bands=hrec["edges"], slot=3)
                lls = ens.loglik_spectrum(hspec["power"], hrec["power"], hrec["counts"], add_to=lls)
                heat["spectrum_target"] = {"edges": hrec["edges"].tolist(), "record_power": hrec["power"]}
            heat["temperature_and_heat_content"] = weigh(lls)
            w = ens.member_weights()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = [np.nanquantile(P[r], q3, weights=w, method="inverted_cdf").tolist() for r in named.values()]
            checks["heat_content_weighted_quantiles_equal_numpy"] = bool(want == [heat["temperature_and_heat_content"][k] for k in named])

        cov = None
        if a.covariability:
            # the relation between the two series: heat uptake (the differences) against the temperature at the midpoints, about its line;
            # alone, and continued from the temperature-plus-heat-content likelihood (lls, in place)
            cnamed = {"sigma": sigma_row, "phi": phi_row, "lambda0": 0, "efficacy": 2, "heat_capacity_surface": 4, "heat_capacity_deep": 5}
            cvec = [ens.params_vector(r) for r in cnamed.values()]

            def cweigh(l):
                ens.set_weights_from_loglik(l)
                q = ens.quantile_vectors(cvec, q3, weighted=True)["quantiles"]
                return {"ess": ens.weights_stats()["ess"], **{k: q[j].tolist() for j, k in enumerate(cnamed)}}

            ct = series_covariability(annual, annual_heat, "linear", "difference", 1)
            cvalues = [ct["corr"], ct["slope"], ct["lead"][0], ct["lag"][0]]
            rsig = lambda r: np.sqrt(2.0) * (1.0 - r * r) / np.sqrt(n_diff)
            csigmas = [rsig(ct["corr"]), np.sqrt(2.0) * np.sqrt((ct["var_y"] - ct["slope"] * ct["cov"]) / (n_diff * ct["var_x"])),
                       rsig(ct["lead"][0]), rsig(ct["lag"][0])]
            cov = {"quantiles": q3, "target": dict(zip(("corr", "slope", "r_plus_1", "r_minus_1"), map(float, cvalues))),
                   "target_sigma": dict(zip(("corr", "slope", "r_plus_1", "r_minus_1"), map(float, csigmas))),
                   "prior": {k: q.tolist() for k, q in zip(cnamed, ens.quantile_vectors(cvec, q3)["quantiles"])}}
            cov["temperature_and_heat_content"] = cweigh(lls)
            c = ens.covariability(TS, hid, 0, NOW + 1, 1, "linear", "difference", 1, slot=1)
            cstats = [c["corr"], c["slope"], c["lead"][0], c["lag"][0]]
            cov["all"] = cweigh(ens.loglik_vectors(cstats, cvalues, csigmas, add_to=lls))
            cov["covariability"] = cweigh(ens.loglik_vectors(cstats, cvalues, csigmas))
            w = ens.member_weights()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = [np.nanquantile(P[r], q3, weights=w, method="inverted_cdf").tolist() for r in cnamed.values()]
            checks["covariability_weighted_quantiles_equal_numpy"] = bool(want == [cov["covariability"][k] for k in cnamed])
            # one member's vectors against the host estimator on its own rows, bit for bit
            one = series_covariability(ens.get_series(TS, 0, NOW + 1)[:, :64], ens.get_series(hid, 0, NOW + 1)[:, :64], "linear", "difference", 1)
            checks["covariability_equals_the_host_estimator"] = bool(all(
                np.array_equal(d.to_host()[:64], h, equal_nan=True) for d, h in zip(cstats, [one["corr"], one["slope"], one["lead"][0], one["lag"][0]])))

        toa = None
        if a.toa_imbalance:
            # the quantity the feedback is observed through: N as a diagnostic variable, its regression on the
            # temperature (both about their lines, lag 0: the Gregory slope of the record) alone and added onto the temperature-plus-
            # heat-content likelihood, which is formed again (the branches above continued it in place)
            tnamed = {"sigma": sigma_row, "phi": phi_row, "lambda0": 0, "efficacy": 2, "heat_capacity_surface": 4, "heat_capacity_deep": 5}
            tvec = [ens.params_vector(r) for r in tnamed.values()]

            def tweigh(l):
                ens.set_weights_from_loglik(l)
                q = ens.quantile_vectors(tvec, q3, weighted=True)["quantiles"]
                return {"ess": ens.weights_stats()["ess"], **{k: q[j].tolist() for j, k in enumerate(tnamed)}}

            lls = ens.loglik_vectors(stats, values, sigmas)
            if a.spectrum:
                spec = ens.spectrum(TS, 0, NOW + 1, detrend="difference", bands=rec["edges"], slot=1)
                lls = ens.loglik_spectrum(spec["power"], rec["power"], rec["counts"], add_to=lls)
            lls = ens.loglik_vectors([hvar["sd"], hvar["r1"]], hvalues, hsigmas, add_to=lls)
            if a.spectrum:
                lls = ens.loglik_spectrum(hspec["power"], hrec["power"], hrec["counts"], add_to=lls)
            tt = series_covariability(annual, annual_toa, "linear", "linear", 0)
            n_rows = annual.size
            tvalues = [tt["corr"], tt["slope"]]
            tsigmas = [np.sqrt(2.0) * (1.0 - tt["corr"] ** 2) / np.sqrt(n_rows),
                       np.sqrt(2.0) * np.sqrt((tt["var_y"] - tt["slope"] * tt["cov"]) / (n_rows * tt["var_x"]))]
            toa = {"quantiles": q3, "target": dict(zip(("corr", "slope"), map(float, tvalues))),
                   "target_sigma": dict(zip(("corr", "slope"), map(float, tsigmas))),
                   "prior": {k: q.tolist() for k, q in zip(tnamed, ens.quantile_vectors(tvec, q3)["quantiles"])},
                   "temperature_and_heat_content": tweigh(lls)}
            nid = ens.define_toa_imbalance()
            ens.compute_diagnostic(nid, 0, NOW + 1)
            c = ens.covariability(TS, nid, 0, NOW + 1, 1, "linear", "linear", 0, slot=1)
            tstats = [c["corr"], c["slope"]]
            toa["all"] = tweigh(ens.loglik_vectors(tstats, tvalues, tsigmas, add_to=lls))
            toa["toa_imbalance"] = tweigh(ens.loglik_vectors(tstats, tvalues, tsigmas))
            w = ens.member_weights()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = [np.nanquantile(P[r], q3, weights=w, method="inverted_cdf").tolist() for r in tnamed.values()]
            checks["toa_imbalance_weighted_quantiles_equal_numpy"] = bool(want == [toa["toa_imbalance"][k] for k in tnamed])
            one = series_covariability(ens.get_series(TS, 0, NOW + 1)[:, :64], ens.get_series(nid, 0, NOW + 1)[:, :64], "linear", "linear", 0)
            checks["toa_imbalance_equals_the_host_estimator"] = bool(all(
                np.array_equal(d.to_host()[:64], h, equal_nan=True) for d, h in zip(tstats, [one["corr"], one["slope"]])))
            for label, key in (("without the imbalance", "temperature_and_heat_content"), ("with it", "all"), ("the imbalance alone", "toa_imbalance")):
                lo, _, hi = toa[key]["lambda0"]
                print(f"lambda0 5-95 % {label}: {lo:.3f} .. {hi:.3f}  (ESS {toa[key]['ess']:.1f})", file=sys.stderr)

        xspec = None
        if a.cross_spectrum:
            # the relation per frequency band, alone and continued from every likelihood above
            xnamed = {"sigma": sigma_row, "phi": phi_row, "lambda0": 0, "efficacy": 2, "heat_capacity_surface": 4, "heat_capacity_deep": 5}
            xvec = [ens.params_vector(r) for r in xnamed.values()]

            def xweigh(l):
                ens.set_weights_from_loglik(l)
                q = ens.quantile_vectors(xvec, q3, weighted=True)["quantiles"]
                return {"ess": ens.weights_stats()["ess"], **{k: q[j].tolist() for j, k in enumerate(xnamed)}}

            # the likelihoods before this one, formed again: the handle has ONE likelihood vector and four slots, and the branches above
            # have reused both (the covariability branch ends on its own likelihood alone, in the spectrum's slot)
            lls = ens.loglik_vectors(stats, values, sigmas)
            if a.spectrum:
                spec = ens.spectrum(TS, 0, NOW + 1, detrend="difference", bands=rec["edges"], slot=1)
                lls = ens.loglik_spectrum(spec["power"], rec["power"], rec["counts"], add_to=lls)
            lls = ens.loglik_vectors([hvar["sd"], hvar["r1"]], hvalues, hsigmas, add_to=lls)
            if a.spectrum:
                lls = ens.loglik_spectrum(hspec["power"], hrec["power"], hrec["counts"], add_to=lls)
            if a.covariability:
                c = ens.covariability(TS, hid, 0, NOW + 1, 1, "linear", "difference", 1, slot=1)
                lls = ens.loglik_vectors([c["corr"], c["slope"], c["lead"][0], c["lag"][0]], cvalues, csigmas, add_to=lls)
            xt = series_cross_spectrum(annual, annual_heat, "linear", "difference")
            x = ens.cross_spectrum(TS, hid, 0, NOW + 1, 1, "linear", "difference", xt["edges"], slot=0)
            xnames, xvalues, xsigmas, xstats = [], [], [], []
            for b, m in enumerate(xt["counts"]):
                coh2 = xt["coherence2"][b]
                # |gain| is the magnitude of the complex gain: its in-phase and quadrature parts carry the same error
                gsig = np.sqrt(2.0) * np.sqrt((1.0 - coh2) / (2.0 * m * coh2)) * np.hypot(xt["gain"][b], xt["gain_quad"][b])
                for key, sig in (("coherence2", np.sqrt(2.0) * np.sqrt(2.0 / m) * (1.0 - coh2) * np.sqrt(coh2)),
                                 ("gain", gsig), ("gain_quad", gsig)):
                    if np.isfinite(sig) and sig > 0.0:         # (a band of one ordinate has coh2 = 1: no sampling error to score against)
                        xnames.append(f"{key}_{b}")
                        xvalues.append(float(xt[key][b]))
                        xsigmas.append(float(sig))
                        xstats.append(x[key][b])
            xspec = {"quantiles": q3, "edges": xt["edges"].tolist(), "counts": xt["counts"].tolist(), "target": dict(zip(xnames, xvalues)),
                     "target_sigma": dict(zip(xnames, xsigmas)),
                     "prior": {k: q.tolist() for k, q in zip(xnamed, ens.quantile_vectors(xvec, q3)["quantiles"])}}
            xspec["before"] = xweigh(lls)
            xspec["all"] = xweigh(ens.loglik_vectors(xstats, xvalues, xsigmas, add_to=lls))
            xspec["cross_spectrum"] = xweigh(ens.loglik_vectors(xstats, xvalues, xsigmas))
            w = ens.member_weights()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = [np.nanquantile(P[r], q3, weights=w, method="inverted_cdf").tolist() for r in xnamed.values()]
            checks["cross_spectrum_weighted_quantiles_equal_numpy"] = bool(want == [xspec["cross_spectrum"][k] for k in xnamed])
            # 64 members' vectors against the host estimator on their own rows, bit for bit
            one = series_cross_spectrum(ens.get_series(TS, 0, NOW + 1)[:, :64], ens.get_series(hid, 0, NOW + 1)[:, :64], "linear", "difference",
                                        xt["edges"])
            checks["cross_spectrum_equals_the_host_estimator"] = bool(all(
                np.array_equal(x[key][b].to_host()[:64], one[key][b], equal_nan=True)
                for key in ("coherence2", "gain", "gain_quad") for b in range(len(xt["counts"]))))

        correlations = None
        if a.correlations:
            # the posterior as numbers: exact weighted means, sd and correlations of all parameter rows under the weights the last
            # estimator asked for has left on the handle
            pnames = ["lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep", "sigma", "phi"]
            prows = [0, 1, 2, 3, 4, 5, sigma_row, phi_row]
            m = ens.moments([ens.params_vector(r) for r in prows], weighted=True)
            correlations = {"parameters": pnames, "weight": int(m["weight"]), "count": int(m["count"]), "mean": m["mean"].tolist(),
                            "sd": m["sd"].tolist(), "corr": m["corr"].tolist()}
            print("posterior correlations (weights of the last estimator):", file=sys.stderr)
            print(" " * 22 + " ".join(f"{k[:8]:>8}" for k in pnames), file=sys.stderr)
            for k, row in zip(pnames, m["corr"]):
                print(f"{k:>22}" + " ".join(f"{v:8.3f}" for v in row), file=sys.stderr)

    res = {"members": a.members, "draws": a.draws, "mode": "FAST" if a.fast else "EXACT", "quantiles": Q, "ess": ess,
           "truth": {"sigma": TRUTH[6], "phi": TRUTH[7]},
           "prior": {"sigma": prior[0].tolist(), "phi": prior[1].tolist()},
           "weighted": {"sigma": post[0].tolist(), "phi": post[1].tolist()},
           "variability_target": {"sd": values[0], "r1": values[1], "sd_sigma": float(sigmas[0]), "r1_sigma": float(sigmas[1])},
           "constraint": {"prior": {"sigma": prior[0].tolist(), "phi": prior[1].tolist()},
                          "point": {"sigma": post[0].tolist(), "phi": post[1].tolist(), "ess": ess},
                          "statistics": constraint["statistics"], "both": constraint["both"]},
           "posterior_plume_2100_K": plume.tolist(), "checks": checks}
    if spectral is not None:
        res["spectrum_target"] = spectral
        res["constraint"]["spectrum"] = constraint["spectrum"]
        res["constraint"]["spectrum_and_statistics"] = constraint["spectrum_and_statistics"]
    if heat is not None:
        res["heat_content"] = heat
    if cov is not None:
        res["covariability"] = cov
    if toa is not None:
        res["toa_imbalance"] = toa
    if xspec is not None:
        res["cross_spectrum"] = xspec
    if crossing is not None:
        res["crossing_1p5K"] = crossing
    if correlations is not None:
        res["correlations"] = correlations
    print(json.dumps(res), flush=True)
    sys.exit(0 if all(checks.values()) else 1)


if __name__ == "__main__":
    main()
