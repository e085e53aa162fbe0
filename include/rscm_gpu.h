/*
 * rscm_gpu.h -- C ABI of the MI355X (gfx950) ensemble runner for RSCM's two-layer hot path.
 *
 * This is the drop-in boundary: every entry point is `extern "C"`, takes plain pointers and
 * sizes (no torch / C++ types), returns an int status (0 = ok) and never unwinds across the
 * ABI.  It is what a Rust `impl ModelRunner for GpuRunner` / `impl Component` shim, or the
 * Python front-end (ctypes), binds -- see INTEGRATION.md for the reference-side stubs.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   - Model::run / step / step_model / step_model_component
 *         crates/rscm-core/src/model/runtime.rs:368-527             -> rscm_ens_run*
 *   - ModelBuilder::build collection initialisation (initial values at index 0,
 *     exogenous series on the model axis)
 *         crates/rscm-core/src/model/builder.rs:735-830             -> rscm_ens_set_initial,
 *                                                                      rscm_ens_set_forcing
 *   - VariableSource index rule (Exogenous/OwnState -> n, UpstreamOutput -> n+1)
 *         crates/rscm-core/src/state/windows.rs:229-234             -> `source` argument
 *   - TwoLayer::solve + IVP RHS   crates/rscm-two-layer/src/component.rs:159-251
 *   - CarbonCycle::solve          crates/rscm-components/src/components/carbon_cycle.rs:102-159
 *   - CO2ERF::solve               crates/rscm-components/src/components/co2_erf.rs:57-80
 *   - scalar Sum aggregate        crates/rscm-core/src/schema.rs:760-773,886-901
 *   - RK4 driver + end-time check crates/rscm-core/src/ivp/mod.rs:73-102,245-253
 *   - ModelRunner::run_batch      crates/rscm-calibrate/src/model_runner.rs:38-85,215-267
 *         (order-preserving, per-member failure)                    -> rscm_ens_set_params*,
 *                                                                      rscm_ens_run, rscm_ens_status
 *   - extract_outputs             crates/rscm-calibrate/src/model_runner.rs:161-212
 *                                                                   -> rscm_ens_get_series
 *   - GaussianLikelihood          crates/rscm-calibrate/src/likelihood.rs:167-250
 *                                                                   -> rscm_ens_loglik
 *   - ParameterSet::sample_lhs    crates/rscm-calibrate/src/parameter_set.rs:207-233
 *                                                                   -> rscm_ens_sample_lhs
 *
 * Data layout (device, HBM): structure-of-arrays, member index fastest.
 *   params   [P][N]      f64
 *   series   [V][T][N]   f64   (index 0 of a state variable holds its initial value; outputs of
 *                               step n are written at index n+1, runtime.rs:480; never-written
 *                               entries are NaN, builder.rs:772-780)
 *   forcing  [S][T]      f64   shared scenarios, staged in LDS by the kernels
 *
 * Environment: the library reads exactly two variables, both once per process, neither changes a result.
 *   RSCM_SPLIT_RUNS=0     whole-axis runs over more members than one wavefront per SIMD are issued as ONE plain launch
 *                         instead of two member blocks on two streams in chunks of model steps (rscm_ens_last_run_plan);
 *                         same kernels on the same operands, the same bits -- an A/B and debugging switch.  Default: on.
 *   RSCM_POISON_ALLOC=1   debug aid: every device allocation starts as 0xFF bytes (NaN as a double, 255 as a status byte) so
 *                         that a read of memory nobody wrote shows in the results.  Default: off (one fill per allocation).
 * Nothing else in the environment reaches a launch plan: the sweep knobs of earlier rounds exist only in the experiments
 * build (csrc/experiment_env.hpp, `make EXPERIMENTS=1`), which rscm_gpu_experiments_build() of the internal header identifies.
 *
 * Threading: a handle is not thread-safe; use one handle per device per thread
 * (the reference calls run_batch from one thread at a time, sampler/ensemble.rs:145).
 * Ownership: the caller owns every input buffer (copied/uploaded before the call returns);
 * the library owns device buffers until rscm_ens_destroy.
 */
#ifndef RSCM_GPU_H
#define RSCM_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSCM_GPU_ABI_VERSION 1
/* Bumped whenever an entry point is added or a mode changes what a kind computes while the major version stays:
 *   1  rscm_sampler_create_graph; four hooks moved to rscm_gpu_internal.h; RSCM_MODE_FAST acts on ClimateUDEB
 *   2  RSCM_MODE_FAST acts on the coupled chain and on CarbonCycle; rscm_gpu_abi_minor itself
 *   3  rscm_ens_last_run_plan.  In the internal header (rscm_gpu_internal.h, not part of this ABI) the same release REMOVED
 *      rscm_gpu_graph_stamps, made rscm_gpu_set_udeb_variant(4) an error (the four-wavefront kernel is gone) and re-used
 *      rscm_gpu_set_lockstep_fusion mode 4 (was: the whole-graph launch; now: mode 1 without the two-wavefront op split): a
 *      host built against the round-3 internal header does not link, or gets the new meaning of mode 4
 *   4  ClimateUDEB keeps its columns on chip at EVERY n_layers <= 64 (no entry point changed: same results, the counts
 *      other than 20 / 30 / 40 / 50 are ~15x faster); internal header: rscm_gpu_fail_chunk_launch, rscm_gpu_set_run_plan,
 *      rscm_gpu_set_udeb_variant(3)
 *   5  no entry point changed.  The shipped library no longer reads RSCM_SPLIT_CHUNK / _CHUNK2 / _FIRST, RSCM_LOCKSTEP_SPLIT or
 *      RSCM_UDEB_VARIANT (section "Environment" above); internal header: rscm_gpu_experiments_build, and
 *      rscm_gpu_fail_chunk_launch is consumed by the next cut run whether or not k is reached
 *   6  exact quantiles of any storage layout (windowed, output store) and of sharded ensembles: rscm_ens_quantile_rows and the
 *      staged select rscm_ens_select_begin / _pass / _commit / _result / _end
 *   7  likelihood-weighted quantiles (numpy "inverted_cdf" with integer weights): rscm_ens_set_member_weights,
 *      rscm_ens_member_weights_devptr, rscm_ens_loglik_max, rscm_ens_set_weights_from_loglik, rscm_ens_weighted_quantile_rows,
 *      rscm_ens_select_begin_weighted
 *   8  anomalies, per-member indicators and exceedance: rscm_ens_set_baseline, rscm_ens_set_baseline_values,
 *      rscm_ens_baseline_devptr, rscm_ens_clear_baseline, rscm_ens_quantile_rows_ex, rscm_ens_select_begin_ex,
 *      rscm_ens_member_indicators, rscm_ens_quantile_vectors, rscm_ens_select_begin_vectors, rscm_ens_exceedance
 *   9  likelihoods against anomalies from a reference period: rscm_ens_loglik_ref, rscm_ens_loglik_ref_device,
 *      rscm_ens_run_loglik_ref, rscm_ens_run_loglik_ref_device, rscm_sampler_set_reference
 *  10  posterior ensembles on the device: rscm_ens_weights_stats, rscm_ens_resample, rscm_gpu_resample_offset,
 *      rscm_ens_gather_members
 *  11  per-group quantiles and exceedance: rscm_ens_set_member_groups, rscm_ens_member_groups_devptr,
 *      rscm_ens_clear_member_groups, RSCM_SELECT_GROUPED, rscm_ens_exceedance_grouped
 *  12  two-layer mix handles -- per-member forcing as a scaled sum of shared components: rscm_ens_create_mix,
 *      rscm_ens_n_forcing_components, RSCM_TL_P_COEFF0, RSCM_TL_MAX_COMPONENTS
 *  13  seeded forcing noise of a two-layer handle (internal variability): rscm_ens_set_forcing_noise, rscm_ens_clear_forcing_noise,
 *      rscm_ens_forcing_noise, rscm_ens_forcing_noise_rows, RSCM_NOISE_STREAM_TAG
 *  14  red (AR(1)) forcing noise: rscm_ens_set_forcing_noise_ar1, rscm_ens_forcing_noise_ar1
 *  15  per-member noise amplitude and persistence as parameter rows: RSCM_FLAG_NOISE_PARAMS, RSCM_TL_P_NOISE_SIGMA, RSCM_TL_P_NOISE_PHI,
 *      rscm_ens_set_forcing_noise_members, rscm_ens_forcing_noise_members
 *  16  per-member variability statistics (mean, trend, variance, sd, lag-one autocorrelation) and a Gaussian likelihood over
 *      per-member device vectors: rscm_ens_member_variability, RSCM_VAR_MEAN, RSCM_VAR_LINEAR, RSCM_VAR_DIFFERENCE,
 *      rscm_ens_loglik_vectors_device
 *  17  per-member power spectra in frequency bands and a spectral (Whittle-type) likelihood over them: rscm_ens_member_spectrum,
 *      rscm_gpu_spectrum_coefficients, rscm_ens_loglik_spectrum_device
 *  18  diagnostic variables: per-member linear combinations of a handle's stored variables (ocean heat content) that every reader of
 *      rows takes by variable id: rscm_ens_define_diagnostic, rscm_ens_diagnostic, rscm_ens_compute_diagnostic,
 *      rscm_ens_clear_diagnostics, rscm_ens_n_diagnostics, RSCM_DIAG_MAX_TERMS, RSCM_DIAG_MAX
 *  19  no entry point changed.  rscm_ens_quantile_series runs the radix select of rscm_ens_quantile_rows instead of a sort: the
 *      same bits, except that where a quantile lands on a zero the sign is the select's (-0.0 orders before +0.0, a function of
 *      the member set); the sort returned whichever zero sat first among the members, which the contract left unspecified
 *  20  per-member covariability of two variables (covariance, correlation, regression slope, cross-correlation at up to three leads
 *      and lags): rscm_ens_member_covariability, RSCM_COV_MAX_LAGS
 *  21  per-member co-spectra of two variables in frequency bands (squared coherence, gain and quadrature gain per band):
 *      rscm_ens_member_cross_spectrum, rscm_gpu_spectrum_sines, RSCM_XSPEC_MAX_BANDS
 *  22  energy-budget diagnostics of a two-layer handle -- the member's forcing, radiative response, deep-ocean heat uptake and
 *      top-of-atmosphere imbalance as diagnostic variables: rscm_ens_define_energy_budget, rscm_ens_diagnostic_quantity,
 *      RSCM_BUDGET_FORCING, RSCM_BUDGET_RESPONSE, RSCM_BUDGET_DEEP_UPTAKE, RSCM_BUDGET_IMBALANCE
 *  23  exact weighted means and covariances of per-member vectors across members, in a fixed-point integer accumulator that shards
 *      add up: rscm_ens_moment_sums, rscm_gpu_moment_finish, rscm_ens_moments, RSCM_MOMENT_MAX_VECTORS, RSCM_MOMENT_BLOCK
 *  24  the same exact weighted mean and spread of a stored variable at every row, with its covariance with up to four per-member
 *      vectors (the regression of each year on a parameter): rscm_ens_moment_rows_sums, rscm_ens_moment_rows,
 *      RSCM_MOMENT_ROWS_MAX_VECTORS, RSCM_MOMENT_ROWS_MAX_BLOCKS
 *  25  the device Latin hypercube through Normal, LogNormal and truncated priors: rscm_ens_sample_lhs_priors, RSCM_PRIOR_UNIFORM,
 *      RSCM_PRIOR_NORMAL, RSCM_PRIOR_LOGNORMAL, RSCM_PRIOR_REFLECT
 *  26  the exceedance of up to eight thresholds, fixed or per row, and the rank of a record inside the plume, for every row of a
 *      stored variable in one launch: rscm_ens_exceedance_rows, RSCM_EXCEEDANCE_ROWS_MAX_THRESHOLDS
 *  27  running means of a stored variable or of a diagnostic over the time axis as diagnostic variables, which every reader of rows
 *      then takes by id: rscm_ens_define_running_mean, rscm_ens_diagnostic_running_mean, RSCM_RUNMEAN_MAX_WINDOW,
 *      RSCM_RUNMEAN_TRAILING, RSCM_RUNMEAN_CENTRED
 *  28  histograms across members, in exact integers that shards add up: of a stored variable at every row, of up to eight
 *      per-member vectors with shared or own edges, and of two vectors jointly: rscm_ens_histogram_rows, rscm_ens_histogram_vectors,
 *      rscm_ens_histogram2d, RSCM_HISTOGRAM_MAX_EDGES, RSCM_HISTOGRAM_MAX_SLOTS, RSCM_HISTOGRAM_MAX_VECTORS */
#define RSCM_GPU_ABI_MINOR 28

#if defined(__GNUC__)
#define RSCM_API __attribute__((visibility("default")))
#else
#define RSCM_API
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define RSCM_OK 0
#define RSCM_ERR_INVALID 1   /* bad argument / size (cf. model_runner.rs:225-231)               */
#define RSCM_ERR_STATE 2     /* call order / time index (cf. runtime.rs:516 assert)               */
#define RSCM_ERR_TIME_AXIS 3 /* RK4 end time misses t_next by >= 5e-3 (ivp/mod.rs:97 panics)   */
#define RSCM_ERR_DEVICE 4    /* HIP runtime error (text in rscm_gpu_last_error)                 */
#define RSCM_ERR_NOMEM 5

/* ---- model kinds -------------------------------------------------------------------------- */
#define RSCM_KIND_TWO_LAYER 0 /* stand-alone TwoLayer with a forcing series                     */
#define RSCM_KIND_COUPLED 1   /* CarbonCycle -> CO2ERF -> Sum aggregate -> TwoLayer             */

#define RSCM_KIND_UDEB 2      /* rscm-magicc ClimateUDEB (4-box upwelling-diffusion EBM)          */
#define RSCM_KIND_GHG_FORCING 3 /* rscm-magicc GhgForcing (CO2/CH4/N2O concentrations -> ERF)     */
#define RSCM_KIND_OZONE_FORCING 4    /* rscm-magicc OzoneForcing                                  */
#define RSCM_KIND_AEROSOL_DIRECT 5   /* rscm-magicc AerosolDirect (FourBox output)                */
#define RSCM_KIND_AEROSOL_INDIRECT 6 /* rscm-magicc AerosolIndirect                               */
#define RSCM_KIND_CH4_CHEMISTRY 7    /* rscm-magicc CH4Chemistry (Prather iteration)              */
#define RSCM_KIND_N2O_CHEMISTRY 8    /* rscm-magicc N2OChemistry (stratospheric delay)            */
#define RSCM_KIND_CO2_BUDGET 9       /* rscm-magicc CO2Budget                                     */
#define RSCM_KIND_TERRESTRIAL_CARBON 10 /* rscm-magicc TerrestrialCarbon (four pools)             */
#define RSCM_KIND_OCEAN_CARBON 11    /* rscm-magicc OceanCarbon (impulse-response mixed layer)    */
#define RSCM_KIND_HALOCARBON 12      /* rscm-magicc HalocarbonChemistry (41 species)              */
#define RSCM_KIND_FOURBOX_OHU 13     /* rscm-components FourBoxOceanHeatUptake                    */
#define RSCM_KIND_OSPP 14            /* rscm-components OceanSurfacePartialPressure               */
/* the members of the coupled chain on their own, for graphs assembled with rscm_ens_link_input */
#define RSCM_KIND_CARBON_CYCLE 15    /* rscm-components CarbonCycle (RK4, three states)           */
#define RSCM_KIND_CO2_ERF 16         /* rscm-components CO2ERF                                    */
#define RSCM_KIND_AGGREGATE 17       /* rscm-core schema aggregate (Sum / Mean / Weighted)        */

/* variable ids, kind TWO_LAYER (V = 3) */
#define RSCM_TL_VAR_ERF 0 /* "Effective Radiative Forcing"  (input, [S][T] shared)              */
#define RSCM_TL_VAR_TS 1  /* "Surface Temperature"          (state)                             */
#define RSCM_TL_VAR_TD 2  /* "Deep Ocean Temperature"       (state)                             */

/* variable ids, kind COUPLED (V = 8) */
#define RSCM_CP_VAR_EMISSIONS 0 /* "Emissions|CO2|Anthropogenic" (input, [S][T] shared)         */
#define RSCM_CP_VAR_TS 1
#define RSCM_CP_VAR_TD 2
#define RSCM_CP_VAR_CONC 3       /* "Atmospheric Concentration|CO2"  (state)                    */
#define RSCM_CP_VAR_CUM_UPTAKE 4 /* "Cumulative Land Uptake"         (state)                    */
#define RSCM_CP_VAR_CUM_EMIS 5   /* "Cumulative Emissions|CO2"       (state)                    */
#define RSCM_CP_VAR_ERF_CO2 6    /* "Effective Radiative Forcing|CO2" (output)                  */
#define RSCM_CP_VAR_ERF 7        /* "Effective Radiative Forcing"     (aggregate output)        */

/* variable ids, kind UDEB (V = 8): crates/rscm-magicc/src/climate/udeb/mod.rs:80-91 */
#define RSCM_UD_VAR_ERF 0          /* "Effective Radiative Forcing" (input, [S][T] shared)      */
#define RSCM_UD_VAR_ST_NH_OCEAN 1  /* "Surface Temperature" FourBox state: NorthernOcean        */
#define RSCM_UD_VAR_ST_NH_LAND 2   /*                                      NorthernLand         */
#define RSCM_UD_VAR_ST_SH_OCEAN 3  /*                                      SouthernOcean        */
#define RSCM_UD_VAR_ST_SH_LAND 4   /*                                      SouthernLand         */
#define RSCM_UD_VAR_HEAT_UPTAKE 5  /* "Heat Uptake"              (output)                       */
#define RSCM_UD_VAR_OHC 6          /* "Ocean Heat Content"       (output)                       */
#define RSCM_UD_VAR_SST 7          /* "Sea Surface Temperature"  (output)                       */

/* GhgForcing (crates/rscm-magicc/src/forcing/ghg.rs:69-83).  The shared input of this kind is a
 * block of three rows per scenario, series[n_scen][3][n_times]: "Atmospheric Concentration|CO2"
 * (ppm), "...|CH4" (ppb), "...|N2O" (ppb). */
#define RSCM_GH_VAR_CONC 0     /* the three concentration rows (input, [S][3][T] shared)         */
#define RSCM_GH_VAR_ERF_CO2 1  /* "Effective Radiative Forcing|CO2" (output)                     */
#define RSCM_GH_VAR_ERF_CH4 2  /* "Effective Radiative Forcing|CH4" (output)                     */
#define RSCM_GH_VAR_ERF_N2O 3  /* "Effective Radiative Forcing|N2O" (output)                     */
/* GhgForcing parameter rows (P = 21): GhgForcingParameters field order
 * (crates/rscm-magicc/src/parameters/ghg_forcing.rs); method 0 = Ipcctar, 1 = Olbl, [u] uniform. */
#define RSCM_GH_NPARAMS 21
#define RSCM_GH_P_METHOD 0      /* [u] */
#define RSCM_GH_P_CO2_PI 1
#define RSCM_GH_P_CH4_PI 2
#define RSCM_GH_P_N2O_PI 3
#define RSCM_GH_P_DELQ2XCO2 4
#define RSCM_GH_P_CH4_RADEFF 5
#define RSCM_GH_P_N2O_RADEFF 6
#define RSCM_GH_P_OLBL_CO2_A1 7
#define RSCM_GH_P_OLBL_CO2_B1 8
#define RSCM_GH_P_OLBL_CO2_C1 9
#define RSCM_GH_P_OLBL_CO2_D1 10
#define RSCM_GH_P_OLBL_CH4_A3 11
#define RSCM_GH_P_OLBL_CH4_B3 12
#define RSCM_GH_P_OLBL_CH4_D3 13
#define RSCM_GH_P_OLBL_N2O_A2 14
#define RSCM_GH_P_OLBL_N2O_B2 15
#define RSCM_GH_P_OLBL_N2O_C2 16
#define RSCM_GH_P_OLBL_N2O_D2 17
#define RSCM_GH_P_ADJUST_CO2 18
#define RSCM_GH_P_ADJUST_CH4 19
#define RSCM_GH_P_ADJUST_N2O 20

/* The three stateless forcing components below follow the same convention: variable 0 is the
 * block of input rows per scenario, series[n_scen][n_inputs][n_times], in the order of the
 * component's #[inputs(...)] declaration; variables 1.. are the outputs; the parameter rows are
 * the fields of the parameter struct in declaration order (arrays expanded, booleans as 0/1).
 *
 * OzoneForcing (crates/rscm-magicc/src/forcing/ozone.rs:69-85, parameters/ozone_forcing.rs):
 *   inputs  EESC, Atmospheric Concentration|CH4, Emissions|NOx, Emissions|CO, Emissions|NMVOC,
 *           Surface Temperature
 *   outputs 1 ERF|O3|Stratospheric, 2 ERF|O3|Tropospheric, 3 ERF|O3|Temperature Feedback
 *   params  eesc_reference, strat_o3_scale, strat_cl_exponent, trop_radeff, trop_oz_ch4,
 *           trop_oz_nox, trop_oz_co, trop_oz_voc, ch4_pi, nox_pi, co_pi, nmvoc_pi,
 *           temp_feedback_scale */
#define RSCM_OZ_NINPUTS 6
#define RSCM_OZ_NPARAMS 13
/* AerosolDirect (forcing/aerosol_direct.rs:53-63, parameters/aerosol.rs:6-70):
 *   inputs  Emissions|SOx, Emissions|BC, Emissions|OC, Emissions|NOx
 *   outputs 1-4 ERF|Aerosol|Direct in NorthernOcean, NorthernLand, SouthernOcean, SouthernLand
 *   params  sox/bc/oc/nitrate_coefficient, sox_regional[4], bc_regional[4], oc_regional[4],
 *           nitrate_regional[4], sox_pi, bc_pi, oc_pi, nox_pi, harmonize, harmonize_year,
 *           harmonize_target (the last three are carried but unused by solve, as upstream) */
#define RSCM_AD_NINPUTS 4
#define RSCM_AD_NPARAMS 27
/* AerosolIndirect (forcing/aerosol_indirect.rs:52-60, parameters/aerosol.rs:75-117):
 *   inputs  Emissions|SOx, Emissions|OC;   output 1 ERF|Aerosol|Indirect
 *   params  cloud_albedo_coefficient, reference_burden, sox_weight, oc_weight, sox_pi, oc_pi,
 *           harmonize, harmonize_year, harmonize_target */
#define RSCM_AI_NINPUTS 2
#define RSCM_AI_NPARAMS 9
/* CH4Chemistry (crates/rscm-magicc/src/chemistry/ch4.rs:50-66, parameters/ch4_chemistry.rs):
 *   inputs  Emissions|CH4, Surface Temperature, Emissions|NOx, Emissions|CO, Emissions|NMVOC
 *   state   1 Atmospheric Concentration|CH4 (needs an initial value);  output 2 Lifetime|CH4
 *   params  ch4_pi, natural_emissions, tau_oh, tau_soil, tau_strat, tau_trop_cl,
 *           ch4_self_feedback, oh_sensitivity_scale, oh_nox_sensitivity, oh_co_sensitivity,
 *           oh_nmvoc_sensitivity, temp_sensitivity, include_temp_feedback,
 *           include_emissions_feedback, ppb_to_tg, nox_reference, co_reference, nmvoc_reference */
#define RSCM_CH4_NINPUTS 5
#define RSCM_CH4_NPARAMS 18
/* N2OChemistry (chemistry/n2o.rs:44-54, parameters/n2o_chemistry.rs):
 *   input   Emissions|N2O;  state 1 Atmospheric Concentration|N2O;  output 2 Lifetime|N2O
 *   params  n2o_pi, natural_emissions, tau_n2o, lifetime_feedback, strat_delay (an integer >= 0
 *           held in a double), ppb_to_tg */
#define RSCM_N2O_NINPUTS 1
#define RSCM_N2O_NPARAMS 6
#define RSCM_CHEM_VAR_CONC 1
#define RSCM_CHEM_VAR_LIFETIME 2
/* CO2Budget (crates/rscm-magicc/src/carbon/budget.rs:60-75, parameters/co2_budget.rs):
 *   inputs  Emissions|CO2|Fossil, Emissions|CO2|Land Use, Carbon Flux|Terrestrial, Carbon Flux|Ocean
 *   state   1 Atmospheric Concentration|CO2;  outputs 2 Emissions|CO2|Net, 3 Airborne Fraction|CO2
 *   params  gtc_per_ppm, co2_pi */
#define RSCM_CB_NINPUTS 4
#define RSCM_CB_NPARAMS 2
/* TerrestrialCarbon (carbon/terrestrial.rs:66-82, parameters/terrestrial_carbon.rs):
 *   inputs  Atmospheric Concentration|CO2, Surface Temperature, Emissions|CO2|Land Use
 *   states  1 Carbon Pool|Plant, 2 Carbon Pool|Detritus, 3 Carbon Pool|Soil, 4 Carbon Pool|Humus
 *   output  5 Carbon Flux|Terrestrial
 *   params  npp_pi, co2_pi, beta, npp/resp/detritus/soil/humus_temp_sensitivity,
 *           plant/detritus/soil/humus_pool_pi, respiration_pi, frac_npp_to_plant,
 *           frac_npp_to_detritus, frac_plant_to_detritus, frac_detritus_to_soil,
 *           frac_soil_to_humus, enable_fertilization, enable_temp_feedback */
#define RSCM_TC_NINPUTS 3
#define RSCM_TC_NPARAMS 20
/* OceanCarbon (crates/rscm-magicc/src/carbon/ocean.rs:46-62, parameters/ocean_carbon.rs:73-196):
 *   inputs  Atmospheric Concentration|CO2, Sea Surface Temperature (the anomaly the component
 *           uses as delta_sst)
 *   states  1 Ocean Surface pCO2, 2 Cumulative Ocean Uptake;  output 3 Carbon Flux|Ocean
 *   params  model [u] (0 = 3D-GFDL, 1 = 2D-BERN, 2 = HILDA: selects the two IrfForm coefficient
 *           sets of the reference's presets; other IrfForm contents are not supported), co2_pi,
 *           pco2_pi, gas_exchange_scale, gas_exchange_tau, temp_sensitivity, irf_scale [u],
 *           mixed_layer_depth, ocean_surface_area, sst_pi, steps_per_year [u] (12),
 *           max_history_months [u], irf_switch_time [u], delta_ospp_offsets[5],
 *           delta_ospp_coefficients[5], enable_temp_feedback.  [u] rows are uniform. */
#define RSCM_OC_NINPUTS 2
#define RSCM_OC_NPARAMS 24
#define RSCM_OC_P_MODEL 0
#define RSCM_OC_P_IRF_SCALE 6
#define RSCM_OC_P_STEPS_PER_YEAR 10
#define RSCM_OC_P_MAX_HISTORY_MONTHS 11
#define RSCM_OC_P_IRF_SWITCH_TIME 12
/* HalocarbonChemistry (crates/rscm-magicc/src/chemistry/halocarbon.rs:262-300,
 * parameters/halocarbon.rs:46-160) with the species list of HalocarbonParameters::default():
 * 23 F-gases then 18 Montreal gases, in that order (41 species; other list lengths are not
 * supported on the device).
 *   inputs  Emissions|<species> x 41 (kt/yr), in species order
 *   states  1..41 Atmospheric Concentration|<species> (ppt)
 *   outputs 42 Forcing|Halocarbons, 43 Forcing|F-gases, 44 Forcing|Montreal Gases, 45 EESC
 *   params  br_multiplier, cfc11_release_normalisation, eesc_delay, air_molar_mass,
 *           atmospheric_mass_tg, mixing_box_fraction, then per species: lifetime,
 *           radiative_efficiency, concentration_pi, molecular_weight, n_cl, n_br,
 *           fractional_release */
#define RSCM_HC_NSPECIES 41
#define RSCM_HC_NINPUTS 41
#define RSCM_HC_NPARAMS (6 + 41 * 7)
/* FourBoxOceanHeatUptake (crates/rscm-components/src/components/four_box_ocean_heat_uptake.rs):
 *   input   Effective Radiative Forcing|Aggregated;  outputs 1-4 Heat Uptake|Ocean in
 *   NorthernOcean, NorthernLand, SouthernOcean, SouthernLand
 *   params  northern_ocean_ratio, northern_land_ratio, southern_ocean_ratio, southern_land_ratio
 *           (from_parameters asserts they average to 1 within 0.01; the front-end mirrors that) */
#define RSCM_FB_NINPUTS 1
#define RSCM_FB_NPARAMS 4
/* OceanSurfacePartialPressure (.../ocean_carbon_cycle/ocean_surface_partial_pressure.rs):
 *   inputs  Sea Surface Temperature, Dissolved Inorganic Carbon (both anomalies)
 *   output  1 Ocean Surface Partial Pressure|CO2
 *   params  ospp_preindustrial, sensitivity_ospp_to_temperature,
 *           sea_surface_temperature_preindustrial, delta_ospp_offsets[5], delta_ospp_coefficients[5] */
#define RSCM_SP_NINPUTS 2
#define RSCM_SP_NPARAMS 13
/* CarbonCycle (crates/rscm-components/src/components/carbon_cycle.rs:102-159):
 *   inputs  Emissions|CO2|Anthropogenic, Surface Temperature
 *   states  1 Atmospheric Concentration|CO2, 2 Cumulative Land Uptake, 3 Cumulative Emissions|CO2
 *   params  tau, conc_pi, alpha_temperature; RK4 step via rscm_ens_set_step_size(RSCM_COMP_CARBON_CYCLE)
 *   Same arithmetic as inside RSCM_KIND_COUPLED: the linked graph reproduces the fused kind's bits. */
#define RSCM_CC_NINPUTS 2
#define RSCM_CC_NPARAMS 3
/* CO2ERF (co2_erf.rs:57-80): input Atmospheric Concentration|CO2; output 1 Effective Radiative
 *   Forcing|CO2; params erf_2xco2, conc_pi */
#define RSCM_CE_NINPUTS 1
#define RSCM_CE_NPARAMS 2
/* Schema aggregate (AggregatorComponent / compute_aggregate, crates/rscm-core/src/schema.rs:760-802,
 * 886-901): up to eight contributors, every one read at index n+1 (at_end(), whatever `source` is
 * passed), NaN contributors skipped, all-NaN -> NaN.  The input block starts out all-NaN, so only the
 * rows that are linked or set take part.  output 1 the aggregate.
 *   params  operation (0 Sum, 1 Mean, 2 Weighted = sum of value * weight, no renormalisation),
 *           weights[8]
 * More than eight contributors are chained through several such ensembles (a partial enters the next stage
 * as its row 0: the additions keep compute_aggregate's order).  For a Mean that takes three helper
 * operations: 3 = number of non-NaN rows, 4 = row 0 (a count carried in) + number of non-NaN rows 1..7,
 * 5 = row 0 / row 1 (sum / count; NaN when the count is 0). */
#define RSCM_AG_NINPUTS 8
#define RSCM_AG_NPARAMS 9

/* UDEB parameter rows (P = 37): ClimateUDEBParameters field order
 * (crates/rscm-magicc/src/parameters/climate_udeb.rs), booleans/enums/integers as doubles.
 * Rows marked [u] are structural and must be equal for every member.  n_layers: any count >= 2 as in the reference
 * (climate/udeb/mod.rs:162-165; at most 4096 here).  Up to 64 layers a member's two columns stay in registers + LDS for a
 * whole launch (20, 30, 40, 50 with the count compiled in; every other count in the next capacity's instance of the same
 * unrolled solve with the count at run time); 65 to 128 layers keep the column in registers and the solve's work array in LDS
 * (about 6x the per-layer cost of the counts up to 64), more than 128 run a slower kernel with the columns in HBM (same
 * arithmetic, same parity bar throughout).  Device memory per handle besides the series: 2 x max(64, n_layers) x N x 8 B of columns,
 * 11 x N x 8 B of scalars, T x N x 8 B of temperature history, and -- for counts other than 20 / 30 / 40 / 50 --
 * n_layers x N x 8 B of work array (e.g. n_layers = 4096, N = 1e5: 9.8 GB; n_layers = 49: 90 MB).  The reference's MAGICC7
 * files pin the 50-layer configuration only: at every other count parity is against the CPU restatement kept with the tests.
 * ocean_temp_profile = 2 (CMIP5) only. */
#define RSCM_UD_NPARAMS 37
#define RSCM_UD_P_N_LAYERS 0              /* [u] */
#define RSCM_UD_P_MIXED_LAYER_DEPTH 1     /* [u] */
#define RSCM_UD_P_LAYER_THICKNESS 2       /* [u] */
#define RSCM_UD_P_KAPPA 3
#define RSCM_UD_P_KAPPA_MIN 4
#define RSCM_UD_P_KAPPA_DKDT 5
#define RSCM_UD_P_W_INITIAL 6
#define RSCM_UD_P_W_VARIABLE_FRACTION 7
#define RSCM_UD_P_W_THRESHOLD_TEMP_NH 8
#define RSCM_UD_P_W_THRESHOLD_TEMP_SH 9
#define RSCM_UD_P_ECS 10
#define RSCM_UD_P_RF_2XCO2 11
#define RSCM_UD_P_RLO 12
#define RSCM_UD_P_FEEDBACK_Q_SENSITIVITY 13
#define RSCM_UD_P_FEEDBACK_CUMT_SENSITIVITY 14
#define RSCM_UD_P_FEEDBACK_CUMT_PERIOD 15   /* [u] */
#define RSCM_UD_P_K_LO 16
#define RSCM_UD_P_K_NS 17
#define RSCM_UD_P_AMPLIFY_OCEAN_TO_LAND 18
#define RSCM_UD_P_NH_LAND_FRACTION 19
#define RSCM_UD_P_SH_LAND_FRACTION 20
#define RSCM_UD_P_DEPTH_DEPENDENT_AREA 21 /* [u] */
#define RSCM_UD_P_TEMP_ADJUST_ALPHA 22
#define RSCM_UD_P_TEMP_ADJUST_GAMMA 23
#define RSCM_UD_P_POLAR_SINKING_RATIO 24
#define RSCM_UD_P_LAND_HC_ENABLED 25      /* [u] */
#define RSCM_UD_P_K_LG 26
#define RSCM_UD_P_LAND_HC_EFF_THICKNESS 27
#define RSCM_UD_P_RF_REGIONS_CO2_0 28     /* ..31: NorthernOcean, NorthernLand, SouthernOcean, SouthernLand */
#define RSCM_UD_P_EFFICACY_APPLY 32       /* [u] */
#define RSCM_UD_P_PRESCRIBED_EFFICACY_CO2 33
#define RSCM_UD_P_OCEAN_TEMP_PROFILE 34   /* [u] */
#define RSCM_UD_P_STEPS_PER_YEAR 35       /* [u] */
#define RSCM_UD_P_MAX_TEMPERATURE 36
/* rscm_ens_status for this kind: 0 ok, 2 invalid prescribed_efficacy_co2, 4 LAMCALC did not
 * converge (ClimateUDEB::from_parameters returns Err; mod.rs:161-205) -- all outputs NaN. */

/* parameter rows.  TWO_LAYER: P = 6, TwoLayerParameters field order (component.rs:38-90):
 *   lambda0, a, efficacy, eta, heat_capacity_surface, heat_capacity_deep
 * COUPLED: P = 10: the six above, then tau, conc_pi, alpha_temperature (carbon_cycle.rs:24-34),
 *   erf_2xco2 (co2_erf.rs:18-25; CO2ERF.conc_pi == conc_pi as in docs/notebooks/coupled_model.py) */
#define RSCM_TL_NPARAMS 6
#define RSCM_CP_NPARAMS 10
/* A two-layer MIX handle (rscm_ens_create_mix) with K forcing components has P = 6 + K: rows RSCM_TL_P_COEFF0 .. RSCM_TL_P_COEFF0 + K - 1
 * are the members' coefficients c_0 .. c_K-1 of the components. */
#define RSCM_TL_P_COEFF0 6
#define RSCM_TL_MAX_COMPONENTS 8
/* A two-layer handle created with RSCM_FLAG_NOISE_PARAMS (plain: K = 0, or mix with K components) has two more rows after the
 * coefficients, P = 6 + K + 2: every member's noise amplitude sigma_i and persistence phi_i (rscm_ens_set_forcing_noise_members). */
#define RSCM_TL_P_NOISE_SIGMA(K) (RSCM_TL_P_COEFF0 + (K))
#define RSCM_TL_P_NOISE_PHI(K) (RSCM_TL_P_COEFF0 + (K) + 1)

/* VariableSource of the shared input as seen by its consumer (state/mod.rs:156-170) */
#define RSCM_SRC_EXOGENOUS 0 /* read index n   */
#define RSCM_SRC_UPSTREAM 1  /* read index n+1 */

/* solver components for rscm_ens_set_step_size */
#define RSCM_COMP_TWO_LAYER 0    /* reference hard-codes 0.1 (component.rs:240)                 */
#define RSCM_COMP_CARBON_CYCLE 1 /* SolverOptions.step_size, default 0.1 (carbon_cycle.rs:83)   */

/* arithmetic modes */
#define RSCM_MODE_EXACT 0 /* op-for-op the reference's f64 expression order, no FMA contraction:
                             bit-identical to the CPU oracle for the two-layer kind            */
#define RSCM_MODE_FAST 1  /* FMA + reciprocal heat capacities; |rel diff| <= 1e-11 on bounded
                             trajectories (tests/test_gpu_parity.py states the tolerance).
                             DOMAIN: the two-layer arithmetic of this mode (two-layer, coupled) folds the heat
                             capacities into its coefficients and requires FINITE 1/Cs and eta/Cd.  Outside that
                             domain -- a subnormal Cs or Cd, which no physical parameter set has -- a member the
                             reference keeps finite (at rest under a zero forcing, 0/Cs = 0) may come out NaN
                             (inf * 0) from the first row on, with its status byte set; nothing guards the hot loop
                             against it.  The arithmetic itself -- every rounding, every member, inf and NaN, the
                             status bytes -- is held bit for bit to a host restatement (tests/test_gpu_fast_bits.py,
                             tests/host_fast.py, which lists exactly that class as its one exception against the
                             oracle's status).
                             RSCM_KIND_OCEAN_CARBON: the history convolution in O(T) -- the last 60 (2D-BERN:
                             120) monthly lags explicitly, the older ones through 21 decaying modes fitted to the
                             impulse response; within 2e-10 of EXACT (tests/test_gpu_ocean.py; the tiled
                             convolution with fused multiply-adds where the fit does not apply).
                             RSCM_KIND_UDEB: one refinement term of the column solve's row reciprocals instead
                             of two (1.4e-13 from the oracle instead of 5e-14; the same 1e-9 bar,
                             tests/test_gpu_udeb.py).
                             RSCM_KIND_COUPLED and RSCM_KIND_CARBON_CYCLE (ABI minor 2): the carbon box's RK4 step
                             in closed form -- its equation is linear over a model step, so the four stages
                             collapse to C += h phi(h/lifetime) (A - C/lifetime) -- with 1/lifetime =
                             exp(-alpha T)/tau (no division), the uptake integral from the concentration
                             increments, cumulative emissions in the reference's own association (bit-exact),
                             and the two-layer half as in the two-layer kind; within 1e-11 of the oracle on
                             bounded members (measured 3e-13; tests/test_gpu_parity.py).
                             The other kinds have one arithmetic.  */

typedef struct rscm_ens rscm_ens;

/* ---- library ------------------------------------------------------------------------------ */
RSCM_API int rscm_gpu_abi_version(void);
RSCM_API int rscm_gpu_abi_minor(void);  /* RSCM_GPU_ABI_MINOR the library was built with */
/* Thread-local text of the last error raised by any call on this thread ("" if none). */
RSCM_API const char* rscm_gpu_last_error(void);
RSCM_API int rscm_gpu_device_count(int32_t* out);
/* Free and total HBM of `device_id` in bytes (sizing an ensemble against the 288 GB of an
 * MI355X: docs in DESIGN.md give the bytes per member of each kind). */
RSCM_API int rscm_gpu_mem_info(int32_t device_id, uint64_t* free_bytes, uint64_t* total_bytes);

/* ---- lifecycle ---------------------------------------------------------------------------- */
/* time_bounds has n_times+1 entries (TimeAxis.bounds, timeseries.rs:66-77) and must increase
 * strictly; step n integrates over [bounds[n], bounds[n+1]]. */
RSCM_API int rscm_ens_create(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                    int32_t device_id, rscm_ens** out);
/* As rscm_ens_create, with flags.  RSCM_FLAG_NO_SERIES (two-layer kind): keep only the initial
 * row of every state series -- for likelihood-only work through rscm_ens_run_loglik, where no
 * time series is ever written to HBM (12 GB per 1e6 members otherwise). */
#define RSCM_FLAG_NO_SERIES 1u
/* RSCM_FLAG_NOISE_PARAMS (ABI minor 15; rscm_ens_create_ex with RSCM_KIND_TWO_LAYER, and rscm_ens_create_mix): the handle gets the two
 * parameter rows RSCM_TL_P_NOISE_SIGMA(K) and RSCM_TL_P_NOISE_PHI(K) that rscm_ens_set_forcing_noise_members reads (described there).
 * RSCM_ERR_INVALID with any other kind, and together with RSCM_FLAG_NO_SERIES or RSCM_FLAG_WINDOWED: the noise needs stored series, so
 * the rows could never be read. */
#define RSCM_FLAG_NOISE_PARAMS 4u
RSCM_API int rscm_ens_create_ex(int32_t kind, int64_t n_members, int32_t n_times,
                                const double* time_bounds, int32_t device_id, uint32_t flags,
                                rscm_ens** out);
/* RSCM_FLAG_WINDOWED (any kind): keep only a sliding window of `window_rows` rows of every series
 * -- enough for what a step and its linked consumers read (indices n and n+1, plus the rows a
 * chemistry kind looks back at) -- instead of all n_times rows, and, if out_stride > 0, every
 * out_stride-th row (t = 0, out_stride, 2 out_stride, ...) of the `out_vars` (n_out_vars < 0: every stored
 * variable) in an output store.  This is what lets a graph of linked ensembles run a long axis: 36
 * series x 9001 monthly points are 2.6 MB per member stored whole, 4.6 KB in a 16-row window plus 216 KB
 * of annual outputs.  Semantics are unchanged: outputs of step n are written at index n+1, consumers
 * read n or n+1 (state/windows.rs:229-234), rows never written read as NaN.  A windowed handle is stepped
 * in ranges shorter than its window (lock-step graphs: one step per launch); rscm_ens_get_series,
 * rscm_ens_loglik and rscm_ens_summary serve the rows that are resident (output store or window) and
 * fail with RSCM_ERR_STATE for the others; rscm_ens_rewind puts the initial rows back.
 * window_rows >= 4 and >= 2 x (look-back + 1); window_rows >= n_times gives plain full storage. */
#define RSCM_FLAG_WINDOWED 2u
RSCM_API int rscm_ens_create_windowed(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                                      int32_t device_id, uint32_t flags, int32_t window_rows, int32_t out_stride,
                                      int32_t n_out_vars, const int32_t* out_vars, rscm_ens** out);
/* A two-layer MIX handle (ABI minor 12): an ensemble whose members differ in their FORCING as well as in the six model parameters.
 * The shared input block is [n_scen][K][n_times], K = n_components forcing components per scenario (rscm_ens_set_forcing takes it in
 * the layout of the multi-input kinds; scenario_of_member and `source` keep their meaning), and member i in scenario s is forced at
 * model index n by
 *     F = S[s][0][n] * c_0[i];   F = F + S[s][k][n] * c_k[i]   for k = 1 .. K-1, in that order
 * -- IEEE f64 multiplies and adds, each rounded on its own (no FMA), in BOTH arithmetic modes: RSCM_MODE_FAST changes what happens
 * to F afterwards, not how F is formed.  NaN and Inf propagate and no contributor is skipped: this is an exogenous series formed per
 * member (what a factory closure that scales exogenous series does in the reference's ModelRunner), NOT the schema aggregate of
 * RSCM_KIND_AGGREGATE, which skips NaN contributors.
 * The coefficients c_k are parameter rows RSCM_TL_P_COEFF0 + k of the handle: rscm_ens_n_params reports 6 + K, and every call that
 * moves parameter rows (rscm_ens_set_params / _aos, rscm_ens_get_params, rscm_ens_params_devptr, rscm_ens_sample_lhs with 6 + K bounds,
 * rscm_ens_sample_lhs_priors with 6 + K priors,
 * the samplers' param_rows, rscm_ens_gather_members) carries them.  rscm_ens_n_inputs reports K.
 * kind must be RSCM_KIND_TWO_LAYER; flags 0, RSCM_FLAG_NO_SERIES or RSCM_FLAG_NOISE_PARAMS (no windowed storage, and not the two
 * together); n_components in [1, RSCM_TL_MAX_COMPONENTS];
 * anything else is RSCM_ERR_INVALID.  A mix handle runs on its own: rscm_ens_link_input onto it, rscm_ens_run_lockstep and
 * rscm_sampler_create_graph with it, and rscm_ens_gather_members between handles of different component counts return
 * RSCM_ERR_INVALID (rscm_sampler_create takes it as the one evaluator). */
RSCM_API int rscm_ens_create_mix(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds, int32_t device_id,
                                 uint32_t flags, int32_t n_components, rscm_ens** out);
RSCM_API int rscm_ens_destroy(rscm_ens* h);

RSCM_API int rscm_ens_n_params(const rscm_ens* h, int32_t* out);
RSCM_API int rscm_ens_n_vars(const rscm_ens* h, int32_t* out);
/* Rows per scenario of the shared input block (variable 0): 1 for the first three kinds, K for a mix handle. */
RSCM_API int rscm_ens_n_inputs(const rscm_ens* h, int32_t* out);
/* K of a handle made by rscm_ens_create_mix, 0 for every other handle (a plain two-layer handle and a mix handle with K = 1 both
 * report one input row). */
RSCM_API int rscm_ens_n_forcing_components(const rscm_ens* h, int32_t* out);
RSCM_API int rscm_ens_n_members(const rscm_ens* h, int64_t* out);
RSCM_API int rscm_ens_n_times(const rscm_ens* h, int32_t* out);

/* ---- configuration ------------------------------------------------------------------------ */
RSCM_API int rscm_ens_set_mode(rscm_ens* h, int32_t mode);
RSCM_API int rscm_ens_set_step_size(rscm_ens* h, int32_t component, double step);
/* [P][N] structure-of-arrays. */
RSCM_API int rscm_ens_set_params(rscm_ens* h, const double* soa);
/* [N][P] row-major, the shape ModelRunner::run_batch receives (&[Vec<f64>]). */
RSCM_API int rscm_ens_set_params_aos(rscm_ens* h, const double* aos);
/* Shared input series already on the model axis: series[n_scen][n_times]
 * (kinds with several inputs -- RSCM_KIND_GHG_FORCING and the three after it -- take the block
 * series[n_scen][n_inputs][n_times], see RSCM_GH_VAR_CONC);
 * scenario_of_member[N] or NULL (all members use scenario 0). */
RSCM_API int rscm_ens_set_forcing(rscm_ens* h, int32_t var_id, int32_t n_scen, const double* series,
                         const int32_t* scenario_of_member, int32_t source);
/* Forcing noise (ABI minor 13): internal variability of a two-layer ensemble as white noise in the heat flux into the upper layer
 * (Hasselmann).  With noise on, member i of the handle reads forcing-axis index t -- the index actually read, n + the offset of
 * `source`, so `source` keeps its meaning -- and is forced there by
 *     F' = F + sigma * z(seed, g, t),        g = member_offset + i, i counted in the whole handle,
 * the product and the sum each rounded on its own (no FMA) in BOTH arithmetic modes.  F is the scenario value, or for a mix handle
 * (rscm_ens_create_mix) the mix sum formed first.  NaN and Inf propagate.  The arithmetic is done whenever noise is on, sigma == 0
 * included (F + 0 * z: a forcing of -0.0 becomes +0.0 where z > 0); off is rscm_ens_clear_forcing_noise.
 * z is a standard normal deviate that is a pure function of (seed, g, t) -- white in t, independent between members, no state: chunked
 * runs, the cut of a large run into member blocks, rscm_ens_rewind, checkpoints and rscm_ens_gather_members see the same noise by
 * construction, and nothing is stored for it.  Its definition, every step exact or a single IEEE f64 operation (a host restates it
 * with the same bits: tests/host_forcing_noise.py):
 *   block    philox4x32_10 with counter {lo32(g), hi32(g), t >> 1, RSCM_NOISE_STREAM_TAG} and key {lo32(seed), hi32(seed)};
 *            even t takes words (0,1) as (lo,hi), odd t words (2,3)
 *   uniform  k = ((hi << 32) | lo) >> 12 (52 bits);  u = (double)(2k + 1) * 2^-53, exact, in (0,1), symmetric about 1/2;  q = u - 0.5
 *   deviate  Wichura's AS241 PPND16 with its published constants, numerators and denominators of degree 7 in Horner form
 *            (((c7 r + c6) r + c5) ...):
 *              |q| <= 0.425:  r = 0.180625 - q*q;  z = (A(r) * q) / B(r)
 *              otherwise      p = q < 0 ? u : 1.0 - u (exact);  r = sqrt(-ln(p));
 *                             r <= 5: r -= 1.6, z = C(r) / D(r);  else r -= 5, z = E(r) / F(r);  z negated if q < 0
 *   ln(p)    for p in [2^-53, 0.075], in + - * / only: p = m 2^e by bits, m in [1,2); if m > 1.4142135623730951 then m *= 0.5, e += 1;
 *            s = (m - 1)/(m + 1);  w = s*s;  P = 1/25, then P = P*w + 1/(2j+1) for j = 11 .. 1 (each constant the f64 nearest the
 *            fraction);  s2 = s + s;  ln(p) = e * 0.6931471805599453 + (s2 + s2*(w*P))
 * (k = 0 gives -8.2095..., k = 2^52 - 1 gives +8.2095...: |z| is bounded.)
 * An option of a RSCM_KIND_TWO_LAYER handle, not a kind.  RSCM_ERR_INVALID: sigma negative or not finite; member_offset < 0 (a shard
 * passes the global index of its first member); another kind; a windowed or RSCM_FLAG_NO_SERIES handle; a handle with a linked input.
 * A handle with noise runs on its own: rscm_ens_link_input onto it, rscm_ens_run_lockstep, rscm_sampler_create* with it and the fused
 * rscm_ens_run_loglik* return RSCM_ERR_INVALID (the likelihood of one noise realisation per walker index is not a target the stretch
 * move samples).  rscm_ens_run* followed by the stored rscm_ens_loglik* is how a noisy ensemble is weighted, resampled and branched.
 * rscm_ens_gather_members leaves the destination's setting alone: like the forcing, the noise belongs to dst -- give dst a seed or an
 * offset of its own and the copies of one ancestor diverge. */
#define RSCM_NOISE_STREAM_TAG 0x4E5Au /* "NZ" */
RSCM_API int rscm_ens_set_forcing_noise(rscm_ens* h, uint64_t seed, double sigma, int64_t member_offset);
RSCM_API int rscm_ens_clear_forcing_noise(rscm_ens* h);
/* The setting: *on 1 or 0, and the three numbers (0 when off).  Any pointer may be NULL. */
RSCM_API int rscm_ens_forcing_noise(const rscm_ens* h, int32_t* on, uint64_t* seed, double* sigma, int64_t* member_offset);
/* The term itself: out[(t - t_begin) * N + i] = sigma * z(seed, member_offset + i, t) for t in [t_begin, t_end) within [0, n_times]
 * (with red noise, below: e_t, formed from index 0 on);
 * `out` is host memory, or with on_device != 0 device memory filled on the handle's stream.  RSCM_ERR_STATE without noise. */
RSCM_API int rscm_ens_forcing_noise_rows(rscm_ens* h, int32_t t_begin, int32_t t_end, double* out, int32_t on_device);
/* Red forcing noise (ABI minor 14): AR(1) internal variability.  The variability that observations carry is persistent; with
 * AR(1) noise on, member i of the handle has the global id g = member_offset + i and is forced at forcing-axis index t -- the index
 * actually read, n + the offset of `source`, as above -- by F'_t = F_t + e_t, F the scenario value or the mix sum formed first.  Every
 * operation below is rounded on its own, with no FMA, in BOTH arithmetic modes:
 *     c     = sqrt(1 - phi*phi)                 three roundings
 *     s_e   = sigma * c
 *     e_0   = sigma * z(seed, g, 0)             stationary start: Var e_t = sigma^2 at every t
 *     e_t   = (phi * e_{t-1}) + (s_e * z(seed, g, t))        t >= 1
 *     F'_t  = F_t + e_t
 * z is the deviate defined above: its stream tag, its Philox counter layout and the AS241 routine are the white noise's.  e does not
 * depend on F: a NaN or Inf in F propagates into F' at that index only and leaves the noise of later indices alone.  The persistence
 * is per forcing-axis index, not per year: on an uneven axis phi is the correlation between consecutive steps, whatever their length.
 * What is stored is a cache of a pure function.  e_t is a function of (seed, sigma, phi, g, t) alone; the handle keeps one device value
 * per member, every member's e at one forcing-axis index, and that index (-1: nothing cached).  A run over [step_begin, step_end) first
 * reads index t0 = step_begin + the offset of `source`: t0 == 0 starts from e_0; a cache that stands at t0 - 1 is loaded; otherwise
 * e_0 .. e_{t0-1} are formed again from the draws, O(t0) deviates per member, once.  The run leaves e at step_end - 1 + the offset, the
 * last index drawn.  The index is dropped before a run is issued and set after all of it -- every member block and chunk of steps --
 * was issued without error, and every setter of the noise drops it.  So rscm_ens_rewind, rscm_ens_set_initial, rscm_ens_set_time_index,
 * rscm_ens_set_state, a restored checkpoint (which carries sigma, seed, member_offset and phi, not the values) and
 * rscm_ens_gather_members into the handle need nothing of their own: the next run finds another index than it needs and forms e again,
 * to the same bits.  rscm_ens_gather_members leaves the destination's noise alone as above: a destination with red noise of its own
 * realises its own e from index 0, it does not inherit an ancestor's.
 * phi == 0 IS the white setting: the same kernels and bits as rscm_ens_set_forcing_noise (which sets phi = 0), nothing cached (the
 * formula's 0 * e term would change signed zeros at sigma == 0).  RSCM_ERR_INVALID: phi not finite or |phi| >= 1, and everything
 * rscm_ens_set_forcing_noise refuses.  What a noise handle is refused (linking, lock-step, the samplers, the fused likelihood) holds
 * unchanged, and rscm_ens_clear_forcing_noise clears phi and the cache with the rest. */
RSCM_API int rscm_ens_set_forcing_noise_ar1(rscm_ens* h, uint64_t seed, double sigma, double phi, int64_t member_offset);
/* *phi of the setting and *cached_index, the forcing-axis index the cache stands at; 0 and -1 when the noise is off or white.  Either
 * pointer may be NULL. */
RSCM_API int rscm_ens_forcing_noise_ar1(const rscm_ens* h, double* phi, int32_t* cached_index);
/* Per-member forcing noise (ABI minor 15): amplitude and persistence as parameter rows.  How much internal variability the system has,
 * and how persistent it is, is as uncertain as any model parameter.  A two-layer handle created with RSCM_FLAG_NOISE_PARAMS (plain, K = 0,
 * or mix with K components) carries member i's sigma_i in parameter row RSCM_TL_P_NOISE_SIGMA(K) = 6 + K and phi_i in row
 * RSCM_TL_P_NOISE_PHI(K) = 6 + K + 1: rscm_ens_n_params reports 6 + K + 2, and every call that moves parameter rows carries the two
 * rows like any other (rscm_ens_set_params / _aos, rscm_ens_get_params, rscm_ens_params_devptr, rscm_ens_sample_lhs with 6 + K + 2 bounds,
 * rscm_ens_sample_lhs_priors with as many priors,
 * rscm_ens_params_vector, rscm_ens_gather_members -- so the draws of a posterior inherit their ancestors' amplitude and persistence).
 * rscm_ens_gather_members between a handle with the rows and one without is RSCM_ERR_INVALID, like differing component counts.
 * With the per-member noise on, member i has the global id g = member_offset + i and is forced at forcing-axis index t by
 * F'_t = F_t + e_t, F the scenario value or the mix sum formed first, where
 *     c_i   = sqrt(1 - phi_i*phi_i)             three roundings
 *     s_i   = sigma_i * c_i
 *     e_0   = sigma_i * z(seed, g, 0)
 *     e_t   = (phi_i * e_{t-1}) + (s_i * z(seed, g, t))        t >= 1
 *     F'_t  = F_t + e_t
 * -- every operation an IEEE f64 operation rounded on its own, with no FMA, in BOTH arithmetic modes; z is the deviate defined above,
 * untouched.  This is the red formula, and it is used for every member, phi_i == 0 included: such a member gets the white VALUES
 * sigma_i * z, and its forcing differs from the white setting's only in the sign of a zero ((0 * e) + (sigma_i z) where sigma_i z is a
 * zero: -0.0 under the white setting can be +0.0 here).  With all rows uniform and phi != 0 the bits are those of
 * rscm_ens_set_forcing_noise_ar1 with the same numbers.
 * The rows are data (rscm_ens_sample_lhs and rscm_ens_sample_lhs_priors fill them on the device), so nothing validates them: what the formula gives is what is
 * defined, the rule for forcing ("NaN and Inf propagate") applied to these two rows.  A NaN or Inf in either row, or |phi_i| > 1 (the
 * square root of a negative number), gives that member NaN forcing: its states are NaN and bit 0 of its status is set.  |phi_i| == 1
 * gives s_i = 0 and a constant (phi_i = 1) or alternating (phi_i = -1) e.  A negative sigma_i mirrors the noise.  None of these touches
 * another member.
 * A handle with the flag and the noise OFF, or under rscm_ens_set_forcing_noise / _ar1, behaves exactly like one without the flag: the
 * same kernels, the same bits, the two rows inert, and it is accepted wherever an unflagged handle is (links, lock-step, the samplers,
 * the fused likelihood).
 * rscm_ens_set_forcing_noise_members turns the per-member noise on.  RSCM_ERR_INVALID on a handle without the flag, and for everything
 * rscm_ens_set_forcing_noise refuses (member_offset < 0, a linked input).  What a noise handle is refused holds unchanged (linking,
 * lock-step, the samplers, the fused rscm_ens_run_loglik*).  rscm_ens_clear_forcing_noise turns it off; the handle-wide setters
 * replace it and it replaces them.
 * THE CACHE.  Here e_t is a function of (seed, sigma_i, phi_i, g, t) with the rows AS THEY STAND AT LAUNCH, so the cache of the red
 * noise (one value per member and the index it stands at, above) is only valid while the rows are.  In this mode the cached index is
 * dropped by everything that can change a parameter row:
 *     rscm_ens_set_params, rscm_ens_set_params_aos, rscm_ens_sample_lhs, rscm_ens_sample_lhs_priors, rscm_ens_gather_members into the handle
 *     (a restored checkpoint sets the parameters, so it is among them),
 * and for good once rscm_ens_params_devptr has been handed out: the caller may then write the rows at any time, so such a handle never
 * trusts the cache across calls -- every run forms e again from index 0, and the index reads -1 after every run.  The chunks and
 * member blocks INSIDE one run still hand e over through the cache as they do for the handle-wide red noise. */
RSCM_API int rscm_ens_set_forcing_noise_members(rscm_ens* h, uint64_t seed, int64_t member_offset);
/* *per_member: 1 while rscm_ens_set_forcing_noise_members is in force, else 0.  *sigma_row and *phi_row: the two parameter rows of a
 * handle created with RSCM_FLAG_NOISE_PARAMS (whether the noise is on or not), -1 on any other handle.  Any pointer may be NULL.
 * In this mode rscm_ens_forcing_noise reports on, seed, member_offset and sigma = 0, rscm_ens_forcing_noise_ar1 reports phi = 0 and
 * the cached index, and rscm_ens_forcing_noise_rows returns e formed from the rows as they stand. */
RSCM_API int rscm_ens_forcing_noise_members(const rscm_ens* h, int32_t* per_member, int32_t* sigma_row, int32_t* phi_row);
/* Initial value(s) at time index 0 of a state variable: n_values == 1 (broadcast) or N.
 * Also rewinds the time index to 0. */
/* Linked input: row `input_row` of h's input block is read, member by member, from the stored series
 * `src_var` of another ensemble `src` (same n_members, n_times and device) instead of the shared
 * scenario table -- the edge of a component graph (ModelBuilder::build, builder.rs:487-518) kept on
 * the device.  `source` is the consumer's VariableSource for that variable: RSCM_SRC_EXOGENOUS reads
 * index n (also the reference's choice for a producer registered *after* the consumer: lagged
 * feedback), RSCM_SRC_UPSTREAM index n+1.  ClimateUDEB reads at_start / at_end (n and n+1) and the
 * aggregate kind always n+1; both ignore `source`.
 * Rows that are not linked keep coming from rscm_ens_set_forcing's block (which is only required if
 * such rows exist).  Both ensembles must run on the same stream (rscm_ens_set_stream), and a run
 * of h over [b, e) needs src to have been stepped to e - 1 + source first: for a chain without
 * feedback run the producers over the whole axis and then the consumers; with feedback step every
 * ensemble one step at a time in graph order (what Model::step does).  `src` must outlive the link:
 * rscm_ens_destroy(src) fails while links to it exist.  Not available for RSCM_KIND_COUPLED and
 * RSCM_KIND_HALOCARBON inputs, nor with RSCM_FLAG_NO_SERIES on either side. */
RSCM_API int rscm_ens_link_input(rscm_ens* h, int32_t input_row, rscm_ens* src, int32_t src_var, int32_t source);
/* The guard "src has been stepped far enough" can be switched off (enabled = 0) for callers that
 * reproduce the reference's execution order as it is: its breadth-first order is not a topological
 * one, so a component can run before the producer of a variable it reads at index n+1 and then
 * sees what the collection holds there -- NaN in a fresh model (builder.rs:772-780).  Default on. */
RSCM_API int rscm_ens_set_link_order_check(rscm_ens* h, int32_t enabled);
/* Row `input_row` reads the scenario table again. */
RSCM_API int rscm_ens_unlink_input(rscm_ens* h, int32_t input_row);

RSCM_API int rscm_ens_set_initial(rscm_ens* h, int32_t var_id, const double* values, int64_t n_values);
/* Checkpoint / resume (the reference serialises time_index + the whole collection,
 * crates/rscm-core/src/model/runtime.rs:270-282): a run can be resumed from
 * (time index k, row k of every state variable).  rscm_ens_set_state writes row `tidx` of a stored
 * series (1 value = broadcast, or N values); rscm_ens_set_time_index moves the stepper there. */
RSCM_API int rscm_ens_set_state(rscm_ens* h, int32_t var_id, int32_t tidx, const double* values,
                                int64_t n_values);
/* RSCM_KIND_UDEB and RSCM_KIND_OCEAN_CARBON keep the reference's internal ComponentState (ocean
 * columns, flux history) on the device: for them tidx must be 0 or the current index. */
RSCM_API int rscm_ens_set_time_index(rscm_ens* h, int32_t tidx);
/* The internal ComponentState of the kinds that have one -- what the reference serialises next to the
 * collection in a checkpoint (runtime.rs:270-282): RSCM_KIND_UDEB: ocean layer temperatures
 * [2][n_layers][N], the per-member scalars [11][N] and the temperature history rows 0..time_index;
 * RSCM_KIND_OCEAN_CARBON: the flux history of the time_index * 12 months so far, or of the last
 * max_history_months (+ a few) of them if that is fewer -- the convolution reads no further back, and the
 * device keeps the history as a ring of that length.  One flat block of
 * doubles whose length depends on the current time index (0 for every other kind).
 * rscm_ens_set_internal_state puts such a block back and moves the stepper to `time_index` (the
 * one it was taken at); the stored series rows are restored with rscm_ens_set_state. */
RSCM_API int rscm_ens_internal_state_size(rscm_ens* h, int64_t* n_doubles);
RSCM_API int rscm_ens_get_internal_state(rscm_ens* h, double* out);
RSCM_API int rscm_ens_set_internal_state(rscm_ens* h, const double* in, int64_t n_doubles, int32_t time_index);
/* Use an existing hipStream_t (as void*) for all launches and copies; NULL = own stream. */
RSCM_API int rscm_ens_set_stream(rscm_ens* h, void* hip_stream);
/* A non-blocking hipStream_t on `device_id` for callers without a HIP runtime of their own (linked
 * ensembles must share one stream); destroy it after the ensembles that use it. */
RSCM_API int rscm_gpu_stream_create(int32_t device_id, void** out_stream);
RSCM_API int rscm_gpu_stream_destroy(int32_t device_id, void* hip_stream);

/* ---- stepping (Model::step / run) --------------------------------------------------------- */
/* Execute steps n = step_begin .. step_end-1 (0 <= step_begin <= step_end <= n_times-1).
 * step_begin must equal the current time index (Model::step advances it by one).
 * Fails with RSCM_ERR_TIME_AXIS, before launching anything, if for the configured RK4 step
 * sizes any model step's end time would be missed by >= 5e-3 (ivp/mod.rs:90-102; the reference
 * panics inside solve()), and with RSCM_ERR_STATE if parameters, the shared input or a state's
 * initial value are missing (builder.rs:704-717 MissingInitialValue).
 * rscm_ens_run returns after the work has completed; rscm_ens_run_async only enqueues. */
RSCM_API int rscm_ens_run(rscm_ens* h, int32_t step_begin, int32_t step_end);
RSCM_API int rscm_ens_run_async(rscm_ens* h, int32_t step_begin, int32_t step_end);
/* Model::run over a graph of linked ensembles (runtime.rs:504-527): for every step n in
 * [step_begin, step_end) each handle, in the order given (the graph order), advances by that one
 * step -- n_handles asynchronous launches per step on the handles' common stream, without
 * returning to the caller in between.  Every handle must stand at step_begin; follow with
 * rscm_ens_sync on any of them.  If a launch is refused part-way (a state error of one handle), the
 * handles before it in the order have advanced one step further than those after it. */
RSCM_API int rscm_ens_run_lockstep(rscm_ens* const* handles, int32_t n_handles, int32_t step_begin, int32_t step_end);
/* rscm_ens_run_lockstep issues one launch per step for every run of consecutive light components (chemistry,
 * forcing formulas, budgets, aggregates, grid transforms, the RK4 box models) instead of one per component:
 * each thread runs the components' per-member bodies in graph order -- every graph edge is per member, so this
 * is the same computation, bit for bit.  ClimateUDEB, OceanCarbon and HalocarbonChemistry keep their own
 * launches.  A graph made of light components only runs ALL its steps in one launch, and between the steps
 * every component keeps its varying parameters, its state and what its consumers read in thread-private LDS
 * slots instead of reading them back from HBM (the series are still written every step).
 * Where the graph order ends a step with light components and begins the next with light components (the MAGICC graph:
 * [8 light] ClimateUDEB OceanCarbon [3 light]), the two runs are consecutive launches and go out as ONE when they fit a
 * table of twelve ops: three launches per model step.  Inside a call of two steps or more the handles of the first run
 * therefore stand one step ahead of the others between the launches -- exactly where they would stand after their own
 * launch of the next step; at the end of the call every handle stands at step_end.
 * (A/B switches and launch counters for tests: include/rscm_gpu_internal.h.) */
RSCM_API int rscm_ens_sync(rscm_ens* h);
RSCM_API int rscm_ens_time_index(const rscm_ens* h, int32_t* out);
/* Rewind to time index 0 keeping parameters, forcing and initial values (outputs are
 * overwritten by the next run). */
RSCM_API int rscm_ens_rewind(rscm_ens* h);
/* Back to a fresh collection: time index 0 and every stored row after index 0 NaN again
 * (builder.rs:772-780), index 0 (initial values) kept.  rscm_ens_rewind alone leaves the rows of the
 * previous run in place, which nothing reads before rewriting them -- except a linked consumer that
 * runs ahead of its producer (rscm_ens_set_link_order_check). */
RSCM_API int rscm_ens_clear_series(rscm_ens* h);
/* Every stored row after `tidx` NaN again, the time index untouched: what a collection restored from
 * a checkpoint taken at `tidx` holds there (runtime.rs:270-282 serialises the collection as it was).
 * Needed when an already advanced model is rolled back and some component reads index n+1 of a
 * producer that runs after it (see rscm_ens_set_link_order_check). */
RSCM_API int rscm_ens_clear_rows_after(rscm_ens* h, int32_t tidx);
/* Device time of the most recent rscm_ens_run* launch sequence, from HIP events recorded on
 * the launch stream (valid after a sync). */
RSCM_API int rscm_ens_last_run_ms(rscm_ens* h, float* out_ms);
/* How the most recent rscm_ens_run* was cut into launches (ABI minor 3).  A whole-axis run of the two-layer or the coupled kind over more
 * members than the chip holds wavefronts at one per SIMD, and over at least ~190 model steps, is issued as TWO member blocks on two
 * streams (the caller's and one of the handle's own, forked and joined with events), each in chunks of ~64 model steps: the same
 * kernels on the same operands -- the same bits -- and the wavefronts even out over the SIMDs (1e5 members x 750 years: 2.7 -> 2.3 ms).
 * An unlinked whole-axis ClimateUDEB run over more than 65 536 members is cut the same way (two HALVES, chunks of ~96 steps; each
 * chunk reloads and stores the block's ocean columns and scalars, which is how rscm_ens_run in pieces resumes anyway; both halves
 * take the kernel variant chosen for the whole ensemble's size, so one run is one kernel).
 * member_blocks x step_chunks launches in all; 1 x 1 otherwise.  To the caller the run is one asynchronous operation on its stream
 * either way: the helper stream and the fork / join events are the handle's own.  Environment RSCM_SPLIT_RUNS=0 turns the cut off. */
RSCM_API int rscm_ens_last_run_plan(rscm_ens* h, int32_t* member_blocks, int32_t* step_chunks);

/* ---- outputs ------------------------------------------------------------------------------ */
/* Copy series[var][t][m] for t in {t_begin, t_begin+t_stride, ...} < t_end and
 * m in [m_begin, m_end) into out, laid out [n_t][m_end-m_begin]. */
RSCM_API int rscm_ens_get_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end,
                        int32_t t_stride, int64_t m_begin, int64_t m_end, double* out);
/* Device pointer of series[var] ([T][N] contiguous) for zero-copy consumers. */
RSCM_API int rscm_ens_series_devptr(rscm_ens* h, int32_t var_id, void** out);
/* Device pointer of the parameter block ([P][N]) for callers that fill it on the device (the device sampler's
 * proposal kernel, a torch view).  The pointer stays valid until rscm_ens_destroy and may be written at any
 * time between launches: from this call on the handle never again treats a parameter row as uniform over the
 * members (the kernels' shortcut for rows rscm_ens_set_params found to hold one value), whatever later
 * rscm_ens_set_params calls upload. */
RSCM_API int rscm_ens_params_devptr(rscm_ens* h, void** out);
/* Per-member status after the last run: bit0 = a state variable is non-finite at the current
 * time index (the reference's failed-member case: NaN/Inf -> Err -> -inf log-posterior). */
RSCM_API int rscm_ens_status(rscm_ens* h, uint8_t* out);

/* Gaussian log-likelihood per member against observations given by (variable id, time index,
 * value, sigma); observations must be grouped by variable.  Non-finite model value -> -inf.
 * out is a host buffer [N]. */
RSCM_API int rscm_ens_loglik(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                    const double* obs_value, const double* obs_sigma, int32_t normalize,
                    double* out);
/* As rscm_ens_loglik, the result left on the device: *out_dev is the device address of the [N] doubles
 * (owned by the handle, valid until its next likelihood call; the work has completed on return).  For
 * callers that reduce or all-gather the per-member values without a host round trip (RCCL all-gather
 * of 8 B per member in the sharded calibration loop). */
RSCM_API int rscm_ens_loglik_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                                    const double* obs_value, const double* obs_sigma, int32_t normalize,
                                    void** out_dev);
/* Device address of the [N] status bytes rscm_ens_status copies out. */
RSCM_API int rscm_ens_status_devptr(rscm_ens* h, void** out);
/* Fused Model::run + GaussianLikelihood for the calibration loop (two-layer kind): steps every
 * member from time index 0 to the end of the axis and accumulates ln L on the fly, writing no
 * series (the time index stays 0, status is updated).  Same value as rscm_ens_run followed by
 * rscm_ens_loglik, bit for bit.  Observations grouped by variable with ascending time indices
 * inside a group. */
RSCM_API int rscm_ens_run_loglik(rscm_ens* h, int32_t n_obs, const int32_t* obs_var,
                                 const int32_t* obs_tidx, const double* obs_value,
                                 const double* obs_sigma, int32_t normalize, double* out);
/* rscm_ens_run_loglik with the result left on the device (see rscm_ens_loglik_device). */
RSCM_API int rscm_ens_run_loglik_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var,
                                        const int32_t* obs_tidx, const double* obs_value,
                                        const double* obs_sigma, int32_t normalize, void** out_dev);
/* ---- likelihoods against anomalies from a reference period (ABI minor 9) ------------------------
 * Observed warming is published as an anomaly from a reference period (relative to 1850-1900); a member's own mean over that
 * period differs from member to member, so the shift belongs to the model side.  Reference periods travel as parallel arrays, one
 * entry per variable that has one (a variable at most once; one without an observation: RSCM_ERR_INVALID): the rows ref_begin[e],
 * ref_begin[e] + ref_stride[e], ... < ref_end[e] of variable ref_var[e] -- the row convention of rscm_ens_set_baseline.  For member
 * i and such a variable
 *     b[i] = the sum of the member's values over the reference rows in row order (f64, no FMA) divided by the row count:
 *            exactly the bits rscm_ens_set_baseline produces,
 *     model value at an observation = x[i](t_obs) - b[i], one IEEE subtraction: the bits of RSCM_SELECT_ANOMALY,
 * and from there on the expressions and summation order of rscm_ens_loglik.  A variable without a period is scored as by
 * rscm_ens_loglik; two variables may have different periods; a member whose b is not finite is a failed member (-inf).  A reference
 * row beyond the current time index gives -inf for every member and one that is not resident RSCM_ERR_STATE, both as for an
 * observation row.  The handle's own baseline (rscm_ens_set_baseline) is neither read nor changed.  With n_ref == 0 each call
 * is its counterpart without _ref.
 *
 * rscm_ens_loglik_ref / _device: the stored series, any kind and any resident storage layout. */
RSCM_API int rscm_ens_loglik_ref(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                                 const double* obs_value, const double* obs_sigma, int32_t normalize, int32_t n_ref,
                                 const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end,
                                 const int32_t* ref_stride, double* out);
RSCM_API int rscm_ens_loglik_ref_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                                        const double* obs_value, const double* obs_sigma, int32_t normalize, int32_t n_ref,
                                        const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end,
                                        const int32_t* ref_stride, void** out_dev);
/* The fused two-layer run + likelihood with reference periods, under the restrictions of rscm_ens_run_loglik: the value of
 * rscm_ens_run followed by rscm_ens_loglik_ref, bit for bit, in both arithmetic modes; no series row is written, the time index
 * stays 0.  Each thread sums its member's reference rows while it steps; the model values of the observations at rows up to a
 * period's last wait in a handle-owned scratch (8 bytes per member each, written once and read once) until that row has formed b. */
RSCM_API int rscm_ens_run_loglik_ref(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                                     const double* obs_value, const double* obs_sigma, int32_t normalize, int32_t n_ref,
                                     const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end,
                                     const int32_t* ref_stride, double* out);
RSCM_API int rscm_ens_run_loglik_ref_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                                            const double* obs_value, const double* obs_sigma, int32_t normalize, int32_t n_ref,
                                            const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end,
                                            const int32_t* ref_stride, void** out_dev);
/* ---- device stretch-move sampler ------------------------------------------------------------
 * EnsembleSampler::run (crates/rscm-calibrate/src/sampler/ensemble.rs:496-547) with StretchMove
 * (sampler/moves.rs:40-125) and the ParameterSet prior kept on the GPU: per half-ensemble update
 * a proposal kernel writes y = c + z (x - c), z = ((a-1)u + 1)^2 / a, straight into the evaluating
 * ensemble's parameter block, the fused run+likelihood kernel scores it and an accept kernel
 * applies q = z^(d-1) p(y)/p(x).  Random numbers are counter-based (Philox, keyed by `seed`), so a
 * run is reproducible; the reference draws from thread_rng, so only distributions compare.
 *
 * `evaluator`: an ensemble of n_walkers/2 members with parameters (rscm_ens_set_params, once: it
 * configures the structural rows of kinds that have them), forcing and initial values set; it must
 * outlive the sampler and is used exclusively by it while iterating.  A two-layer evaluator whose
 * observations have ascending time indices inside each variable group is scored by the fused
 * run+likelihood kernel (RSCM_FLAG_NO_SERIES is enough), whose launches end at the last observed time index
 * (later steps cannot change ln L; the evaluator's status then refers to that index); any other kind, or observation order,
 * is run through rscm_ens_run_async and scored from its stored series.  Sampled dimension d drives parameter row param_rows[d]; the other rows hold
 * base_params[P].  prior_kind: 0 = Uniform(low = a, high = b), 1 = Normal(mean = a, std = b),
 * 2 = LogNormal(mu = a, sigma = b); prior_low / prior_high truncate dimension d to [low, high]
 * like the reference's Bound wrapper (both NULL, or -inf / +inf entries: no truncation)
 * (distribution.rs).  Observations as for rscm_ens_run_loglik. */
typedef struct rscm_sampler rscm_sampler;
RSCM_API int rscm_sampler_create(rscm_ens* evaluator, int32_t n_walkers, int32_t n_dims,
                                 const int32_t* param_rows, const double* base_params,
                                 const int32_t* prior_kind, const double* prior_a, const double* prior_b,
                                 const double* prior_low, const double* prior_high,
                                 int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                                 const double* obs_value, const double* obs_sigma, int32_t normalize,
                                 double stretch_a, uint64_t seed, rscm_sampler** out);
/* The same sampler sharded over n_ranks processes (one per GPU): every rank holds a replica of the walker
 * positions and owns the half-walkers [rank * n, (rank + 1) * n), n = n_walkers / 2 / n_ranks, of BOTH
 * halves; `evaluator` has n members.  Per half-step a rank proposes, evaluates and accepts its block and
 * packs the block's new positions and log probabilities ([n_dims + 1][n] doubles); the ranks all-gather
 * the blocks (RCCL over xGMI: 2.8 MB in all at 1e5 walkers x 6 dimensions) and unpack them into their
 * replicas.  Proposals, complementary walkers and acceptance draws are keyed on the global walker index,
 * so the chain is the same for every n_ranks, bit for bit.  The driver loop
 * (rscm_amd.calibrate.DeviceEnsembleSampler):
 *     rscm_sampler_set_positions(s, pos)                    -- the same positions on every rank
 *     for half in 0, 1: rscm_sampler_half_step(s, half, 1); all-gather; rscm_sampler_apply_exchange(s, half)
 *     per iteration: rscm_sampler_begin_iteration(s);
 *         for half in 0, 1: rscm_sampler_half_step(s, half, 0); all-gather; rscm_sampler_apply_exchange(s, half)
 * with the all-gather from *send into *recv of rscm_sampler_exchange_buffers (device memory, on the
 * evaluator's stream: call rscm_sampler_sync first unless the collective runs on that stream).
 * rscm_sampler_get then returns all positions and log probabilities on every rank and this rank's
 * acceptance counters (zero for walkers of other ranks).  n_groups must be 1. */
RSCM_API int rscm_sampler_create_sharded(rscm_ens* evaluator, int32_t n_walkers, int32_t n_dims,
                                         const int32_t* param_rows, const double* base_params,
                                         const int32_t* prior_kind, const double* prior_a, const double* prior_b,
                                         const double* prior_low, const double* prior_high,
                                         int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                                         const double* obs_value, const double* obs_sigma, int32_t normalize,
                                         double stretch_a, uint64_t seed, int32_t rank, int32_t n_ranks,
                                         rscm_sampler** out);
RSCM_API int rscm_sampler_begin_iteration(rscm_sampler* s);
/* One half-ensemble update of this rank's block, enqueued: propose (identity != 0: score the walkers where
 * they stand), evaluate, accept, pack.  Also usable on an unsharded sampler (no pack). */
RSCM_API int rscm_sampler_half_step(rscm_sampler* s, int32_t half, int32_t identity);
RSCM_API int rscm_sampler_exchange_buffers(rscm_sampler* s, void** send, void** recv, int64_t* doubles_per_rank);
RSCM_API int rscm_sampler_apply_exchange(rscm_sampler* s, int32_t half);
RSCM_API int rscm_sampler_sync(rscm_sampler* s);
/* The same sampler over a GRAPH of linked ensembles as the evaluator -- EnsembleSampler<R: ModelRunner, L> is generic over the
 * runner (sampler/ensemble.rs:86-106,143-177); here the runner is any component graph stepped by rscm_ens_run_lockstep.
 * handles[0 .. n_handles) in graph order, n_walkers / 2 / n_ranks members each, whole series stored, one stream.  Sampled
 * dimension d is parameter row param_rows[d] of handles[param_owner[d]] (every other parameter keeps what rscm_ens_set_params
 * gave it); observation j is variable obs_var[j] of handles[obs_owner[j]] at time index obs_tidx[j].  Every half-step: the
 * handles are rewound (clear_between_runs != 0: their stored rows NaN again, for graphs in which a consumer runs ahead of its
 * producer, rscm_ens_set_link_order_check), the proposal kernel writes each proposed value into its owner's parameter block,
 * the graph is stepped to the last observed index -- later steps cannot change ln L -- and the likelihood kernel sums over the
 * observation rows where their owners store them: no host round trip per sweep.  Everything else (priors, groups, sharding,
 * driving calls, reproducibility) as for rscm_sampler_create_sharded. */
RSCM_API int rscm_sampler_create_graph(rscm_ens* const* handles, int32_t n_handles, int32_t clear_between_runs, int32_t n_walkers,
                              int32_t n_dims, const int32_t* param_owner, const int32_t* param_rows, const int32_t* prior_kind,
                              const double* prior_a, const double* prior_b, const double* prior_low, const double* prior_high,
                              int32_t n_obs, const int32_t* obs_owner, const int32_t* obs_var, const int32_t* obs_tidx,
                              const double* obs_value, const double* obs_sigma, int32_t normalize, double stretch_a, uint64_t seed,
                              int32_t rank, int32_t n_ranks, rscm_sampler** out);
RSCM_API int rscm_sampler_destroy(rscm_sampler* s);
/* Split the walkers into n_groups independent ensembles of n_walkers / n_groups walkers each
 * (consecutive blocks of the walker index): every group is a sampler of its own -- its own two
 * halves, complementary walkers drawn from itself only -- and all groups advance in the same
 * launches.  This is how ensembles of the reference's usual size (tens of walkers) fill a GPU:
 * thousands of them side by side, e.g. for an R-hat across independent runs.  Default 1. */
RSCM_API int rscm_sampler_set_groups(rscm_sampler* s, int32_t n_groups);
/* Reference periods for the sampler's observations (see rscm_ens_loglik_ref), after any of the three rscm_sampler_create* calls and
 * before rscm_sampler_set_positions (RSCM_ERR_STATE once positions are set).  ref_owner: the handle index of each period's variable
 * for a graph sampler, NULL otherwise.  A fused evaluator's launches, and a graph's lock-step runs, then end at the later of the
 * last observed index and the last reference row.  Every rank of a sharded sampler is given the same periods.  n_ref == 0 removes
 * them. */
RSCM_API int rscm_sampler_set_reference(rscm_sampler* s, int32_t n_ref, const int32_t* ref_owner, const int32_t* ref_var,
                                        const int32_t* ref_begin, const int32_t* ref_end, const int32_t* ref_stride);
/* positions[n_walkers][n_dims] row-major (the Chain layout); scores every walker and zeroes the
 * acceptance counters. */
RSCM_API int rscm_sampler_set_positions(rscm_sampler* s, const double* positions);
/* n_iterations full sweeps (first half against the second, then the second against the updated
 * first); synchronous.  rscm_sampler_last_ms reports the device time of the last call. */
RSCM_API int rscm_sampler_iterate(rscm_sampler* s, int32_t n_iterations);
RSCM_API int rscm_sampler_last_ms(const rscm_sampler* s, float* out);
/* Any output may be NULL.  positions[n_walkers][n_dims], log_prob[n_walkers] (log prior + log
 * likelihood, -inf for failed members), per-walker acceptance counters. */
RSCM_API int rscm_sampler_get(rscm_sampler* s, double* positions, double* log_prob, int64_t* n_accepted,
                              int64_t* n_proposed);

/* Ensemble summary of one variable at one time index over finite members:
 * out[0]=count_finite, out[1]=sum, out[2]=min, out[3]=max (wavefront + block reductions). */
RSCM_API int rscm_ens_summary(rscm_ens* h, int32_t var_id, int32_t tidx, double out[4]);
/* The same four numbers for every time index in [t_begin, t_end) in two launches:
 * out[(t_end - t_begin)][4].  Each row carries the bits rscm_ens_summary returns for it. */
RSCM_API int rscm_ens_summary_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, double* out);
/* Ensemble quantiles of a stored variable at every time index of [t_begin, t_end): the plume (median,
 * 5-95 % band ...) reduced on the device.  Definition: numpy.nanquantile(row, q, method="linear") --
 * NaN members left out, virtual index (n - 1) q, numpy's interpolation -- so the results carry numpy's
 * bits.  out[(t - t_begin)][n_q]; count[(t - t_begin)] (or NULL) = members that are not NaN.  Rows beyond
 * the current time index: count 0, quantiles NaN.  An extension: the reference has no ensemble
 * statistics; q in [0, 1], any n_q >= 1.  It is rscm_ens_quantile_rows with stride 1 on a handle that stores
 * whole series (any other: RSCM_ERR_STATE), run over blocks of the list where n_q > 128: the same radix select,
 * the same bits.  Where a quantile lands on a zero, -0.0 orders before +0.0, so the sign is a function of the
 * member set and not of where the members sit. */
RSCM_API int rscm_ens_quantile_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t n_q,
                                      const double* q, double* out, double* count);

/* ---- exact quantiles of any storage layout and of sharded ensembles (ABI minor 6) ----------- */
/* The quantiles rscm_ens_quantile_series defines (numpy.nanquantile, method "linear", the same bits) of stored variable var_id
 * over the rows t_begin, t_begin + t_stride, ... < t_end, read wherever each row is resident: full storage, the window of a
 * RSCM_FLAG_WINDOWED handle or its output store.  No sort and no member-sized scratch: a radix select of eight passes, each
 * one histogram of 256 int64 counts per row and target (two targets per quantile).
 * out[rows][n_q]; count[rows] (or NULL) = members that are not NaN.  Rows beyond the current time index: count 0, quantiles
 * NaN.  A row that is not resident (slid out of the window and not in the output store), or any row but 0 of a
 * RSCM_FLAG_NO_SERIES handle: RSCM_ERR_STATE.  q in [0, 1], 1 <= n_q <= 128. */
RSCM_API int rscm_ens_quantile_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q,
                                    const double* q, double* out, double* count);
/* The same select in stages, so that a host holding one shard of an ensemble per handle (one rank per GPU, or several
 * handles in one process) can sum the handles' histograms between the passes -- the quantiles of the WHOLE ensemble with
 * int64 SUM as the only collective, so the result carries the same bits at any number of ranks:
 *
 *     rscm_ens_select_begin(h, var, t0, t1, stride, n_q, q);
 *     for (;;) {
 *         rscm_ens_select_pass(h, &done, &buf, &n);     // this handle's counts; the stream is synchronised on return
 *         if (done) break;
 *         SUM-all-reduce buf[n] (int64, in place, device memory) over all handles; wait for it to complete
 *         rscm_ens_select_commit(h);                    // consumes the reduced buffer
 *     }
 *     rscm_ens_select_result(h, out, count);            // every handle returns the same numbers
 *     rscm_ens_select_end(h);
 *
 * Every handle must be given the same q, the same row range and stride and be at the same time index; anything else is a
 * caller error (the buffers then differ in size or meaning and the result is undefined).  With RSCM_SELECT_GROUPED every handle
 * must also carry the same n_groups (the group ids themselves are each handle's own members').  The handle must not run, and its
 * rows must not be written, between begin and the last pass.  One staged select per handle at a time: begin on a handle
 * with one in flight is RSCM_ERR_STATE; rscm_ens_destroy ends one in flight.  The buffer belongs to the handle and stays
 * valid until the next pass or end.  Passes: eight while any row of the range is computed, none otherwise. */
RSCM_API int rscm_ens_select_begin(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q,
                                   const double* q);
RSCM_API int rscm_ens_select_pass(rscm_ens* h, int32_t* done, int64_t** buf_dev, int64_t* n);
RSCM_API int rscm_ens_select_commit(rscm_ens* h);
RSCM_API int rscm_ens_select_result(rscm_ens* h, double* out, double* count);
RSCM_API int rscm_ens_select_end(rscm_ens* h);

/* ---- likelihood-weighted quantiles (ABI minor 7) ------------------------------------------------ */
/* Member weights: int64, one per member, >= 0, summing over the handle's N members to at most 2^53; handle-owned, kept across
 * rscm_ens_run and rscm_ens_rewind, freed by rscm_ens_destroy.  w (host, or device memory on the handle's device with
 * on_device != 0) holds N values; a negative one, or a total above 2^53, is RSCM_ERR_INVALID and leaves the weights set
 * before.  (The bound keeps every histogram sum of the weighted select from wrapping, over up to 2^10 handles.)  Not while a
 * staged select is in flight (RSCM_ERR_STATE). */
RSCM_API int rscm_ens_set_member_weights(rscm_ens* h, const int64_t* w, int32_t on_device);
/* Device address of the [N] int64 weights; RSCM_ERR_STATE (and NULL) if none are set. */
RSCM_API int rscm_ens_member_weights_devptr(rscm_ens* h, void** out);
/* *out = max ll[i] over members with status 0 and a finite ll[i]; -inf if there is none.  ll[N]: host or (on_device) device
 * memory, e.g. the vector of rscm_ens_loglik_device.  A max is exact, so the maxima of shards reduce to the global one. */
RSCM_API int rscm_ens_loglik_max(rscm_ens* h, const double* ll, int32_t on_device, double* out);
/* Member weights from a log-likelihood: w[i] = llround(exp(min(ll[i] - ll_max, 0)) * 2^bits) for members with status 0 and a
 * finite ll[i], else 0.  0 <= bits <= 52; ll_max finite or -inf (members above it get 2^bits).  Members whose likelihood
 * ratio to ll_max is below 2^-(bits+1) get weight 0.  Sharded ensembles pass one global ll_max and bits, so that every rank's
 * weights are on one scale; bits <= 53 - ceil(log2(N_total)) keeps every row weight W <= 2^53.  Weights whose total exceeds
 * 2^53 are refused as by rscm_ens_set_member_weights (RSCM_ERR_INVALID; the weights set before stay). */
RSCM_API int rscm_ens_set_weights_from_loglik(rscm_ens* h, const double* ll, int32_t on_device, double ll_max, int32_t bits);
/* numpy.nanquantile(row, q, weights=w, method="inverted_cdf") of stored variable var_id over the rows of
 * rscm_ens_quantile_rows, with the handle's member weights: per (row, q) the smallest integer C >= 1 with
 * (double)C / (double)W >= q, W the summed weight of the row's non-NaN members, and the first member in key order at which
 * the cumulative weight reaches C.  NaN members are left out with their weights; a zero-weight member is never returned.
 * out[rows][n_q]; weight[rows] (or NULL) = W, exact as a double.  W == 0 (and rows beyond the time index): weight 0,
 * quantiles NaN.  Signed zeros as rscm_ens_quantile_rows.  No weights set: RSCM_ERR_STATE; a row with W > 2^53:
 * RSCM_ERR_INVALID; other errors as rscm_ens_quantile_rows. */
RSCM_API int rscm_ens_weighted_quantile_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride,
                                             int32_t n_q, const double* q, double* out, double* weight);
/* The weighted select in stages: begin with this, then the loop of rscm_ens_select_pass / _commit / _result / _end above,
 * unchanged.  The buffer holds int64 weight sums (one histogram per row and quantile after pass 0); _result's count receives
 * W.  The first commit checks W <= 2^53 on the reduced buffer, so every handle of a sharded select returns RSCM_ERR_INVALID
 * together; end the select then.  The weights must not change between begin and the last pass. */
RSCM_API int rscm_ens_select_begin_weighted(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride,
                                            int32_t n_q, const double* q);

/* ---- anomalies, per-member indicators and exceedance (ABI minor 8) ------------------------------ */
/* Rows are those of rscm_ens_quantile_rows (t_begin, t_begin + t_stride, ... < t_end, any storage layout); the time of row t is
 * time_bounds[t] of the handle.  The baseline b[N] is handle-owned, kept across rscm_ens_run and rscm_ens_rewind, freed by
 * rscm_ens_destroy; one per handle.  It does not change while a staged select is in flight (RSCM_ERR_STATE).
 * rscm_ens_set_baseline: b[i] = the sum of member i's values over the rows in row order (f64, no FMA) divided by the row count
 * (IEEE division); a NaN in a member's rows makes its b[i] NaN.  At least one row; every row computed (RSCM_ERR_STATE) and
 * resident (RSCM_ERR_STATE, as rscm_ens_quantile_rows).  On failure the baseline set before stays. */
RSCM_API int rscm_ens_set_baseline(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride);
/* b: N values, host or (on_device != 0) device memory on the handle's device. */
RSCM_API int rscm_ens_set_baseline_values(rscm_ens* h, const double* b, int32_t on_device);
/* Device address of the [N] baseline; RSCM_ERR_STATE (and NULL) if none is set. */
RSCM_API int rscm_ens_baseline_devptr(rscm_ens* h, void** out);
RSCM_API int rscm_ens_clear_baseline(rscm_ens* h);
/* Flags of the _ex and vector selects (RSCM_SELECT_GROUPED, 4: with the member groups below) */
#define RSCM_SELECT_WEIGHTED 1 /* the member weights, numpy "inverted_cdf" (rscm_ens_weighted_quantile_rows) */
#define RSCM_SELECT_ANOMALY 2  /* of the anomalies x[i] - b[i] (one IEEE subtraction) against the baseline; stored rows only */
/* rscm_ens_quantile_rows (flags 0) and rscm_ens_weighted_quantile_rows (RSCM_SELECT_WEIGHTED) with flags: the same
 * definitions applied to each member's anomaly with RSCM_SELECT_ANOMALY (a NaN anomaly is left out).  count[rows] receives the
 * count, or W when weighted.  Anomaly without a baseline: RSCM_ERR_STATE; an unknown flag: RSCM_ERR_INVALID. */
RSCM_API int rscm_ens_quantile_rows_ex(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q,
                                       const double* q, int32_t flags, double* out, double* count);
/* The staged form: begin with this, then rscm_ens_select_pass / _commit / _result / _end, unchanged. */
RSCM_API int rscm_ens_select_begin_ex(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q,
                                      const double* q, int32_t flags);
/* Per-member indicators over the rows, of x or (anomaly != 0) of x - b: a member with a NaN value in any row gets NaN in every
 * indicator, else mean = sum in row order / row count, peak = the maximum, peak_time = time of the first row attaining it
 * (numpy.argmax), crossing[k] = time of the first row with value >= thr[k], +inf if none; 0 <= n_thr <= 8.  Written to the
 * handle-owned block of `slot` (0 <= slot < 4), [3 + n_thr][N] doubles from *out_dev: mean, peak, peak_time, crossings.  A slot's
 * address stays for the handle's life; its contents until the next call on the slot.  Rows as rscm_ens_set_baseline; anomaly
 * without a baseline and a select in flight: RSCM_ERR_STATE; a bad slot: RSCM_ERR_INVALID. */
RSCM_API int rscm_ens_member_indicators(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t anomaly,
                                        int32_t n_thr, const double* thr, int32_t slot, void** out_dev);
/* The quantiles of rscm_ens_quantile_rows_ex with vec_dev[n_vec] (a host array) of device addresses of N doubles on the handle's
 * device (indicators, rscm_ens_params_devptr rows, a log-likelihood) as the rows: out[n_vec][n_q], count[n_vec].
 * RSCM_SELECT_ANOMALY: RSCM_ERR_INVALID; so is an address that is not device memory of N doubles on the handle's device.  The
 * vectors must not change between begin and the last pass of the staged form. */
RSCM_API int rscm_ens_quantile_vectors(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t n_q, const double* q,
                                       int32_t flags, double* out, double* count);
RSCM_API int rscm_ens_select_begin_vectors(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t n_q, const double* q,
                                           int32_t flags);
/* Exceedance of the device vector vec_dev[N]: hits[k] = the number of non-NaN members with v >= thr[k] (weighted != 0: the sum of
 * their member weights), *total = the number (summed weight) of non-NaN members; 0 <= n_thr <= 8.  int64, exact, so the sums of
 * shards are those of the whole ensemble; the probability is hits / total.  Weighted without weights: RSCM_ERR_STATE. */
RSCM_API int rscm_ens_exceedance(rscm_ens* h, const double* vec_dev, int32_t n_thr, const double* thr, int32_t weighted, int64_t* hits,
                                 int64_t* total);

/* ---- member groups: per-group quantiles and exceedance (ABI minor 11) ---------------------------- */
/* group[N]: int32, -1 = the member belongs to no group and is left out of every grouped statistic, else 0 <= id < n_groups.
 * 1 <= n_groups <= 64.  Host memory, or device memory on the handle's device (on_device != 0).  The groups are handle-owned (a
 * copy is taken), kept across rscm_ens_run, rscm_ens_rewind and rscm_ens_gather_members INTO the handle (a branch does not touch
 * the destination's groups, as it does not touch its forcing), freed by rscm_ens_destroy; they are not part of a checkpoint.  The
 * ids are checked on the device: one outside [-1, n_groups), or n_groups outside [1, 64], is RSCM_ERR_INVALID and leaves the
 * groups set before.  Not while a staged select is in flight (RSCM_ERR_STATE). */
RSCM_API int rscm_ens_set_member_groups(rscm_ens* h, const int32_t* group, int32_t on_device, int32_t n_groups);
/* Device address of the [N] int32 group ids and their n_groups; RSCM_ERR_STATE (and NULL, 0) if none are set. */
RSCM_API int rscm_ens_member_groups_devptr(rscm_ens* h, void** out, int32_t* n_groups);
RSCM_API int rscm_ens_clear_member_groups(rscm_ens* h);
/* A further flag of rscm_ens_quantile_rows_ex, rscm_ens_select_begin_ex, rscm_ens_quantile_vectors and
 * rscm_ens_select_begin_vectors, alone or with the flags those calls already take: one result per row AND group.  For every row r
 * and group g the result is exactly what the same call without the flag returns for an ensemble consisting of the members with
 * group[i] == g, in member order (plain: count = the group's non-NaN members; weighted: W = their summed weight, checked against
 * 2^53 per (row, group) at the first commit; anomaly: of x[i] - b[i]; signed zeros as rscm_ens_quantile_rows).  A group with no
 * non-NaN member in a row: count 0, quantiles NaN.  out[rows][n_groups][n_q], count[rows][n_groups]; rows beyond the time index
 * as without the flag, for every group.  The staged buffer is [rows][n_groups][256] int64 in pass 0 and
 * [rows][n_groups][n_t][256] later (n_t = 2 n_q, weighted n_q); rscm_ens_select_pass reports its size, and _commit, _result and
 * _end keep their protocol.  No groups set: RSCM_ERR_STATE.  The groups must not change between begin and the last pass. */
#define RSCM_SELECT_GROUPED 4
/* hits[n_groups][n_thr], total[n_groups]: rscm_ens_exceedance per group; int64, exact, so shards add up.  Members of no group
 * (-1) are left out.  No groups set, or weighted without weights: RSCM_ERR_STATE. */
RSCM_API int rscm_ens_exceedance_grouped(rscm_ens* h, const double* vec_dev, int32_t n_thr, const double* thr, int32_t weighted,
                                         int64_t* hits, int64_t* total);

/* ---- exact weighted means and covariances across members (ABI minor 23) --------------------------- */
/* The weighted mean vector and covariance matrix of K per-member vectors over the members of a handle (of each member group, if
 * asked), accumulated in integers: exact, independent of the order of summation, and summable across handles and ranks with a plain
 * int64 SUM.  This is the one definition; the kernel (moments.hip), the finishing step (moments_finish.hpp) and the tests'
 * restatement in Python integers and fractions apply it.
 *   Inputs: vec_dev[K] (a host array), 1 <= K <= RSCM_MOMENT_MAX_VECTORS, of device addresses of N doubles on the handle's device,
 *   as for rscm_ens_quantile_vectors.  flags: RSCM_SELECT_WEIGHTED and RSCM_SELECT_GROUPED; RSCM_SELECT_ANOMALY and unknown flags
 *   are RSCM_ERR_INVALID; weighted without weights, or grouped without groups, RSCM_ERR_STATE.  G = n_groups when grouped, else 1.
 *   Which members count: member i is counted in group g when group[i] == g (every member when not grouped) and all K of its values
 *   are finite -- listwise, so that the matrix belongs to one population.  w_i is its member weight, 1 when not weighted (weights
 *   that are set are ignored without the flag).  n_g is the number of counted members, W_g the sum of their w_i.
 *   Order 1: S_a = sum_i w_i x_ia as an exact integer; mean_a = RN(S_a / W_g), the exact quotient rounded once, ties to even.
 *   Order 2, about a centre c[G][K] of host doubles (the means above, or any finite doubles), for a <= b:
 *     d_ia = x_ia - c_ga (one IEEE subtraction),  p_iab = d_ia * d_ib (one IEEE multiplication, no FMA),
 *     C_ab = sum_i w_i p_iab, exact;  cov_ab = RN(C_ab / W_g).  The weights are frequencies and the divisor is W: a caller who
 *   wants W - 1 has W.  A non-finite p_iab (a difference or a product of finite values that overflows) is not added: every
 *   counted member with such a term, whatever its weight, adds one to the count of its sum's block, and a block with a non-zero
 *   count finishes as NaN.  If any c_ga of a group is not finite, every term of every block of that group is counted so (the
 *   limbs stay zero, n_g and W_g stay in place).  W == 0 finishes as NaN, a zero sum as +0.0.
 *   The accumulator: one sum is a block of RSCM_MOMENT_BLOCK = 69 int64: 68 signed limbs, limb k in units of 2^(32 k - 1088), then
 *   the count of non-finite terms.  A term is taken from the raw fields of the double (sign, E, fraction): the mantissa is the
 *   fraction if E == 0, else 2^52 + fraction, and its lowest bit sits at accumulator bit max(E, 1) + 13.  w * mantissa (at most
 *   106 bits) is cut into 32-bit digits at limb boundaries and each digit is added, with the term's sign, into its limb; carries
 *   are deferred.  The 68 limbs cover every finite double times a total weight of 2^63: 2^53 per handle (the bound the member
 *   weights already have) over 2^10 handles.  An int64 limb takes 2^31 digits before it can wrap: the number of counted members
 *   over everything that is summed together must stay below 2^31, and the finishing step refuses more.
 *   Raw limbs of two accumulations of the same terms need not be equal (deferred carries differ with the order); their canonical
 *   value sum_k limb_k 2^(32 k) is.  That is what lets blocks of shards add up limb by limb.
 *   Result of rscm_ens_moment_sums: out[G][2 + B * 69] int64, per group n, W, then B blocks: order 1 B = K, block a = S_a; order 2
 *   B = K (K + 1) / 2 in the order (0,0), (0,1), ..., (0,K-1), (1,1), ....  out is host memory, or (on_device != 0) device memory on
 *   the handle's device, e.g. the buffer of a collective.  order outside {1, 2}, order 2 without center, a NULL out or vec_dev, K out
 *   of range, a vector that is not device memory of N doubles on the handle's device, N >= 2^31: RSCM_ERR_INVALID.  center is read
 *   for order 2 only. */
#define RSCM_MOMENT_MAX_VECTORS 8
#define RSCM_MOMENT_BLOCK 69
RSCM_API int rscm_ens_moment_sums(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t flags, int32_t order,
                                  const double* center, int64_t* out, int32_t on_device);
/* The finishing step; it needs no device and no handle, so that a host can finish after a reduction of its own:
 * out[b] = RN(canonical(blocks[b]) * 2^-1088 / divisor[b]) for b < n_blocks over blocks[n_blocks][69].  The carries are normalised,
 * the exact quotient is formed and rounded once: ties to even, results in the subnormal range exact on their grid, a result
 * beyond the largest finite double infinite, a non-zero sum that rounds to zero keeps its sign, a zero sum is +0.0.  A block with
 * a non-zero count, or divisor[b] == 0: NaN.  n_terms is the number of counted members over everything that was summed into the
 * blocks: n_terms < 0 or >= 2^31, a negative divisor, a negative n_blocks or a NULL argument with n_blocks > 0: RSCM_ERR_INVALID. */
RSCM_API int rscm_gpu_moment_finish(const int64_t* blocks, int32_t n_blocks, const int64_t* divisor, int64_t n_terms, double* out);
/* The two passes and the finish on one handle: mean[G][K], cov[G][K][K] (symmetric, both triangles written), n[G], weight[G]; the
 * centre of order 2 is mean.  A group with W == 0: NaN in mean and cov.  n and weight may be NULL.  Errors as rscm_ens_moment_sums. */
RSCM_API int rscm_ens_moments(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t flags, double* mean, double* cov,
                              int64_t* n, int64_t* weight);

/* ---- exact weighted mean and spread of a stored variable at every row (ABI minor 24) ---------------- */
/* The moments above for the rows of a stored variable instead of vectors: per row (and member group) the weighted mean and second
 * moment of the variable across members, and its covariance with K per-member vectors, from one launch per order over all rows.
 * This is the one definition; the kernel (moment_rows.hip), its integer pieces (moment_window.hpp) and the tests' restatement in
 * Python integers (tests/host_moment_rows.py) apply it.
 *   Rows: those of rscm_ens_quantile_rows, t_begin, t_begin + t_stride, ... < t_end of var_id, read where they are resident (full
 *   storage, the window, the output store); a diagnostic by its id, RSCM_ERR_STATE when it is stale.  A row beyond the current time
 *   index has n = 0, W = 0 and zero blocks (NaN once finished); a computed row that is not resident is RSCM_ERR_STATE, as is a call
 *   while a staged select is in flight on the handle.
 *   The value of member i in row t: x = series[t][i], or with RSCM_SELECT_ANOMALY x = series[t][i] - b[i], one rounded subtraction,
 *   the bits rscm_ens_quantile_rows_ex sees under that flag; without a baseline RSCM_ERR_STATE.
 *   Vectors: vec_dev[K], 0 <= K <= RSCM_MOMENT_ROWS_MAX_VECTORS, device addresses of N doubles on the handle's device (vec_dev may
 *   be NULL when K == 0).
 *   Which members count, per row: member i counts in row t when x is finite, all K of its vector values are finite and, with
 *   RSCM_SELECT_GROUPED, its group is valid (it then counts in that group).  Every row has its own n and W: a member that is NaN
 *   from some row on drops out of those rows only.  w_i is the member weight with RSCM_SELECT_WEIGHTED, else 1.
 *   Sums: the limb scheme of rscm_ens_moment_sums, block for block (RSCM_MOMENT_BLOCK int64: 68 limbs, then the count of non-finite
 *   terms).  Order 1, B = 1 + K blocks: S_x, S_v0 .. S_v(K-1) over the row's counted members.  Order 2, B = 1 + 2 K blocks about
 *   center[rows][G][1 + K] (host doubles: the centre of x, then of each vector), in the order xx, x v_0 .. x v_(K-1),
 *   v_0 v_0 .. v_(K-1) v_(K-1); a term is RN(RN(p - c_p) * RN(q - c_q)), no FMA.  A non-finite term is counted, not added; a
 *   (row, group) with any non-finite centre has every term of every block counted so.
 *   Result: out[rows][G][2 + B * 69] int64 -- n, W, the blocks -- for either order; host memory, or device memory on the handle's
 *   device when on_device != 0.  Raw limbs of shards add element by element; canonical values are what compares.
 *   rows * G * B may not exceed RSCM_MOMENT_ROWS_MAX_BLOCKS = 2^19 (751 rows x 64 groups x 9 blocks are 432 576; the array then
 *   takes 552 bytes per block): RSCM_ERR_INVALID.  Also RSCM_ERR_INVALID: unknown flags, order outside {1, 2}, order 2 without
 *   center, K out of range, a NULL out, a vector or a device out that is not device memory of the size on the handle's device, a
 *   bad row range, N >= 2^31.  Weighted without weights, grouped without groups: RSCM_ERR_STATE. */
#define RSCM_MOMENT_ROWS_MAX_VECTORS 4
#define RSCM_MOMENT_ROWS_MAX_BLOCKS (1 << 19)
RSCM_API int rscm_ens_moment_rows_sums(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_vec,
                                       const double* const* vec_dev, int32_t flags, int32_t order, const double* center, int64_t* out,
                                       int32_t on_device);
/* The two passes and the finish (rscm_gpu_moment_finish) on one handle: mean[rows][G][1 + K] (of x, then of the vectors over the row's
 * counted members), second[rows][G][1 + 2 K] (the order-2 sums about mean, divided by W, in the order above: the variance of x, its
 * covariances with the vectors, the vectors' variances), n[rows][G], weight[rows][G]; n and weight may be NULL.  W == 0: NaN.
 * Errors as rscm_ens_moment_rows_sums. */
RSCM_API int rscm_ens_moment_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_vec,
                                  const double* const* vec_dev, int32_t flags, double* mean, double* second, int64_t* n, int64_t* weight);

/* ---- exceedance and observation rank of a stored variable at every row (ABI minor 26) --------------- */
/* rscm_ens_exceedance for the rows of a stored variable instead of one vector, with thresholds that may differ per row: the
 * exceedance probability as a series, and, with a record as the per-row threshold, the rank of the record inside the plume.  This
 * is the one definition; the kernel (exceedance_rows.hip), rscm_amd's finishers and the tests' restatement in numpy and Python
 * integers (tests/host_exceedance_rows.py) apply it.
 *   Rows: those of rscm_ens_moment_rows_sums, t_begin, t_begin + t_stride, ... < t_end of var_id, read where they are resident (full
 *   storage, the window, the output store); a diagnostic by its id, RSCM_ERR_STATE when it is stale.  A computed row that is not
 *   resident is RSCM_ERR_STATE, as is a call while a staged select is in flight on the handle.
 *   Thresholds: K = n_thr per row, 1 <= K <= RSCM_EXCEEDANCE_ROWS_MAX_THRESHOLDS, host doubles: thr[K], the same for every row
 *   (thr_per_row == 0), or thr[rows][K] (thr_per_row != 0).
 *   The value of member i in row t: x = series[t][i], or with RSCM_SELECT_ANOMALY x = series[t][i] - b[i], one rounded subtraction,
 *   the bits rscm_ens_quantile_rows_ex and rscm_ens_moment_rows_sums see under that flag; without a baseline RSCM_ERR_STATE.
 *   Which members take part, per row: member i takes part in row t when x is not NaN; infinities take part, as in
 *   rscm_ens_exceedance.  Its weight is 1, or the member weight w[i] with RSCM_SELECT_WEIGHTED (without weights RSCM_ERR_STATE).
 *   With RSCM_SELECT_GROUPED it counts in group g[i], and a member of no group (-1) is left out (without groups RSCM_ERR_STATE);
 *   G = n_groups when grouped, else 1.
 *   Per row and group, as int64:
 *     total   = the summed weight of the members that take part;
 *     hits[k] = the summed weight of those with x >= thr[k];
 *     equal[k] = the summed weight of those with x == thr[k] (IEEE comparison: -0 equals +0).
 *   A NaN threshold gives hits[k] = equal[k] = 0 for that row and k and leaves total alone: how a record marks a row without an
 *   observation.  Thresholds of +-Inf compare as IEEE compares them.  A row beyond the current time index has zeros everywhere.
 *   The sums are integers: exact, independent of the order of summation, and those of shards add up to the whole ensemble's.  The
 *   limit on the summed weight is that of rscm_ens_exceedance: a handle's member weights sum to at most 2^53
 *   (rscm_ens_set_member_weights), so nothing wraps over fewer than 2^10 handles.
 *   Result: hits[rows][G][K], equal[rows][G][K] (may be NULL: not formed), total[rows][G], host memory.
 *   RSCM_ERR_INVALID: unknown flags, K out of range, a NULL thr, hits or total, a bad row range or stride, a variable without a
 *   stored series. */
#define RSCM_EXCEEDANCE_ROWS_MAX_THRESHOLDS 8
RSCM_API int rscm_ens_exceedance_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_thr,
                                      const double* thr, int32_t thr_per_row, int32_t flags, int64_t* hits, int64_t* equal,
                                      int64_t* total);

/* ---- histograms across members: of a stored variable at every row, of member vectors, of two vectors jointly (ABI minor 28) ---- */
/* The distribution itself, where rscm_ens_exceedance_rows gives its tail at a few thresholds: per row and member group the summed
 * weight of the members in each bin between ascending edges.  This is the one definition; the kernels (histogram.hip, with the bin
 * of a value in histogram_bin.hpp), rscm_amd's finishers and the tests' restatement in numpy and Python integers
 * (tests/host_histogram.py) apply it.
 *   Edges: e[0] < e[1] < ... < e[E-1], host doubles, finite and strictly ascending, 2 <= E <= RSCM_HISTOGRAM_MAX_EDGES; B = E - 1
 *   bins.  Anything else is RSCM_ERR_INVALID.
 *   Binning: for a value v that is not NaN let k be the number of edges with e[j] <= v (IEEE comparisons: -0 equals +0, and
 *   infinities take part).  k == 0: v counts in `below`.  1 <= k <= B: in bin k - 1, so bin j holds e[j] <= v < e[j+1].  k == E: in
 *   the last bin when v == e[E-1] (the last edge is closed), else in `above`.  This is numpy.histogram(x, bins=e, weights=w) with
 *   int64 weights, plus the two counts outside.
 *   Who takes part follows rscm_ens_exceedance_rows: a member takes part when its value is not NaN; its weight is 1, or the member
 *   weight w[i] with RSCM_SELECT_WEIGHTED; with RSCM_SELECT_GROUPED it counts in group g[i], and a member whose id is outside
 *   [0, G) is left out (G = n_groups when grouped, else 1); with RSCM_SELECT_ANOMALY the value is series[t][i] - b[i], one rounded
 *   subtraction.  A flag without its weights, groups or baseline is RSCM_ERR_STATE.
 *   All sums are int64: exact, independent of the order of summation, total = below + sum(counts) + above holds exactly, and the
 *   sums of shards add up to the whole ensemble's.  The limit on the summed weight is that of rscm_ens_exceedance.
 *   Slots: a block of the kernel keeps a call's bins in LDS, G (B + 2) slots in one dimension and G (Bx By + 1) in two; more than
 *   RSCM_HISTOGRAM_MAX_SLOTS is RSCM_ERR_INVALID, and the message names the product.  That holds 3 groups x 1024 bins, 64 groups x
 *   126 bins and a joint histogram of 64 x 64.
 * rscm_ens_histogram_rows: the rows t_begin, t_begin + t_stride, ... < t_end of var_id, resolved as rscm_ens_exceedance_rows
 * resolves them (full storage, the window, the output store; a diagnostic by its id, RSCM_ERR_STATE when it is stale or a computed
 * row is not resident, or while a staged select is in flight).  Result, host memory: counts[rows][G][B], below[rows][G],
 * above[rows][G], total[rows][G]; a row beyond the current time index has zeros everywhere.  One launch for all rows.
 * RSCM_ERR_INVALID besides: unknown flags, a NULL result, a bad row range or stride, a variable without a stored series. */
#define RSCM_HISTOGRAM_MAX_EDGES 1025
#define RSCM_HISTOGRAM_MAX_SLOTS 8192
#define RSCM_HISTOGRAM_MAX_VECTORS 8
RSCM_API int rscm_ens_histogram_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_edges,
                                     const double* edges, int32_t flags, int64_t* counts, int64_t* below, int64_t* above, int64_t* total);
/* The same of 1 <= n_vec <= RSCM_HISTOGRAM_MAX_VECTORS per-member device vectors (vec_dev[n_vec], a host array of device addresses
 * of N doubles, checked as rscm_ens_quantile_vectors checks its vectors), which serve as the rows: indicators, parameter rows, a
 * log-likelihood.  edges[E] is shared (edges_per_vector == 0), or edges[n_vec][E] gives every vector its own, each table checked as
 * above.  NaN is left out per vector, not listwise.  RSCM_SELECT_ANOMALY is RSCM_ERR_INVALID.  Result: counts[n_vec][G][B], below,
 * above, total [n_vec][G].  The kernel is that of the rows with an edge table per row. */
RSCM_API int rscm_ens_histogram_vectors(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t n_edges, const double* edges,
                                        int32_t edges_per_vector, int32_t flags, int64_t* counts, int64_t* below, int64_t* above,
                                        int64_t* total);
/* The joint histogram of two per-member device vectors: a member takes part when neither value is NaN, and counts in
 * counts[G][Bx][By] at (bin of x among edges_x, bin of y among edges_y) when both values fall into a bin, in outside[G] when either
 * is below its first or above its last edge; total[G] = sum(counts) + outside is the weight taking part.  Flags, edges and errors as
 * rscm_ens_histogram_vectors. */
RSCM_API int rscm_ens_histogram2d(rscm_ens* h, const double* x_dev, const double* y_dev, int32_t n_edges_x, const double* edges_x,
                                  int32_t n_edges_y, const double* edges_y, int32_t flags, int64_t* counts, int64_t* outside,
                                  int64_t* total);

/* ---- per-member variability statistics and a likelihood over per-member vectors (ABI minor 16) ---- */
/* How variable is each member's series of var_id over a period: its mean, its trend, the variance and standard deviation about the
 * trend and the lag-one autocorrelation of what is left, per member, on the device.  This is the one definition; the kernel
 * (variability.hip), rscm_amd.variability.series_variability and the tests' numpy restatement apply it operation by operation.
 *   Rows x_0 .. x_{R-1}: those of rscm_ens_set_baseline (t_begin, t_begin + t_stride, ... < t_end; any storage layout; every row
 *   computed and resident, else RSCM_ERR_STATE).
 *   Working series u_0 .. u_{n-1}:  RSCM_VAR_MEAN and RSCM_VAR_LINEAR  u_k = x_k, n = R;
 *                                   RSCM_VAR_DIFFERENCE                u_k = x_{k+1} - x_k (one IEEE subtraction), n = R - 1.
 *   n >= 3, else RSCM_ERR_INVALID.
 *   Every operation below is one f64 operation rounded on its own (no FMA); sums run left to right from their first term.
 *     tau_k = (double)k - h,  h = (n - 1) * 0.5  (exact)
 *     S = u_0 + u_1 + ...                        m = S / n
 *     RSCM_VAR_LINEAR:  Q = tau_0*u_0 + tau_1*u_1 + ...,  b = Q / Stt,  Stt = (double)(n (n^2 - 1)) / 12.0 with n (n^2 - 1) formed in int64;
 *     the other modes:  b = +0.0
 *     a_k = u_k - m;  RSCM_VAR_LINEAR:  a_k = (u_k - m) - b*tau_k
 *     C0 = a_0*a_0 + a_1*a_1 + ...               C1 = a_0*a_1 + a_1*a_2 + ...  (n - 1 terms)
 *     variance = C0 / n    sd = sqrt(variance)   r1 = C1 / C0
 *   r1 is the biased estimator, so |r1| <= 1 up to rounding; C0 == 0 (a constant working series) gives NaN by 0/0.
 * [5][N] doubles from *out_dev: mean (m), slope (b, per row index: per t_stride steps of the axis), variance, sd, r1.  A member
 * with a non-finite value in any of its rows gets NaN in all five.
 * The result is written to the handle-owned block of indicator slot `slot` (0 <= slot < 4): the slots are those of
 * rscm_ens_member_indicators, and a slot holds the vectors of the last call on it, indicators or variability alike, until the next
 * call on that slot.  A bad slot or mode: RSCM_ERR_INVALID; a select in flight: RSCM_ERR_STATE. */
#define RSCM_VAR_MEAN 0       /* about the member's mean */
#define RSCM_VAR_LINEAR 1     /* about the member's least-squares line over the row index */
#define RSCM_VAR_DIFFERENCE 2 /* of the first differences of the rows, about their mean */
RSCM_API int rscm_ens_member_variability(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode,
                                         int32_t slot, void** out_dev);
/* A Gaussian likelihood over per-member device vectors, continuing a point likelihood: vec_dev[n_vec] (a host array) holds device
 * addresses of N doubles on the handle's device (variability statistics, indicators, rscm_ens_params_devptr rows), checked as
 * rscm_ens_quantile_vectors checks its vectors; 1 <= n_vec <= 16; value[j] finite, sigma[j] finite and > 0 (RSCM_ERR_INVALID).
 * Per member i: partial = 0.0; for j in order r = value[j] - v_j[i], chi = (r*r)/(sigma[j]*sigma[j]), partial += -0.5*chi -- the
 * expressions of rscm_ens_loglik; the result is add_dev[i] + partial, or 0.0 + partial with add_dev NULL: the vectors count as one
 * more variable group after the point likelihood's groups, so the sum is rscm_ens_loglik's total continued.  A non-finite v_j[i]
 * gives -inf; so does a non-finite add_dev[i] (-inf stays -inf).
 * There is no normalize flag: ln(2 pi) and ln(sigma[j]) are the same for every member and cancel in the weights; leaving them out
 * keeps the call free of the device logarithm, and so bit-exact against the expressions above.
 * The result lands in the handle's likelihood vector, the buffer of rscm_ens_loglik_device (*out_dev).  add_dev may BE that
 * buffer -- each thread reads its own element before it writes it -- which is the intended use: rscm_ens_loglik_device, then this
 * call with add_dev = its result. */
RSCM_API int rscm_ens_loglik_vectors_device(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, const double* value,
                                            const double* sigma, const double* add_dev, void** out_dev);

/* ---- per-member power spectra and a spectral likelihood (ABI minor 17) ---------------------------- */
/* How each member's variability of var_id is spread over periods: the periodogram of the detrended series, averaged over bands of
 * frequencies, per member, on the device.  The lag-one autocorrelation of rscm_ens_member_variability cannot tell strong short-lived
 * noise from weak persistent noise once the ocean has filtered it; the shape of the spectrum over all resolved periods can.  This is
 * the one definition; the kernel (spectrum.hip), rscm_amd.variability.series_spectrum and the tests' numpy restatement apply it
 * operation by operation.
 *   Rows, working series u_k, n, m, b, tau_k and the residuals a_k: EXACTLY those of rscm_ens_member_variability for the same mode --
 *   the same three detrenders, n >= 3, the same operations in the same order.  Also n <= 4096 (RSCM_ERR_INVALID beyond), which bounds
 *   the rounding error of the recurrence below (it grows with n and towards the lowest frequencies).
 *   Frequencies j = 1 .. J, J = (n - 1) / 2 in integer division: the mean and, for even n, the Nyquist term are left out, so every
 *   ordinate has two degrees of freedom.
 *   Coefficients c2_j = 2 * C_j, C_j the double nearest cos(2 pi j / n), formed by the library on the host (j / n reduced by symmetry in
 *   integers, then evaluated in long double; the doubling is exact); rscm_gpu_spectrum_coefficients returns the table the kernel is
 *   given, and a restatement takes it from there, so that nothing depends on the caller's cosine.
 *   Ordinate, by Goertzel's recurrence; every operation is one f64 operation rounded on its own (no FMA):
 *     s1 = s2 = +0.0;  for k = 0 .. n - 1 in order:  s0 = (a_k + c2_j*s1) - s2;  s2 = s1;  s1 = s0
 *     I_j = ((s1*s1 + s2*s2) - (c2_j*s1)*s2) / (double)n
 *   With this scaling the mean ordinate of white noise is its variance, and (2 / n) (I_1 + ... + I_J) is the variance for odd n.
 *   Bands: n_bands (1 .. 8) and edges[n_bands + 1], strictly ascending with edges[0] >= 1 and edges[n_bands] <= J + 1, else
 *   RSCM_ERR_INVALID.  Band b holds the frequencies edges[b] <= j < edges[b + 1], m_b of them;
 *     P_b = (I_{edges[b]} + I_{edges[b] + 1} + ...) / (double)m_b,  summed left to right in ascending j.
 * [3 + n_bands][N] doubles from *out_dev: mean (m), slope (b), variance (C0 / n, the bits of rscm_ens_member_variability's: the band
 * powers should add up to it), then P_0 .. P_{n_bands - 1}.  A member with a non-finite value in any of its rows gets NaN in every
 * vector.  A constant working series has variance 0 and every P_b = 0.
 * The result is written to indicator slot `slot` (a slot's block is [3 + 8][N]); slot rules and refusals are those of
 * rscm_ens_member_variability: a bad slot or mode RSCM_ERR_INVALID, rows not computed or not resident or a select in flight
 * RSCM_ERR_STATE.  Bit-exact against the restatement. */
RSCM_API int rscm_ens_member_spectrum(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode,
                                      int32_t n_bands, const int32_t* edges, int32_t slot, void** out_dev);
/* out[J], J = (n - 1) / 2: c2_j = 2 * (the double nearest cos(2 pi j / n)) at out[j - 1], the table rscm_ens_member_spectrum gives its
 * kernel for a working series of n terms; within 1 ulp of 2 cos(2 pi j / n), and +0.0 exactly where the cosine is zero.  Host only
 * (no device is touched).  3 <= n <= 4096, else RSCM_ERR_INVALID. */
RSCM_API int rscm_gpu_spectrum_coefficients(int32_t n, double* out /*[J]*/);
/* A spectral likelihood over per-member band powers, continuing a point likelihood.  Under the hypothesis that the record is one more
 * realisation of the member's process, the member's band power P_b and the record's I_b are two independent estimates of the same
 * spectrum with 2 m_b degrees of freedom each, so I_b / P_b ~ F(2 m_b, 2 m_b) -- the approximation Whittle makes, applied to both
 * sides.  The log density of I_b given P_b, member-independent terms dropped, is
 *     ll_b = m_b * (ln P_b - 2 ln(P_b + I_b)),
 * maximal at P_b = I_b; as m_b grows it tends to Whittle's -(ln S + I / S) per ordinate.
 * vec_dev[n_vec] (a host array) holds device addresses of N doubles (band powers of rscm_ens_member_spectrum), checked as
 * rscm_ens_loglik_vectors_device checks its vectors; 1 <= n_vec <= 16; record[j] (the record's I_b) finite and > 0, count[j] (m_b) >= 1,
 * else RSCM_ERR_INVALID.  Per member i: partial = 0.0; for j in order t = P + record[j], term = (double)count[j] * (ln(P) - 2.0 * ln(t)),
 * partial += term, with P = v_j[i]; the result is add_dev[i] + partial, or 0.0 + partial with add_dev NULL.  P non-finite or <= 0 gives
 * -inf (a constant series has no spectrum); so does a non-finite add_dev[i].
 * Because of the logarithm (the library's hand-written ln, within 1 ulp) this call is TOLERANCE-parity, not bit-exact: per member
 * within (4 + n_vec) 2^-52 (|add_i| + sum_j m_j (|ln P_j| + 2 |ln t_j|)) of the expressions above evaluated exactly.  The statistic
 * itself, rscm_ens_member_spectrum, stays bit-exact.
 * The result lands in the handle's likelihood vector (*out_dev); add_dev may BE that buffer, as for rscm_ens_loglik_vectors_device. */
RSCM_API int rscm_ens_loglik_spectrum_device(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, const double* record,
                                             const int32_t* count, const double* add_dev, void** out_dev);

/* ---- per-member covariability of two variables (ABI minor 20) -------------------------------------- */
/* How two variables of one member move together over a period: the covariance, the correlation and the regression slope of y on x of
 * their detrended series and the cross-correlation at up to RSCM_COV_MAX_LAGS leads and lags, per member, on the device -- how much
 * heat a member takes up per degree of warming, and which of the two series leads.  This is the one definition; the kernel
 * (covariability.hip), rscm_amd.variability.series_covariability and the tests' numpy restatement apply it operation by operation.
 *   Rows x_0 .. x_{R-1} of var_x and y_0 .. y_{R-1} of var_y: those of rscm_ens_member_variability over the same t_begin, t_end,
 *   t_stride.  Either variable may be a diagnostic (its rows must be held and not stale); var_x == var_y is allowed.
 *   Working series u_0 .. u_{n-1} of x under mode_x and v_0 .. v_{n-1} of y under mode_y (RSCM_VAR_MEAN, _LINEAR, _DIFFERENCE):
 *     neither mode is RSCM_VAR_DIFFERENCE:        u_k = x_k, v_k = y_k, n = R (rscm_ens_member_variability's);
 *     a variable whose mode is RSCM_VAR_DIFFERENCE:  u_k = x_{k+1} - x_k (one IEEE subtraction), n = R - 1;
 *     exactly one mode is RSCM_VAR_DIFFERENCE:    the OTHER variable is taken at the midpoints the differences span,
 *                                                 u_k = (x_k + x_{k+1}) * 0.5 (one addition, one exact multiplication), n = R - 1, and is
 *                                                 then detrended by its own mode: a year's heat uptake against that year's temperature.
 *   0 <= n_lags <= RSCM_COV_MAX_LAGS and n >= 3 + n_lags, else RSCM_ERR_INVALID.
 *   Residuals: rscm_ens_member_variability's, operation for operation.  tau_k, S, m, Q, Stt and b are formed per variable under its own
 *   mode over the n terms; a_k is the residual of u and c_k the residual of v.  Every operation is one f64 operation rounded on its
 *   own (no FMA); sums run left to right from their first term.
 *   Products:
 *     G_l    = a_0*c_l + a_1*c_{l+1} + ... + a_{n-1-l}*c_{n-1}   (l >= 0: x leads y by l terms)
 *     G_{-l} = a_l*c_0 + a_{l+1}*c_1 + ... + a_{n-1}*c_{n-1-l}   (y leads x)
 *     Cxx = a_0*a_0 + a_1*a_1 + ...     Cyy = c_0*c_0 + c_1*c_1 + ...
 *     D = sqrt(Cxx) * sqrt(Cyy)         (two square roots, so that the product of two sums cannot overflow first)
 * [5 + 2 n_lags][N] doubles from *out_dev, in this order: var_x = Cxx / n, var_y = Cyy / n, cov = G_0 / n, corr = G_0 / D,
 * slope = G_0 / Cxx (of y on x), then r_{+1} = G_1 / D, r_{-1} = G_{-1} / D, ... r_{+n_lags}, r_{-n_lags}.  A member with a non-finite
 * value in any row of EITHER variable gets NaN everywhere; a constant x or y gives NaN in corr, slope (x) and the lags by 0/0 and 0 in
 * its variance.  |corr| and every |r_l| are <= 1 up to rounding (Cauchy-Schwarz over the terms each sum holds).
 * Equalities that follow from the definition, bit for bit:
 *   with no mode mixed (both or neither RSCM_VAR_DIFFERENCE), var_x is rscm_ens_member_variability's variance of var_x for the same
 *   rows and mode_x, and var_y that of var_y;
 *   exchanging (var_x, mode_x) with (var_y, mode_y) exchanges var_x with var_y and r_{+l} with r_{-l} and leaves cov and corr
 *   unchanged: products commute and the order in k is the same.
 * The regression of uptake on temperature is NOT an unbiased estimate of a feedback parameter (the noise sits in the flux and the
 * temperature responds to it); a likelihood compares a member's estimate with a record's under the same estimator.
 * The result is written to indicator slot `slot` (a slot's block is [3 + 8][N]: at three lags the 11 vectors fill it); slot rules and
 * refusals are those of rscm_ens_member_variability: a bad slot, mode or n_lags RSCM_ERR_INVALID; rows not computed or not resident,
 * a stale diagnostic or a select in flight RSCM_ERR_STATE.  Bit-exact against the restatement. */
#define RSCM_COV_MAX_LAGS 3
RSCM_API int rscm_ens_member_covariability(rscm_ens* h, int32_t var_x, int32_t var_y, int32_t t_begin, int32_t t_end, int32_t t_stride,
                                           int32_t mode_x, int32_t mode_y, int32_t n_lags, int32_t slot, void** out_dev);

/* ---- per-member co-spectra and coherence of two variables (ABI minor 21) --------------------------- */
/* How two variables of one member move together PER FREQUENCY BAND: the squared coherence of their detrended series, the in-phase
 * gain of y on x (uptake per degree in the band) and its out-of-phase part, per member, on the device.  Over a period the time-domain
 * relation of rscm_ens_member_covariability mixes the slow band, where a feedback acts, with the fast band the noise fills; this
 * scores them apart.  This is the one definition; the kernel (cross_spectrum.hip), rscm_amd.variability.series_cross_spectrum and the
 * tests' numpy restatement apply it operation by operation.
 *   Rows, working series u_k, v_k and their common length n: EXACTLY those of rscm_ens_member_covariability for the same var_x, var_y,
 *   t_begin, t_end, t_stride, mode_x, mode_y -- each variable its own mode (RSCM_VAR_MEAN, _LINEAR, _DIFFERENCE); when exactly one is
 *   differenced the other is taken at the midpoints (x_k + x_{k+1}) * 0.5; either may be a diagnostic; var_x == var_y is allowed.
 *   Residuals a_k (of x) and c_k (of y), Cxx = a_0*a_0 + a_1*a_1 + ..., Cyy = c_0*c_0 + ...: that definition's, operation for operation.
 *   3 <= n <= 4096, else RSCM_ERR_INVALID (the upper limit is rscm_ens_member_spectrum's, for the same reason).
 *   Frequencies j = 1 .. J, J = (n - 1) / 2; c2_j from rscm_gpu_spectrum_coefficients; g_j, the double nearest sin(2 pi j / n), from
 *   rscm_gpu_spectrum_sines; h_j = c2_j * 0.5 (exact).
 *   Every operation is one f64 operation rounded on its own (no FMA); sums run left to right from their first term.
 *   Two Goertzel recurrences with the same c2_j:
 *     s1 = s2 = t1 = t2 = +0.0;  for k = 0 .. n - 1 in order:
 *       s0 = (a_k + c2_j*s1) - s2;  s2 = s1;  s1 = s0          t0 = (c_k + c2_j*t1) - t2;  t2 = t1;  t1 = t0
 *   Ordinates per frequency:
 *     Ixx_j = ((s1*s1 + s2*s2) - (c2_j*s1)*s2) / (double)n     (rscm_ens_member_spectrum's I_j of x);   Iyy_j the same on t
 *     K_j   = ((s1*t1 + s2*t2) - h_j*(s1*t2 + s2*t1)) / (double)n      the co-spectrum, Re X_a conj(X_c) / n
 *     Q_j   = (g_j*(s2*t1 - s1*t2)) / (double)n                         the quadrature spectrum, Im X_a conj(X_c) / n
 *   Q_j > 0 means x leads y: for c_k = a_{k-1} the cross term is |X_a|^2 e^{+iw}.
 *   Bands: n_bands (1 .. RSCM_XSPEC_MAX_BANDS) and edges[n_bands + 1] under rscm_ens_member_spectrum's rules: strictly ascending,
 *   edges[0] >= 1, edges[n_bands] <= J + 1, else RSCM_ERR_INVALID.  Only the frequencies inside [edges[0], edges[n_bands]) are
 *   computed; a caller who wants more bands calls again on another slot.  Band b holds edges[b] <= j < edges[b + 1], m_b of them;
 *     Pxx_b, Pyy_b, K_b, Q_b = the four ordinates summed in ascending j over the band, each sum divided by (double)m_b
 *     D_b = sqrt(Pxx_b) * sqrt(Pyy_b),  kc = K_b / D_b,  qc = Q_b / D_b
 * [2 + 3 n_bands][N] doubles from *out_dev, in this order: var_x = Cxx / n, var_y = Cyy / n, then per band
 *   coh2_b = kc*kc + qc*qc,  gain_b = K_b / Pxx_b,  gain_quad_b = Q_b / Pxx_b.
 * gain_b is the in-phase transfer of y on x in the band and gain_quad_b the out-of-phase part.  coh2_b <= 1 up to rounding
 * (Cauchy-Schwarz over the band's ordinates); a band of ONE ordinate has coh2 = 1 to rounding, whatever the series.
 * A member with a non-finite value in any row of EITHER variable gets NaN everywhere; a constant series gives 0 in its variance and
 * NaN by 0/0: a constant x in every band output, a constant y in coh2_b (its gains are 0 / Pxx_b = 0).
 * Equalities that follow from the definition, bit for bit:
 *   var_x, var_y are rscm_ens_member_covariability's for the same arguments;
 *   exchanging (var_x, mode_x) with (var_y, mode_y) leaves every coh2_b unchanged and exchanges var_x with var_y: K is symmetric in
 *   the two state pairs and Q changes sign exactly;
 *   with x == y every gain_quad_b is +-0.0 exactly; with y = 2 x (a diagnostic of one term of scale 2.0) coh2_b equals that of x with
 *   itself, gain_b is exactly twice it and every gain_quad_b is +-0.0 exactly.
 * The result is written to indicator slot `slot` (a slot's block is [3 + 8][N]: at three bands the 11 vectors fill it); slot rules and
 * refusals are those of rscm_ens_member_covariability and rscm_ens_member_spectrum: a bad slot, mode, band count or edge list
 * RSCM_ERR_INVALID; rows not computed or not resident, a stale diagnostic or a select in flight RSCM_ERR_STATE.  Bit-exact against
 * the restatement. */
#define RSCM_XSPEC_MAX_BANDS 3
RSCM_API int rscm_ens_member_cross_spectrum(rscm_ens* h, int32_t var_x, int32_t var_y, int32_t t_begin, int32_t t_end, int32_t t_stride,
                                            int32_t mode_x, int32_t mode_y, int32_t n_bands, const int32_t* edges, int32_t slot,
                                            void** out_dev);
/* out[J], J = (n - 1) / 2: g_j = the double nearest sin(2 pi j / n) at out[j - 1], the second table rscm_ens_member_cross_spectrum
 * gives its kernel; formed as rscm_gpu_spectrum_coefficients forms the cosines (the angle folded in integers into the first octant,
 * then evaluated in long double), within 1 ulp of sin(2 pi j / n) and always > 0 (j < n / 2).  Host only (no device is touched).
 * 3 <= n <= 4096, else RSCM_ERR_INVALID. */
RSCM_API int rscm_gpu_spectrum_sines(int32_t n, double* out /*[J]*/);

/* ---- diagnostic variables (ABI minor 18) ---------------------------------------------------------- */
/* A diagnostic variable of a handle is a linear combination of that handle's stored variables with per-member weights.  For member i
 * and row t, with K terms (1 <= K <= RSCM_DIAG_MAX_TERMS), x_k = row t of the stored variable term_var[k], p the parameter block:
 *     w_k[i] = term_scale[k] * p[term_param_row[k]][i]      (term_param_row[k] >= 0)
 *     w_k[i] = term_scale[k]                                (term_param_row[k] == -1)
 *     y[i]   = w_0[i] * x_0[i];   then for k = 1 .. K - 1 in order   y[i] = y[i] + w_k[i] * x_k[i]
 * Every product and every sum is one f64 operation rounded on its own (no FMA); the weight is formed once per member and is the same
 * for every row; NaN and Inf propagate by IEEE arithmetic (there is no per-member "bad" flag: the readers have their own).  Bit-exact
 * against this statement.  The ocean heat content of a two-layer handle is (Ts, row 4), (Td, row 5): C Ts + Cd Td in W yr m^-2.
 *
 * Ids.  Diagnostics get the variable ids V, V + 1, ... (V = rscm_ens_n_vars, which keeps reporting the stored variables) in order
 * of definition, at most RSCM_DIAG_MAX per handle; rscm_ens_n_diagnostics reports how many are defined.
 *
 * rscm_ens_define_diagnostic: RSCM_ERR_INVALID for n_terms outside 1..4, a term variable that is 0 (the input), negative or >= V (no
 * diagnostic of a diagnostic), a parameter row outside -1 .. P - 1, a scale that is not finite, a fifth definition.
 * rscm_ens_diagnostic reads a definition back (unused terms: 0, -1, 0.0) with the rows it holds now: *rows_held rows from *t_begin
 * with *t_stride (0, 0, 1 when none are held or they are stale).  Any out pointer may be NULL.
 * rscm_ens_compute_diagnostic forms the rows t_begin, t_begin + t_stride, ... < t_end into a store [R][N] the handle owns (allocated
 * at first use, reused when large enough, freed by rscm_ens_destroy and rscm_ens_clear_diagnostics).  Every source row must be computed
 * and resident: full storage, the window and the output store serve as for rscm_ens_member_indicators, with its refusals (a bad range
 * or stride RSCM_ERR_INVALID; rows beyond the time index, rows no longer resident, a RSCM_FLAG_NO_SERIES handle with t_end > 1
 * RSCM_ERR_STATE; on these the rows held before stay).  One range per diagnostic at a time: a new compute replaces the old rows.
 * rscm_ens_clear_diagnostics removes the definitions and frees the stores.  A var_id that names no diagnostic: RSCM_ERR_INVALID.
 * Define, compute and clear refuse with RSCM_ERR_STATE while a staged select is in flight (it may be reading the rows).
 *
 * Readers.  The id of a defined diagnostic is accepted by rscm_ens_select_begin* / rscm_ens_quantile_rows* (plain, weighted, anomaly,
 * grouped), rscm_ens_set_baseline, rscm_ens_member_indicators, _variability, _spectrum, _covariability, _cross_spectrum, the stored likelihoods rscm_ens_loglik,
 * _device, _ref, _ref_device (observation rows and reference-period rows), rscm_ens_summary and rscm_ens_get_series.  A row outside
 * the held range is to them what a row that is not resident is on a windowed handle: RSCM_ERR_STATE.  Everything else keeps refusing
 * the id as it refuses any var_id >= V (RSCM_ERR_INVALID): rscm_ens_series_devptr, rscm_ens_summary_series, rscm_ens_quantile_series,
 * rscm_ens_link_input, rscm_ens_set_state, rscm_ens_set_initial, the fused rscm_ens_run_loglik*, the samplers' observation and
 * reference lists, output_vars of rscm_ens_create_windowed.
 *
 * Staleness.  The rows are a snapshot of the sources at compute time.  The handle keeps a write epoch that moves with every entry
 * point that can change a stored row, a parameter row or the time index: rscm_ens_run, _run_async, rscm_ens_run_lockstep (every
 * handle of the run), rscm_ens_run_loglik*, a sampler's evaluation runs, rscm_ens_rewind, _clear_series, _clear_rows_after,
 * _set_time_index, _set_state, _set_initial, _set_internal_state, _set_params, _set_params_aos, _sample_lhs, _sample_lhs_priors, rscm_ens_gather_members
 * (the destination), rscm_ens_set_forcing_noise*, _clear_forcing_noise, rscm_ens_set_mode.  A reader that finds the rows computed at
 * another epoch gets RSCM_ERR_STATE, "diagnostic N is stale: compute it again".  Definitions survive all of these; only the rows go
 * stale.  rscm_ens_params_devptr and rscm_ens_series_devptr do NOT move the epoch: writes through pointers the library handed out
 * are the caller's to follow with a new rscm_ens_compute_diagnostic. */
#define RSCM_DIAG_MAX_TERMS 4
#define RSCM_DIAG_MAX 4
RSCM_API int rscm_ens_define_diagnostic(rscm_ens* h, int32_t n_terms, const int32_t* term_var, const int32_t* term_param_row,
                                        const double* term_scale, int32_t* var_id_out);
RSCM_API int rscm_ens_diagnostic(rscm_ens* h, int32_t var_id, int32_t* n_terms, int32_t term_var[4], int32_t term_param_row[4],
                                 double term_scale[4], int32_t* rows_held, int32_t* t_begin, int32_t* t_stride);
RSCM_API int rscm_ens_compute_diagnostic(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride);
RSCM_API int rscm_ens_clear_diagnostics(rscm_ens* h);
RSCM_API int rscm_ens_n_diagnostics(const rscm_ens* h, int32_t* out);

/* ---- energy-budget diagnostics (ABI minor 22) ------------------------------------------------------ */
/* The terms of a two-layer member's energy budget as diagnostic variables: RSCM_KIND_TWO_LAYER handles only -- plain, mix
 * (rscm_ens_create_mix) and every forcing-noise kind.  For member i and row t, Ts and Td its stored rows at t, p its parameter rows
 * 0 .. 5 (lambda0, a, efficacy, eta, C, Cd), F its forcing (below), every line ONE f64 operation rounded on its own (no FMA), the same
 * in either arithmetic mode:
 *     ee  = p2 * p3              once per member
 *     d   = Ts - Td
 *     u   = p1 * Ts
 *     lam = p0 - u
 *     R   = lam * Ts             RSCM_BUDGET_RESPONSE      the radiative response (lambda0 - a Ts) Ts
 *     X   = ee * d
 *     H   = p3 * d               RSCM_BUDGET_DEEP_UPTAKE   the heat the deep ocean takes up, eta (Ts - Td)
 *     g   = F - R
 *     g   = g - X
 *     N   = g + H                RSCM_BUDGET_IMBALANCE     the top-of-atmosphere imbalance, C dTs/dt + Cd dTd/dt
 *     F                          RSCM_BUDGET_FORCING       the member's forcing
 *     y   = scale * q            q the chosen quantity; multiplied even by 1.0
 * (F - R) - X is the numerator of the reference's surface tendency (TwoLayer::calculate_dy_dt), N its third tendency.
 *
 * F is the forcing the stepping kernel applies to the step OUT of row t, bit for bit: forcing-axis index f = t + off, off = 0 for
 * RSCM_SRC_EXOGENOUS and 1 for RSCM_SRC_UPSTREAM; the member's scenario's table value; on a mix handle S_0[f] * c_0, then
 * + S_k[f] * c_k for k = 1 .. K - 1 in order; then + sigma * z(seed, member_offset + i, f) for white noise, or + e_f of the red or
 * per-member recurrence formed from index 0 on (rscm_ens_set_forcing_noise*).  NaN and Inf propagate by IEEE arithmetic; there is no
 * per-member flag.
 *
 * rscm_ens_define_energy_budget takes one of the RSCM_DIAG_MAX diagnostic slots; ids, rscm_ens_n_diagnostics and
 * rscm_ens_clear_diagnostics work as for rscm_ens_define_diagnostic, and every reader of a diagnostic's rows takes the id.
 * RSCM_ERR_INVALID for another kind, an unknown quantity, a scale that is not finite, a fifth definition, and for RSCM_BUDGET_FORCING
 * and RSCM_BUDGET_IMBALANCE on a handle with a linked input (rscm_ens_link_input: the forcing is then another ensemble's series;
 * the other two quantities need no forcing and are allowed).  RSCM_ERR_STATE while a staged select is in flight.
 * rscm_ens_diagnostic_quantity reads a definition back; a linear diagnostic gives quantity 0 and scale 0.0.  rscm_ens_diagnostic on
 * such an id reports n_terms = 0, the unused-term values and the held range.
 * rscm_ens_compute_diagnostic serves both sorts; the source rows (Ts and Td) are resolved as a linear diagnostic's.  For the two
 * quantities that read the forcing the host checks every forcing index before the launch: a row t with t + off >= n_times gets
 * RSCM_ERR_INVALID naming the row (the last row of a RSCM_SRC_UPSTREAM handle: no step leaves it), a handle that has been linked since
 * RSCM_ERR_INVALID, forcing that was never set RSCM_ERR_STATE.  Parameters that were never set: RSCM_ERR_STATE.
 *
 * Staleness.  The rows go stale with the write epoch like every diagnostic's.  Those of RSCM_BUDGET_FORCING and _IMBALANCE go stale
 * as well with whatever replaces the forcing table, the scenario assignment or the source: rscm_ens_set_forcing (a mix handle's
 * included), rscm_ens_link_input, rscm_ens_unlink_input.  The linear diagnostics and the other two quantities do not. */
#define RSCM_BUDGET_FORCING 1
#define RSCM_BUDGET_RESPONSE 2
#define RSCM_BUDGET_DEEP_UPTAKE 3
#define RSCM_BUDGET_IMBALANCE 4
RSCM_API int rscm_ens_define_energy_budget(rscm_ens* h, int32_t quantity, double scale, int32_t* var_id_out);
RSCM_API int rscm_ens_diagnostic_quantity(rscm_ens* h, int32_t var_id, int32_t* quantity, double* scale);

/* ---- running means (ABI minor 27) ------------------------------------------------------------------ */
/* The mean of W = window rows of a variable, `step` time indices apart, as a diagnostic variable.  For member i, x[u] row u of the
 * source for that member, and back = W - 1 (RSCM_RUNMEAN_TRAILING: the window ends at t) or (W - 1) / 2 in integer division
 * (RSCM_RUNMEAN_CENTRED: W = 20 spans t - 9 .. t + 10), the row at time index t is
 *     s = x[t - back * step];   then for j = 1 .. W - 1 in that order   s = s + x[t + (j - back) * step];   y = s / (double)W
 * Every add and the one division is one IEEE f64 operation rounded on its own: no FMA, no reciprocal, no pairwise tree, and no sliding
 * update (s + new - old) -- a row is a pure function of its own W terms.  An Inf or NaN in row k of the source therefore reaches
 * exactly the rows whose window holds k, and every later row is untouched.  Bit-exact against this statement.
 * step is the spacing of the window's terms: step = 12 gives a 20-year mean from every twelfth row of a monthly axis; step = 1 and
 * window = 12 computed with t_stride = 12 gives the annual means of monthly rows.
 *
 * rscm_ens_define_running_mean.  source_var is a stored variable 1 .. V - 1 or a linear or energy-budget diagnostic defined earlier
 * on the handle: the first diagnostic whose source may be a diagnostic.  RSCM_ERR_INVALID for the input (0), a source that is itself
 * a running mean, an id that is not defined, a window outside 2 .. RSCM_RUNMEAN_MAX_WINDOW, an align other than the two constants,
 * step < 1, a fifth definition; RSCM_ERR_STATE while a staged select is in flight.  The definition takes one of the RSCM_DIAG_MAX
 * slots; ids, rscm_ens_n_diagnostics and rscm_ens_clear_diagnostics work as for rscm_ens_define_diagnostic, and every reader of a
 * diagnostic's rows takes the id.  rscm_ens_diagnostic and rscm_ens_diagnostic_quantity answer as for an energy-budget diagnostic: no
 * terms, quantity 0.  rscm_ens_diagnostic_running_mean reads the definition back; a diagnostic that is no running mean gives
 * source_var 0 (and 0 for the rest).  Any out pointer may be NULL.
 *
 * rscm_ens_compute_diagnostic forms the rows t_begin, t_begin + t_stride, ... < t_end, the last of them t_last.  t_stride must be a
 * multiple of step (RSCM_ERR_INVALID).  The source rows reach from t_begin - back * step to t_last + (W - 1 - back) * step at spacing
 * step, and every one of them -- those between two windows where t_stride > W * step included -- must lie on the axis
 * (RSCM_ERR_INVALID) and be computed and resident, in full storage, the window or the output store (RSCM_ERR_STATE, as for a
 * linear diagnostic's sources); the rows of a diagnostic source must be held and current at exactly those time indices
 * (RSCM_ERR_STATE).  Nothing is padded with NaN: a row whose window is incomplete is refused, not invented.  A refused compute
 * leaves the rows held before in place.
 *
 * Staleness.  The rows are a snapshot at the write epoch like every diagnostic's.  A running mean whose source reads the forcing
 * (RSCM_BUDGET_FORCING, RSCM_BUDGET_IMBALANCE) goes stale with the forcing as that source does.  Once formed the rows do not depend
 * on the source's store: computing the source again over another range leaves them valid. */
#define RSCM_RUNMEAN_MAX_WINDOW 64
#define RSCM_RUNMEAN_TRAILING 0
#define RSCM_RUNMEAN_CENTRED  1
RSCM_API int rscm_ens_define_running_mean(rscm_ens* h, int32_t source_var, int32_t window, int32_t align, int32_t step, int32_t* var_id_out);
RSCM_API int rscm_ens_diagnostic_running_mean(rscm_ens* h, int32_t var_id, int32_t* source_var, int32_t* window, int32_t* align, int32_t* step);

/* ---- posterior ensembles: systematic resampling and branching (ABI minor 10) --------------------- */
/* Exact statistics of the member weights, formed on the device in integers: *total = sum w, *n_nonzero = the members with w != 0,
 * *w_max = the largest weight, sum_sq = sum w^2 as a 128-bit integer {high word, low word}.  The sums are exact, so the sums of
 * shards are those of the whole ensemble (the effective sample size is total^2 / sum_sq).  No weights set: RSCM_ERR_STATE. */
RSCM_API int rscm_ens_weights_stats(rscm_ens* h, int64_t* total, int64_t* n_nonzero, int64_t* w_max, uint64_t sum_sq[2]);
/* Systematic resampling in integer form.  W = w_total is the summed weight of the whole ensemble, M the number of draws
 * (1 <= M <= 2^31), s an integer offset (0 <= s < W).  Draw k (0 <= k < M) sits at the integer point
 *     t_k = floor((s + k W) / M) = k q + floor((s + k r) / M),   W = q M + r,
 * and its ancestor is the member i with C[i-1] <= t_k < C[i], C the inclusive running sum of the weights in member order: a
 * zero-weight member is never drawn, member i is drawn floor(M w_i / W) or ceil(M w_i / W) times, ancestors are non-decreasing
 * in k.  This handle owns the weight range [w_before, w_before + W_local) of the global order (W_local = its own summed weight):
 * the call returns the contiguous run of draws k_first .. k_first + count - 1 whose points fall in that range and their LOCAL
 * member indices, int64, in a handle-owned device buffer *anc_dev that stays valid until the next rscm_ens_resample on the handle
 * or its destruction.  Every step is 64-bit integer arithmetic, so the runs of the handles of a split ensemble concatenate to the
 * draw of the whole ensemble on one handle, bit for bit.  One handle alone passes w_before = 0 and w_total = W_local and gets
 * count == M.  No weights set, or a staged select in flight: RSCM_ERR_STATE; w_total <= 0, M or s out of range, or
 * w_before + W_local > w_total: RSCM_ERR_INVALID (the buffer of an earlier call keeps its contents). */
RSCM_API int rscm_ens_resample(rscm_ens* h, int64_t M, int64_t s, int64_t w_before, int64_t w_total, int64_t* k_first, int64_t* count,
                               void** anc_dev);
/* The offset of a seeded draw, computed on the host so that every rank derives the same one: *s = floor(R W / 2^64), W = w_total,
 * R = (x1 << 32) | x0 of the Philox4x32-10 block (x0, x1, x2, x3) with key (seed & 0xFFFFFFFF, seed >> 32) and counter
 * (0, 0, 0, RSCM_RESAMPLE_STREAM_TAG).  w_total <= 0: RSCM_ERR_INVALID. */
#define RSCM_RESAMPLE_STREAM_TAG 0x52534D50u /* "RSMP" */
RSCM_API int rscm_gpu_resample_offset(uint64_t seed, int64_t w_total, int64_t* s);
/* Members [dst_offset, dst_offset + count) of dst become copies of src's members anc[0 .. count) (int64; host memory, or with
 * on_device != 0 device memory on the handles' device, e.g. the buffer of rscm_ens_resample) AT src's CURRENT TIME INDEX k:
 * every parameter row, row k of every stored variable and the rows before it that the kind looks back at, the status bytes and
 * the internal component state (ClimateUDEB: ocean columns, scalars and history rows 0..k; OceanCarbon: the flux ring).  dst
 * needs no rscm_ens_set_params of its own: it takes the configuration src derived from its structural rows.  Afterwards dst
 * stands at time index k with parameters and state rows set, sums parked by another run void and its member constants to be
 * re-formed.  Its forcing is NOT touched: the caller gives dst its own scenarios (rscm_ens_set_forcing) before or after.
 * dst must be of src's kind, on its device, with bitwise the same time bounds, the same mode and the same RK4 step sizes, else
 * RSCM_ERR_INVALID; any member count.  Both may be windowed (row k and the look-back rows must be resident in src, else
 * RSCM_ERR_STATE; dst's window is moved to k); RSCM_FLAG_NO_SERIES on either side: RSCM_ERR_INVALID.  The first call onto a
 * destination fixes k; later calls for other blocks, while dst still stands where the first call left it, must come from a
 * source at the same k with the same structural parameter rows (RSCM_ERR_STATE / RSCM_ERR_INVALID).  Members of dst that no
 * call has written keep whatever they held: running them is the caller's business.  A staged select in flight on either
 * handle: RSCM_ERR_STATE.  An ancestor outside [0, n_members of src): RSCM_ERR_INVALID, checked on the device before anything
 * is copied.  dst == src: RSCM_ERR_INVALID. */
RSCM_API int rscm_ens_gather_members(rscm_ens* dst, int64_t dst_offset, rscm_ens* src, const int64_t* anc, int32_t on_device, int64_t count);

/* Copy the parameter matrix back to the host as [P][N] (e.g. after rscm_ens_sample_lhs). */
RSCM_API int rscm_ens_get_params(rscm_ens* h, double* out_soa);

/* ---- device-side Latin hypercube ---------------------------------------------------------- */
/* Fill params[j][i] = low[j] + u * (high[j] - low[j]) with one sample per stratum and dimension:
 * u = (perm_j(g) + U_j(g)) / n_total, g = member_offset + i, perm_j a keyed bijection of
 * [0, n_total).  Counter-based, so ranks that own disjoint member blocks of one global
 * ensemble generate their rows with no communication. */
RSCM_API int rscm_ens_sample_lhs(rscm_ens* h, uint64_t seed, const double* low, const double* high,
                        int64_t member_offset, int64_t n_total);

/* The same hypercube through each row's own inverse CDF: a prior ensemble of Uniform, Normal and LogNormal rows, each optionally
 * truncated, drawn where it runs.  The seven arrays hold one entry per parameter row.  For member i (global id g = member_offset + i)
 * and row j, u is EXACTLY what rscm_ens_sample_lhs forms -- the same keys, the same Feistel stratum, u = stratum * interval +
 * U_j(g) * interval with interval = 1 / n_total -- so the strata of a row are those of rscm_ens_sample_lhs with the same seed.  Then
 *   RSCM_PRIOR_UNIFORM    x = a + u * (b - a): the bits of rscm_ens_sample_lhs with low = a, high = b; a == b fixes the row.  p0, p1,
 *                         lo, hi are not read.
 *   RSCM_PRIOR_NORMAL     t = p0 + u * (p1 - p0), moved into [2^-1022, 1 - 2^-53] (t below the first becomes it, t above the second
 *   RSCM_PRIOR_LOGNORMAL  becomes it: u = 0 and a sum that rounds to 1 stay away from -inf / +inf; Q gives -37.52 and 8.21 there);
 *                         z = Q(t), negated when kind carries RSCM_PRIOR_REFLECT; y = a + b * z; x = y (NORMAL: mean a, standard
 *                         deviation b) or x = exp(y), the device library's exp (LOGNORMAL: ln x has mean a, standard deviation b);
 *                         last x below lo becomes lo and x above hi becomes hi (the inverse of a rounded p0 may land an ulp outside
 *                         the support, and a log-prior must never see such a draw).  Without truncation p0 = 0, p1 = 1, lo = -inf,
 *                         hi = +inf.
 * Q is the standard normal quantile, Wichura's AS241 PPND16 on the double t: q = t - 1/2; for |q| <= 0.425 the central rational
 * q A(r) / B(r), r = 0.180625 - q q; otherwise p = min(t, 1 - t) (t if q < 0, else 1 - t), r = sqrt(-ln p) with ln written out in
 * + - * / (the logarithm of the forcing noise), the near-tail pair C, D at r - 1.6 for r <= 5 and the far-tail pair E, F at r - 5
 * beyond, the quotient negated for q < 0; one division.  Every operation is an f64 + - * / or sqrt rounded on its own, nothing is
 * fused, so a host restatement gives the same bits (tests/host_lhs_priors.py); on t = (2k + 1) 2^-53 it is the forcing noise's deviate
 * of the integer k (rscm_ens_set_forcing_noise).  The exponential of a LOGNORMAL row is the library's: within 2 ulp, not pinned.
 * p0 < p1 are the prior's CDF at the truncation bounds and the caller supplies them: Phi((lo - a) / b) and Phi((hi - a) / b) (ln lo,
 * ln hi for LOGNORMAL).  When the support lies above the centre (lo >= a, or ln lo >= a) the caller passes the SURVIVAL probabilities
 * p0 = Phi(-beta), p1 = Phi(-alpha) with alpha = (lo - a) / b, beta = (hi - a) / b, and the flag: the doubles are dense near 0 and not
 * near 1, so this keeps the resolution of a far upper tail (a standard normal truncated to [6, 8]: unreflected, 1e5 strata give 99 998
 * distinct values; reflected, all 1e5).  A reflected column DECREASES with its stratum; it holds one draw per stratum of the truncated
 * prior all the same, a Latin hypercube.
 * RSCM_ERR_INVALID: a NULL array; a member block outside the global ensemble; a kind that is none of the three, with or without the
 * flag; the flag on RSCM_PRIOR_UNIFORM; for NORMAL and LOGNORMAL b <= 0 or not finite, not 0 <= p0 < p1 <= 1, not lo <= hi; a row
 * marked [u] of the handle's kind that is not RSCM_PRIOR_UNIFORM with a == b; N2O's stratospheric delay that is not RSCM_PRIOR_UNIFORM
 * (its b sizes the look-back, as `high` does).  Afterwards the handle stands as rscm_ens_sample_lhs leaves it: parameters set, every
 * cache of the parameter block dropped (the per-member noise cache among them), the diagnostics' epoch moved. */
#define RSCM_PRIOR_UNIFORM 0
#define RSCM_PRIOR_NORMAL 1
#define RSCM_PRIOR_LOGNORMAL 2
#define RSCM_PRIOR_REFLECT 0x100 /* or-ed into NORMAL / LOGNORMAL: p0, p1 are survival probabilities, z = -Q(t) */
RSCM_API int rscm_ens_sample_lhs_priors(rscm_ens* h, uint64_t seed, const int32_t* kind, const double* a, const double* b,
                                        const double* p0, const double* p1, const double* lo, const double* hi,
                                        int64_t member_offset, int64_t n_total);

/* ---- pinned host buffers -------------------------------------------------------------------- */
/* Page-locked host memory for the buffers handed to rscm_ens_get_series / rscm_ens_set_params:
 * the copy then runs as one DMA at PCIe rate instead of being staged through pageable memory
 * (measured 601 MB of Ts: 11 GB/s into a fresh pageable buffer vs the pinned rate quoted in
 * DESIGN.md section 6). */
RSCM_API int rscm_gpu_host_alloc(int64_t n_bytes, void** out);
/* Blocking copy of n_bytes from a device address handed out by this library (rscm_ens_*_devptr,
 * rscm_ens_loglik_device) into host memory, for callers without a HIP runtime of their own. */
RSCM_API int rscm_gpu_copy_to_host(int32_t device_id, void* host, const void* device_ptr, int64_t n_bytes);
RSCM_API int rscm_gpu_copy_to_device(int32_t device_id, void* device_ptr, const void* host, int64_t n_bytes);
RSCM_API int rscm_gpu_host_free(void* p);

/* ---- diagnostics --------------------------------------------------------------------------- */
/* Whether this OceanCarbon ensemble's RSCM_MODE_FAST runs the recurrence, and the fit's deviation. */
RSCM_API int rscm_ens_ocean_fast_info(rscm_ens* h, int32_t* uses_recurrence, double* fit_error);
#ifdef __cplusplus
}
#endif
#endif /* RSCM_GPU_H */
