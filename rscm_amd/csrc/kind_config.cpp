// What the host builds from a kind's parameters and time axis: the RK4 sub-step tables, the configuration derived from the structural
// rows (configure_kind) and -- tabulated with the host's libm -- the concentration-only factors of GhgForcing (ghg_tables) and OceanCarbon's
// impulse response per lag (ocean_irf_table) with its mode fit.  Both are tolerance-parity kinds for that reason among others (tests/
// test_gpu_ghg.py, test_gpu_ocean.py state the bounds; test_gpu_links.py compares GhgForcing's table path with its device-library path).
#include "ens.hpp"

#include "udeb_tables.hpp"

constexpr double kTThreshold = 5e-3;  // crates/rscm-core/src/ivp/mod.rs:73

// ode_solvers Rk4::integrate: n = ceil((t1 - t0)/h) steps of t += h; the caller
// (get_last_step, ivp/mod.rs:90-102) asserts more than one stored point and
// |t_last - t1| < 5e-3.
static bool rk4_schedule(const std::vector<double>& bounds, double h, std::vector<int32_t>& nsub,
                  int32_t* bad_step)
{
    const size_t K = bounds.size() - 2;  // T-1 steps
    nsub.assign(K, 0);
    for (size_t n = 0; n < K; ++n) {
        const double t0 = bounds[n], t1 = bounds[n + 1];
        const double m = std::ceil((t1 - t0) / h);
        if (!(m >= 1.0) || m > 1e7) {
            *bad_step = (int32_t)n;
            return false;
        }
        double t = t0;
        for (int32_t s = 0; s < (int32_t)m; ++s) t = t + h;
        if (!(std::fabs(t - t1) < kTThreshold)) {
            *bad_step = (int32_t)n;
            return false;
        }
        nsub[n] = (int32_t)m;
    }
    return true;
}

// GhgForcing: everything that depends on the concentrations alone, once per scenario and year
// (forcing/ghg.rs:119-269 evaluates these per call; csrc/ghg.hip documents the factorisation).
// conc is [S][3][T] (CO2, CH4, N2O); the result [S][kGhgRows][T].
std::vector<double> ghg_tables(const double* conc, int32_t n_scen, int32_t T)
{
    std::vector<double> t((size_t)n_scen * rscm::kGhgRows * T);
    for (int32_t s = 0; s < n_scen; ++s) {
        const double* c = conc + (size_t)s * 3 * T;
        double* o = t.data() + (size_t)s * rscm::kGhgRows * T;
        for (int32_t n = 0; n < T; ++n) {
            const double co2 = c[n], ch4 = c[(size_t)T + n], n2o = c[(size_t)2 * T + n];
            o[(size_t)rscm::kGhgCo2 * T + n] = co2;
            o[(size_t)rscm::kGhgLnCo2 * T + n] = std::log(co2);
            o[(size_t)rscm::kGhgSqrtCo2 * T + n] = std::sqrt(co2);
            o[(size_t)rscm::kGhgSqrtCh4 * T + n] = std::sqrt(ch4);
            o[(size_t)rscm::kGhgSqrtN2o * T + n] = std::sqrt(n2o);
            o[(size_t)rscm::kGhgCh4P75 * T + n] = std::pow(ch4, 0.75);
            o[(size_t)rscm::kGhgCh4TimesP152 * T + n] = ch4 * std::pow(ch4, 1.52);
            o[(size_t)rscm::kGhgN2oP75 * T + n] = std::pow(n2o, 0.75);
            o[(size_t)rscm::kGhgN2oP152 * T + n] = std::pow(n2o, 1.52);
        }
    }
    return t;
}

// OceanCarbon: the scaled mixed-layer impulse response at lag k/12 years, k = 0 .. n-1
// (OceanCarbonParameters::irf + scale_irf, parameters/ocean_carbon.rs:202-216, with the IrfForm
// coefficient sets of the gfdl_3d / bern_2d / hilda presets, :88-196).  The expressions are the
// reference's, evaluated once per lag instead of once per (pulse, sub-step) pair.
struct OceanIrfForm { bool poly; int n; double c[8]; double tau[8]; };

static void ocean_forms(int model, const OceanIrfForm** early_out, const OceanIrfForm** late_out)
{
    typedef OceanIrfForm Form;
    static const Form gfdl_e = {true, 7, {1.0, -2.2617, 14.002, -48.770, 82.986, -67.527, 21.037}, {0}};
    static const Form gfdl_l = {false, 6, {0.01481, 0.019439, 0.038344, 0.066485, 0.24966, 0.70367},
                                {1.0e10, 347.55, 65.359, 15.281, 2.3488, 0.70177}};
    static const Form bern_e = {false, 6, {0.058648, 0.07515, 0.079338, 0.41413, 0.24845, 0.12429},
                                {1.0e10, 9.6218, 9.2364, 0.7603, 0.16294, 0.0032825}};
    static const Form bern_l = {false, 6, {0.01369, 0.012456, 0.026933, 0.026994, 0.036608, 0.06738},
                                {1.0e10, 331.54, 107.57, 38.946, 11.677, 10.515}};
    static const Form hilda_e = {false, 5, {0.12935, 0.24093, 0.24071, 0.17003, 0.21898},
                                 {1.0e10, 4.9792, 0.96083, 0.26936, 0.034569}};
    static const Form hilda_l = {false, 6, {0.022936, 0.035549, 0.037820, 0.089318, 0.13963, 0.24278},
                                 {1.0e10, 232.30, 68.736, 18.601, 5.2528, 1.2679}};
    *early_out = model == 1 ? &bern_e : model == 2 ? &hilda_e : &gfdl_e;
    *late_out = model == 1 ? &bern_l : model == 2 ? &hilda_l : &gfdl_l;
}

static std::vector<double> ocean_irf_table(int model, double irf_scale, double switch_time, int64_t n)
{
    typedef OceanIrfForm Form;
    const Form *early_p, *late_p;
    ocean_forms(model, &early_p, &late_p);
    const Form &early = *early_p, &late = *late_p;
    auto eval = [](const Form& f, double t) {
        if (f.poly) {
            double r = 0.0;
            for (int i = f.n - 1; i >= 0; --i) r = r * t + f.c[i];
            return r;
        }
        double s = 0.0;
        for (int i = 0; i < f.n; ++i) s += f.c[i] * std::exp(-t / f.tau[i]);
        return s;
    };
    std::vector<double> tab((size_t)std::max<int64_t>(n, 1), 0.0);
    for (int64_t k = 0; k < n; ++k) {
        const double t = (double)k * (1.0 / 12.0);
        const double raw = t < switch_time ? eval(early, t) : eval(late, t);
        tab[(size_t)k] = (raw * irf_scale) / (raw * irf_scale + 1.0 - raw);
    }
    return tab;
}

// RSCM_MODE_FAST for OceanCarbon: fit  tab[lag] ~ sum_q c_q d_q^(lag - near)  for lag in [near, H) with
// d_q = exp(-rate_q / 12) and rate_q in {1/tau_i} u {1/tau_i + 1/tau_j} of the late form (the scaled
// response s raw / (s raw + 1 - raw) expands in powers of (1 - s) raw; first and second order carry it to
// ~1e-11).  Linear least squares for the amplitudes by Householder QR in long double (the columns are
// strongly correlated: condition numbers of 1e8 and more).  Returns the largest deviation from the table
// over the window, or a negative number if the parameters do not allow the recurrence or the device could not sum the fit.
constexpr double kOceanFitTolerance = 5e-10;  // largest deviation of the fitted far response accepted for RSCM_MODE_FAST
// That deviation is evaluated in long double; the device forms sum_q c_q S_q in double, and at short windows the fit
// reproduces a far response of a few per cent with amplitudes of up to 1.5e4 and alternating sign.  What the sum then loses
// is governed by its condition, sum_q |c_q| G_q / sum_lag r(lag) with G_q = sum of d_q^k over the window's far lags (the
// weight a steady flux gives mode q): a fit whose condition is larger is declined like a short window, and FAST keeps the
// fused tiles.  Measured on an MI355X against the CPU oracle (130 members, 61 years, the windows 240 .. 720 months of the
// three presets in steps of 8; tests/test_gpu_ocean_edges.py has the set-up), largest relative deviation of FAST:
//   condition up to 3329: every 3D-GFDL window (240: 2170), 2D-BERN 480 .. 648, 672 and 704, HILDA from 640 on (640: 3329), and
//                         (over 600 years) the three presets at 6000 months (1.07 / 1106 / 1.00)     <= 4.95e-11
//   3508 .. 5551:         the other 2D-BERN 656 .. 720, HILDA 632, 624                               3.1e-11 .. 8.1e-11
//   beyond:               HILDA 600 (9612) 1.2e-10, 576 (1.9e4) 2.3e-10, 245 (2.4e4) 2.3e-10, 480 (3.3e5, max |c_q| 1.5e4) 4.9e-9
//   long windows (64 members, 600 years, against EXACT): 2D-BERN at 6000 months with irf_scale 0.5 / 0.7 / 1.3 (2.0e5 / 5.5e4 /
//                         2.2e4) 2.6e-9 / 6.7e-10 / 3.7e-10; at the default scale with 3000 / 1200 months (3.1e4 / 1.3e4) 4.1e-10 / 1.9e-10
// i.e. about 1.5e-14 times the condition.  max |c_q| alone does not order these: 2D-BERN at 6000 months has 670 in
// fast-decaying modes of small weight (1.6e-11), HILDA at 600 months 437 (1.2e-10).  3329 is the largest condition up to
// which every measured fit stays under a quarter of the 2e-10 that tests/test_gpu_ocean.py states for FAST (the headroom
// that test keeps); the limit sits a tenth below it, because the ill-conditioned amplitudes move by a per cent or so with
// the host's exp().
constexpr double kOceanFitMaxCondition = 3000.0;

static double ocean_fit_modes(const std::vector<double>& tab, int model, double switch_time, int64_t H, int32_t* near_out,
                              rscm::OceanModes* out)
{
    const OceanIrfForm *early, *late;
    ocean_forms(model, &early, &late);
    if (late->poly) return -1.0;
    const int64_t sw = (int64_t)std::ceil(switch_time * 12.0 - 1e-9);   // first lag of the late regime
    const int32_t near = sw <= 60 ? 60 : sw <= 120 ? 120 : 0;
    if (!near || H < 4 * (int64_t)near) return -1.0;   // short windows: the tiled convolution is cheap already
    std::vector<double> rates;
    auto add = [&](double r) {
        for (double x : rates)
            if (std::fabs(x - r) <= 1e-7 * (1.0 + std::fabs(r))) return;
        rates.push_back(r);
    };
    for (int i = 0; i < late->n; ++i) add(1.0 / late->tau[i]);
    for (int i = 0; i < late->n; ++i)
        for (int j = i; j < late->n; ++j) add(1.0 / late->tau[i] + 1.0 / late->tau[j]);
    std::sort(rates.begin(), rates.end());
    const int M = (int)rates.size();
    if (M > rscm::kOceanModes) return -1.0;
    const int64_t rows = std::min<int64_t>(H, 24000) - near;   // beyond 2000 years only the constant mode is left
    typedef long double ld;
    std::vector<ld> A((size_t)rows * M), b((size_t)rows);
    for (int64_t r = 0; r < rows; ++r) {
        for (int q = 0; q < M; ++q) A[(size_t)r * M + q] = std::exp(-(ld)rates[q] * (ld)r / 12.0L);
        b[(size_t)r] = tab[(size_t)(near + r)];
    }
    // Householder QR, applied to b on the fly
    std::vector<ld> R((size_t)M * M, 0.0L), v((size_t)rows);
    for (int k = 0; k < M; ++k) {
        ld norm = 0.0L;
        for (int64_t r = k; r < rows; ++r) norm += A[(size_t)r * M + k] * A[(size_t)r * M + k];
        norm = std::sqrt(norm);
        if (norm == 0.0L) return -1.0;
        const ld akk = A[(size_t)k * M + k];
        const ld alpha = akk > 0 ? -norm : norm;
        ld vnorm = 0.0L;
        for (int64_t r = k; r < rows; ++r) {
            v[(size_t)r] = A[(size_t)r * M + k] - (r == k ? alpha : 0.0L);
            vnorm += v[(size_t)r] * v[(size_t)r];
        }
        if (vnorm == 0.0L) return -1.0;
        for (int c = k; c < M; ++c) {
            ld dot = 0.0L;
            for (int64_t r = k; r < rows; ++r) dot += v[(size_t)r] * A[(size_t)r * M + c];
            const ld f = 2.0L * dot / vnorm;
            for (int64_t r = k; r < rows; ++r) A[(size_t)r * M + c] -= f * v[(size_t)r];
        }
        ld dot = 0.0L;
        for (int64_t r = k; r < rows; ++r) dot += v[(size_t)r] * b[(size_t)r];
        const ld f = 2.0L * dot / vnorm;
        for (int64_t r = k; r < rows; ++r) b[(size_t)r] -= f * v[(size_t)r];
        for (int c = k; c < M; ++c) R[(size_t)k * M + c] = A[(size_t)k * M + c];
    }
    std::vector<ld> x((size_t)M);
    for (int k = M - 1; k >= 0; --k) {
        ld acc = b[(size_t)k];
        for (int c = k + 1; c < M; ++c) acc -= R[(size_t)k * M + c] * x[(size_t)c];
        if (R[(size_t)k * M + k] == 0.0L) return -1.0;
        x[(size_t)k] = acc / R[(size_t)k * M + k];
    }
    *out = rscm::OceanModes{};
    for (int q = 0; q < M; ++q) {
        out->d[q] = (double)std::exp(-(ld)rates[q] / 12.0L);
        out->c[q] = (double)x[(size_t)q];
        out->e[q] = (double)std::exp(-(ld)rates[q] * (ld)(H - near) / 12.0L);
        if (!std::isfinite(out->c[q])) return -1.0;
    }
    out->n_modes = M;
    {   // the condition of the far sum (above)
        const ld n_far = (ld)(H - near);
        ld weighted = 0.0L, far = 0.0L;
        for (int q = 0; q < M; ++q) {
            const ld gain = rates[q] > 0.0 ? std::expm1(-(ld)rates[q] * n_far / 12.0L) / std::expm1(-(ld)rates[q] / 12.0L) : n_far;
            weighted += std::fabs((ld)out->c[q]) * gain;
        }
        for (int64_t lag = near; lag < H; ++lag) far += tab[(size_t)lag];
        if (!(weighted <= (ld)kOceanFitMaxCondition * far)) {
            *out = rscm::OceanModes{};
            return -1.0;
        }
    }
    // rates ascend, so the exit weights e_q descend: the first n_exit modes still matter at lag H
    out->n_exit = 0;
    for (int q = 0; q < M; ++q)
        if (std::fabs(out->c[q]) * out->e[q] >= 1e-19) out->n_exit = q + 1;
    for (int q = out->n_exit; q < rscm::kOceanModes; ++q) out->e[q] = 0.0;  // the kernel applies a fixed number of exit terms
    // the fit as the device will evaluate it (double coefficients), against the whole window
    double worst = 0.0;
    for (int64_t lag = near; lag < H; ++lag) {
        ld acc = 0.0L;
        for (int q = 0; q < M; ++q) acc += (ld)out->c[q] * std::exp(-(ld)rates[q] * (ld)(lag - near) / 12.0L);
        worst = std::max(worst, std::fabs((double)acc - tab[(size_t)lag]));
    }
    *near_out = near;
    return worst;
}

int refresh_schedule(rscm_ens* h)
{
    if (!h->schedule_dirty) return RSCM_OK;
    if (h->kind != RSCM_KIND_TWO_LAYER && h->kind != RSCM_KIND_COUPLED && h->kind != RSCM_KIND_CARBON_CYCLE) {  // no RK4 component
        h->schedule_dirty = false;
        return RSCM_OK;
    }
    int32_t bad = -1;
    if (h->kind == RSCM_KIND_CARBON_CYCLE) {
        h->nsub_tl.assign(h->bounds.size() - 2, 1);
    } else if (!rk4_schedule(h->bounds, h->h_tl, h->nsub_tl, &bad))
        return fail(RSCM_ERR_TIME_AXIS,
                    "TwoLayer RK4 step %.17g does not land on the end of model step %d "
                    "([%.17g, %.17g]) within 5e-3 (the reference panics in get_last_step)",
                    h->h_tl, bad, h->bounds[bad], h->bounds[bad + 1]);
    if (h->kind == RSCM_KIND_TWO_LAYER) h->year_facts.set_schedule(h->nsub_tl.data(), h->nsub_tl.size());
    HIPCHK(hipMemcpyAsync(h->d_nsub_tl, h->nsub_tl.data(), h->nsub_tl.size() * sizeof(int32_t),
                          hipMemcpyHostToDevice, h->stream));
    if (h->kind == RSCM_KIND_COUPLED || h->kind == RSCM_KIND_CARBON_CYCLE) {
        if (!rk4_schedule(h->bounds, h->h_cc, h->nsub_cc, &bad))
            return fail(RSCM_ERR_TIME_AXIS,
                        "CarbonCycle RK4 step %.17g does not land on the end of model step %d "
                        "within 5e-3 (the reference panics in get_last_step)", h->h_cc, bad);
        HIPCHK(hipMemcpyAsync(h->d_nsub_cc, h->nsub_cc.data(), h->nsub_cc.size() * sizeof(int32_t),
                              hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));  // host vectors may be rebuilt afterwards
    h->schedule_dirty = false;
    return RSCM_OK;
}

// OceanCarbon: the response table and the loop bounds from its structural rows (uniform: configure_kind has checked)
static int configure_ocean(rscm_ens* h, const ParamView& row, bool state_replaced)
{
    const double model = row.at(RSCM_OC_P_MODEL), steps = row.at(RSCM_OC_P_STEPS_PER_YEAR);
    const double max_hist = row.at(RSCM_OC_P_MAX_HISTORY_MONTHS);
    if (model != 0.0 && model != 1.0 && model != 2.0)
        return fail(RSCM_ERR_INVALID, "OceanCarbon model must be 0 (3D-GFDL), 1 (2D-BERN) or 2 (HILDA), got %g", model);
    if (steps != 12.0) return fail(RSCM_ERR_INVALID, "OceanCarbon on the device supports steps_per_year = 12, got %g", steps);
    if (!(max_hist >= 0.0) || max_hist > 1e7 || max_hist != std::floor(max_hist))
        return fail(RSCM_ERR_INVALID, "max_history_months must be a non-negative integer, got %g", max_hist);
    const std::vector<double> tab = ocean_irf_table((int)model, row.at(RSCM_OC_P_IRF_SCALE),
                                                    row.at(RSCM_OC_P_IRF_SWITCH_TIME), (int64_t)max_hist);
    HIPCHK(hipStreamSynchronize(h->stream));
    // The two small tables are built aside and moved in at the end, with the host's facts about them, once nothing can fail any
    // more: until then -- and after a failure or the refusal below -- the old response is in force, whole.
    rscm::DevBuf<double> d_irf, d_mode_table;
    HIPCHK(d_irf.alloc(tab.size()));
    HIPCHK(hipMemcpy(d_irf, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    // The flux history is a ring: the convolution reads at most max_history_months pulses back, a tile writes
    // up to 48 new ones before it is done reading (ocean.hip), the O(T) recurrence reads the pulse that leaves
    // the window.  On a monthly axis that is 48 KB per member instead of 864 KB (108 000 pulses).
    const int64_t all_pulses = (int64_t)(h->T - 1) * 12;
    const int64_t ring = (((int64_t)max_hist + 60 + 11) / 12) * 12;
    const int64_t rows = std::min(all_pulses, ring);
    if (!h->d_ocean_hist || rows != h->ocean_hist_rows) {
        // the ring holds the pulses of the steps taken so far (internal state): a new length mid-run would
        // throw them away and leave the next convolution reading whatever the new allocation contains
        if (h->d_ocean_hist && h->time_index > 0 && !state_replaced)
            return fail(RSCM_ERR_STATE, "max_history_months changes the flux-history ring from %lld to %lld rows at time index %d: "
                        "rewind (rscm_ens_rewind / rscm_ens_set_time_index(0)) before changing it", (long long)h->ocean_hist_rows,
                        (long long)rows, h->time_index);
        // too large to hold twice: the old ring goes first, and the handle is not ready until this call has come through
        h->ocean_ready = false;
        h->ocean_hist_rows = 0;
        if (int rc = alloc_or_fail(h->d_ocean_hist, (size_t)rows * h->N, false, "flux history of %lld members x %lld months", (long long)h->N, (long long)rows))
            return rc;
        // cleared on the handle's own stream, where every later use of the ring is.  Measured: after a synchronous hipMemset, which
        // goes through the null stream, with nothing else issued there afterwards, a process that had run for a while did not get the
        // ring back from hipFree, handle after handle (tests/test_gpu_handle_teardown.py); presumably that fill command kept a reference
        HIPCHK(hipMemsetAsync(h->d_ocean_hist, 0, (size_t)rows * h->N * sizeof(double), h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->ocean_hist_rows = rows;
    }
    if (int rc = alloc_or_fail(h->d_ocean_partial, (size_t)(rscm::kOceanSplitYears - 1) * 12 * h->N, true, "split-tile sums of %lld members", (long long)h->N))
        return rc;
    rscm::OceanModes modes{};
    int32_t near = 0;
    const double fit_error = ocean_fit_modes(tab, (int)model, row.at(RSCM_OC_P_IRF_SWITCH_TIME), (int64_t)max_hist, &near, &modes);
    const bool recur_ok = fit_error >= 0.0 && fit_error <= kOceanFitTolerance;
    if (recur_ok)
        if (int rc = alloc_or_fail(h->d_ocean_mode_state, (size_t)rscm::kOceanModes * h->N, true, "mode sums of %lld members", (long long)h->N)) return rc;
    if (recur_ok) {
        HIPCHK(d_mode_table.alloc((size_t)3 * rscm::kOceanModes));
        double t3[3 * rscm::kOceanModes];
        for (int q = 0; q < rscm::kOceanModes; ++q) {
            t3[q] = modes.d[q];
            t3[rscm::kOceanModes + q] = modes.c[q];
            t3[2 * rscm::kOceanModes + q] = modes.e[q];
        }
        HIPCHK(hipMemcpy(d_mode_table, t3, sizeof t3, hipMemcpyHostToDevice));
        h->d_ocean_mode_table = std::move(d_mode_table);
    }
    h->d_ocean_irf = std::move(d_irf);
    h->ocean_forget_partial_sums();  // sums parked under another response table are void
    h->ocean_steps = 12;
    h->ocean_max_hist = (int64_t)max_hist;
    h->ocean_modes = modes;
    h->ocean_near = near;
    h->ocean_fit_error = fit_error;
    h->ocean_recur_ok = recur_ok;
    h->ocean_ready = true;
    return RSCM_OK;
}

// ClimateUDEB: one set of geometry tables and one unrolled column length from its structural rows (uniform: configure_kind has checked)
static int configure_udeb(rscm_ens* h, const ParamView& row, bool state_replaced)
{
    const double nl = row.at(RSCM_UD_P_N_LAYERS), steps = row.at(RSCM_UD_P_STEPS_PER_YEAR);
    // mod.rs:162-165: "invalid n_layers: must be >= 2".  Up to 64 layers a member's columns stay in registers + LDS (20 / 30 / 40 / 50
    // with the count compiled in, the others in the next capacity's runtime-count instance); more run the columns-in-HBM kernel
    // (csrc/udeb_any_body.hpp).  The upper bound is this library's.
    if (nl != std::floor(nl) || nl < 2.0) return fail(RSCM_ERR_INVALID, "invalid n_layers: must be >= 2, got %g", nl);
    if (nl > 4096.0) return fail(RSCM_ERR_INVALID, "n_layers = %g: the device path takes at most 4096 ocean layers", nl);
    if (h->udeb_ready && (int32_t)nl != h->udeb_n_layers && h->time_index > 0 && !state_replaced)
        return fail(RSCM_ERR_STATE, "n_layers changes the ocean columns (internal state) at time index %d: rewind first", h->time_index);
    if (row.at(RSCM_UD_P_OCEAN_TEMP_PROFILE) != 2.0)
        return fail(RSCM_ERR_INVALID, "ClimateUDEB on the device supports ocean_temp_profile = 2 (CMIP5)");
    if (!(steps >= 1.0) || steps > 1000.0 || steps != std::floor(steps))
        return fail(RSCM_ERR_INVALID, "steps_per_year must be a positive integer, got %g", steps);
    const double eff = row.at(RSCM_UD_P_EFFICACY_APPLY);
    if (eff != 0.0 && eff != 1.0 && eff != 2.0) return fail(RSCM_ERR_INVALID, "efficacy_apply must be 0, 1 or 2");
    // From here on the handle's facts and buffers change one by one: it is not ready until all of them stand, so a failed
    // allocation or copy below leaves nothing that would launch on a missing column or a table of another layer count
    h->udeb_ready = false;
    h->udeb_n_layers = (int32_t)nl;
    h->udeb_steps = (int32_t)steps;
    h->udeb_land_hc = row.at(RSCM_UD_P_LAND_HC_ENABLED) != 0.0 ? 1 : 0;
    h->udeb_efficacy = (int32_t)eff;
    const std::vector<double> t = rscm::udeb_tables(h->udeb_n_layers, row.at(RSCM_UD_P_MIXED_LAYER_DEPTH),
                                                    row.at(RSCM_UD_P_LAYER_THICKNESS), row.at(RSCM_UD_P_DEPTH_DEPENDENT_AREA));
    h->udeb_tables = t;
    {   // the backwards walk of adjusted_ecs() (mod.rs:302-331) over the time axis, once per year
        const double period = row.at(RSCM_UD_P_FEEDBACK_CUMT_PERIOD);
        std::vector<int32_t> kfull((size_t)h->T, 0);
        std::vector<double> partw((size_t)h->T, 0.0);
        for (int32_t n = 0; n < h->T; ++n) {
            double years_remaining = period;
            int32_t kf = n;
            double pw = 0.0;
            for (int32_t k = n - 1; k >= 0; --k) {
                if (years_remaining <= 0.0) break;
                const double dt = h->bounds[k + 1] - h->bounds[k];
                if (dt <= years_remaining) {
                    kf = k;
                    years_remaining -= dt;
                } else {
                    pw = years_remaining / dt;
                    years_remaining = 0.0;
                }
            }
            kfull[n] = kf;
            partw[n] = pw;
        }
        HIPCHK(h->d_win_kfull.reserve((size_t)h->T));
        HIPCHK(h->d_win_partw.reserve((size_t)h->T));
        HIPCHK(hipMemcpyAsync(h->d_win_kfull, kfull.data(), kfull.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_win_partw, partw.data(), partw.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    {   // the columns: room for 50 layers at least (any of the unrolled kernels), more if asked for.  Too large to hold twice: they
        // grow in place (a failure leaves the handle not ready, above)
        const int32_t want = std::max(rscm::kUdebMaxOnChipLayers, h->udeb_n_layers);
        if (int rc = alloc_or_fail(h->d_ocean, (size_t)2 * want * h->N, true, "ocean columns of %d layers x %lld members", want, (long long)h->N)) return rc;
    }
    if (!rscm::udeb_layers_fixed(h->udeb_n_layers)) {   // the columns-in-HBM kernel (more than 64 layers; up to 64 only on request, as the
        // yardstick of the runtime-count kernels -- rscm_gpu_set_udeb_variant(3)): its c' array and its table live in device memory
        if (int rc = alloc_or_fail(h->d_udeb_work, (size_t)h->udeb_n_layers * h->N, true, "work array of %d layers x %lld members", h->udeb_n_layers, (long long)h->N))
            return rc;
        // (room for the largest on-chip capacity: the unrolled sweeps request the table rows of their whole capacity, and the rows past
        // the layer count must read as zeros -- they are what makes those rows of the column exact no-ops)
        // The table is rewritten where it stands while it is large enough; a larger one is built aside and moved in once it is written
        rscm::DevBuf<double> d_grown;
        const size_t table_elems = (size_t)6 * std::max(h->udeb_n_layers, (int32_t)rscm::kUdebDevTableRows);
        if (h->d_udeb_tables.size() < table_elems) HIPCHK(d_grown.alloc(table_elems));
        const rscm::DevBuf<double>& d_table = d_grown ? d_grown : h->d_udeb_tables;
        HIPCHK(hipMemsetAsync(d_table, 0, d_table.size() * sizeof(double), h->stream));
        HIPCHK(hipMemcpyAsync(d_table, h->udeb_tables.data(), h->udeb_tables.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (d_grown) h->d_udeb_tables = std::move(d_grown);
    }
    h->udeb_ready = true;
    return RSCM_OK;
}

int configure_kind(rscm_ens* h, const ParamView& p, bool state_replaced)
{
    for (const rscm::StructuralRow& s : rscm::kStructuralRows)
        if (s.kind == h->kind && s.uniform)
            for (int64_t i = 1; i < p.n_check; ++i)
                if (p.at(s.row, i) != p.at(s.row, 0))
                    return fail(RSCM_ERR_INVALID, "%s parameter row %d (%s) must be the same for every member", h->info().name, s.row, s.name);
    if (h->kind == RSCM_KIND_UDEB) return configure_udeb(h, p, state_replaced);
    if (h->kind == RSCM_KIND_OCEAN_CARBON) return configure_ocean(h, p, state_replaced);
    if (h->kind == RSCM_KIND_GHG_FORCING) {  // one forcing method per ensemble (one kernel instance)
        const double m = p.at(RSCM_GH_P_METHOD);
        if (m != 0.0 && m != 1.0) return fail(RSCM_ERR_INVALID, "GhgForcing method must be 0 (Ipcctar) or 1 (Olbl), got %g", m);
        h->ghg_method = (int32_t)m;
    }
    return RSCM_OK;
}

extern "C" {

int rscm_gpu_ocean_fit_selftest(int32_t model, double irf_scale, double irf_switch_time, int64_t max_history_months,
                                double* max_error, int32_t* n_modes, int32_t* near_lags, int32_t* n_exit, double* max_abs_coefficient)
{
    GUARD_BEGIN
    if (!max_error || !n_modes || !near_lags || !n_exit) return fail(RSCM_ERR_INVALID, "NULL output");
    if (model < 0 || model > 2 || max_history_months < 1 || max_history_months > 10000000)
        return fail(RSCM_ERR_INVALID, "bad model or history length");
    const std::vector<double> tab = ocean_irf_table(model, irf_scale, irf_switch_time, max_history_months);
    rscm::OceanModes m{};
    int32_t near = 0;
    *max_error = ocean_fit_modes(tab, model, irf_switch_time, max_history_months, &near, &m);
    *n_modes = m.n_modes;
    *near_lags = near;
    *n_exit = m.n_exit;
    if (max_abs_coefficient) {
        *max_abs_coefficient = 0.0;
        for (int q = 0; q < m.n_modes; ++q) *max_abs_coefficient = std::max(*max_abs_coefficient, std::fabs(m.c[q]));
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_ocean_fast_info(rscm_ens* h, int32_t* uses_recurrence, double* fit_error)
{
    NEED(h);
    if (h->kind != RSCM_KIND_OCEAN_CARBON || !h->ocean_ready) return fail(RSCM_ERR_STATE, "not a configured OceanCarbon ensemble");
    if (uses_recurrence) *uses_recurrence = h->ocean_recur_ok ? 1 : 0;
    if (fit_error) *fit_error = h->ocean_fit_error;
    return RSCM_OK;
}

}  // extern "C"
