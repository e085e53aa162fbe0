// C-ABI layer of the MI355X ensemble runner: handle management, validation mirroring the
// reference's error behaviour, host<->device plumbing.  The arithmetic of the hot path lives in
// the .hip kernels.  Two things are tabulated here, once per scenario / parameter set, with the
// host's libm: the concentration-only factors of GhgForcing (ghg_tables: ln, sqrt, pow of the shared
// scenario rows) and OceanCarbon's impulse response per lag (ocean_irf_table).  Both kinds are
// tolerance-parity kinds for that reason among others (tests/test_gpu_ghg.py, tests/test_gpu_ocean.py
// state the bounds; GhgForcing's linked-input path evaluates the same factors with the device
// library and is compared with the table path in tests/test_gpu_links.py).
#include "ens.hpp"
#include "experiment_env.hpp"

#include "udeb_tables.hpp"

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

namespace {

constexpr double kTThreshold = 5e-3;  // crates/rscm-core/src/ivp/mod.rs:73

// ode_solvers Rk4::integrate: n = ceil((t1 - t0)/h) steps of t += h; the caller
// (get_last_step, ivp/mod.rs:90-102) asserts more than one stored point and
// |t_last - t1| < 5e-3.
bool rk4_schedule(const std::vector<double>& bounds, double h, std::vector<int32_t>& nsub,
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

}  // namespace

// GhgForcing: everything that depends on the concentrations alone, once per scenario and year
// (forcing/ghg.rs:119-269 evaluates these per call; csrc/ghg.hip documents the factorisation).
// conc is [S][3][T] (CO2, CH4, N2O); the result [S][kGhgRows][T].
static std::vector<double> ghg_tables(const double* conc, int32_t n_scen, int32_t T)
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
// over the window, or a negative number if the parameters do not allow the recurrence.
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

constexpr double kOceanFitTolerance = 5e-10;  // largest deviation of the fitted far response accepted for RSCM_MODE_FAST

static_assert(rscm::kNoiseStreamTag == RSCM_NOISE_STREAM_TAG, "the noise stream's tag in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(RSCM_NOISE_STREAM_TAG != 0x57A7u && RSCM_NOISE_STREAM_TAG != 0xACCEu && RSCM_NOISE_STREAM_TAG != 0x5EEDu &&
                  RSCM_NOISE_STREAM_TAG != 0xA5A5u && RSCM_NOISE_STREAM_TAG != RSCM_RESAMPLE_STREAM_TAG,
              "every Philox stream of the library has a tag of its own");
static_assert(rscm::kMaxForcingComponents == RSCM_TL_MAX_COMPONENTS && rscm::kTwoLayerCoeff0 == RSCM_TL_P_COEFF0 && RSCM_TL_P_COEFF0 == RSCM_TL_NPARAMS,
              "the mix handle's constants in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(rscm::kKindOzoneForcing == RSCM_KIND_OZONE_FORCING && rscm::kKindAerosolDirect == RSCM_KIND_AEROSOL_DIRECT &&
                  rscm::kKindAerosolIndirect == RSCM_KIND_AEROSOL_INDIRECT && rscm::kKindCh4Chemistry == RSCM_KIND_CH4_CHEMISTRY &&
                  rscm::kKindN2oChemistry == RSCM_KIND_N2O_CHEMISTRY && rscm::kKindCo2Budget == RSCM_KIND_CO2_BUDGET &&
                  rscm::kKindTerrestrialCarbon == RSCM_KIND_TERRESTRIAL_CARBON && rscm::kKindFourBoxOhu == RSCM_KIND_FOURBOX_OHU &&
                  rscm::kKindOspp == RSCM_KIND_OSPP && rscm::kKindCarbonCycle == RSCM_KIND_CARBON_CYCLE &&
                  rscm::kKindCo2Erf == RSCM_KIND_CO2_ERF && rscm::kKindAggregate == RSCM_KIND_AGGREGATE,
              "rscm_device.hpp and include/rscm_gpu.h disagree on a kind value");

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

namespace {

// OceanCarbon: the rows that select the response table and the loop bounds must be uniform.
template <typename Row>
int configure_ocean(rscm_ens* h, int64_t n_check, Row row)
{
    static const int structural[] = {RSCM_OC_P_MODEL, RSCM_OC_P_IRF_SCALE, RSCM_OC_P_STEPS_PER_YEAR,
                                     RSCM_OC_P_MAX_HISTORY_MONTHS, RSCM_OC_P_IRF_SWITCH_TIME};
    for (int j : structural)
        for (int64_t i = 1; i < n_check; ++i)
            if (row(j, i) != row(j, 0))
                return fail(RSCM_ERR_INVALID, "OceanCarbon parameter row %d must be the same for every member", j);
    const double model = row(RSCM_OC_P_MODEL, 0), steps = row(RSCM_OC_P_STEPS_PER_YEAR, 0);
    const double max_hist = row(RSCM_OC_P_MAX_HISTORY_MONTHS, 0);
    if (model != 0.0 && model != 1.0 && model != 2.0)
        return fail(RSCM_ERR_INVALID, "OceanCarbon model must be 0 (3D-GFDL), 1 (2D-BERN) or 2 (HILDA), got %g", model);
    if (steps != 12.0) return fail(RSCM_ERR_INVALID, "OceanCarbon on the device supports steps_per_year = 12, got %g", steps);
    if (!(max_hist >= 0.0) || max_hist > 1e7 || max_hist != std::floor(max_hist))
        return fail(RSCM_ERR_INVALID, "max_history_months must be a non-negative integer, got %g", max_hist);
    const std::vector<double> tab = ocean_irf_table((int)model, row(RSCM_OC_P_IRF_SCALE, 0),
                                                    row(RSCM_OC_P_IRF_SWITCH_TIME, 0), (int64_t)max_hist);
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
        if (h->d_ocean_hist && h->time_index > 0)
            return fail(RSCM_ERR_STATE, "max_history_months changes the flux-history ring from %lld to %lld rows at time index %d: "
                        "rewind (rscm_ens_rewind / rscm_ens_set_time_index(0)) before changing it", (long long)h->ocean_hist_rows,
                        (long long)rows, h->time_index);
        // too large to hold twice: the old ring goes first, and the handle is not ready until this call has come through
        h->ocean_ready = false;
        h->ocean_hist_rows = 0;
        const hipError_t e = h->d_ocean_hist.alloc((size_t)rows * h->N);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? RSCM_ERR_NOMEM : RSCM_ERR_DEVICE,
                        "flux history of %lld members x %lld months: %s", (long long)h->N, (long long)rows, hipGetErrorString(e));
        // cleared on the handle's own stream, where every later use of the ring is.  Measured: after a synchronous hipMemset, which
        // goes through the null stream, with nothing else issued there afterwards, a process that had run for a while did not get the
        // ring back from hipFree, handle after handle (tests/test_gpu_handle_teardown.py); presumably that fill command kept a reference
        HIPCHK(hipMemsetAsync(h->d_ocean_hist, 0, (size_t)rows * h->N * sizeof(double), h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->ocean_hist_rows = rows;
    }
    if (!h->d_ocean_partial) {
        const hipError_t e = h->d_ocean_partial.alloc((size_t)(rscm::kOceanSplitYears - 1) * 12 * h->N);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? RSCM_ERR_NOMEM : RSCM_ERR_DEVICE, "split-tile sums of %lld members: %s",
                        (long long)h->N, hipGetErrorString(e));
    }
    rscm::OceanModes modes{};
    int32_t near = 0;
    const double fit_error = ocean_fit_modes(tab, (int)model, row(RSCM_OC_P_IRF_SWITCH_TIME, 0), (int64_t)max_hist, &near, &modes);
    const bool recur_ok = fit_error >= 0.0 && fit_error <= kOceanFitTolerance;
    if (recur_ok && !h->d_ocean_mode_state) {
        const hipError_t e = h->d_ocean_mode_state.alloc((size_t)rscm::kOceanModes * h->N);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? RSCM_ERR_NOMEM : RSCM_ERR_DEVICE, "mode sums of %lld members: %s", (long long)h->N, hipGetErrorString(e));
    }
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

// ClimateUDEB: the structural parameters must be uniform over the ensemble (one set of geometry
// tables, one unrolled column length); `row(j, i)` reads parameter j of member i.
template <typename Row>
int configure_udeb(rscm_ens* h, int64_t n_check, Row row)
{
    static const int structural[] = {RSCM_UD_P_N_LAYERS, RSCM_UD_P_MIXED_LAYER_DEPTH, RSCM_UD_P_LAYER_THICKNESS,
                                     RSCM_UD_P_DEPTH_DEPENDENT_AREA, RSCM_UD_P_LAND_HC_ENABLED,
                                     RSCM_UD_P_EFFICACY_APPLY, RSCM_UD_P_OCEAN_TEMP_PROFILE, RSCM_UD_P_STEPS_PER_YEAR,
                                     RSCM_UD_P_FEEDBACK_CUMT_PERIOD};
    for (int j : structural)
        for (int64_t i = 1; i < n_check; ++i)
            if (row(j, i) != row(j, 0))
                return fail(RSCM_ERR_INVALID, "ClimateUDEB parameter row %d must be the same for every member", j);
    const double nl = row(RSCM_UD_P_N_LAYERS, 0), steps = row(RSCM_UD_P_STEPS_PER_YEAR, 0);
    // mod.rs:162-165: "invalid n_layers: must be >= 2".  Up to 64 layers a member's columns stay in registers + LDS (20 / 30 / 40 / 50
    // with the count compiled in, the others in the next capacity's runtime-count instance); more run the columns-in-HBM kernel
    // (csrc/udeb_any_body.hpp).  The upper bound is this library's.
    if (nl != std::floor(nl) || nl < 2.0) return fail(RSCM_ERR_INVALID, "invalid n_layers: must be >= 2, got %g", nl);
    if (nl > 4096.0) return fail(RSCM_ERR_INVALID, "n_layers = %g: the device path takes at most 4096 ocean layers", nl);
    if (h->udeb_ready && (int32_t)nl != h->udeb_n_layers && h->time_index > 0)
        return fail(RSCM_ERR_STATE, "n_layers changes the ocean columns (internal state) at time index %d: rewind first", h->time_index);
    if (row(RSCM_UD_P_OCEAN_TEMP_PROFILE, 0) != 2.0)
        return fail(RSCM_ERR_INVALID, "ClimateUDEB on the device supports ocean_temp_profile = 2 (CMIP5)");
    if (!(steps >= 1.0) || steps > 1000.0 || steps != std::floor(steps))
        return fail(RSCM_ERR_INVALID, "steps_per_year must be a positive integer, got %g", steps);
    const double eff = row(RSCM_UD_P_EFFICACY_APPLY, 0);
    if (eff != 0.0 && eff != 1.0 && eff != 2.0) return fail(RSCM_ERR_INVALID, "efficacy_apply must be 0, 1 or 2");
    // From here on the handle's facts and buffers change one by one: it is not ready until all of them stand, so a failed
    // allocation or copy below leaves nothing that would launch on a missing column or a table of another layer count
    h->udeb_ready = false;
    h->udeb_n_layers = (int32_t)nl;
    h->udeb_steps = (int32_t)steps;
    h->udeb_land_hc = row(RSCM_UD_P_LAND_HC_ENABLED, 0) != 0.0 ? 1 : 0;
    h->udeb_efficacy = (int32_t)eff;
    const std::vector<double> t = rscm::udeb_tables(h->udeb_n_layers, row(RSCM_UD_P_MIXED_LAYER_DEPTH, 0),
                                                    row(RSCM_UD_P_LAYER_THICKNESS, 0), row(RSCM_UD_P_DEPTH_DEPENDENT_AREA, 0));
    h->udeb_tables = t;
    {   // the backwards walk of adjusted_ecs() (mod.rs:302-331) over the time axis, once per year
        const double period = row(RSCM_UD_P_FEEDBACK_CUMT_PERIOD, 0);
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
        const hipError_t e = h->d_ocean.reserve((size_t)2 * want * h->N);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? RSCM_ERR_NOMEM : RSCM_ERR_DEVICE, "ocean columns of %d layers x %lld members: %s", want,
                        (long long)h->N, hipGetErrorString(e));
    }
    if (!rscm::udeb_layers_fixed(h->udeb_n_layers)) {   // the columns-in-HBM kernel (more than 64 layers; up to 64 only on request, as the
        // yardstick of the runtime-count kernels -- rscm_gpu_set_udeb_variant(3)): its c' array and its table live in device memory
        const hipError_t e = h->d_udeb_work.reserve((size_t)h->udeb_n_layers * h->N);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? RSCM_ERR_NOMEM : RSCM_ERR_DEVICE, "work array of %d layers x %lld members: %s",
                        h->udeb_n_layers, (long long)h->N, hipGetErrorString(e));
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

}  // namespace

// ---- windowed series -----------------------------------------------------------------------
// Back to the start of the axis: window at row 0, the saved initial rows put back, the rest NaN if
// asked (a fresh collection) or if a consumer may read rows this producer has not written yet.
int window_reset(rscm_ens* h, bool clear)
{
    if (!h->windowed) return RSCM_OK;
    h->win0 = 0;
    if (h->row0_saved)
        HIPCHK(rscm::launch_scatter_rows(h->d_series, h->N, h->rows, 0, nullptr, h->V - 1, h->d_row0, 1, 0, h->stream));
    if (clear || h->read_ahead)
        HIPCHK(rscm::launch_fill_rows(h->d_series, h->N, h->rows, h->V - 1, 1, std::numeric_limits<double>::quiet_NaN(), h->stream));
    return RSCM_OK;
}

// Move the window forward to start at new_win0, keeping the rows both windows share.
int window_slide(rscm_ens* h, int32_t new_win0)
{
    const int32_t shift = new_win0 - h->win0;
    if (!h->windowed || shift <= 0) return RSCM_OK;
    const int32_t cnt = std::max(0, h->rows - shift);  // rows still inside the new window
    if (h->defer && shift >= cnt) {
        // a lock-step run: the move is issued with every other handle's at the end of the model step; until then this handle's
        // base address and win0 stay what they are (consumers later in the step read the rows where they still lie)
        for (const auto& pending : h->defer->new_win0)
            if (pending.first == h) return fail(RSCM_ERR_STATE, "two window slides of one handle in one lock-step flush");
        if (cnt > 0) {
            rscm::WindowOp op{};
            op.buf = h->d_series; op.N = h->N; op.R = h->rows; op.n_vars = h->V - 1; op.kind = 0; op.shift = shift; op.keep = cnt;
            h->defer->first.push_back(op);
        }
        if (h->read_ahead || cnt == 0) {
            rscm::WindowOp op{};
            op.buf = h->d_series; op.N = h->N; op.R = h->rows; op.n_vars = h->V - 1; op.kind = 2; op.fill_from = cnt;
            h->defer->second.push_back(op);
        }
        h->defer->new_win0.emplace_back(h, new_win0);
        return RSCM_OK;
    }
    HIPCHK(rscm::launch_slide_rows(h->d_series, h->N, h->rows, h->V - 1, shift, cnt, h->stream));
    if (h->read_ahead || cnt == 0)
        HIPCHK(rscm::launch_fill_rows(h->d_series, h->N, h->rows, h->V - 1, cnt, std::numeric_limits<double>::quiet_NaN(), h->stream));
    h->win0 = new_win0;
    return RSCM_OK;
}

// Re-position the window for a stepper that is put at time index k from outside (checkpoint restore):
// the contents are the caller's to fill in (rscm_ens_set_state); everything is NaN until then.
static int window_seek(rscm_ens* h, int32_t k)
{
    if (!h->windowed) return RSCM_OK;
    if (k == 0) return window_reset(h, true);
    const int32_t w0 = std::max(0, k - h->keep_rows() + 1);
    if (k >= h->win0 && k < h->win0 + h->rows - 1 && w0 >= h->win0) return window_slide(h, w0);
    HIPCHK(rscm::launch_fill_rows(h->d_series, h->N, h->rows, h->V - 1, 0, std::numeric_limits<double>::quiet_NaN(), h->stream));
    h->win0 = w0;
    return RSCM_OK;
}

// every out_stride-th row into the output store
int window_store_row(rscm_ens* h, int32_t t)
{
    if (!h->windowed || h->n_out == 0 || t % h->out_stride != 0) return RSCM_OK;
    if (h->defer) {
        rscm::WindowOp op{};
        op.buf = h->d_series; op.N = h->N; op.R = h->rows; op.n_vars = h->V - 1; op.kind = 1;
        op.vars = h->d_out_vars; op.dst = h->d_out; op.src_row = t - h->win0; op.n_out = h->n_out; op.dst_rows = h->out_rows;
        op.dst_row = t / h->out_stride;
        h->defer->first.push_back(op);
        return RSCM_OK;
    }
    HIPCHK(rscm::launch_gather_rows(h->d_series, h->N, h->rows, t - h->win0, h->d_out_vars, h->n_out, h->d_out, h->out_rows,
                                    t / h->out_stride, h->stream));
    return RSCM_OK;
}

int window_flush(WindowDeferral* d, hipStream_t stream)
{
    for (std::vector<rscm::WindowOp>* list : {&d->first, &d->second}) {
        for (size_t at = 0; at < list->size(); at += rscm::kMaxWindowOps) {
            const size_t n = std::min(list->size() - at, (size_t)rscm::kMaxWindowOps);
            rscm::WindowBatch batch;
            memset((void*)&batch, 0, sizeof batch);
            memcpy((void*)batch.ops, list->data() + at, n * sizeof(rscm::WindowOp));
            HIPCHK(rscm::launch_window_batch(batch, (int32_t)n, stream));
        }
        list->clear();
    }
    for (const auto& w : d->new_win0) w.first->win0 = w.second;
    d->new_win0.clear();
    return RSCM_OK;
}

extern "C" {

int rscm_gpu_abi_version(void) { return RSCM_GPU_ABI_VERSION; }
int rscm_gpu_abi_minor(void) { return RSCM_GPU_ABI_MINOR; }

const char* rscm_gpu_last_error(void) { return g_last_error.c_str(); }

int rscm_gpu_device_count(int32_t* out)
{
    GUARD_BEGIN
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out = 0;
        return fail(RSCM_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out = n;
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_mem_info(int32_t device_id, uint64_t* free_bytes, uint64_t* total_bytes)
{
    GUARD_BEGIN
    if (!free_bytes || !total_bytes) return fail(RSCM_ERR_INVALID, "output pointer is NULL");
    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    size_t f = 0, t = 0;
    e = hipMemGetInfo(&f, &t);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "hipMemGetInfo: %s", hipGetErrorString(e));
    *free_bytes = (uint64_t)f;
    *total_bytes = (uint64_t)t;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_create(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                    int32_t device_id, rscm_ens** out)
{
    return rscm_ens_create_ex(kind, n_members, n_times, time_bounds, device_id, 0, out);
}

int rscm_ens_create_ex(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                       int32_t device_id, uint32_t flags, rscm_ens** out)
{
    return rscm_ens_create_windowed(kind, n_members, n_times, time_bounds, device_id, flags, 16, 0, -1, nullptr, out);
}

// n_components > 0: a two-layer mix handle (rscm_ens_create_mix, which has checked kind, flags and the count)
static int create_handle(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds, int32_t device_id, uint32_t flags,
                         int32_t window_rows, int32_t out_stride, int32_t n_out_vars, const int32_t* out_vars, int32_t n_components,
                         rscm_ens** out);

int rscm_ens_create_windowed(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                             int32_t device_id, uint32_t flags, int32_t window_rows, int32_t out_stride,
                             int32_t n_out_vars, const int32_t* out_vars, rscm_ens** out)
{
    return create_handle(kind, n_members, n_times, time_bounds, device_id, flags, window_rows, out_stride, n_out_vars, out_vars, 0, out);
}

int rscm_ens_create_mix(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds, int32_t device_id, uint32_t flags,
                        int32_t n_components, rscm_ens** out)
{
    GUARD_BEGIN
    if (out) *out = nullptr;
    if (kind != RSCM_KIND_TWO_LAYER)
        return fail(RSCM_ERR_INVALID, "forcing components are available for the two-layer kind only (RSCM_KIND_TWO_LAYER), got kind %d", kind);
    if (flags & ~(uint32_t)(RSCM_FLAG_NO_SERIES | RSCM_FLAG_NOISE_PARAMS))
        return fail(RSCM_ERR_INVALID, "a mix handle takes flags 0, RSCM_FLAG_NO_SERIES or RSCM_FLAG_NOISE_PARAMS (no windowed storage), got 0x%x", flags);
    if (n_components < 1 || n_components > RSCM_TL_MAX_COMPONENTS)
        return fail(RSCM_ERR_INVALID, "n_components must be in [1, %d], got %d", RSCM_TL_MAX_COMPONENTS, n_components);
    return create_handle(kind, n_members, n_times, time_bounds, device_id, flags, 16, 0, -1, nullptr, n_components, out);
    GUARD_END
}

static int create_handle(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds, int32_t device_id, uint32_t flags,
                         int32_t window_rows, int32_t out_stride, int32_t n_out_vars, const int32_t* out_vars, int32_t n_components,
                         rscm_ens** out)
{
    GUARD_BEGIN
    if (flags & ~(uint32_t)(RSCM_FLAG_NO_SERIES | RSCM_FLAG_WINDOWED | RSCM_FLAG_NOISE_PARAMS)) return fail(RSCM_ERR_INVALID, "unknown flags 0x%x", flags);
    if ((flags & RSCM_FLAG_NOISE_PARAMS) && kind != RSCM_KIND_TWO_LAYER)
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NOISE_PARAMS is only available for the two-layer kind");
    if ((flags & RSCM_FLAG_NOISE_PARAMS) && (flags & (RSCM_FLAG_NO_SERIES | RSCM_FLAG_WINDOWED)))
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NOISE_PARAMS needs a handle that stores its whole series (no RSCM_FLAG_NO_SERIES, no windowed storage): "
                    "the noise that reads the two rows is refused without");
    if ((flags & RSCM_FLAG_NO_SERIES) && kind != RSCM_KIND_TWO_LAYER)
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NO_SERIES is only available for the two-layer kind");
    if ((flags & RSCM_FLAG_NO_SERIES) && (flags & RSCM_FLAG_WINDOWED))
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NO_SERIES and RSCM_FLAG_WINDOWED exclude each other");
    const bool windowed = (flags & RSCM_FLAG_WINDOWED) != 0;
    if (windowed && (window_rows < 4 || out_stride < 0 || (n_out_vars > 0 && !out_vars)))
        return fail(RSCM_ERR_INVALID, "a windowed ensemble needs window_rows >= 4, out_stride >= 0 and a variable list if n_out_vars > 0");
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (kind < RSCM_KIND_TWO_LAYER || kind > RSCM_KIND_AGGREGATE)
        return fail(RSCM_ERR_INVALID, "unknown kind %d", kind);
    if (n_members < 1) return fail(RSCM_ERR_INVALID, "n_members must be >= 1, got %lld", (long long)n_members);
    if (n_times < 2) return fail(RSCM_ERR_INVALID, "n_times must be >= 2 (TimeAxis::from_values asserts len >= 2)");
    if (!time_bounds) return fail(RSCM_ERR_INVALID, "time_bounds is NULL");
    for (int32_t i = 0; i < n_times; ++i)
        if (!(time_bounds[i + 1] > time_bounds[i]))  // timeseries.rs:47-52 assert!(is_monotonic)
            return fail(RSCM_ERR_INVALID, "time_bounds must be strictly increasing (index %d)", i);
    if ((uint64_t)n_members > (uint64_t)std::numeric_limits<int32_t>::max() * 256ull)
        return fail(RSCM_ERR_INVALID, "n_members too large for one launch grid");

    std::unique_ptr<rscm_ens> h(new rscm_ens());   // every return before the last goes through ~rscm_ens
    h->kind = kind;
    h->N = n_members;
    h->T = n_times;
    h->rows = (flags & RSCM_FLAG_NO_SERIES) ? 1 : n_times;
    if (windowed && window_rows < n_times) {  // a window as long as the axis is plain full storage
        h->windowed = true;
        h->rows = window_rows;
    }
    h->device = device_id;
    h->P = h->info().n_params;
    h->V = h->info().n_vars;
    h->n_inputs = h->info().n_inputs;
    if (n_components > 0) {   // the coefficients are parameter rows 6 .. 6 + K - 1, the components the K rows of the input block
        h->n_comp = n_components;
        h->P = RSCM_TL_P_COEFF0 + n_components;
        h->n_inputs = n_components;
    }
    if (flags & RSCM_FLAG_NOISE_PARAMS) {   // sigma_i and phi_i follow the six parameters and the coefficients
        h->noise_rows = true;
        h->P += 2;
    }
    h->bounds.assign(time_bounds, time_bounds + n_times + 1);
    h->initial_set.assign(h->V, 0);
    h->out_slot.assign(h->V, -1);
    h->lookback = h->info().lookback;   // (N2O: refreshed by set_params)
    if (h->windowed && out_stride > 0) {
        h->out_stride = out_stride;
        h->out_rows = (n_times - 1) / out_stride + 1;
        if (n_out_vars < 0)
            for (int32_t v = 1; v < h->V; ++v) h->out_vars.push_back(v);
        else
            for (int32_t k = 0; k < n_out_vars; ++k) {
                if (out_vars[k] < 1 || out_vars[k] >= h->V || h->out_slot[out_vars[k]] >= 0)
                    return fail(RSCM_ERR_INVALID, "output variable %d: not a stored variable of this kind, or listed twice", out_vars[k]);
                h->out_slot[out_vars[k]] = k;
                h->out_vars.push_back(out_vars[k]);
            }
        h->n_out = (int32_t)h->out_vars.size();
        for (int32_t k = 0; k < h->n_out; ++k) h->out_slot[h->out_vars[k]] = k;
    }

    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    const size_t series_elems = (size_t)(h->V - 1) * (size_t)h->rows * (size_t)h->N;
    HIPCHK(h->d_params.alloc((size_t)h->P * h->N));
    HIPCHK(h->d_series.alloc(series_elems));
    HIPCHK(h->d_status.alloc((size_t)h->N));
    if (h->windowed) {
        HIPCHK(h->d_row0.alloc((size_t)(h->V - 1) * h->N));
        if (h->n_out > 0) {
            const size_t out_elems = (size_t)h->n_out * h->out_rows * h->N;
            HIPCHK(h->d_out.alloc(out_elems));
            HIPCHK(h->d_out_vars.alloc((size_t)h->n_out));
            HIPCHK(hipMemcpy(h->d_out_vars, h->out_vars.data(), (size_t)h->n_out * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHK(rscm::launch_fill(h->d_out, (int64_t)out_elems, std::numeric_limits<double>::quiet_NaN(), h->stream));
        }
    }
    HIPCHK(h->d_nsub_tl.alloc((size_t)(h->T - 1)));
    HIPCHK(h->d_nsub_cc.alloc((size_t)(h->T - 1)));
    HIPCHK(h->d_partial.alloc(4 * 1024));
    HIPCHK(h->d_out4.alloc(4));
    if (kind == RSCM_KIND_UDEB) {
        HIPCHK(h->d_scal.alloc((size_t)rscm::kUdebScalars * h->N));
        HIPCHK(h->d_hist.alloc((size_t)h->T * h->N));
    }
    if (h->info().needs_bounds) {  // kinds that use the step length
        HIPCHK(h->d_bounds.alloc((size_t)(h->T + 1)));
        HIPCHK(hipMemcpyAsync(h->d_bounds, h->bounds.data(), (size_t)(h->T + 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (kind == RSCM_KIND_AGGREGATE) {  // contributors that are neither linked nor set stay NaN = skipped
        HIPCHK(h->d_forcing.alloc((size_t)h->n_inputs * h->T));
        HIPCHK(rscm::launch_fill(h->d_forcing, (int64_t)h->n_inputs * h->T, std::numeric_limits<double>::quiet_NaN(), h->stream));
        h->n_scen = 1;
        h->forcing_set = true;
    }
    HIPCHK(hipMemsetAsync(h->d_status, 0, (size_t)h->N, h->stream));
    // never-written entries are NaN (builder.rs:772-780)
    HIPCHK(rscm::launch_fill(h->d_series, (int64_t)series_elems, std::numeric_limits<double>::quiet_NaN(),
                         h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h.release();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_destroy(rscm_ens* h)
{
    if (!h) return RSCM_OK;
    if (h->link_refs > 0)
        return fail(RSCM_ERR_STATE, "%d linked input(s) of other ensembles still read this one's series: destroy or unlink them first", h->link_refs);
    (void)hipSetDevice(h->device);
    delete h;
    return RSCM_OK;
}

// What a handle holds that is not device memory; the buffers and then the stream follow (ens.hpp, at the struct).  The stream is
// synchronised here, not in rscm_ens_destroy, so that a handle whose construction failed half-way goes the same way.
rscm_ens::~rscm_ens()
{
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& l : links)
        if (l.src) --l.src->link_refs;
    select_release(this);
    delete plan;
}


int rscm_ens_n_params(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->P; return RSCM_OK; }
int rscm_ens_n_vars(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->V; return RSCM_OK; }
int rscm_ens_n_diagnostics(const rscm_ens* h, int32_t* out) { NEED(h); if (!out) return fail(RSCM_ERR_INVALID, "out is NULL"); *out = h->n_diag; return RSCM_OK; }
int rscm_ens_n_inputs(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->n_inputs; return RSCM_OK; }
int rscm_ens_n_forcing_components(const rscm_ens* h, int32_t* out) { NEED(h); if (!out) return fail(RSCM_ERR_INVALID, "out is NULL"); *out = h->n_comp; return RSCM_OK; }
int rscm_ens_n_members(const rscm_ens* h, int64_t* out) { NEED(h); *out = h->N; return RSCM_OK; }
int rscm_ens_n_times(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->T; return RSCM_OK; }
int rscm_ens_time_index(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->time_index; return RSCM_OK; }

int rscm_ens_set_mode(rscm_ens* h, int32_t mode)
{
    NEED(h);
    if (mode != RSCM_MODE_EXACT && mode != RSCM_MODE_FAST) return fail(RSCM_ERR_INVALID, "unknown mode %d", mode);
    if (mode != h->mode) {  // sums parked / carried by the other arithmetic cannot be resumed
        h->ocean_forget_partial_sums();
    }
    h->mode = mode;
    h->rows_written();   // the next run writes other bits
    return RSCM_OK;
}

int rscm_ens_set_step_size(rscm_ens* h, int32_t component, double step)
{
    NEED(h);
    if (!(step > 0.0) || !std::isfinite(step)) return fail(RSCM_ERR_INVALID, "step must be positive and finite");
    if (component == RSCM_COMP_TWO_LAYER && h->kind != RSCM_KIND_CARBON_CYCLE)
        h->h_tl = step;
    else if (component == RSCM_COMP_CARBON_CYCLE && (h->kind == RSCM_KIND_COUPLED || h->kind == RSCM_KIND_CARBON_CYCLE))
        h->h_cc = step;
    else
        return fail(RSCM_ERR_INVALID, "component %d not part of this model kind", component);
    h->schedule_dirty = true;
    return RSCM_OK;
}

int rscm_gpu_stream_create(int32_t device_id, void** out_stream)
{
    GUARD_BEGIN
    if (!out_stream) return fail(RSCM_ERR_INVALID, "out_stream is NULL");
    HIPCHK(hipSetDevice(device_id));
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out_stream = (void*)s;
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_stream_destroy(int32_t device_id, void* hip_stream)
{
    GUARD_BEGIN
    if (!hip_stream) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    HIPCHK(hipStreamDestroy((hipStream_t)hip_stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_stream(rscm_ens* h, void* hip_stream)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->own_stream) {
        HIPCHK(hipStreamDestroy(h->stream));
        h->own_stream = false;
    }
    if (hip_stream) {
        h->stream = (hipStream_t)hip_stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_params(rscm_ens* h, const double* soa)
{
    GUARD_BEGIN
    NEED(h);
    if (!soa) return fail(RSCM_ERR_INVALID, "params is NULL");
    if (int rc = set_device(h)) return rc;
    if (h->kind == RSCM_KIND_UDEB)
        if (int rc = configure_udeb(h, h->N, [&](int j, int64_t i) { return soa[(size_t)j * h->N + i]; })) return rc;
    if (h->kind == RSCM_KIND_OCEAN_CARBON)
        if (int rc = configure_ocean(h, h->N, [&](int j, int64_t i) { return soa[(size_t)j * h->N + i]; })) return rc;
    if (h->kind == RSCM_KIND_GHG_FORCING) {  // one forcing method per ensemble (one kernel instance)
        const double m = soa[(size_t)RSCM_GH_P_METHOD * h->N];
        if (m != 0.0 && m != 1.0) return fail(RSCM_ERR_INVALID, "GhgForcing method must be 0 (Ipcctar) or 1 (Olbl), got %g", m);
        for (int64_t i = 1; i < h->N; ++i)
            if (soa[(size_t)RSCM_GH_P_METHOD * h->N + i] != m)
                return fail(RSCM_ERR_INVALID, "GhgForcing parameter row %d (method) must be the same for every member", RSCM_GH_P_METHOD);
        h->ghg_method = (int32_t)m;
    }
    if (h->kind == RSCM_KIND_N2O_CHEMISTRY) {  // rows the stratospheric delay looks back (n2o.rs:203-218)
        double d = 1.0;
        for (int64_t i = 0; i < h->N; ++i) d = std::max(d, soa[(size_t)4 * h->N + i]);
        const int32_t lookback = (int32_t)std::min(d, 1e6) + 1;
        // a window that has already slid kept only keep_rows() of the OLD look-back: the rows a longer delay
        // reads are gone (the body would read before the window's first row)
        if (h->windowed && h->win0 > 0 && std::max(0, h->time_index - lookback) < h->win0 && lookback > h->lookback)
            return fail(RSCM_ERR_STATE, "a stratospheric delay that looks %d rows back needs row %d, but the window already starts at row %d: "
                        "rewind (rscm_ens_rewind) or restore a checkpoint before raising the delay", lookback,
                        std::max(0, h->time_index - lookback), h->win0);
        h->lookback = lookback;
    }
    HIPCHK(hipMemcpyAsync(h->d_params, soa, (size_t)h->P * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    {   // rows that hold the same bits for every member
        uint64_t uni = 0;
        for (int32_t j = 0; j < h->P && j < 64; ++j) {
            const double* row = soa + (size_t)j * h->N;
            bool same = true;
            for (int64_t i = 1; i < h->N && same; ++i) same = memcmp(&row[i], &row[0], sizeof(double)) == 0;
            if (same) uni |= 1ull << j;
        }
        h->uniform_rows = h->params_exposed ? 0 : uni;  // a caller holding the device pointer may rewrite any row
        h->params_written();
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->params_set = true;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_params_aos(rscm_ens* h, const double* aos)
{
    GUARD_BEGIN
    NEED(h);
    if (!aos) return fail(RSCM_ERR_INVALID, "params is NULL");
    std::vector<double> soa((size_t)h->P * h->N);
    for (int64_t i = 0; i < h->N; ++i)
        for (int32_t j = 0; j < h->P; ++j) soa[(size_t)j * h->N + i] = aos[(size_t)i * h->P + j];
    return rscm_ens_set_params(h, soa.data());
    GUARD_END
}

int rscm_ens_set_forcing(rscm_ens* h, int32_t var_id, int32_t n_scen, const double* series,
                         const int32_t* scenario_of_member, int32_t source)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id != 0) return fail(RSCM_ERR_INVALID, "variable %d is not the shared input of this kind", var_id);
    if (n_scen < 1 || !series) return fail(RSCM_ERR_INVALID, "need n_scen >= 1 and a series pointer");
    if (source != RSCM_SRC_EXOGENOUS && source != RSCM_SRC_UPSTREAM) return fail(RSCM_ERR_INVALID, "unknown source %d", source);
    if (h->kind == RSCM_KIND_COUPLED && source != RSCM_SRC_EXOGENOUS)
        return fail(RSCM_ERR_INVALID, "emissions of the coupled chain are exogenous (no component produces them)");
    if (h->kind == RSCM_KIND_UDEB && source != RSCM_SRC_EXOGENOUS)
        return fail(RSCM_ERR_INVALID, "ClimateUDEB reads its forcing as an exogenous series (at_start / at_end)");
    if (h->kind >= RSCM_KIND_GHG_FORCING && source != RSCM_SRC_EXOGENOUS)
        return fail(RSCM_ERR_INVALID, "the stateless forcing kinds read their inputs as exogenous series");
    if (scenario_of_member)
        for (int64_t i = 0; i < h->N; ++i)
            if (scenario_of_member[i] < 0 || scenario_of_member[i] >= n_scen)
                return fail(RSCM_ERR_INVALID, "scenario_of_member[%lld] = %d out of range [0, %d)", (long long)i,
                            scenario_of_member[i], n_scen);
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->year_facts.drop_forcing();   // from here on the table may change: the verdict on the new one is formed once it stands
    // Tables of the same scenario count are rewritten where they stand.  Tables of another count are built aside and moved in,
    // with n_scen, once they are written: a failure on the way leaves the handle with the tables and the count it had.
    const bool resize = n_scen != h->n_scen || !h->d_forcing;
    rscm::DevBuf<double> d_forcing_new, d_ghg_new;
    rscm::DevBuf<int32_t> d_scen_new;
    if (resize) {
        HIPCHK(d_forcing_new.alloc((size_t)n_scen * h->n_inputs * h->T));
        if (h->kind == RSCM_KIND_GHG_FORCING) HIPCHK(d_ghg_new.alloc((size_t)n_scen * rscm::kGhgRows * h->T));
    }
    double* const d_forcing = resize ? d_forcing_new : h->d_forcing;
    double* const d_ghg = resize ? d_ghg_new : h->d_ghg_tables;
    HIPCHK(hipMemcpyAsync(d_forcing, series, (size_t)n_scen * h->n_inputs * h->T * sizeof(double), hipMemcpyHostToDevice, h->stream));
    std::vector<double> ghg_tab;  // must outlive the copy below (synchronised before return)
    if (h->kind == RSCM_KIND_GHG_FORCING) {
        ghg_tab = ghg_tables(series, n_scen, h->T);
        HIPCHK(hipMemcpyAsync(d_ghg, ghg_tab.data(), ghg_tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (scenario_of_member) {   // (indices into the new tables: never written over the old ones' while those may stay)
        if (resize || !h->d_scen) HIPCHK(d_scen_new.alloc((size_t)h->N));
        HIPCHK(hipMemcpyAsync(d_scen_new ? d_scen_new : h->d_scen, scenario_of_member, (size_t)h->N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (resize) {
        h->d_forcing = std::move(d_forcing_new);
        if (h->kind == RSCM_KIND_GHG_FORCING) h->d_ghg_tables = std::move(d_ghg_new);
    }
    if (d_scen_new || !scenario_of_member) h->d_scen = std::move(d_scen_new);   // (omitted: the members' scenario table goes)
    h->n_scen = n_scen;
    h->source = source;
    h->forcing_set = true;
    if (h->kind == RSCM_KIND_TWO_LAYER && h->n_comp == 0) h->year_facts.set_forcing(series, n_scen, h->T);   // (a plain table: [S][T])
    if (h->kind == RSCM_KIND_AGGREGATE) {  // rows after the last non-NaN one of the block stay out of the sums anyway
        int32_t used = 0;
        for (int32_t sidx = 0; sidx < n_scen; ++sidx)
            for (int32_t k = 0; k < h->n_inputs; ++k)
                for (int32_t t = 0; t < h->T; ++t)
                    if (!std::isnan(series[((size_t)sidx * h->n_inputs + k) * h->T + t])) used = std::max(used, k + 1);
        h->ag_rows_set = used;
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_link_input(rscm_ens* h, int32_t input_row, rscm_ens* src, int32_t src_var, int32_t source)
{
    GUARD_BEGIN
    NEED(h);
    if (!src) return fail(RSCM_ERR_INVALID, "source ensemble is NULL");
    if (src == h) return fail(RSCM_ERR_INVALID, "an ensemble cannot link to itself (its own states are read in the kernel)");
    if (h->kind == RSCM_KIND_COUPLED || h->kind == RSCM_KIND_HALOCARBON)
        return fail(RSCM_ERR_INVALID, "the inputs of this kind cannot be linked (they are exogenous emissions)");
    if (h->n_comp > 0)
        return fail(RSCM_ERR_INVALID, "the forcing components of a mix handle (rscm_ens_create_mix) cannot be linked: they are shared "
                                      "scenario rows scaled per member");
    if (h->noise_kind)
        return fail(RSCM_ERR_INVALID, "a handle with forcing noise (rscm_ens_set_forcing_noise) takes no linked input: the noise is added to "
                                      "its own shared forcing; clear the noise first");
    if (input_row < 0 || input_row >= h->n_inputs || input_row >= rscm::kMaxLinks)
        return fail(RSCM_ERR_INVALID, "input row %d out of range [0, %d)", input_row, h->n_inputs);
    if (src_var < 1 || src_var >= src->V) return fail(RSCM_ERR_INVALID, "variable %d of the source has no stored series", src_var);
    if (source != RSCM_SRC_EXOGENOUS && source != RSCM_SRC_UPSTREAM) return fail(RSCM_ERR_INVALID, "unknown source %d", source);
    if (src->N != h->N || src->T != h->T || src->device != h->device)
        return fail(RSCM_ERR_INVALID, "linked ensembles need the same members, time points and device (%lld x %d on %d vs %lld x %d on %d)",
                    (long long)src->N, src->T, src->device, (long long)h->N, h->T, h->device);
    if ((!src->windowed && src->rows != src->T) || (!h->windowed && h->rows != h->T))
        return fail(RSCM_ERR_INVALID, "linked ensembles must store their series (no RSCM_FLAG_NO_SERIES)");
    if (!h->link_order_check) src->read_ahead = true;
    auto& l = h->links[input_row];
    if (l.src) --l.src->link_refs;
    else ++h->n_linked;
    l.src = src;
    l.var = src_var;
    l.off = source == RSCM_SRC_UPSTREAM ? 1 : 0;
    ++src->link_refs;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_link_order_check(rscm_ens* h, int32_t enabled)
{
    NEED(h);
    h->link_order_check = enabled != 0;
    if (!h->link_order_check)  // the producers' rows beyond what they have written must read as NaN
        for (auto& l : h->links)
            if (l.src) l.src->read_ahead = true;
    return RSCM_OK;
}

int rscm_ens_unlink_input(rscm_ens* h, int32_t input_row)
{
    NEED(h);
    if (input_row < 0 || input_row >= h->n_inputs || input_row >= rscm::kMaxLinks)
        return fail(RSCM_ERR_INVALID, "input row %d out of range [0, %d)", input_row, h->n_inputs);
    auto& l = h->links[input_row];
    if (l.src) {
        --l.src->link_refs;
        --h->n_linked;
        l = rscm_ens::Link{};
    }
    return RSCM_OK;
}

int rscm_ens_set_initial(rscm_ens* h, int32_t var_id, const double* values, int64_t n_values)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (!values || (n_values != 1 && n_values != h->N))
        return fail(RSCM_ERR_INVALID, "initial values: need 1 or n_members values, got %lld", (long long)n_values);
    if (int rc = set_device(h)) return rc;
    if (h->windowed) {
        if (h->win0 != 0)
            if (int rc = window_reset(h, false)) return rc;
        h->row0_saved = false;  // saved again when step 0 starts
    }
    if (n_values == 1)
        HIPCHK(rscm::launch_fill(h->series(var_id), h->N, values[0], h->stream));
    else
        HIPCHK(hipMemcpyAsync(h->series(var_id), values, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->initial_set[var_id] = 1;
    h->time_index = 0;
    h->rows_written();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_state(rscm_ens* h, int32_t var_id, int32_t tidx, const double* values, int64_t n_values)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (h->windowed ? (tidx < h->win0 || tidx >= h->win0 + h->rows) : (tidx < 0 || tidx >= h->rows))
        return fail(RSCM_ERR_INVALID, h->windowed ? "time index %d is outside the stored window (move the stepper there first: rscm_ens_set_time_index)"
                                                   : "time index %d out of range", tidx);
    if (!values || (n_values != 1 && n_values != h->N))
        return fail(RSCM_ERR_INVALID, "state values: need 1 or n_members values, got %lld", (long long)n_values);
    if (int rc = set_device(h)) return rc;
    if (h->windowed && tidx == 0) h->row0_saved = false;
    double* row = h->series(var_id) + (size_t)tidx * h->N;
    if (n_values == 1)
        HIPCHK(rscm::launch_fill(row, h->N, values[0], h->stream));
    else
        HIPCHK(hipMemcpyAsync(row, values, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (tidx == 0) h->initial_set[var_id] = 1;
    h->rows_written();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_time_index(rscm_ens* h, int32_t tidx)
{
    GUARD_BEGIN
    NEED(h);
    if (tidx < 0 || tidx > (h->windowed ? h->T : h->rows) - 1) return fail(RSCM_ERR_INVALID, "time index %d out of range", tidx);
    // kinds whose components keep internal state in the reference (ComponentState: the UDEB ocean
    // columns, the OceanCarbon flux history) can only continue from where that state stands
    if ((h->kind == RSCM_KIND_UDEB || h->kind == RSCM_KIND_OCEAN_CARBON) && tidx != 0 && tidx != h->time_index)
        return fail(RSCM_ERR_STATE, "this kind carries internal component state on the device: the time index can "
                                    "only be rewound to 0 or left at %d", h->time_index);
    if (tidx > 0) h->mark_states_set();   // a restored checkpoint carries its own state rows
    if (h->windowed && tidx != h->time_index) {
        if (int rc = set_device(h)) return rc;
        if (int rc = window_seek(h, tidx)) return rc;
    }
    h->time_index = tidx;
    h->rows_written();
    h->ocean_forget_partial_sums();
    return RSCM_OK;
    GUARD_END
}

typedef std::vector<std::pair<double*, int64_t>> StatePieces;

// the pieces of a handle's internal component state at time index k: (device pointer, doubles)
static void internal_pieces(const rscm_ens* h, int32_t k, StatePieces& p)
{
    if (h->kind == RSCM_KIND_UDEB && h->d_ocean && h->d_scal && h->d_hist) {
        p.emplace_back(h->d_ocean, (int64_t)2 * h->udeb_n_layers * h->N);
        p.emplace_back(h->d_scal, (int64_t)rscm::kUdebScalars * h->N);
        p.emplace_back(h->d_hist, (int64_t)(k + 1) * h->N);
    } else if (h->kind == RSCM_KIND_OCEAN_CARBON && h->d_ocean_hist) {
        // the pulses still held, oldest first: the ring unrolled into (at most) two pieces
        const int64_t total = (int64_t)k * h->ocean_steps, R = h->ocean_hist_rows;
        const int64_t cnt = std::min(total, R), first = (total - cnt) % R;
        const int64_t head = std::min(cnt, R - first);
        if (head > 0) p.emplace_back(h->d_ocean_hist + (size_t)first * h->N, head * h->N);
        if (cnt > head) p.emplace_back(h->d_ocean_hist, (cnt - head) * h->N);
    }
}

int rscm_ens_internal_state_size(rscm_ens* h, int64_t* n_doubles)
{
    NEED(h);
    if (!n_doubles) return fail(RSCM_ERR_INVALID, "n_doubles is NULL");
    int64_t n = 0;
    StatePieces pieces;
    internal_pieces(h, h->time_index, pieces);
    for (const auto& piece : pieces) n += piece.second;
    *n_doubles = n;
    return RSCM_OK;
}

int rscm_ens_get_internal_state(rscm_ens* h, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    StatePieces pieces;
    internal_pieces(h, h->time_index, pieces);
    for (const auto& piece : pieces) {
        if (piece.second > 0)
            HIPCHK(hipMemcpyAsync(out, piece.first, (size_t)piece.second * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        out += piece.second;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_internal_state(rscm_ens* h, const double* in, int64_t n_doubles, int32_t time_index)
{
    GUARD_BEGIN
    NEED(h);
    if (time_index < 0 || time_index > (h->windowed ? h->T : h->rows) - 1) return fail(RSCM_ERR_INVALID, "time index %d out of range", time_index);
    if ((h->kind == RSCM_KIND_UDEB && !h->udeb_ready) || (h->kind == RSCM_KIND_OCEAN_CARBON && !h->ocean_ready))
        return fail(RSCM_ERR_STATE, "set the parameters first: they size the internal state");
    StatePieces pieces;
    internal_pieces(h, time_index, pieces);
    int64_t n = 0;
    for (const auto& piece : pieces) n += piece.second;
    if (n != n_doubles) return fail(RSCM_ERR_INVALID, "internal state at time index %d is %lld doubles, got %lld", time_index, (long long)n, (long long)n_doubles);
    if (n > 0 && !in) return fail(RSCM_ERR_INVALID, "in is NULL");
    if (int rc = set_device(h)) return rc;
    for (const auto& piece : pieces) {
        if (piece.second > 0)
            HIPCHK(hipMemcpyAsync(piece.first, in, (size_t)piece.second * sizeof(double), hipMemcpyHostToDevice, h->stream));
        in += piece.second;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (time_index > 0) h->mark_states_set();
    if (h->windowed && time_index != h->time_index)
        if (int rc = window_seek(h, time_index)) return rc;
    h->time_index = time_index;
    h->rows_written();
    h->ocean_forget_partial_sums();
    return RSCM_OK;
    GUARD_END
}

// ---- branching: members of one handle copied into another at the source's time index (ABI minor 10) ----
namespace {

struct GatherRow { const void* src; void* dst; int32_t elem_bytes; };

// Rows that follow each other at one pair of strides become one piece; the pieces go out kMaxGatherPieces per launch.
int gather_launch(const std::vector<GatherRow>& rows, int64_t src_N, int64_t dst_N, const int64_t* d_anc, int64_t count, hipStream_t stream)
{
    rscm::GatherBatch batch;
    memset((void*)&batch, 0, sizeof batch);
    int32_t n = 0;
    auto flush = [&]() -> hipError_t {
        const hipError_t e = n > 0 ? rscm::launch_gather_members(batch, n, d_anc, count, src_N, stream) : hipSuccess;
        n = 0;
        return e;
    };
    for (const GatherRow& r : rows) {
        if (n > 0) {
            rscm::GatherPiece& g = batch.pieces[n - 1];
            if (g.elem_bytes == r.elem_bytes) {
                const int64_t ds = ((const char*)r.src - (const char*)g.src) / r.elem_bytes, dd = ((char*)r.dst - (char*)g.dst) / r.elem_bytes;
                if (g.rows == 1 && ds > 0 && dd > 0) {
                    g.src_stride = ds; g.dst_stride = dd; g.rows = 2;
                    continue;
                }
                if (g.rows > 1 && ds == g.src_stride * g.rows && dd == g.dst_stride * g.rows && g.rows < (1 << 20)) {
                    ++g.rows;
                    continue;
                }
            }
        }
        if (n == rscm::kMaxGatherPieces) HIPCHK(flush());
        rscm::GatherPiece& g = batch.pieces[n++];
        g.src = r.src; g.dst = r.dst; g.src_stride = src_N; g.dst_stride = dst_N; g.rows = 1; g.elem_bytes = r.elem_bytes;
    }
    HIPCHK(flush());
    return RSCM_OK;
}

}  // namespace

int rscm_ens_gather_members(rscm_ens* dst, int64_t dst_offset, rscm_ens* src, const int64_t* anc, int32_t on_device, int64_t count)
{
    GUARD_BEGIN
    NEED(dst);
    NEED(src);
    if (dst == src) return fail(RSCM_ERR_INVALID, "source and destination are the same handle");
    if (count < 0 || dst_offset < 0 || dst_offset > dst->N || count > dst->N - dst_offset)
        return fail(RSCM_ERR_INVALID, "members [%lld, %lld + %lld) are outside the destination's %lld", (long long)dst_offset,
                    (long long)dst_offset, (long long)count, (long long)dst->N);
    if (count > 0 && !anc) return fail(RSCM_ERR_INVALID, "ancestors are NULL");
    if (dst->kind != src->kind) return fail(RSCM_ERR_INVALID, "kinds differ: destination %d, source %d", dst->kind, src->kind);
    if (dst->n_comp != src->n_comp)
        return fail(RSCM_ERR_INVALID, "the forcing component counts differ: destination %d, source %d", dst->n_comp, src->n_comp);
    if (dst->noise_rows != src->noise_rows)
        return fail(RSCM_ERR_INVALID, "one handle has the noise parameter rows (RSCM_FLAG_NOISE_PARAMS) and the other has not: destination %d, source %d",
                    (int)dst->noise_rows, (int)src->noise_rows);
    if (dst->device != src->device) return fail(RSCM_ERR_INVALID, "the handles live on devices %d and %d", dst->device, src->device);
    if (dst->T != src->T || memcmp(dst->bounds.data(), src->bounds.data(), src->bounds.size() * sizeof(double)) != 0)
        return fail(RSCM_ERR_INVALID, "the time axes differ");
    if (dst->mode != src->mode) return fail(RSCM_ERR_INVALID, "the arithmetic modes differ");
    if (memcmp(&dst->h_tl, &src->h_tl, sizeof(double)) != 0 || memcmp(&dst->h_cc, &src->h_cc, sizeof(double)) != 0)
        return fail(RSCM_ERR_INVALID, "the RK4 step sizes differ");
    if ((!dst->windowed && dst->rows != dst->T) || (!src->windowed && src->rows != src->T))
        return fail(RSCM_ERR_INVALID, "a handle without stored series (RSCM_FLAG_NO_SERIES) cannot be branched");
    if (dst->select || src->select) return fail(RSCM_ERR_STATE, "a select is in flight: rscm_ens_select_end it first");
    if (!src->params_set) return fail(RSCM_ERR_STATE, "the source has no parameters");
    if ((src->kind == RSCM_KIND_UDEB && !src->udeb_ready) || (src->kind == RSCM_KIND_OCEAN_CARBON && !src->ocean_ready))
        return fail(RSCM_ERR_STATE, "the source is not configured");
    const int32_t k = src->time_index, P = src->P, V = src->V;
    const int32_t t0 = std::max(0, k - src->lookback);
    for (int32_t v = 1; v < V; ++v)
        for (int32_t t = t0; t <= k; ++t)
            if (!src->row_ptr(v, t))
                return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident in the source any more", t, v);
    const bool later = dst->gather_k >= 0 && dst->time_index == dst->gather_k && dst->params_set;   // another block of the same branch
    if (later && dst->gather_k != k)
        return fail(RSCM_ERR_STATE, "the destination was gathered at time index %d, this source stands at %d", dst->gather_k, k);
    if (int rc = set_device(src)) return rc;
    HIPCHK(hipStreamSynchronize(src->stream));
    HIPCHK(hipStreamSynchronize(dst->stream));

    // element 0 of every parameter row of the source: its structural rows are uniform, and they configure the destination
    std::vector<double> p0((size_t)P);
    HIPCHK(hipMemcpy2D(p0.data(), sizeof(double), src->d_params, (size_t)src->N * sizeof(double), sizeof(double), (size_t)P, hipMemcpyDeviceToHost));
    if (later) {
        for (int32_t j = 0; j < P; ++j)
            if (structural_row(src->kind, j) && memcmp(&p0[j], &dst->gather_p0[j], sizeof(double)) != 0)
                return fail(RSCM_ERR_INVALID, "parameter row %d (%s) of this source differs from the one the destination was configured from", j,
                            structural_row(src->kind, j));
        if (src->lookback != dst->lookback) return fail(RSCM_ERR_INVALID, "the look-back of this source differs from the destination's");
    }

    // the ancestors on the device, checked there before anything is written
    rscm::DevBuf<int64_t> d_tmp;
    rscm::DevBuf<int32_t> d_flag;
    const int64_t* d_anc = anc;
    if (count > 0) {
        if (!on_device) {
            HIPCHK(d_tmp.alloc((size_t)count));
            HIPCHK(hipMemcpyAsync(d_tmp.get(), anc, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, dst->stream));
            d_anc = d_tmp.get();
        }
        int32_t bad = 0;
        HIPCHK(d_flag.alloc(1));
        HIPCHK(hipMemsetAsync(d_flag.get(), 0, sizeof(int32_t), dst->stream));
        HIPCHK(rscm::launch_ancestors_check(d_anc, count, src->N, d_flag.get(), dst->stream));
        HIPCHK(hipMemcpyAsync(&bad, d_flag.get(), sizeof bad, hipMemcpyDeviceToHost, dst->stream));
        HIPCHK(hipStreamSynchronize(dst->stream));
        if (bad) return fail(RSCM_ERR_INVALID, "an ancestor is outside [0, %lld)", (long long)src->N);
    }

    if (!later) {
        // the destination takes the configuration the source derived from its structural rows
        const int32_t was = dst->time_index;
        dst->time_index = 0;   // its own internal state is about to be replaced: a change of its shape is no error
        int rc = RSCM_OK;
        if (dst->kind == RSCM_KIND_UDEB) rc = configure_udeb(dst, 1, [&](int j, int64_t) { return p0[(size_t)j]; });
        if (dst->kind == RSCM_KIND_OCEAN_CARBON) rc = configure_ocean(dst, 1, [&](int j, int64_t) { return p0[(size_t)j]; });
        dst->time_index = was;
        if (rc) return rc;
        dst->ghg_method = src->ghg_method;
        dst->lookback = src->lookback;
        if (dst->windowed) {
            if (dst->rows < 2 * dst->keep_rows())
                return fail(RSCM_ERR_INVALID, "the destination's window of %d rows is too short for a look-back of %d rows", dst->rows, dst->lookback);
            if (int rc2 = window_seek(dst, k)) return rc2;
            if (k == 0) dst->row0_saved = false;
        }
        dst->gather_p0 = p0;
    }
    if (dst->windowed && (t0 < dst->win0 || k >= dst->win0 + dst->rows))
        return fail(RSCM_ERR_STATE, "rows %d..%d do not lie in the destination's window [%d, %d)", t0, k, dst->win0, dst->win0 + dst->rows);

    std::vector<GatherRow> rows;
    for (int32_t j = 0; j < P; ++j)
        rows.push_back({src->d_params + (size_t)j * src->N, dst->d_params + (size_t)j * dst->N + dst_offset, 8});
    for (int32_t t = t0; t <= k; ++t)
        for (int32_t v = 1; v < V; ++v)
            rows.push_back({src->row_ptr(v, t), dst->series(v) + (size_t)t * dst->N + dst_offset, 8});
    if (src->kind == RSCM_KIND_UDEB) {
        for (int32_t r = 0; r < 2 * src->udeb_n_layers; ++r)
            rows.push_back({src->d_ocean + (size_t)r * src->N, dst->d_ocean + (size_t)r * dst->N + dst_offset, 8});
        for (int32_t r = 0; r < rscm::kUdebScalars; ++r)
            rows.push_back({src->d_scal + (size_t)r * src->N, dst->d_scal + (size_t)r * dst->N + dst_offset, 8});
        for (int32_t r = 0; r <= k; ++r)
            rows.push_back({src->d_hist + (size_t)r * src->N, dst->d_hist + (size_t)r * dst->N + dst_offset, 8});
    } else if (src->kind == RSCM_KIND_OCEAN_CARBON) {
        if (dst->ocean_hist_rows != src->ocean_hist_rows || dst->ocean_steps != src->ocean_steps)
            return fail(RSCM_ERR_INVALID, "the flux-history rings differ: %lld and %lld rows", (long long)dst->ocean_hist_rows, (long long)src->ocean_hist_rows);
        // the pulses still held sit at the same ring positions on both sides
        const int64_t total = (int64_t)k * src->ocean_steps, R = src->ocean_hist_rows;
        const int64_t cnt = std::min(total, R), first = cnt > 0 ? (total - cnt) % R : 0;
        for (int64_t i = 0; i < cnt; ++i) {
            const int64_t r = (first + i) % R;
            rows.push_back({src->d_ocean_hist + (size_t)r * src->N, dst->d_ocean_hist + (size_t)r * dst->N + dst_offset, 8});
        }
    }
    rows.push_back({src->d_status, dst->d_status + dst_offset, 1});
    if (count > 0)
        if (int rc = gather_launch(rows, src->N, dst->N, d_anc, count, dst->stream)) return rc;
    HIPCHK(hipStreamSynchronize(dst->stream));

    // rows that hold one value for every member: only those that did in the source and, for a later block, hold the same bits as before
    uint64_t uni = dst->params_exposed ? 0 : src->uniform_rows;
    if (later) {
        uni &= dst->uniform_rows;
        for (int32_t j = 0; j < P && j < 64; ++j)
            if (memcmp(&p0[j], &dst->gather_p0[j], sizeof(double)) != 0) uni &= ~(1ull << j);
    } else if (dst_offset != 0)
        uni = 0;   // element 0, which the kernels read for such a row, is not among the members written
    dst->uniform_rows = uni;
    dst->params_written();
    dst->params_set = true;
    dst->mark_states_set();
    dst->time_index = k;
    dst->gather_k = k;
    dst->ocean_forget_partial_sums();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_rewind(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (h->windowed) {
        if (int rc = set_device(h)) return rc;
        if (int rc = window_reset(h, false)) return rc;
    }
    h->time_index = 0;
    h->rows_written();
    h->ocean_forget_partial_sums();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_clear_series(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = set_device(h)) return rc;
    if (h->windowed) {
        if (int rc = window_reset(h, true)) return rc;
        if (h->d_out)
            HIPCHK(rscm::launch_fill(h->d_out, (int64_t)h->n_out * h->out_rows * h->N, std::numeric_limits<double>::quiet_NaN(), h->stream));
    } else if (h->rows > 1)
        for (int32_t v = 1; v < h->V; ++v)
            HIPCHK(rscm::launch_fill(h->series(v) + h->N, (int64_t)(h->rows - 1) * h->N,
                                     std::numeric_limits<double>::quiet_NaN(), h->stream));
    h->time_index = 0;
    h->rows_written();
    h->ocean_forget_partial_sums();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_clear_rows_after(rscm_ens* h, int32_t tidx)
{
    GUARD_BEGIN
    NEED(h);
    if (tidx < 0 || tidx > h->T - 1) return fail(RSCM_ERR_INVALID, "time index %d out of range", tidx);
    if (int rc = set_device(h)) return rc;
    if (h->windowed) {
        const int32_t first = std::max(0, tidx + 1 - h->win0);
        HIPCHK(rscm::launch_fill_rows(h->d_series, h->N, h->rows, h->V - 1, first, std::numeric_limits<double>::quiet_NaN(), h->stream));
    } else if (h->rows == h->T && tidx < h->T - 1)
        for (int32_t v = 1; v < h->V; ++v)
            HIPCHK(rscm::launch_fill(h->series(v) + (size_t)(tidx + 1) * h->N, (int64_t)(h->T - 1 - tidx) * h->N,
                                     std::numeric_limits<double>::quiet_NaN(), h->stream));
    h->rows_written();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_run_async(rscm_ens* h, int32_t step_begin, int32_t step_end)
{
    GUARD_BEGIN
    return run_range(h, step_begin, step_end, true);
    GUARD_END
}

int rscm_ens_sync(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_run(rscm_ens* h, int32_t step_begin, int32_t step_end)
{
    if (int rc = rscm_ens_run_async(h, step_begin, step_end)) return rc;
    return rscm_ens_sync(h);
}

int rscm_ens_last_run_plan(rscm_ens* h, int32_t* member_blocks, int32_t* step_chunks)
{
    NEED(h);
    if (member_blocks) *member_blocks = h->last_blocks;
    if (step_chunks) *step_chunks = h->last_chunks;
    return RSCM_OK;
}

int rscm_ens_last_run_ms(rscm_ens* h, float* out_ms)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_ms) return fail(RSCM_ERR_INVALID, "out_ms is NULL");
    if (!h->timed) return fail(RSCM_ERR_STATE, "no run has been launched yet");
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(out_ms, h->ev0, h->ev1));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_get_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride,
                        int64_t m_begin, int64_t m_end, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!h->has_rows(var_id)) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (t_begin < 0 || t_end > h->T || t_begin > t_end || t_stride < 1)
        return fail(RSCM_ERR_INVALID, "bad time range [%d, %d) stride %d", t_begin, t_end, t_stride);
    if (!h->windowed && h->rows != h->T && t_end > 1)
        return fail(RSCM_ERR_STATE, "this handle stores only the initial row (RSCM_FLAG_NO_SERIES)");
    if (m_begin < 0 || m_end > h->N || m_begin > m_end || !out)
        return fail(RSCM_ERR_INVALID, "bad member range [%lld, %lld)", (long long)m_begin, (long long)m_end);
    const bool diagnostic = h->is_diagnostic(var_id);
    if (int rc = check_diagnostic_current(h, var_id)) return rc;
    const int64_t width = m_end - m_begin;
    if (width == 0 || t_begin == t_end) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    if (h->windowed || diagnostic) {  // row by row from wherever each row is resident: the output store or the window; a diagnostic's store
        int64_t r = 0;
        for (int32_t t = t_begin; t < t_end; t += t_stride, ++r) {
            double* dst = out + r * width;
            if (t > h->time_index) {
                for (int64_t m = 0; m < width; ++m) dst[m] = std::numeric_limits<double>::quiet_NaN();
                continue;
            }
            const double* src = h->row_ptr(var_id, t);
            if (!src && diagnostic) {
                (void)hipStreamSynchronize(h->stream);   // the copies enqueued so far read the caller's buffer no longer
                return fail(RSCM_ERR_STATE, "row %d of diagnostic %d is not held: rscm_ens_compute_diagnostic over a range with it first", t, var_id);
            }
            if (!src)
                return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident: the window holds [%d, %d) and the output store every %d-th row%s",
                            t, var_id, h->win0, h->win0 + h->rows, h->out_stride, h->out_slot[var_id] < 0 ? " of other variables" : "");
            HIPCHK(hipMemcpyAsync(dst, src + m_begin, (size_t)width * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        return RSCM_OK;
    }
    // rows beyond the current time index were never computed by this model instance: NaN
    int64_t n_rows = 0, n_valid = 0;
    for (int32_t t = t_begin; t < t_end; t += t_stride) {
        ++n_rows;
        if (t <= h->time_index) ++n_valid;
    }
    if (n_valid > 0)
        HIPCHK(hipMemcpy2DAsync(out, (size_t)width * sizeof(double),
                                h->series(var_id) + (size_t)t_begin * h->N + m_begin,
                                (size_t)h->N * sizeof(double) * (size_t)t_stride, (size_t)width * sizeof(double),
                                (size_t)n_valid, hipMemcpyDeviceToHost, h->stream));
    for (int64_t r = n_valid; r < n_rows; ++r)
        for (int64_t m = 0; m < width; ++m) out[r * width + m] = std::numeric_limits<double>::quiet_NaN();
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_series_devptr(rscm_ens* h, int32_t var_id, void** out)
{
    NEED(h);
    if (!out || var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (h->windowed) return fail(RSCM_ERR_STATE, "a windowed ensemble has no contiguous [T][N] series: read rows with rscm_ens_get_series");
    *out = h->series(var_id);
    return RSCM_OK;
}

int rscm_ens_params_devptr(rscm_ens* h, void** out)
{
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = h->d_params;
    // Whatever the caller writes there, now or later through a pointer it kept: from here on no row of this
    // handle is ever treated as uniform again (rscm_ens_set_params keeps the flag clear as well).
    h->params_exposed = true;
    h->uniform_rows = 0;
    h->params_may_change();   // (and noise_cache_kept() is false from here on; the diagnostics' epoch does not move: rscm_gpu.h)
    h->params_set = true;  // the caller fills it on the device
    return RSCM_OK;
}

int rscm_ens_status(rscm_ens* h, uint8_t* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipMemcpyAsync(out, h->d_status, (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_status_devptr(rscm_ens* h, void** out)
{
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = h->d_status;
    return RSCM_OK;
}

// Everything rscm_ens_run_loglik needs of the handle besides the observations.
int check_loglik_ready(rscm_ens* h)
{
    if (h->time_index != 0) return fail(RSCM_ERR_STATE, "run_loglik starts from time index 0 (call rscm_ens_rewind)");
    if (!h->params_set) return fail(RSCM_ERR_STATE, "parameters not set");
    if (h->n_linked) return fail(RSCM_ERR_STATE, "the fused run+likelihood launch takes no linked inputs: use rscm_ens_run and rscm_ens_loglik");
    if (!h->forcing_set) return fail(RSCM_ERR_STATE, "shared input series not set");
    for (int32_t v = 1; v < h->V; ++v)
        if (h->is_state(v) && !h->initial_set[v])
            return fail(RSCM_ERR_STATE, "state variable %d has no initial value (MissingInitialValue)", v);
    if (int rc = set_device(h)) return rc;
    return refresh_schedule(h);
}

int rscm_gpu_copy_to_device(int32_t device_id, void* device_ptr, const void* host, int64_t n_bytes)
{
    GUARD_BEGIN
    if (n_bytes < 0 || (n_bytes > 0 && (!host || !device_ptr))) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n_bytes == 0) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipMemcpy(device_ptr, host, (size_t)n_bytes, hipMemcpyHostToDevice));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_summary_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id < 1 || var_id >= h->V || t_begin < 0 || t_end > h->T || t_begin > t_end || !out)
        return fail(RSCM_ERR_INVALID, "bad variable / time range");
    if (h->windowed || h->rows != h->T) return fail(RSCM_ERR_STATE, "this handle does not store whole series (RSCM_FLAG_NO_SERIES / RSCM_FLAG_WINDOWED): use rscm_ens_summary row by row");
    const int32_t n_rows = t_end - t_begin;
    // rows beyond the current time index have not been computed: empty summaries, as rscm_ens_summary
    const int32_t computed = std::max(0, std::min(t_end, h->time_index + 1) - t_begin);
    for (int32_t r = computed; r < n_rows; ++r) {
        out[4 * r + 0] = 0.0; out[4 * r + 1] = 0.0;
        out[4 * r + 2] = std::numeric_limits<double>::infinity();
        out[4 * r + 3] = -std::numeric_limits<double>::infinity();
    }
    if (computed == 0) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    const int32_t nb = rscm::summary_blocks(h->N);
    rscm::DevBuf<double> d_partial, d_out;
    HIPCHK(d_partial.alloc((size_t)computed * nb * 4));
    HIPCHK(d_out.alloc((size_t)computed * 4));
    HIPCHK(rscm::launch_summary_rows(h->series(var_id) + (size_t)t_begin * h->N, h->N, computed, d_partial.get(), nb, d_out.get(), h->stream));
    HIPCHK(hipMemcpyAsync(out, d_out.get(), (size_t)computed * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_summary(rscm_ens* h, int32_t var_id, int32_t tidx, double out[4])
{
    GUARD_BEGIN
    NEED(h);
    if (!h->has_rows(var_id) || tidx < 0 || tidx >= h->T || !out)
        return fail(RSCM_ERR_INVALID, "bad variable/time index");
    if (int rc = check_diagnostic_current(h, var_id)) return rc;
    if (tidx > h->time_index) {
        out[0] = 0.0; out[1] = 0.0;
        out[2] = std::numeric_limits<double>::infinity();
        out[3] = -std::numeric_limits<double>::infinity();
        return RSCM_OK;
    }
    if (int rc = set_device(h)) return rc;
    const int32_t nb = rscm::summary_blocks(h->N);
    const double* row = h->row_ptr(var_id, tidx);
    if (!row) return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident on this handle", tidx, var_id);
    HIPCHK(rscm::launch_summary_rows(row, h->N, 1, h->d_partial, nb, h->d_out4, h->stream));
    HIPCHK(hipMemcpyAsync(out, h->d_out4, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_sample_lhs(rscm_ens* h, uint64_t seed, const double* low, const double* high,
                        int64_t member_offset, int64_t n_total)
{
    GUARD_BEGIN
    NEED(h);
    if (!low || !high) return fail(RSCM_ERR_INVALID, "low/high is NULL");
    if (member_offset < 0 || n_total < 1 || member_offset + h->N > n_total)
        return fail(RSCM_ERR_INVALID, "member block [%lld, %lld) outside the global ensemble of %lld",
                    (long long)member_offset, (long long)(member_offset + h->N), (long long)n_total);
    if (int rc = set_device(h)) return rc;
    if (h->kind != RSCM_KIND_N2O_CHEMISTRY)   // (N2O's delay may vary over the members: the look-back is sized for the largest)
        for (int32_t j = 0; j < h->P; ++j)
            if (const char* name = structural_row(h->kind, j))
                if (low[j] != high[j])
                    return fail(RSCM_ERR_INVALID, "parameter row %d (%s) is structural: low must equal high", j, name);
    if (h->kind == RSCM_KIND_UDEB)
        if (int rc = configure_udeb(h, 1, [&](int j, int64_t) { return low[j]; })) return rc;
    if (h->kind == RSCM_KIND_OCEAN_CARBON)
        if (int rc = configure_ocean(h, 1, [&](int j, int64_t) { return low[j]; })) return rc;
    if (h->kind == RSCM_KIND_N2O_CHEMISTRY) h->lookback = (int32_t)std::min(std::max(1.0, high[4]), 1e6) + 1;
    if (h->kind == RSCM_KIND_GHG_FORCING) {
        const double m = low[RSCM_GH_P_METHOD];
        if (m != 0.0 && m != 1.0) return fail(RSCM_ERR_INVALID, "GhgForcing method must be 0 or 1");
        h->ghg_method = (int32_t)m;
    }
    rscm::DevBuf<double> d_lh;   // [P] low, then [P] high
    HIPCHK(d_lh.alloc(2 * (size_t)h->P));
    HIPCHK(hipMemcpyAsync(d_lh.get(), low, (size_t)h->P * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_lh.get() + h->P, high, (size_t)h->P * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(rscm::launch_lhs(h->d_params, h->P, h->N, seed, d_lh.get(), d_lh.get() + h->P, member_offset, n_total, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->uniform_rows = 0;   // conservatively: low + u (high - low) need not reproduce low's bits for every u
    h->params_written();
    h->params_set = true;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_get_params(rscm_ens* h, double* out_soa)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_soa) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipMemcpyAsync(out_soa, h->d_params, (size_t)h->P * h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_copy_to_host(int32_t device_id, void* host, const void* device_ptr, int64_t n_bytes)
{
    GUARD_BEGIN
    if (n_bytes < 0 || (n_bytes > 0 && (!host || !device_ptr))) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n_bytes == 0) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipMemcpy(host, device_ptr, (size_t)n_bytes, hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_host_alloc(int64_t n_bytes, void** out)
{
    GUARD_BEGIN
    if (!out || n_bytes <= 0) return fail(RSCM_ERR_INVALID, "bad arguments");
    *out = nullptr;
    HIPCHK(hipHostMalloc(out, (size_t)n_bytes, hipHostMallocDefault));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_host_free(void* p)
{
    GUARD_BEGIN
    if (p) HIPCHK(hipHostFree(p));
    return RSCM_OK;
    GUARD_END
}

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

// The one writer of a handle's forcing-noise setting (ens.hpp).  sigma: white and red; phi: red; 0 where the kind does not read them
static int set_noise(rscm_ens* h, int32_t kind, uint64_t seed, double sigma, double phi, int64_t member_offset)
{
    GUARD_BEGIN
    if (kind != rscm::kNoiseKindNone) {
        if (h->kind != RSCM_KIND_TWO_LAYER)
            return fail(RSCM_ERR_INVALID, "forcing noise is available for the two-layer kind only (RSCM_KIND_TWO_LAYER), this handle has kind %d", h->kind);
        if (!(sigma >= 0.0) || !std::isfinite(sigma)) return fail(RSCM_ERR_INVALID, "sigma must be finite and not negative, got %g", sigma);
        if (!std::isfinite(phi) || !(std::fabs(phi) < 1.0)) return fail(RSCM_ERR_INVALID, "phi must be finite with |phi| < 1, got %g", phi);
        if (member_offset < 0) return fail(RSCM_ERR_INVALID, "member_offset must not be negative, got %lld", (long long)member_offset);
        if (h->windowed || h->rows != h->T)
            return fail(RSCM_ERR_INVALID, "forcing noise needs a handle that stores its whole series (no windowed storage, no RSCM_FLAG_NO_SERIES)");
        if (h->n_linked > 0) return fail(RSCM_ERR_INVALID, "this handle has a linked input: the noise is added to a handle's own shared forcing");
    }
    if (rscm::noise_kind_keeps_state(kind) && !h->d_noise_state) {
        if (int rc = set_device(h)) return rc;
        HIPCHK(h->d_noise_state.alloc((size_t)h->N));
    }
    h->noise_kind = kind;
    h->noise_seed = seed;
    h->noise_sigma = sigma;
    h->noise_phi = phi;
    h->noise_offset = member_offset;
    h->noise_state_index = -1;   // the cache belonged to the setting before
    h->rows_written();           // and so did every row a run has written
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_forcing_noise_ar1(rscm_ens* h, uint64_t seed, double sigma, double phi, int64_t member_offset)
{
    NEED(h);
    if (phi == 0.0) return set_noise(h, rscm::kNoiseKindWhite, seed, sigma, 0.0, member_offset);   // (-0.0 is white too: the white kernels, no buffer)
    return set_noise(h, rscm::kNoiseKindRed, seed, sigma, phi, member_offset);
}

int rscm_ens_set_forcing_noise(rscm_ens* h, uint64_t seed, double sigma, int64_t member_offset)
{
    NEED(h);
    return set_noise(h, rscm::kNoiseKindWhite, seed, sigma, 0.0, member_offset);
}

int rscm_ens_set_forcing_noise_members(rscm_ens* h, uint64_t seed, int64_t member_offset)
{
    NEED(h);
    if (!h->noise_rows)
        return fail(RSCM_ERR_INVALID, "this handle has no noise parameter rows: create it with RSCM_FLAG_NOISE_PARAMS");
    return set_noise(h, rscm::kNoiseKindMembers, seed, 0.0, 0.0, member_offset);   // sigma and phi are the rows'
}

int rscm_ens_clear_forcing_noise(rscm_ens* h)
{
    NEED(h);
    return set_noise(h, rscm::kNoiseKindNone, 0, 0.0, 0.0, 0);
}

int rscm_ens_forcing_noise(const rscm_ens* h, int32_t* on, uint64_t* seed, double* sigma, int64_t* member_offset)
{
    NEED(h);
    if (on) *on = h->noise_kind != rscm::kNoiseKindNone ? 1 : 0;
    if (seed) *seed = h->noise_seed;
    if (sigma) *sigma = h->noise_sigma;
    if (member_offset) *member_offset = h->noise_offset;
    return RSCM_OK;
}

int rscm_ens_forcing_noise_ar1(const rscm_ens* h, double* phi, int32_t* cached_index)
{
    NEED(h);
    if (phi) *phi = h->noise_phi;
    if (cached_index) *cached_index = h->noise_red() ? h->noise_state_index : -1;
    return RSCM_OK;
}

int rscm_ens_forcing_noise_members(const rscm_ens* h, int32_t* per_member, int32_t* sigma_row, int32_t* phi_row)
{
    NEED(h);
    if (per_member) *per_member = h->noise_kind == rscm::kNoiseKindMembers ? 1 : 0;
    if (sigma_row) *sigma_row = h->noise_sigma_row();
    if (phi_row) *phi_row = h->noise_phi_row();
    return RSCM_OK;
}

int rscm_ens_forcing_noise_rows(rscm_ens* h, int32_t t_begin, int32_t t_end, double* out, int32_t on_device)
{
    GUARD_BEGIN
    NEED(h);
    if (!h->noise_kind) return fail(RSCM_ERR_STATE, "this handle has no forcing noise (rscm_ens_set_forcing_noise)");
    if (t_begin < 0 || t_end < t_begin || t_end > h->T)
        return fail(RSCM_ERR_INVALID, "rows [%d, %d) are not within the forcing axis [0, %d)", t_begin, t_end, h->T);
    if (t_end == t_begin) return RSCM_OK;
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    const size_t elems = (size_t)(t_end - t_begin) * (size_t)h->N;
    rscm::DevBuf<double> tmp;   // host output: the rows are formed here
    if (!on_device) HIPCHK(tmp.alloc(elems));
    double* d = on_device ? out : tmp.get();
    HIPCHK(rscm::launch_forcing_noise_rows(h->noise_kind, h->noise_seed, h->noise_sigma, h->noise_phi, h->d_params, h->uniform_rows,
                                           h->noise_sigma_row(), h->noise_phi_row(), h->noise_offset, h->N, t_begin, t_end, d, h->stream));
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(out, d, elems * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_selftest_normal(const uint64_t* k52, int64_t n, double* z)
{
    GUARD_BEGIN
    if (n < 0 || !k52 || !z) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n == 0) return RSCM_OK;
    rscm::DevBuf<double> buf;   // [n] integers, then [n] deviates
    HIPCHK(buf.alloc(2 * (size_t)n));
    double* d = buf.get();
    HIPCHK(hipMemcpy(d, k52, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(rscm::launch_normal_selftest(reinterpret_cast<const uint64_t*>(d), n, d + n, nullptr));
    HIPCHK(hipMemcpy(z, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_selftest_math(int32_t op, int64_t n, const double* x, const double* y, double* out)
{
    GUARD_BEGIN
    const bool two = op == 3;   // pow_ratio reads y
    if (op < 0 || op >= rscm::kMathTestOps) return fail(RSCM_ERR_INVALID, "selftest_math: op %d is not in [0, %d)", op, rscm::kMathTestOps);
    if (n < 0 || !x || !out || (two && !y)) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n == 0) return RSCM_OK;
    rscm::DevBuf<double> buf;   // [n] x, [n] out, then [n] y for the two-argument op
    HIPCHK(buf.alloc((two ? 3 : 2) * (size_t)n));
    double* d = buf.get();
    HIPCHK(hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    if (two) HIPCHK(hipMemcpy(d + 2 * n, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(rscm::launch_mathtest(op, d, two ? d + 2 * n : nullptr, d + n, n, nullptr));
    HIPCHK(hipMemcpy(out, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_selftest_div(int32_t device_id, int64_t n, const double* num, const double* den,
                          double* out_ref, double* out_fast, uint8_t* used_fast)
{
    GUARD_BEGIN
    if (n < 0 || !num || !den || !out_ref || !out_fast || !used_fast) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n == 0) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    rscm::DevBuf<double> buf;   // [n] num, den, out_ref, out_fast
    rscm::DevBuf<uint8_t> du;
    HIPCHK(buf.alloc(4 * (size_t)n));
    HIPCHK(du.alloc((size_t)n));
    double* d = buf.get();
    HIPCHK(hipMemcpy(d, num, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + n, den, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(rscm::launch_divtest(d, d + n, d + 2 * n, d + 3 * n, du.get(), n, nullptr));
    HIPCHK(hipMemcpy(out_ref, d + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_fast, d + 3 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(used_fast, du.get(), (size_t)n, hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
