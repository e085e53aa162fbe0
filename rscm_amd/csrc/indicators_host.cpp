// Host side of the handle's baseline (rscm_ens_set_baseline*, the anomaly select's b[i]), of the per-member indicators
// (rscm_ens_member_indicators) and of the exceedance counts (rscm_ens_exceedance, rscm_ens_exceedance_grouped); kernels in indicators.hip.
// Also of the per-member variability statistics (rscm_ens_member_variability), which share the rows and the slots of the indicators,
// and of the Gaussian likelihood over per-member vectors (rscm_ens_loglik_vectors_device); kernels in variability.hip.
// Also of the per-member band powers (rscm_ens_member_spectrum), their coefficient table (rscm_gpu_spectrum_coefficients) and the
// spectral likelihood over band powers (rscm_ens_loglik_spectrum_device); kernels in spectrum.hip.
// Also of the per-member covariability of two variables (rscm_ens_member_covariability); kernel in covariability.hip.
// Also of their co-spectra in frequency bands (rscm_ens_member_cross_spectrum) and its sine table (rscm_gpu_spectrum_sines); kernel in
// cross_spectrum.hip.
//
// Rows are resolved as the radix select resolves them (resolve_rows: full storage, the window, the output store) and must all be
// computed.  The baseline and the indicator slots are handle-owned and kept across run and rewind, as the member weights are; a
// staged select may read either, so neither changes while one is in flight.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "ens.hpp"

// The device row pointers and row times of the computed rows t_begin, t_begin + t_stride, ... < t_end of var_id; every row of the
// range must be computed and resident
int period_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, std::vector<const double*>& rows,
                std::vector<double>& times)
{
    if (int rc = check_row_range(h, var_id, t_begin, t_end, t_stride, true)) return rc;
    if (int rc = check_series_stored(h, t_end)) return rc;
    int32_t n_range = 0;
    if (int rc = resolve_rows(h, var_id, t_begin, t_end, t_stride, rows, &n_range)) return rc;
    if ((int32_t)rows.size() != n_range)
        return fail(RSCM_ERR_STATE, "rows of [%d, %d) are beyond the current time index %d", t_begin, t_end, h->time_index);
    for (int32_t t = t_begin; t < t_end; t += t_stride) times.push_back(h->bounds[t]);
    return RSCM_OK;
}

namespace {

// The device array of the row pointers, enqueued on the handle's stream: rows must live until the caller has synchronised it
int upload_rows(rscm_ens* h, const std::vector<const double*>& rows, rscm::DevBuf<const double*>& d_rows)
{
    HIPCHK(d_rows.alloc(rows.size()));
    HIPCHK(hipMemcpyAsync(d_rows.get(), rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice, h->stream));
    return RSCM_OK;
}

rscm::Thresholds thresholds(int32_t n_thr, const double* thr)
{
    rscm::Thresholds th{};
    for (int32_t k = 0; k < n_thr; ++k) th.v[k] = thr[k];
    return th;
}

// Runs the indicator kernel over the rows into d_out ([1][N] with all false, else [3 + n_thr][N]) and waits for it
int run_indicators(rscm_ens* h, const std::vector<const double*>& rows, const std::vector<double>& times, const double* d_base, bool all,
                   int32_t n_thr, const double* thr, double* d_out)
{
    rscm::DevBuf<const double*> d_rows;
    rscm::DevBuf<double> d_time;
    if (int rc = upload_rows(h, rows, d_rows)) return rc;
    HIPCHK(d_time.alloc(times.size()));
    HIPCHK(hipMemcpyAsync(d_time.get(), times.data(), times.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(rscm::launch_indicators(d_rows.get(), d_time.get(), (int32_t)rows.size(), d_base, h->N, all, n_thr, thresholds(n_thr, thr), d_out,
                                   h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
}

int check_thresholds(int32_t n_thr, const double* thr, int32_t lo)
{
    if (n_thr < lo || n_thr > rscm::kMaxThresholds || (n_thr > 0 && !thr))
        return fail(RSCM_ERR_INVALID, "bad threshold list (%d to %d thresholds)", lo, rscm::kMaxThresholds);
    return RSCM_OK;
}

int no_select(const rscm_ens* h)
{
    if (h->select) return fail(RSCM_ERR_STATE, "a select is in flight on this handle: rscm_ens_select_end it first");
    return RSCM_OK;
}

// The slots of rscm_ens_member_indicators, _variability and _spectrum: the check, and the slot's buffer, allocated at first use
int check_slot(int32_t slot)
{
    if (slot < 0 || slot >= rscm_ens::kIndSlots) return fail(RSCM_ERR_INVALID, "slot %d: must be in [0, %d)", slot, rscm_ens::kIndSlots);
    return RSCM_OK;
}

int slot_buffer(rscm_ens* h, int32_t slot)
{
    HIPCHK(h->d_ind[slot].reserve((size_t)(3 + rscm::kMaxThresholds) * (size_t)h->N));
    return RSCM_OK;
}

int check_detrending(int32_t mode)
{
    if (mode != RSCM_VAR_MEAN && mode != RSCM_VAR_LINEAR && mode != RSCM_VAR_DIFFERENCE)
        return fail(RSCM_ERR_INVALID, "unknown detrending mode %d (RSCM_VAR_MEAN, RSCM_VAR_LINEAR, RSCM_VAR_DIFFERENCE)", mode);
    return RSCM_OK;
}

// The working series of n_rows rows under a detrending mode: its length n, 3 to max_terms (0: no upper bound), and stt = n (n^2 - 1) / 12
struct WorkingSeries {
    int64_t n = 0;
    double stt = 0.0;
};
int working_series(size_t n_rows, int32_t mode, int32_t max_terms, WorkingSeries* w)
{
    const int64_t n = (int64_t)n_rows - (mode == RSCM_VAR_DIFFERENCE ? 1 : 0);
    if (n < 3 && !max_terms) return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: at least 3 are needed", (int)n_rows, (long long)n);
    if (max_terms && (n < 3 || n > max_terms))
        return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: 3 to %d are needed", (int)n_rows, (long long)n, max_terms);
    w->n = n;
    w->stt = (double)(n * (n * n - 1)) / 12.0;
    return RSCM_OK;
}

static_assert(rscm::kVarMean == RSCM_VAR_MEAN && rscm::kVarLinear == RSCM_VAR_LINEAR && rscm::kVarDifference == RSCM_VAR_DIFFERENCE,
              "the detrending modes in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(5 <= 3 + rscm::kMaxThresholds, "the variability statistics share the indicator slots");
static_assert(rscm::kCovMaxLags == RSCM_COV_MAX_LAGS && 5 + 2 * RSCM_COV_MAX_LAGS <= 3 + rscm::kMaxThresholds,
              "the covariability statistics at every lag share the indicator slots");
static_assert(rscm::kMaxCrossSpectrumBands == RSCM_XSPEC_MAX_BANDS && 2 + 3 * RSCM_XSPEC_MAX_BANDS <= 3 + rscm::kMaxThresholds,
              "the cross-spectrum statistics of every band share the indicator slots");

constexpr int32_t kSpectrumMaxTerms = 4096;   // the cap on the working series' length that bounds the recurrence's error

// c2[j - 1] = 2 C_j, C_j the double nearest cos(2 pi j / n), j = 1 .. (n - 1) / 2.  The angle is pi p / q with p = 2 j, q = n, 0 < p / q < 1;
// in integers it is folded first into the first quadrant (p -> q - p, the sign kept) and then into the first octant, where the cosine
// of the complement is the sine of what is left: both functions are evaluated in long double below pi / 4 only, so no argument loses
// bits to cancellation near pi / 2, and 2 p == q is +0.0 exactly.
void spectrum_coefficients(int32_t n, double* c2)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    const int64_t q = n;
    for (int64_t j = 1; j <= (n - 1) / 2; ++j) {
        int64_t p = 2 * j;
        const bool neg = 2 * p > q;
        if (neg) p = q - p;
        long double v;
        if (2 * p == q)
            v = 0.0L;
        else if (4 * p <= q)
            v = cosl(pi * (long double)p / (long double)q);
        else
            v = sinl(pi * (long double)(q - 2 * p) / (long double)(2 * q));
        const double C = (double)v;
        c2[j - 1] = 2.0 * (neg ? -C : C);
    }
}

// g[j - 1] = the double nearest sin(2 pi j / n), j = 1 .. (n - 1) / 2: the same angle pi p / q, folded in integers into the first quadrant
// (p -> q - p: the sine keeps its sign) and then into the first octant, where the sine of the complement is the cosine of what is left;
// 2 p == q is 1.0 exactly.  j < n / 2 keeps every entry > 0.
void spectrum_sines(int32_t n, double* g)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    const int64_t q = n;
    for (int64_t j = 1; j <= (n - 1) / 2; ++j) {
        int64_t p = 2 * j;
        if (2 * p > q) p = q - p;
        long double v;
        if (2 * p == q)
            v = 1.0L;
        else if (4 * p <= q)
            v = sinl(pi * (long double)p / (long double)q);
        else
            v = cosl(pi * (long double)(q - 2 * p) / (long double)(2 * q));
        g[j - 1] = (double)v;
    }
}

// The band list of rscm_ens_member_spectrum and rscm_ens_member_cross_spectrum against a working series of n terms
int check_band_edges(int64_t n, int32_t n_bands, const int32_t* edges)
{
    const int32_t J = (int32_t)((n - 1) / 2);
    if (edges[0] < 1 || edges[n_bands] > J + 1) return fail(RSCM_ERR_INVALID, "the band edges must lie in [1, %d] (J + 1 of %lld terms)", J + 1, (long long)n);
    for (int32_t b = 0; b < n_bands; ++b)
        if (edges[b] >= edges[b + 1]) return fail(RSCM_ERR_INVALID, "the band edges must be strictly ascending (edge %d)", b + 1);
    return RSCM_OK;
}

// What the two likelihoods over per-member vectors check once their own numbers are in: every vector and add_dev (may be null) is a
// member vector of the handle's device; vec takes the vectors, and d_loglik is there
int loglik_vector_list(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, const double* add_dev, const double** vec)
{
    if (int rc = set_device(h)) return rc;
    for (int32_t j = 0; j < n_vec; ++j) {
        char what[24];
        std::snprintf(what, sizeof what, "vector %d", j);
        if (int rc = check_member_vector(h, vec_dev[j], what)) return rc;
        vec[j] = vec_dev[j];
    }
    if (add_dev)
        if (int rc = check_member_vector(h, add_dev, "add_dev")) return rc;
    HIPCHK(h->d_loglik.reserve((size_t)h->N));
    return RSCM_OK;
}

// rscm_ens_exceedance and, grouped, rscm_ens_exceedance_grouped: hits[G][n_thr] and total[G] over G = the handle's groups, else 1
int exceedance(rscm_ens* h, const double* vec_dev, int32_t n_thr, const double* thr, int32_t weighted, bool grouped, int64_t* hits,
               int64_t* total)
{
    if (!total || (n_thr > 0 && !hits)) return fail(RSCM_ERR_INVALID, "hits or total is NULL");
    if (int rc = check_thresholds(n_thr, thr, 0)) return rc;
    if (grouped && !h->d_groups) return fail(RSCM_ERR_STATE, "no member groups: rscm_ens_set_member_groups first");
    if (weighted && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if (int rc = set_device(h)) return rc;
    if (int rc = check_member_vector(h, vec_dev, "vector")) return rc;
    const rscm::Thresholds th = thresholds(n_thr, thr);
    const int64_t* d_w = weighted ? h->d_weights : nullptr;
    const int32_t G = grouped ? h->n_groups : 1;
    std::vector<unsigned long long> acc((size_t)G * (n_thr + 1));
    rscm::DevBuf<unsigned long long> d_acc;
    HIPCHK(d_acc.alloc(acc.size()));
    HIPCHK(hipMemsetAsync(d_acc.get(), 0, acc.size() * sizeof(unsigned long long), h->stream));
    if (grouped)
        HIPCHK(rscm::launch_exceedance_grouped(vec_dev, d_w, h->d_groups, G, h->N, n_thr, th, d_acc.get(), h->stream));
    else
        HIPCHK(rscm::launch_exceedance(vec_dev, d_w, h->N, n_thr, th, d_acc.get(), h->stream));
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc.get(), acc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int32_t g = 0; g < G; ++g) {
        for (int32_t k = 0; k < n_thr; ++k) hits[(size_t)g * n_thr + k] = (int64_t)acc[(size_t)g * (n_thr + 1) + k];
        total[g] = (int64_t)acc[(size_t)g * (n_thr + 1) + n_thr];
    }
    return RSCM_OK;
}

}  // namespace

extern "C" {

int rscm_ens_set_baseline(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, var_id, t_begin, t_end, t_stride, rows, times)) return rc;
    if (int rc = set_device(h)) return rc;
    rscm::DevBuf<double> d_new;
    HIPCHK(d_new.alloc((size_t)h->N));
    if (int rc = run_indicators(h, rows, times, nullptr, false, 0, nullptr, d_new.get())) return rc;
    h->d_base = std::move(d_new);
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_baseline_values(rscm_ens* h, const double* b, int32_t on_device)
{
    GUARD_BEGIN
    NEED(h);
    if (!b) return fail(RSCM_ERR_INVALID, "baseline is NULL");
    if (int rc = no_select(h)) return rc;
    if (int rc = set_device(h)) return rc;
    if (on_device)
        if (int rc = check_member_vector(h, b, "baseline")) return rc;
    rscm::DevBuf<double> d_new;
    HIPCHK(d_new.alloc((size_t)h->N));
    HIPCHK(hipMemcpyAsync(d_new.get(), b, (size_t)h->N * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->d_base = std::move(d_new);
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_baseline_devptr(rscm_ens* h, void** out)
{
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = h->d_base;
    if (!h->d_base) return fail(RSCM_ERR_STATE, "no baseline set");
    return RSCM_OK;
}

int rscm_ens_clear_baseline(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = no_select(h)) return rc;
    if (h->d_base) {
        if (int rc = set_device(h)) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        h->d_base.reset();
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_member_indicators(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t anomaly, int32_t n_thr,
                               const double* thr, int32_t slot, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (int rc = check_slot(slot)) return rc;
    if (int rc = check_thresholds(n_thr, thr, 0)) return rc;
    if (anomaly && !h->d_base) return fail(RSCM_ERR_STATE, "no baseline: rscm_ens_set_baseline or rscm_ens_set_baseline_values first");
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, var_id, t_begin, t_end, t_stride, rows, times)) return rc;
    if (int rc = set_device(h)) return rc;
    if (int rc = slot_buffer(h, slot)) return rc;
    if (int rc = run_indicators(h, rows, times, anomaly ? h->d_base : nullptr, true, n_thr, thr, h->d_ind[slot])) return rc;
    *out_dev = h->d_ind[slot];
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_member_variability(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode, int32_t slot,
                                void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (int rc = check_slot(slot)) return rc;
    if (int rc = check_detrending(mode)) return rc;
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, var_id, t_begin, t_end, t_stride, rows, times)) return rc;
    WorkingSeries w;
    if (int rc = working_series(rows.size(), mode, 0, &w)) return rc;
    if (int rc = set_device(h)) return rc;
    if (int rc = slot_buffer(h, slot)) return rc;
    rscm::DevBuf<const double*> d_rows;
    if (int rc = upload_rows(h, rows, d_rows)) return rc;
    HIPCHK(rscm::launch_variability(d_rows.get(), (int32_t)rows.size(), mode, w.stt, h->N, h->d_ind[slot], h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out_dev = h->d_ind[slot];
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_member_covariability(rscm_ens* h, int32_t var_x, int32_t var_y, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode_x,
                                  int32_t mode_y, int32_t n_lags, int32_t slot, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (int rc = check_slot(slot)) return rc;
    if (int rc = check_detrending(mode_x)) return rc;
    if (int rc = check_detrending(mode_y)) return rc;
    if (n_lags < 0 || n_lags > RSCM_COV_MAX_LAGS) return fail(RSCM_ERR_INVALID, "n_lags = %d: must be in [0, %d]", n_lags, RSCM_COV_MAX_LAGS);
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows_x, rows_y;
    std::vector<double> times_x, times_y;
    if (int rc = period_rows(h, var_x, t_begin, t_end, t_stride, rows_x, times_x)) return rc;
    if (int rc = period_rows(h, var_y, t_begin, t_end, t_stride, rows_y, times_y)) return rc;
    // both working series have the length of the differenced one as soon as either variable is differenced (the other is taken at the midpoints)
    const bool differenced = mode_x == RSCM_VAR_DIFFERENCE || mode_y == RSCM_VAR_DIFFERENCE;
    WorkingSeries w;
    if (int rc = working_series(rows_x.size(), differenced ? RSCM_VAR_DIFFERENCE : RSCM_VAR_MEAN, 0, &w)) return rc;
    if (w.n < 3 + n_lags)
        return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: at least %d are needed at %d lags", (int)rows_x.size(), (long long)w.n,
                    3 + n_lags, n_lags);
    if (int rc = set_device(h)) return rc;
    if (int rc = slot_buffer(h, slot)) return rc;
    rscm::DevBuf<const double*> d_rows_x, d_rows_y;
    if (int rc = upload_rows(h, rows_x, d_rows_x)) return rc;
    if (int rc = upload_rows(h, rows_y, d_rows_y)) return rc;
    HIPCHK(rscm::launch_covariability(d_rows_x.get(), d_rows_y.get(), (int32_t)rows_x.size(), mode_x, mode_y, n_lags, w.stt, h->N, h->d_ind[slot],
                                      h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out_dev = h->d_ind[slot];
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_spectrum_coefficients(int32_t n, double* out)
{
    GUARD_BEGIN
    if (n < 3 || n > kSpectrumMaxTerms) return fail(RSCM_ERR_INVALID, "n = %d: the working series has 3 to %d terms", n, kSpectrumMaxTerms);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    spectrum_coefficients(n, out);
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_member_spectrum(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode, int32_t n_bands,
                             const int32_t* edges, int32_t slot, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (int rc = check_slot(slot)) return rc;
    if (int rc = check_detrending(mode)) return rc;
    if (n_bands < 1 || n_bands > rscm::kMaxSpectrumBands || !edges)
        return fail(RSCM_ERR_INVALID, "bad band list (1 to %d bands, n_bands + 1 edges)", rscm::kMaxSpectrumBands);
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, var_id, t_begin, t_end, t_stride, rows, times)) return rc;
    WorkingSeries w;
    if (int rc = working_series(rows.size(), mode, kSpectrumMaxTerms, &w)) return rc;
    const int64_t n = w.n;
    const int32_t J = (int32_t)((n - 1) / 2);
    if (int rc = check_band_edges(n, n_bands, edges)) return rc;
    // the table the kernel is given: c2[J], kSpectrumTablePad zeros the last tile may read, then the edges (8-byte aligned: int32 pairs)
    const size_t n_c2 = (size_t)J + rscm::kSpectrumTablePad;
    std::vector<double> table(n_c2 + (size_t)(n_bands + 2) / 2, 0.0);
    spectrum_coefficients((int32_t)n, table.data());
    std::memcpy(table.data() + n_c2, edges, (size_t)(n_bands + 1) * sizeof(int32_t));
    if (int rc = set_device(h)) return rc;
    if (int rc = slot_buffer(h, slot)) return rc;
    rscm::DevBuf<const double*> d_rows;
    rscm::DevBuf<double> d_table;
    if (int rc = upload_rows(h, rows, d_rows)) return rc;
    HIPCHK(d_table.alloc(table.size()));
    HIPCHK(hipMemcpyAsync(d_table.get(), table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(rscm::launch_spectrum(d_rows.get(), (int32_t)rows.size(), mode, w.stt, d_table.get(),
                                 reinterpret_cast<const int32_t*>(d_table.get() + n_c2), n_bands, h->N, h->d_ind[slot], h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out_dev = h->d_ind[slot];
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_spectrum_sines(int32_t n, double* out)
{
    GUARD_BEGIN
    if (n < 3 || n > kSpectrumMaxTerms) return fail(RSCM_ERR_INVALID, "n = %d: the working series has 3 to %d terms", n, kSpectrumMaxTerms);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    spectrum_sines(n, out);
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_member_cross_spectrum(rscm_ens* h, int32_t var_x, int32_t var_y, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode_x,
                                   int32_t mode_y, int32_t n_bands, const int32_t* edges, int32_t slot, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (int rc = check_slot(slot)) return rc;
    if (int rc = check_detrending(mode_x)) return rc;
    if (int rc = check_detrending(mode_y)) return rc;
    if (n_bands < 1 || n_bands > RSCM_XSPEC_MAX_BANDS || !edges)
        return fail(RSCM_ERR_INVALID, "bad band list (1 to %d bands, n_bands + 1 edges)", RSCM_XSPEC_MAX_BANDS);
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows_x, rows_y;
    std::vector<double> times_x, times_y;
    if (int rc = period_rows(h, var_x, t_begin, t_end, t_stride, rows_x, times_x)) return rc;
    if (int rc = period_rows(h, var_y, t_begin, t_end, t_stride, rows_y, times_y)) return rc;
    // the common length of rscm_ens_member_covariability's working series, under the spectrum's cap
    const bool differenced = mode_x == RSCM_VAR_DIFFERENCE || mode_y == RSCM_VAR_DIFFERENCE;
    WorkingSeries w;
    if (int rc = working_series(rows_x.size(), differenced ? RSCM_VAR_DIFFERENCE : RSCM_VAR_MEAN, kSpectrumMaxTerms, &w)) return rc;
    const int64_t n = w.n;
    const int32_t J = (int32_t)((n - 1) / 2);
    if (int rc = check_band_edges(n, n_bands, edges)) return rc;
    // the one table the kernel is given: c2[J] and the sines g[J], each followed by kSpectrumTablePad zeros the last tile may read, then
    // the edges (8-byte aligned: int32 pairs)
    const size_t n_tab = (size_t)J + rscm::kSpectrumTablePad;
    std::vector<double> table(2 * n_tab + (size_t)(n_bands + 2) / 2, 0.0);
    spectrum_coefficients((int32_t)n, table.data());
    spectrum_sines((int32_t)n, table.data() + n_tab);
    std::memcpy(table.data() + 2 * n_tab, edges, (size_t)(n_bands + 1) * sizeof(int32_t));
    if (int rc = set_device(h)) return rc;
    if (int rc = slot_buffer(h, slot)) return rc;
    rscm::DevBuf<const double*> d_rows_x, d_rows_y;
    rscm::DevBuf<double> d_table;
    if (int rc = upload_rows(h, rows_x, d_rows_x)) return rc;
    if (int rc = upload_rows(h, rows_y, d_rows_y)) return rc;
    HIPCHK(d_table.alloc(table.size()));
    HIPCHK(hipMemcpyAsync(d_table.get(), table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(rscm::launch_cross_spectrum(d_rows_x.get(), d_rows_y.get(), (int32_t)rows_x.size(), mode_x, mode_y, w.stt, d_table.get(),
                                       d_table.get() + n_tab, reinterpret_cast<const int32_t*>(d_table.get() + 2 * n_tab), n_bands, h->N,
                                       h->d_ind[slot], h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out_dev = h->d_ind[slot];
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_loglik_spectrum_device(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, const double* record, const int32_t* count,
                                    const double* add_dev, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (n_vec < 1 || n_vec > rscm::kMaxLoglikVectors || !vec_dev || !record || !count)
        return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors, each with the record's power and a count)", rscm::kMaxLoglikVectors);
    rscm::LoglikSpectrum v{};
    for (int32_t j = 0; j < n_vec; ++j) {
        if (!std::isfinite(record[j]) || !(record[j] > 0.0)) return fail(RSCM_ERR_INVALID, "vector %d: the record's power must be finite and > 0", j);
        if (count[j] < 1) return fail(RSCM_ERR_INVALID, "vector %d: the count must be >= 1", j);
        v.record[j] = record[j];
        v.count[j] = (double)count[j];
    }
    if (int rc = loglik_vector_list(h, n_vec, vec_dev, add_dev, v.vec)) return rc;
    HIPCHK(rscm::launch_loglik_spectrum(v, n_vec, add_dev, h->N, h->d_loglik, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out_dev = h->d_loglik;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_loglik_vectors_device(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, const double* value, const double* sigma,
                                   const double* add_dev, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (n_vec < 1 || n_vec > rscm::kMaxLoglikVectors || !vec_dev || !value || !sigma)
        return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors, each with a value and a sigma)", rscm::kMaxLoglikVectors);
    rscm::LoglikVectors v{};
    for (int32_t j = 0; j < n_vec; ++j) {
        if (!std::isfinite(value[j])) return fail(RSCM_ERR_INVALID, "vector %d: the target value is not finite", j);
        if (!std::isfinite(sigma[j]) || !(sigma[j] > 0.0)) return fail(RSCM_ERR_INVALID, "vector %d: sigma must be finite and > 0", j);
        v.value[j] = value[j];
        v.sigma[j] = sigma[j];
    }
    if (int rc = loglik_vector_list(h, n_vec, vec_dev, add_dev, v.vec)) return rc;
    HIPCHK(rscm::launch_loglik_vectors(v, n_vec, add_dev, h->N, h->d_loglik, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out_dev = h->d_loglik;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_exceedance(rscm_ens* h, const double* vec_dev, int32_t n_thr, const double* thr, int32_t weighted, int64_t* hits,
                        int64_t* total)
{
    GUARD_BEGIN
    NEED(h);
    return exceedance(h, vec_dev, n_thr, thr, weighted, false, hits, total);
    GUARD_END
}

int rscm_ens_exceedance_grouped(rscm_ens* h, const double* vec_dev, int32_t n_thr, const double* thr, int32_t weighted, int64_t* hits,
                                int64_t* total)
{
    GUARD_BEGIN
    NEED(h);
    return exceedance(h, vec_dev, n_thr, thr, weighted, true, hits, total);
    GUARD_END
}

}  // extern "C"
