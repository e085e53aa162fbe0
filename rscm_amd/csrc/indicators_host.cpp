// Host side of the handle's baseline (rscm_ens_set_baseline*, the anomaly select's b[i]), of the per-member indicators
// (rscm_ens_member_indicators) and of the exceedance counts (rscm_ens_exceedance, rscm_ens_exceedance_grouped); kernels in indicators.hip.
// Also of the per-member variability statistics (rscm_ens_member_variability), which share the rows and the slots of the indicators,
// and of the Gaussian likelihood over per-member vectors (rscm_ens_loglik_vectors_device); kernels in variability.hip.
// Also of the per-member band powers (rscm_ens_member_spectrum), their coefficient table (rscm_gpu_spectrum_coefficients) and the
// spectral likelihood over band powers (rscm_ens_loglik_spectrum_device); kernels in spectrum.hip.
//
// Rows are resolved as the radix select resolves them (resolve_rows: full storage, the window, the output store) and must all be
// computed.  The baseline and the indicator slots are handle-owned and kept across run and rewind, as the member weights are; a
// staged select may read either, so neither changes while one is in flight.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "ens.hpp"

namespace {

// The device row pointers and row times of the computed rows t_begin, t_begin + t_stride, ... < t_end of var_id; every row of the
// range must be computed and resident
int period_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, std::vector<const double*>& rows,
                std::vector<double>& times)
{
    if (var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (t_begin < 0 || t_end > h->T || t_begin >= t_end || t_stride < 1)
        return fail(RSCM_ERR_INVALID, "bad time range [%d, %d) stride %d (at least one row)", t_begin, t_end, t_stride);
    if (!h->windowed && h->rows != h->T && t_end > 1)
        return fail(RSCM_ERR_STATE, "this handle stores only the initial row (RSCM_FLAG_NO_SERIES)");
    int32_t n_range = 0;
    if (int rc = resolve_rows(h, var_id, t_begin, t_end, t_stride, rows, &n_range)) return rc;
    if ((int32_t)rows.size() != n_range)
        return fail(RSCM_ERR_STATE, "rows of [%d, %d) are beyond the current time index %d", t_begin, t_end, h->time_index);
    for (int32_t t = t_begin; t < t_end; t += t_stride) times.push_back(h->bounds[t]);
    return RSCM_OK;
}

// Runs the indicator kernel over the rows into d_out ([1][N] with all false, else [3 + n_thr][N]) and waits for it
int run_indicators(rscm_ens* h, const std::vector<const double*>& rows, const std::vector<double>& times, const double* d_base, bool all,
                   int32_t n_thr, const double* thr, double* d_out)
{
    rscm::Thresholds th{};
    for (int32_t k = 0; k < n_thr; ++k) th.v[k] = thr[k];
    const double** d_rows = nullptr;
    double* d_time = nullptr;
    hipError_t e = rscm::dev_malloc(&d_rows, rows.size() * sizeof(double*));
    if (e == hipSuccess) e = rscm::dev_malloc(&d_time, times.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_time, times.data(), times.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = rscm::launch_indicators(d_rows, d_time, (int32_t)rows.size(), d_base, h->N, all, n_thr, th, d_out, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(d_rows);
    (void)hipFree(d_time);
    HIPCHK(e);
    HIPCHK(es);
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

static_assert(rscm::kVarMean == RSCM_VAR_MEAN && rscm::kVarLinear == RSCM_VAR_LINEAR && rscm::kVarDifference == RSCM_VAR_DIFFERENCE,
              "the detrending modes in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(5 <= 3 + rscm::kMaxThresholds, "the variability statistics share the indicator slots");

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
    double* d_new = nullptr;
    HIPCHK(rscm::dev_malloc(&d_new, (size_t)h->N * sizeof(double)));
    if (int rc = run_indicators(h, rows, times, nullptr, false, 0, nullptr, d_new)) {
        (void)hipFree(d_new);
        return rc;
    }
    (void)hipFree(h->d_base);
    h->d_base = d_new;
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
    double* d_new = nullptr;
    HIPCHK(rscm::dev_malloc(&d_new, (size_t)h->N * sizeof(double)));
    hipError_t e = hipMemcpyAsync(d_new, b, (size_t)h->N * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                  h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipFree(d_new);
        HIPCHK(e);
    }
    (void)hipFree(h->d_base);
    h->d_base = d_new;
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
        (void)hipFree(h->d_base);
        h->d_base = nullptr;
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
    if (slot < 0 || slot >= rscm_ens::kIndSlots) return fail(RSCM_ERR_INVALID, "slot %d: must be in [0, %d)", slot, rscm_ens::kIndSlots);
    if (int rc = check_thresholds(n_thr, thr, 0)) return rc;
    if (anomaly && !h->d_base) return fail(RSCM_ERR_STATE, "no baseline: rscm_ens_set_baseline or rscm_ens_set_baseline_values first");
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, var_id, t_begin, t_end, t_stride, rows, times)) return rc;
    if (int rc = set_device(h)) return rc;
    if (!h->d_ind[slot]) HIPCHK(rscm::dev_malloc(&h->d_ind[slot], (size_t)(3 + rscm::kMaxThresholds) * (size_t)h->N * sizeof(double)));
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
    if (slot < 0 || slot >= rscm_ens::kIndSlots) return fail(RSCM_ERR_INVALID, "slot %d: must be in [0, %d)", slot, rscm_ens::kIndSlots);
    if (mode != RSCM_VAR_MEAN && mode != RSCM_VAR_LINEAR && mode != RSCM_VAR_DIFFERENCE)
        return fail(RSCM_ERR_INVALID, "unknown detrending mode %d (RSCM_VAR_MEAN, RSCM_VAR_LINEAR, RSCM_VAR_DIFFERENCE)", mode);
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, var_id, t_begin, t_end, t_stride, rows, times)) return rc;
    const int64_t n = (int64_t)rows.size() - (mode == RSCM_VAR_DIFFERENCE ? 1 : 0);   // the working series' length
    if (n < 3) return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: at least 3 are needed", (int)rows.size(), (long long)n);
    const double stt = (double)(n * (n * n - 1)) / 12.0;
    if (int rc = set_device(h)) return rc;
    if (!h->d_ind[slot]) HIPCHK(rscm::dev_malloc(&h->d_ind[slot], (size_t)(3 + rscm::kMaxThresholds) * (size_t)h->N * sizeof(double)));
    const double** d_rows = nullptr;
    hipError_t e = rscm::dev_malloc(&d_rows, rows.size() * sizeof(double*));
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = rscm::launch_variability(d_rows, (int32_t)rows.size(), mode, stt, h->N, h->d_ind[slot], h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(d_rows);
    HIPCHK(e);
    HIPCHK(es);
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
    if (slot < 0 || slot >= rscm_ens::kIndSlots) return fail(RSCM_ERR_INVALID, "slot %d: must be in [0, %d)", slot, rscm_ens::kIndSlots);
    if (mode != RSCM_VAR_MEAN && mode != RSCM_VAR_LINEAR && mode != RSCM_VAR_DIFFERENCE)
        return fail(RSCM_ERR_INVALID, "unknown detrending mode %d (RSCM_VAR_MEAN, RSCM_VAR_LINEAR, RSCM_VAR_DIFFERENCE)", mode);
    if (n_bands < 1 || n_bands > rscm::kMaxSpectrumBands || !edges)
        return fail(RSCM_ERR_INVALID, "bad band list (1 to %d bands, n_bands + 1 edges)", rscm::kMaxSpectrumBands);
    if (int rc = no_select(h)) return rc;
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, var_id, t_begin, t_end, t_stride, rows, times)) return rc;
    const int64_t n = (int64_t)rows.size() - (mode == RSCM_VAR_DIFFERENCE ? 1 : 0);   // the working series' length
    if (n < 3 || n > kSpectrumMaxTerms)
        return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: 3 to %d are needed", (int)rows.size(), (long long)n,
                    kSpectrumMaxTerms);
    const int32_t J = (int32_t)((n - 1) / 2);
    if (edges[0] < 1 || edges[n_bands] > J + 1) return fail(RSCM_ERR_INVALID, "the band edges must lie in [1, %d] (J + 1 of %lld terms)", J + 1, (long long)n);
    for (int32_t b = 0; b < n_bands; ++b)
        if (edges[b] >= edges[b + 1]) return fail(RSCM_ERR_INVALID, "the band edges must be strictly ascending (edge %d)", b + 1);
    const double stt = (double)(n * (n * n - 1)) / 12.0;
    // the table the kernel is given: c2[J], kSpectrumTablePad zeros the last tile may read, then the edges (8-byte aligned: int32 pairs)
    const size_t n_c2 = (size_t)J + rscm::kSpectrumTablePad;
    std::vector<double> table(n_c2 + (size_t)(n_bands + 2) / 2, 0.0);
    spectrum_coefficients((int32_t)n, table.data());
    std::memcpy(table.data() + n_c2, edges, (size_t)(n_bands + 1) * sizeof(int32_t));
    if (int rc = set_device(h)) return rc;
    if (!h->d_ind[slot]) HIPCHK(rscm::dev_malloc(&h->d_ind[slot], (size_t)(3 + rscm::kMaxThresholds) * (size_t)h->N * sizeof(double)));
    const double** d_rows = nullptr;
    double* d_table = nullptr;
    hipError_t e = rscm::dev_malloc(&d_rows, rows.size() * sizeof(double*));
    if (e == hipSuccess) e = rscm::dev_malloc(&d_table, table.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
        e = rscm::launch_spectrum(d_rows, (int32_t)rows.size(), mode, stt, d_table, reinterpret_cast<const int32_t*>(d_table + n_c2), n_bands, h->N,
                                  h->d_ind[slot], h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(d_rows);
    (void)hipFree(d_table);
    HIPCHK(e);
    HIPCHK(es);
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
    if (int rc = set_device(h)) return rc;
    for (int32_t j = 0; j < n_vec; ++j) {
        char what[24];
        std::snprintf(what, sizeof what, "vector %d", j);
        if (int rc = check_member_vector(h, vec_dev[j], what)) return rc;
        v.vec[j] = vec_dev[j];
    }
    if (add_dev)
        if (int rc = check_member_vector(h, add_dev, "add_dev")) return rc;
    if (!h->d_loglik) HIPCHK(rscm::dev_malloc(&h->d_loglik, (size_t)h->N * sizeof(double)));
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
    if (int rc = set_device(h)) return rc;
    for (int32_t j = 0; j < n_vec; ++j) {
        char what[24];
        std::snprintf(what, sizeof what, "vector %d", j);
        if (int rc = check_member_vector(h, vec_dev[j], what)) return rc;
        v.vec[j] = vec_dev[j];
    }
    if (add_dev)
        if (int rc = check_member_vector(h, add_dev, "add_dev")) return rc;
    if (!h->d_loglik) HIPCHK(rscm::dev_malloc(&h->d_loglik, (size_t)h->N * sizeof(double)));
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
    if (!total || (n_thr > 0 && !hits)) return fail(RSCM_ERR_INVALID, "hits or total is NULL");
    if (int rc = check_thresholds(n_thr, thr, 0)) return rc;
    if (weighted && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if (int rc = set_device(h)) return rc;
    if (int rc = check_member_vector(h, vec_dev, "vector")) return rc;
    rscm::Thresholds th{};
    for (int32_t k = 0; k < n_thr; ++k) th.v[k] = thr[k];
    unsigned long long acc[rscm::kMaxThresholds + 1] = {};
    unsigned long long* d_acc = nullptr;
    const size_t bytes = (size_t)(n_thr + 1) * sizeof(unsigned long long);
    hipError_t e = rscm::dev_malloc(&d_acc, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, bytes, h->stream);
    if (e == hipSuccess) e = rscm::launch_exceedance(vec_dev, weighted ? h->d_weights : nullptr, h->N, n_thr, th, d_acc, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(acc, d_acc, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(d_acc);
    HIPCHK(e);
    HIPCHK(es);
    for (int32_t k = 0; k < n_thr; ++k) hits[k] = (int64_t)acc[k];
    *total = (int64_t)acc[n_thr];
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_exceedance_grouped(rscm_ens* h, const double* vec_dev, int32_t n_thr, const double* thr, int32_t weighted, int64_t* hits,
                                int64_t* total)
{
    GUARD_BEGIN
    NEED(h);
    if (!total || (n_thr > 0 && !hits)) return fail(RSCM_ERR_INVALID, "hits or total is NULL");
    if (int rc = check_thresholds(n_thr, thr, 0)) return rc;
    if (!h->d_groups) return fail(RSCM_ERR_STATE, "no member groups: rscm_ens_set_member_groups first");
    if (weighted && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if (int rc = set_device(h)) return rc;
    if (int rc = check_member_vector(h, vec_dev, "vector")) return rc;
    rscm::Thresholds th{};
    for (int32_t k = 0; k < n_thr; ++k) th.v[k] = thr[k];
    const int32_t G = h->n_groups;
    std::vector<unsigned long long> acc((size_t)G * (n_thr + 1));
    unsigned long long* d_acc = nullptr;
    const size_t bytes = acc.size() * sizeof(unsigned long long);
    hipError_t e = rscm::dev_malloc(&d_acc, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, bytes, h->stream);
    if (e == hipSuccess)
        e = rscm::launch_exceedance_grouped(vec_dev, weighted ? h->d_weights : nullptr, h->d_groups, G, h->N, n_thr, th, d_acc, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(acc.data(), d_acc, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    (void)hipFree(d_acc);
    HIPCHK(e);
    HIPCHK(es);
    for (int32_t g = 0; g < G; ++g) {
        for (int32_t k = 0; k < n_thr; ++k) hits[(size_t)g * n_thr + k] = (int64_t)acc[(size_t)g * (n_thr + 1) + k];
        total[g] = (int64_t)acc[(size_t)g * (n_thr + 1) + n_thr];
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
