// Host side of the handle's baseline (rscm_ens_set_baseline*, the anomaly select's b[i]), of the per-member indicators
// (rscm_ens_member_indicators) and of the exceedance counts (rscm_ens_exceedance, rscm_ens_exceedance_grouped); kernels in indicators.hip.
// Also of the Gaussian likelihood over per-member vectors (rscm_ens_loglik_vectors_device; kernel in variability.hip) and of the spectral
// likelihood over band powers (rscm_ens_loglik_spectrum_device; kernel in spectrum.hip).  The per-member series statistics, which share
// the rows and the slots of the indicators, are in series_host.cpp.
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

// The device array of the row pointers, enqueued on the handle's stream: rows must live until the caller has synchronised it
int upload_rows(rscm_ens* h, const std::vector<const double*>& rows, rscm::DevBuf<const double*>& d_rows)
{
    HIPCHK(d_rows.alloc(rows.size()));
    HIPCHK(hipMemcpyAsync(d_rows.get(), rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice, h->stream));
    return RSCM_OK;
}

int no_select(const rscm_ens* h)
{
    if (h->select) return fail(RSCM_ERR_STATE, "a select is in flight on this handle: rscm_ens_select_end it first");
    return RSCM_OK;
}

// The slots of rscm_ens_member_indicators and of the series statistics (series_host.cpp): the check, and the slot's buffer, allocated at first use
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

namespace {

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
