// Host side of the exceedance and rank sums of stored rows (rscm_ens_exceedance_rows; the definition is stated in include/rscm_gpu.h,
// the kernel is in exceedance_rows.hip).
//
// A call resolves the rows where they are resident (resolve_rows: full storage, the window, the output store), uploads their
// addresses and, for per-row thresholds, the table of the computed rows, and launches once for all rows.  The sums land in one
// zeroed int64 array [computed rows][G][total, hits[K], equal[K]] on the device, which is copied out and dealt to the caller's three
// arrays; rows beyond the time index stay zero.  Every temporary is a DevBuf, everything runs on the handle's stream, and one
// synchronise ends the call.
#include <algorithm>
#include <vector>

#include "ens.hpp"

static_assert(RSCM_EXCEEDANCE_ROWS_MAX_THRESHOLDS == rscm::kMaxThresholds, "the header states the kernel's threshold limit");

extern "C" {

int rscm_ens_exceedance_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_thr, const double* thr,
                             int32_t thr_per_row, int32_t flags, int64_t* hits, int64_t* equal, int64_t* total)
{
    GUARD_BEGIN
    NEED(h);
    if (flags & ~(RSCM_SELECT_WEIGHTED | RSCM_SELECT_ANOMALY | RSCM_SELECT_GROUPED)) return fail(RSCM_ERR_INVALID, "unknown exceedance flags 0x%x", flags);
    if (n_thr < 1 || n_thr > RSCM_EXCEEDANCE_ROWS_MAX_THRESHOLDS || !thr)
        return fail(RSCM_ERR_INVALID, "bad threshold list (1 to %d thresholds)", RSCM_EXCEEDANCE_ROWS_MAX_THRESHOLDS);
    if (!hits || !total) return fail(RSCM_ERR_INVALID, "hits or total is NULL");
    const bool weighted = (flags & RSCM_SELECT_WEIGHTED) != 0, grouped = (flags & RSCM_SELECT_GROUPED) != 0;
    const bool anomaly = (flags & RSCM_SELECT_ANOMALY) != 0;
    if (weighted && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if (grouped && !h->d_groups) return fail(RSCM_ERR_STATE, "no member groups: rscm_ens_set_member_groups first");
    if (anomaly && !h->d_base) return fail(RSCM_ERR_STATE, "no baseline: rscm_ens_set_baseline or rscm_ens_set_baseline_values first");
    if (int rc = no_select(h)) return rc;
    if (int rc = check_row_range(h, var_id, t_begin, t_end, t_stride, false)) return rc;
    if (int rc = check_series_stored(h, t_end)) return rc;
    if (int rc = set_device(h)) return rc;
    const int32_t G = grouped ? h->n_groups : 1;
    const size_t n_range = t_begin < t_end ? (size_t)(((int64_t)t_end - t_begin + t_stride - 1) / t_stride) : 0;
    std::vector<const double*> rows;
    int32_t n_rows = 0;
    if (int rc = resolve_rows(h, var_id, t_begin, t_end, t_stride, rows, &n_rows)) return rc;
    std::fill(hits, hits + n_range * G * n_thr, (int64_t)0);
    if (equal) std::fill(equal, equal + n_range * G * n_thr, (int64_t)0);
    std::fill(total, total + n_range * G, (int64_t)0);
    if (rows.empty()) return RSCM_OK;   // the computed rows come first: resolve_rows leaves out the rows beyond the time index

    const size_t S = (size_t)rscm::exceedance_rows_stride(n_thr, equal != nullptr), n_acc = rows.size() * G * S;
    rscm::DevBuf<const double*> d_rows;
    rscm::DevBuf<double> d_thr;
    rscm::DevBuf<unsigned long long> d_acc;
    std::vector<unsigned long long> acc(n_acc);
    if (int rc = upload_rows(h, rows, d_rows)) return rc;
    rscm::ExceedanceRowsArgs a{};
    if (thr_per_row) {
        HIPCHK(d_thr.alloc(rows.size() * n_thr));
        HIPCHK(hipMemcpyAsync(d_thr.get(), thr, rows.size() * n_thr * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else {
        std::copy(thr, thr + n_thr, a.thr.v);
    }
    HIPCHK(d_acc.alloc(n_acc));
    HIPCHK(hipMemsetAsync(d_acc.get(), 0, n_acc * sizeof(unsigned long long), h->stream));
    a.rows = d_rows.get();
    a.thr_rows = d_thr.get();
    a.w = weighted ? h->d_weights.get() : nullptr;
    a.group = grouped ? h->d_groups.get() : nullptr;
    a.base = anomaly ? h->d_base.get() : nullptr;
    a.acc = d_acc.get();
    a.N = h->N;
    a.n_rows = (int32_t)rows.size();
    a.n_groups = G;
    a.n_thr = n_thr;
    HIPCHK(rscm::launch_exceedance_rows(a, equal != nullptr, h->stream));
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc.get(), n_acc * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the temporaries and host copies go out of scope after this
    for (size_t rg = 0; rg < rows.size() * G; ++rg) {
        const unsigned long long* rec = acc.data() + rg * S;
        total[rg] = (int64_t)rec[0];
        for (int32_t k = 0; k < n_thr; ++k) {
            hits[rg * n_thr + k] = (int64_t)rec[1 + k];
            if (equal) equal[rg * n_thr + k] = (int64_t)rec[1 + n_thr + k];
        }
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
