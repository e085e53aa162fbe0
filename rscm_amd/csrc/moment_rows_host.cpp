// Host side of the exact moments of stored rows (rscm_ens_moment_rows_sums, rscm_ens_moment_rows, rscm_gpu_moment_rows_last_stats; the
// definition is stated in include/rscm_gpu.h, the kernel is in moment_rows.hip, the finishing step in moments_finish.hpp).
//
// A call resolves the rows where they are resident (resolve_rows: full storage, the window, the output store), uploads their
// addresses and, for order 2, the centre of the computed rows, and launches once for all rows.  Everything lands in one int64 array
// [rows][G][2 + blocks * 69], the caller's if it is on the device, else a temporary that is copied out; rows beyond the time index
// stay zero.  Every temporary is a DevBuf, everything runs on the handle's stream, and one synchronise ends the call.
#include <algorithm>
#include <vector>

#include "ens.hpp"
#include "moments_finish.hpp"

static_assert(RSCM_MOMENT_ROWS_MAX_VECTORS == rscm::kMaxMomentRowVectors, "the header states the kernel's vector limit");

namespace {

thread_local int64_t t_last_stats[3] = {0, 0, 0};   // window terms, walked terms, rebases of the calling thread's last launch

int moment_rows_sums(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_vec, const double* const* vec_dev,
                     int32_t flags, int32_t order, const double* center, int64_t* out, int32_t on_device)
{
    if (int rc = check_moment_call(h, flags, RSCM_SELECT_WEIGHTED | RSCM_SELECT_ANOMALY | RSCM_SELECT_GROUPED, order, center, n_vec, vec_dev, 0,
                                   RSCM_MOMENT_ROWS_MAX_VECTORS, out))
        return rc;
    const bool weighted = (flags & RSCM_SELECT_WEIGHTED) != 0, grouped = (flags & RSCM_SELECT_GROUPED) != 0;
    const bool anomaly = (flags & RSCM_SELECT_ANOMALY) != 0;
    if (int rc = no_select(h)) return rc;
    if (int rc = check_row_range(h, var_id, t_begin, t_end, t_stride, false)) return rc;
    if (int rc = check_series_stored(h, t_end)) return rc;
    const int32_t G = grouped ? h->n_groups : 1, B = rscm::moment_rows_blocks(n_vec, order);
    const int64_t n_range = t_begin < t_end ? ((int64_t)t_end - t_begin + t_stride - 1) / t_stride : 0;
    if (n_range * G * B > RSCM_MOMENT_ROWS_MAX_BLOCKS)
        return fail(RSCM_ERR_INVALID, "%lld rows x %d groups x %d blocks: more than %d blocks in one call", (long long)n_range, G, B,
                    RSCM_MOMENT_ROWS_MAX_BLOCKS);
    rscm::MomentRowsArgs a{};
    if (int rc = check_member_vectors(h, n_vec, vec_dev)) return rc;
    std::copy(vec_dev, vec_dev + n_vec, a.vec);
    const size_t stride = 2 + (size_t)B * rscm::kMomentBlock, total = (size_t)n_range * G * stride;
    if (on_device && total)
        if (int rc = check_device_out(h, out, total)) return rc;
    std::vector<const double*> rows;
    int32_t n_rows = 0;
    if (int rc = resolve_rows(h, var_id, t_begin, t_end, t_stride, rows, &n_rows)) return rc;
    std::fill(t_last_stats, t_last_stats + 3, 0);
    if (total == 0) return RSCM_OK;

    rscm::DevBuf<const double*> d_rows;
    rscm::DevBuf<double> d_centre;
    rscm::DevBuf<unsigned long long> d_tmp, d_stats;
    std::vector<double> c;
    unsigned long long stats[3] = {0ull, 0ull, 0ull};
    unsigned long long* d_out = nullptr;
    if (int rc = begin_moment_out(h, out, total, on_device, d_tmp, &d_out)) return rc;
    if (!rows.empty()) {   // the computed rows come first: resolve_rows leaves out the rows beyond the time index
        if (int rc = upload_rows(h, rows, d_rows)) return rc;
        // one record per computed (row, group)
        if (int rc = upload_moment_centre(h, order == 2 ? center : nullptr, rows.size() * G, 1 + (size_t)n_vec, c, d_centre)) return rc;
        HIPCHK(d_stats.alloc(3));
        HIPCHK(hipMemsetAsync(d_stats.get(), 0, sizeof stats, h->stream));
        a.rows = d_rows.get();
        a.w = weighted ? h->d_weights.get() : nullptr;
        a.group = grouped ? h->d_groups.get() : nullptr;
        a.base = anomaly ? h->d_base.get() : nullptr;
        a.centre = d_centre.get();
        a.out = d_out;
        a.stats = d_stats.get();
        a.N = h->N;
        a.n_rows = (int32_t)rows.size();
        a.n_groups = G;
        HIPCHK(rscm::launch_moment_rows(a, n_vec, order, h->stream));
        HIPCHK(hipMemcpyAsync(stats, d_stats.get(), sizeof stats, hipMemcpyDeviceToHost, h->stream));
    }
    if (int rc = end_moment_out(h, out, d_out, total, on_device)) return rc;
    for (int k = 0; k < 3; ++k) t_last_stats[k] = (int64_t)stats[k];
    return RSCM_OK;
}

}  // namespace

extern "C" {

int rscm_ens_moment_rows_sums(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_vec,
                              const double* const* vec_dev, int32_t flags, int32_t order, const double* center, int64_t* out, int32_t on_device)
{
    GUARD_BEGIN
    NEED(h);
    return moment_rows_sums(h, var_id, t_begin, t_end, t_stride, n_vec, vec_dev, flags, order, center, out, on_device);
    GUARD_END
}

int rscm_ens_moment_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_vec,
                         const double* const* vec_dev, int32_t flags, double* mean, double* second, int64_t* n, int64_t* weight)
{
    GUARD_BEGIN
    NEED(h);
    if (!mean || !second) return fail(RSCM_ERR_INVALID, "mean or second is NULL");
    if (n_vec < 0 || n_vec > RSCM_MOMENT_ROWS_MAX_VECTORS)
        return fail(RSCM_ERR_INVALID, "bad vector list (0 to %d vectors)", RSCM_MOMENT_ROWS_MAX_VECTORS);
    if (t_stride < 1 || t_begin > t_end) return fail(RSCM_ERR_INVALID, "bad time range [%d, %d) stride %d", t_begin, t_end, t_stride);
    const int32_t B1 = rscm::moment_rows_blocks(n_vec, 1), B2 = rscm::moment_rows_blocks(n_vec, 2);
    const size_t RG = (size_t)(((int64_t)t_end - t_begin + t_stride - 1) / t_stride) *
                      ((flags & RSCM_SELECT_GROUPED) && h->d_groups ? (size_t)h->n_groups : 1);
    if ((int64_t)RG * B2 > RSCM_MOMENT_ROWS_MAX_BLOCKS)
        return fail(RSCM_ERR_INVALID, "%zu rows x groups x %d blocks: more than %d blocks in one call", RG, B2, RSCM_MOMENT_ROWS_MAX_BLOCKS);
    std::vector<int64_t> sums(std::max<size_t>(RG * (2 + (size_t)B2 * rscm::kMomentBlock), 1));   // (an empty range still passes a buffer)
    if (int rc = moment_rows_sums(h, var_id, t_begin, t_end, t_stride, n_vec, vec_dev, flags, 1, nullptr, sums.data(), 0)) return rc;
    if (int rc = finish_moment_sums(sums.data(), RG, B1, mean, n, weight)) return rc;
    if (int rc = moment_rows_sums(h, var_id, t_begin, t_end, t_stride, n_vec, vec_dev, flags, 2, mean, sums.data(), 0)) return rc;
    return finish_moment_sums(sums.data(), RG, B2, second, n, weight);
    GUARD_END
}

int rscm_gpu_moment_rows_last_stats(int64_t out[3])
{
    GUARD_BEGIN
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    std::copy(t_last_stats, t_last_stats + 3, out);
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
