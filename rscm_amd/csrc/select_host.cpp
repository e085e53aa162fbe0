// Host side of the staged quantile select (rscm_ens_select_*, rscm_ens_quantile_rows and rscm_ens_quantile_series; kernels in select.hip), of its weighted
// form (rscm_ens_select_begin_weighted, rscm_ens_weighted_quantile_rows), of the flagged and vector forms
// (rscm_ens_quantile_rows_ex, rscm_ens_select_begin_ex: anomalies against the handle's baseline; rscm_ens_quantile_vectors,
// rscm_ens_select_begin_vectors: device vectors of N doubles as rows) and of the member weights it reads (weights.hip).
//
// A select resolves its rows once, at begin, into a device array of row pointers (rscm_ens::row_ptr: full storage, the window or
// the strided output store), then alternates pass (histograms of this handle's members) and commit (the reduced histograms move
// every target one digit on) kSelPasses times.  Between the two a caller with several handles -- ranks of one sharded ensemble,
// or two ensembles on one GPU -- sums the int64 buffers of all of them; every handle then commits the same sums and so reaches
// the same keys.  The weighted select runs the same stages over the handle's int64 member weights: one target per quantile, and
// pass 0's reduced histograms give each row's weight W, which the first commit checks against 2^53 on every handle.
//
// The grouped select (RSCM_SELECT_GROUPED) is the same again with (row, group) as the row of the commit and finish launches: the
// histogram pass counts each member into its own group's histograms (select.hip), the buffers are [rows][n_groups][...], and
// count, prefix, rank and out have n_comp x n_groups rows.  The member groups themselves (rscm_ens_set_member_groups) are at the end.
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <utility>

#include "ens.hpp"
#include "select_keys.hpp"

struct SelectState {
    int32_t var = 0, t_begin = 0, t_stride = 1;
    int32_t n_rows = 0;     // rows of the range
    int32_t n_comp = 0;     // the first n_comp of them are computed (t <= time_index); the others report count 0, NaN
    int32_t n_q = 0, n_t = 0;
    int32_t pass = 0;       // the next pass to histogram
    bool awaiting_commit = false;
    bool weighted = false;  // RSCM_SELECT_WEIGHTED, the mode of the kernels: count holds W, n_t == n_q
    int32_t n_groups = 0;   // RSCM_SELECT_GROUPED: the handle's groups (they cannot change while the select is staged), else 0
    const int32_t* d_group = nullptr;
    int32_t v_rows() const { return n_comp * (n_groups ? n_groups : 1); }   // (row, group) pairs: the rows of commit and finish
    const double* d_base = nullptr;   // RSCM_SELECT_ANOMALY: the handle's baseline (it cannot change while the select is staged)
    // the select's own buffers: they go with the state
    rscm::DevBuf<const double*> d_rows;
    rscm::DevBuf<double> d_q;
    rscm::DevBuf<int64_t> d_hist;
    size_t hist_elems = 0;
    rscm::DevBuf<int64_t> d_count;
    rscm::DevBuf<uint64_t> d_prefix;
    rscm::DevBuf<int64_t> d_rank;
    rscm::DevBuf<double> d_out;
    rscm::DevBuf<int32_t> d_over;   // weighted: set by the first commit if a row's W exceeds 2^53
};

namespace {

constexpr int32_t kMaxSelectQuantiles = 128;

constexpr int32_t kMaxSelectVectors = 4096;

// The checks every select makes first: the flags and what they need, then the quantile list (after the caller's own checks)
int select_flags(rscm_ens* h, int32_t flags)
{
    if (flags & ~(RSCM_SELECT_WEIGHTED | RSCM_SELECT_ANOMALY | RSCM_SELECT_GROUPED)) return fail(RSCM_ERR_INVALID, "unknown select flags 0x%x", flags);
    if ((flags & RSCM_SELECT_WEIGHTED) && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if ((flags & RSCM_SELECT_ANOMALY) && !h->d_base)
        return fail(RSCM_ERR_STATE, "no baseline: rscm_ens_set_baseline or rscm_ens_set_baseline_values first");
    if ((flags & RSCM_SELECT_GROUPED) && !h->d_groups) return fail(RSCM_ERR_STATE, "no member groups: rscm_ens_set_member_groups first");
    return RSCM_OK;
}

int check_quantiles(int32_t n_q, const double* q)
{
    if (n_q < 1 || n_q > kMaxSelectQuantiles || !q) return fail(RSCM_ERR_INVALID, "bad quantile list (1 to %d quantiles)", kMaxSelectQuantiles);
    for (int32_t k = 0; k < n_q; ++k)
        if (!(q[k] >= 0.0 && q[k] <= 1.0)) return fail(RSCM_ERR_INVALID, "Quantiles must be in the range [0, 1], got %g", q[k]);
    return RSCM_OK;
}

// Fills s for the computed rows `rows` (of s.n_rows) and uploads the row pointers and quantiles
int select_setup(rscm_ens* h, SelectState& s, const std::vector<const double*>& rows, int32_t n_q, const double* q, int32_t flags)
{
    const bool weighted = (flags & RSCM_SELECT_WEIGHTED) != 0;
    s.n_q = n_q;
    s.n_t = weighted ? n_q : 2 * n_q;
    s.weighted = weighted;
    s.d_base = (flags & RSCM_SELECT_ANOMALY) ? h->d_base : nullptr;
    s.n_groups = (flags & RSCM_SELECT_GROUPED) ? h->n_groups : 0;
    s.d_group = s.n_groups ? h->d_groups : nullptr;
    s.n_comp = (int32_t)rows.size();
    if (s.n_comp == 0) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    const size_t nr = (size_t)s.n_comp, nc = (size_t)s.v_rows(), nt = (size_t)s.n_t;
    s.hist_elems = nc * nt * rscm::kSelBins;
    HIPCHK(s.d_rows.alloc(nr));
    HIPCHK(s.d_q.alloc((size_t)n_q));
    HIPCHK(s.d_hist.alloc(s.hist_elems));
    HIPCHK(s.d_count.alloc(nc));
    HIPCHK(s.d_prefix.alloc(nc * nt));
    HIPCHK(s.d_rank.alloc(nc * nt));
    HIPCHK(s.d_out.alloc(nc * (size_t)(n_q + 1)));
    if (weighted) HIPCHK(s.d_over.alloc(1));
    HIPCHK(hipMemcpyAsync(s.d_rows.get(), rows.data(), nr * sizeof(double*), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s.d_q.get(), q, (size_t)n_q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the host vectors go out of scope
    return RSCM_OK;
}

int select_init(rscm_ens* h, SelectState& s, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q,
                int32_t flags)
{
    if (int rc = select_flags(h, flags)) return rc;
    if (int rc = check_row_range(h, var_id, t_begin, t_end, t_stride, false)) return rc;
    if (int rc = check_quantiles(n_q, q)) return rc;
    if (int rc = check_series_stored(h, t_end)) return rc;
    s.var = var_id;
    s.t_begin = t_begin;
    s.t_stride = t_stride;
    std::vector<const double*> rows;
    if (int rc = resolve_rows(h, var_id, t_begin, t_end, t_stride, rows, &s.n_rows)) return rc;
    return select_setup(h, s, rows, n_q, q, flags);
}

// The select over n_vec device vectors of N doubles (the rows are the vectors; every one is "computed")
int select_init_vectors(rscm_ens* h, SelectState& s, int32_t n_vec, const double* const* vec, int32_t n_q, const double* q, int32_t flags)
{
    if (flags & RSCM_SELECT_ANOMALY) return fail(RSCM_ERR_INVALID, "RSCM_SELECT_ANOMALY applies to stored rows, not to vectors");
    if (int rc = select_flags(h, flags)) return rc;
    if (n_vec < 1 || n_vec > kMaxSelectVectors || !vec) return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors)", kMaxSelectVectors);
    if (int rc = check_quantiles(n_q, q)) return rc;
    if (int rc = set_device(h)) return rc;
    std::vector<const double*> rows(vec, vec + n_vec);
    for (int32_t k = 0; k < n_vec; ++k) {
        char what[32];
        std::snprintf(what, sizeof what, "vector %d", k);
        if (int rc = check_member_vector(h, rows[k], what)) return rc;
    }
    s.n_rows = n_vec;
    return select_setup(h, s, rows, n_q, q, flags);
}

int select_pass(rscm_ens* h, SelectState& s, int32_t* done, int64_t** buf_dev, int64_t* n)
{
    if (s.awaiting_commit) return fail(RSCM_ERR_STATE, "select: commit the previous pass first");
    if (s.n_comp == 0 || s.pass == rscm::kSelPasses) {
        *done = 1;
        if (buf_dev) *buf_dev = nullptr;
        if (n) *n = 0;
        return RSCM_OK;
    }
    if (int rc = set_device(h)) return rc;
    const size_t elems = (size_t)s.v_rows() * rscm::kSelBins * (s.pass == 0 ? 1 : (size_t)s.n_t);
    HIPCHK(rscm::launch_select_hist(s.d_rows.get(), s.weighted ? h->d_weights : nullptr, s.d_base, s.d_group, s.n_groups, h->N, s.n_comp, s.pass,
                                    s.d_prefix.get(), s.n_t, s.d_hist.get(), elems, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    s.awaiting_commit = true;
    *done = 0;
    if (buf_dev) *buf_dev = s.d_hist.get();
    if (n) *n = (int64_t)elems;
    return RSCM_OK;
}

int select_commit(rscm_ens* h, SelectState& s)
{
    if (!s.awaiting_commit) return fail(RSCM_ERR_STATE, "select: no pass to commit");
    if (int rc = set_device(h)) return rc;
    const bool check_w = s.weighted && s.pass == 0;   // the first weighted commit checks every row's W against 2^53
    if (check_w) HIPCHK(hipMemsetAsync(s.d_over.get(), 0, sizeof(int32_t), h->stream));
    HIPCHK(rscm::launch_select_commit(s.d_hist.get(), s.pass, s.v_rows(), s.n_t, s.d_q.get(), s.d_count.get(), s.d_prefix.get(), s.d_rank.get(),
                                      s.d_over.get(), h->stream));
    s.awaiting_commit = false;
    if (++s.pass == rscm::kSelPasses)
        HIPCHK(rscm::launch_select_finish(s.d_count.get(), s.d_prefix.get(), s.v_rows(), s.n_q, s.d_q.get(), s.weighted, s.d_out.get(), h->stream));
    if (check_w) {
        int32_t over = 0;
        HIPCHK(hipMemcpyAsync(&over, s.d_over.get(), sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (over)
            return fail(RSCM_ERR_INVALID, "weighted select: the weights of a row's non-NaN members%s sum to more than 2^53",
                        s.n_groups ? " in one group" : "");
    }
    return RSCM_OK;
}

int select_result(rscm_ens* h, SelectState& s, double* out, double* count)
{
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (s.n_comp > 0 && s.pass < rscm::kSelPasses)
        return fail(RSCM_ERR_STATE, "select: %d of %d passes are still to run", rscm::kSelPasses - s.pass, rscm::kSelPasses);
    const int32_t G = s.n_groups ? s.n_groups : 1;   // out[rows][G][n_q], count[rows][G]
    std::vector<double> host((size_t)s.v_rows() * (s.n_q + 1));
    if (s.n_comp > 0) {
        if (int rc = set_device(h)) return rc;
        HIPCHK(hipMemcpyAsync(host.data(), s.d_out.get(), host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    for (size_t r = 0; r < (size_t)s.n_rows * G; ++r) {
        const bool c = r < (size_t)s.v_rows();
        if (count) count[r] = c ? host[r * (s.n_q + 1)] : 0.0;
        for (int32_t k = 0; k < s.n_q; ++k)
            out[r * s.n_q + k] = c ? host[r * (s.n_q + 1) + 1 + k] : std::numeric_limits<double>::quiet_NaN();
    }
    return RSCM_OK;
}

// vec == nullptr: the rows of var_id; else the n_vec vectors (var_id .. t_stride unused)
int select_begin(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q, int32_t flags,
                 int32_t n_vec = 0, const double* const* vec = nullptr)
{
    if (h->select) return fail(RSCM_ERR_STATE, "a select is already in flight on this handle: rscm_ens_select_end it first");
    auto s = std::make_unique<SelectState>();
    if (int rc = vec || n_vec ? select_init_vectors(h, *s, n_vec, vec, n_q, q, flags)
                              : select_init(h, *s, var_id, t_begin, t_end, t_stride, n_q, q, flags))
        return rc;
    h->select = s.release();
    return RSCM_OK;
}

int quantile_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q, double* out,
                  double* count, int32_t flags, int32_t n_vec = 0, const double* const* vec = nullptr)
{
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    SelectState s;   // its own state: a staged select in flight on the handle is left alone
    int rc = vec || n_vec ? select_init_vectors(h, s, n_vec, vec, n_q, q, flags)
                          : select_init(h, s, var_id, t_begin, t_end, t_stride, n_q, q, flags);
    int32_t done = 0;
    while (rc == RSCM_OK) {
        if ((rc = select_pass(h, s, &done, nullptr, nullptr)) != RSCM_OK || done) break;
        rc = select_commit(h, s);
    }
    if (rc == RSCM_OK) rc = select_result(h, s, out, count);
    if (s.d_rows) {   // the stream is done with the buffers before s frees them
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
    }
    return rc;
}

}  // namespace

int check_row_range(const rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, bool at_least_one)
{
    if (!h->has_rows(var_id)) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (t_begin < 0 || t_end > h->T || t_begin > t_end || (at_least_one && t_begin == t_end) || t_stride < 1)
        return fail(RSCM_ERR_INVALID, "bad time range [%d, %d) stride %d%s", t_begin, t_end, t_stride, at_least_one ? " (at least one row)" : "");
    return check_diagnostic_current(h, var_id);
}

int check_series_stored(const rscm_ens* h, int32_t t_end)
{
    if (!h->windowed && h->rows != h->T && t_end > 1)
        return fail(RSCM_ERR_STATE, "this handle stores only the initial row (RSCM_FLAG_NO_SERIES)");
    return RSCM_OK;
}

int resolve_rows(const rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, std::vector<const double*>& rows,
                 int32_t* n_range)
{
    *n_range = 0;
    for (int32_t t = t_begin; t < t_end; t += t_stride) {
        ++*n_range;
        if (t > h->time_index) continue;   // never computed by this model instance
        const double* p = h->row_ptr(var_id, t);
        if (!p && h->is_diagnostic(var_id)) {
            const rscm_ens::Diagnostic& d = h->diag[var_id - h->V];
            return fail(RSCM_ERR_STATE, "row %d of diagnostic %d is not held: it holds %d rows from %d with stride %d", t, var_id, d.held, d.t_begin,
                        d.t_stride);
        }
        if (!p)
            return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident: the window holds [%d, %d) and the output store every %d-th row%s",
                        t, var_id, h->win0, h->win0 + h->rows, h->out_stride,
                        h->out_slot.empty() || h->out_slot[var_id] < 0 ? " of other variables" : "");
        rows.push_back(p);
    }
    return RSCM_OK;
}

int check_member_vector(const rscm_ens* h, const double* p, const char* what)
{
    if (!p) return fail(RSCM_ERR_INVALID, "%s is NULL", what);
    if ((uintptr_t)p & 7) return fail(RSCM_ERR_INVALID, "%s is not 8-byte aligned", what);
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != h->device) {
        (void)hipGetLastError();
        return fail(RSCM_ERR_INVALID, "%s is not device memory on device %d", what, h->device);
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess ||
        (const char*)p + (size_t)h->N * sizeof(double) > (const char*)base + size) {
        (void)hipGetLastError();
        return fail(RSCM_ERR_INVALID, "%s does not hold %lld doubles", what, (long long)h->N);
    }
    return RSCM_OK;
}

void select_release(rscm_ens* h)
{
    delete h->select;
    h->select = nullptr;
}

extern "C" {

int rscm_ens_select_begin(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q)
{
    GUARD_BEGIN
    NEED(h);
    return select_begin(h, var_id, t_begin, t_end, t_stride, n_q, q, 0);
    GUARD_END
}

int rscm_ens_select_begin_weighted(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q)
{
    GUARD_BEGIN
    NEED(h);
    return select_begin(h, var_id, t_begin, t_end, t_stride, n_q, q, RSCM_SELECT_WEIGHTED);
    GUARD_END
}

int rscm_ens_select_begin_ex(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q,
                             int32_t flags)
{
    GUARD_BEGIN
    NEED(h);
    return select_begin(h, var_id, t_begin, t_end, t_stride, n_q, q, flags);
    GUARD_END
}

int rscm_ens_select_begin_vectors(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t n_q, const double* q, int32_t flags)
{
    GUARD_BEGIN
    NEED(h);
    if (!vec_dev || n_vec < 1) return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors)", kMaxSelectVectors);
    return select_begin(h, 0, 0, 0, 1, n_q, q, flags, n_vec, vec_dev);
    GUARD_END
}

int rscm_ens_select_pass(rscm_ens* h, int32_t* done, int64_t** buf_dev, int64_t* n)
{
    GUARD_BEGIN
    NEED(h);
    if (!h->select) return fail(RSCM_ERR_STATE, "no select in flight: rscm_ens_select_begin first");
    if (!done) return fail(RSCM_ERR_INVALID, "done is NULL");
    return select_pass(h, *h->select, done, buf_dev, n);
    GUARD_END
}

int rscm_ens_select_commit(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (!h->select) return fail(RSCM_ERR_STATE, "no select in flight: rscm_ens_select_begin first");
    return select_commit(h, *h->select);
    GUARD_END
}

int rscm_ens_select_result(rscm_ens* h, double* out, double* count)
{
    GUARD_BEGIN
    NEED(h);
    if (!h->select) return fail(RSCM_ERR_STATE, "no select in flight: rscm_ens_select_begin first");
    return select_result(h, *h->select, out, count);
    GUARD_END
}

int rscm_ens_select_end(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (h->select) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
    }
    select_release(h);
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_quantile_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q,
                           double* out, double* count)
{
    GUARD_BEGIN
    NEED(h);
    return quantile_rows(h, var_id, t_begin, t_end, t_stride, n_q, q, out, count, 0);
    GUARD_END
}

int rscm_ens_quantile_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t n_q, const double* q, double* out,
                             double* count)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id < 1 || var_id >= h->V || t_begin < 0 || t_end > h->T || t_begin > t_end || !out || n_q < 1 || !q)
        return fail(RSCM_ERR_INVALID, "bad variable / time range / quantile list");
    for (int32_t k = 0; k < n_q; ++k)
        if (!(q[k] >= 0.0 && q[k] <= 1.0)) return fail(RSCM_ERR_INVALID, "Quantiles must be in the range [0, 1], got %g", q[k]);
    if (h->windowed || h->rows != h->T) return fail(RSCM_ERR_STATE, "this handle does not store whole series (RSCM_FLAG_NO_SERIES / RSCM_FLAG_WINDOWED)");
    if (t_begin == t_end) return RSCM_OK;
    // any n_q: the select over consecutive blocks of the list, each block's columns into out[row][n_q]; every block counts alike
    const size_t n_rows = (size_t)(t_end - t_begin);
    std::vector<double> part(n_rows * (size_t)std::min(n_q, kMaxSelectQuantiles));
    for (int32_t k0 = 0; k0 < n_q; k0 += kMaxSelectQuantiles) {
        const int32_t nk = std::min(n_q - k0, kMaxSelectQuantiles);
        if (int rc = quantile_rows(h, var_id, t_begin, t_end, 1, nk, q + k0, part.data(), k0 == 0 ? count : nullptr, 0)) return rc;
        for (size_t r = 0; r < n_rows; ++r) std::copy_n(&part[r * nk], nk, &out[r * n_q + k0]);
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_weighted_quantile_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q,
                                    const double* q, double* out, double* weight)
{
    GUARD_BEGIN
    NEED(h);
    return quantile_rows(h, var_id, t_begin, t_end, t_stride, n_q, q, out, weight, RSCM_SELECT_WEIGHTED);
    GUARD_END
}

int rscm_ens_quantile_rows_ex(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q,
                              int32_t flags, double* out, double* count)
{
    GUARD_BEGIN
    NEED(h);
    return quantile_rows(h, var_id, t_begin, t_end, t_stride, n_q, q, out, count, flags);
    GUARD_END
}

int rscm_ens_quantile_vectors(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t n_q, const double* q, int32_t flags,
                              double* out, double* count)
{
    GUARD_BEGIN
    NEED(h);
    if (!vec_dev || n_vec < 1) return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors)", kMaxSelectVectors);
    return quantile_rows(h, 0, 0, 0, 1, n_q, q, out, count, flags, n_vec, vec_dev);
    GUARD_END
}

}  // extern "C"

// ---- member weights of the weighted select ----

namespace {

// Makes d_new[N] the handle's weights if no weight is negative and they sum to at most 2^53.  That bound on every handle keeps
// every histogram sum of the weighted select from wrapping (select.hip); on any failure the weights set before stay.
int install_weights(rscm_ens* h, rscm::DevBuf<int64_t> d_new)
{
    rscm::DevBuf<int32_t> d_flag;
    rscm::DevBuf<unsigned long long> d_total;
    int32_t neg = 0;
    unsigned long long total = 0;
    HIPCHK(d_flag.alloc(1));
    HIPCHK(d_total.alloc(1));
    HIPCHK(hipMemsetAsync(d_flag.get(), 0, sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(d_total.get(), 0, sizeof total, h->stream));
    HIPCHK(rscm::launch_weights_check(d_new.get(), h->N, d_flag.get(), d_total.get(), h->stream));
    HIPCHK(hipMemcpyAsync(&neg, d_flag.get(), sizeof neg, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&total, d_total.get(), sizeof total, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (neg) return fail(RSCM_ERR_INVALID, "a member weight is negative");
    if (total > (1ull << 53)) return fail(RSCM_ERR_INVALID, "the member weights of this handle sum to more than 2^53");
    h->d_weights = std::move(d_new);
    return RSCM_OK;
}

// ll on the device: the caller's pointer, or (host input) a copy enqueued on the handle's stream into tmp
int device_loglik(rscm_ens* h, const double* ll, int32_t on_device, rscm::DevBuf<double>& tmp, const double** d_ll)
{
    *d_ll = ll;
    if (on_device) return RSCM_OK;
    HIPCHK(tmp.alloc((size_t)h->N));
    HIPCHK(hipMemcpyAsync(tmp.get(), ll, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    *d_ll = tmp.get();
    return RSCM_OK;
}

int loglik_max(rscm_ens* h, const double* d_ll, double* out)
{
    rscm::DevBuf<unsigned long long> d_key;
    unsigned long long key = rscm::order_key(-std::numeric_limits<double>::infinity());
    HIPCHK(d_key.alloc(1));
    HIPCHK(hipMemcpyAsync(d_key.get(), &key, sizeof key, hipMemcpyHostToDevice, h->stream));
    HIPCHK(rscm::launch_loglik_max(d_ll, h->d_status, h->N, d_key.get(), h->stream));
    HIPCHK(hipMemcpyAsync(&key, d_key.get(), sizeof key, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = rscm::key_value(key);
    return RSCM_OK;
}

}  // namespace

extern "C" {

int rscm_ens_set_member_weights(rscm_ens* h, const int64_t* w, int32_t on_device)
{
    GUARD_BEGIN
    NEED(h);
    if (!w) return fail(RSCM_ERR_INVALID, "weights are NULL");
    if (h->select) return fail(RSCM_ERR_STATE, "a select is in flight on this handle: rscm_ens_select_end it first");
    if (int rc = set_device(h)) return rc;
    rscm::DevBuf<int64_t> d_new;
    HIPCHK(d_new.alloc((size_t)h->N));
    HIPCHK(hipMemcpyAsync(d_new.get(), w, (size_t)h->N * sizeof(int64_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return install_weights(h, std::move(d_new));
    GUARD_END
}

int rscm_ens_member_weights_devptr(rscm_ens* h, void** out)
{
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = h->d_weights;
    if (!h->d_weights) return fail(RSCM_ERR_STATE, "no member weights set");
    return RSCM_OK;
}

int rscm_ens_loglik_max(rscm_ens* h, const double* ll, int32_t on_device, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!ll || !out) return fail(RSCM_ERR_INVALID, "ll or out is NULL");
    if (int rc = set_device(h)) return rc;
    rscm::DevBuf<double> tmp;
    const double* d_ll = nullptr;
    if (int rc = device_loglik(h, ll, on_device, tmp, &d_ll)) return rc;
    return loglik_max(h, d_ll, out);   // synchronised: tmp has been read
    GUARD_END
}

int rscm_ens_set_weights_from_loglik(rscm_ens* h, const double* ll, int32_t on_device, double ll_max, int32_t bits)
{
    GUARD_BEGIN
    NEED(h);
    if (!ll) return fail(RSCM_ERR_INVALID, "ll is NULL");
    if (bits < 0 || bits > 52) return fail(RSCM_ERR_INVALID, "bits = %d: must be in [0, 52]", bits);
    if (std::isnan(ll_max) || ll_max == std::numeric_limits<double>::infinity())
        return fail(RSCM_ERR_INVALID, "ll_max must be finite or -inf, got %g", ll_max);
    if (h->select) return fail(RSCM_ERR_STATE, "a select is in flight on this handle: rscm_ens_select_end it first");
    if (int rc = set_device(h)) return rc;
    rscm::DevBuf<int64_t> d_new;
    HIPCHK(d_new.alloc((size_t)h->N));
    {
        rscm::DevBuf<double> tmp;
        const double* d_ll = nullptr;
        if (int rc = device_loglik(h, ll, on_device, tmp, &d_ll)) return rc;
        HIPCHK(rscm::launch_weights_from_loglik(d_ll, h->d_status, h->N, ll_max, bits, d_new.get(), h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return install_weights(h, std::move(d_new));   // refused if N weights of up to 2^bits sum to more than 2^53
    GUARD_END
}

}  // extern "C"

// ---- member groups of the grouped select and exceedance ----

extern "C" {

int rscm_ens_set_member_groups(rscm_ens* h, const int32_t* group, int32_t on_device, int32_t n_groups)
{
    GUARD_BEGIN
    NEED(h);
    if (!group) return fail(RSCM_ERR_INVALID, "groups are NULL");
    if (n_groups < 1 || n_groups > rscm::kMaxMemberGroups)
        return fail(RSCM_ERR_INVALID, "n_groups = %d: must be in [1, %d]", n_groups, rscm::kMaxMemberGroups);
    if (h->select) return fail(RSCM_ERR_STATE, "a select is in flight on this handle: rscm_ens_select_end it first");
    if (int rc = set_device(h)) return rc;
    rscm::DevBuf<int32_t> d_new, d_flag;
    int32_t bad = 0;
    HIPCHK(d_new.alloc((size_t)h->N));
    HIPCHK(d_flag.alloc(1));
    HIPCHK(hipMemcpyAsync(d_new.get(), group, (size_t)h->N * sizeof(int32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(d_flag.get(), 0, sizeof(int32_t), h->stream));
    HIPCHK(rscm::launch_groups_check(d_new.get(), h->N, n_groups, d_flag.get(), h->stream));
    HIPCHK(hipMemcpyAsync(&bad, d_flag.get(), sizeof bad, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (bad) return fail(RSCM_ERR_INVALID, "a member's group id is outside [-1, %d)", n_groups);
    h->d_groups = std::move(d_new);
    h->n_groups = n_groups;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_member_groups_devptr(rscm_ens* h, void** out, int32_t* n_groups)
{
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = h->d_groups;
    if (n_groups) *n_groups = h->d_groups ? h->n_groups : 0;
    if (!h->d_groups) return fail(RSCM_ERR_STATE, "no member groups set");
    return RSCM_OK;
}

int rscm_ens_clear_member_groups(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (h->select) return fail(RSCM_ERR_STATE, "a select is in flight on this handle: rscm_ens_select_end it first");
    if (h->d_groups) {
        if (int rc = set_device(h)) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        h->d_groups.reset();
        h->n_groups = 0;
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
