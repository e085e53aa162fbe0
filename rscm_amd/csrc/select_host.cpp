// Host side of the staged quantile select (rscm_ens_select_* and rscm_ens_quantile_rows; kernels in select.hip).
//
// A select resolves its rows once, at begin, into a device array of row pointers (rscm_ens::row_ptr: full storage, the window or
// the strided output store), then alternates pass (histograms of this handle's members) and commit (the reduced histograms move
// every target one digit on) kSelPasses times.  Between the two a caller with several handles -- ranks of one sharded ensemble,
// or two ensembles on one GPU -- sums the int64 buffers of all of them; every handle then commits the same sums and so reaches
// the same keys.
#include "ens.hpp"

struct SelectState {
    int32_t var = 0, t_begin = 0, t_stride = 1;
    int32_t n_rows = 0;     // rows of the range
    int32_t n_comp = 0;     // the first n_comp of them are computed (t <= time_index); the others report count 0, NaN
    int32_t n_q = 0, n_t = 0;
    int32_t pass = 0;       // the next pass to histogram
    bool awaiting_commit = false;
    const double** d_rows = nullptr;
    double* d_q = nullptr;
    int64_t* d_hist = nullptr;
    size_t hist_elems = 0;
    int64_t* d_count = nullptr;
    uint64_t* d_prefix = nullptr;
    int64_t* d_rank = nullptr;
    double* d_out = nullptr;

    void release()
    {
        (void)hipFree(d_rows);
        (void)hipFree(d_q);
        (void)hipFree(d_hist);
        (void)hipFree(d_count);
        (void)hipFree(d_prefix);
        (void)hipFree(d_rank);
        (void)hipFree(d_out);
        d_rows = nullptr;
        d_q = nullptr;
        d_hist = nullptr;
        d_count = nullptr;
        d_prefix = nullptr;
        d_rank = nullptr;
        d_out = nullptr;
    }
};

namespace {

constexpr int32_t kMaxSelectQuantiles = 128;

int select_init(rscm_ens* h, SelectState& s, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q)
{
    if (var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (t_begin < 0 || t_end > h->T || t_begin > t_end || t_stride < 1)
        return fail(RSCM_ERR_INVALID, "bad time range [%d, %d) stride %d", t_begin, t_end, t_stride);
    if (n_q < 1 || n_q > kMaxSelectQuantiles || !q) return fail(RSCM_ERR_INVALID, "bad quantile list (1 to %d quantiles)", kMaxSelectQuantiles);
    for (int32_t k = 0; k < n_q; ++k)
        if (!(q[k] >= 0.0 && q[k] <= 1.0)) return fail(RSCM_ERR_INVALID, "Quantiles must be in the range [0, 1], got %g", q[k]);
    if (!h->windowed && h->rows != h->T && t_end > 1)
        return fail(RSCM_ERR_STATE, "this handle stores only the initial row (RSCM_FLAG_NO_SERIES)");
    s.var = var_id;
    s.t_begin = t_begin;
    s.t_stride = t_stride;
    s.n_q = n_q;
    s.n_t = 2 * n_q;
    std::vector<const double*> rows;
    for (int32_t t = t_begin; t < t_end; t += t_stride) {
        ++s.n_rows;
        if (t > h->time_index) continue;   // never computed by this model instance
        const double* p = h->row_ptr(var_id, t);
        if (!p)
            return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident: the window holds [%d, %d) and the output store every %d-th row%s",
                        t, var_id, h->win0, h->win0 + h->rows, h->out_stride,
                        h->out_slot.empty() || h->out_slot[var_id] < 0 ? " of other variables" : "");
        rows.push_back(p);
    }
    s.n_comp = (int32_t)rows.size();
    if (s.n_comp == 0) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    const size_t nc = (size_t)s.n_comp, nt = (size_t)s.n_t;
    s.hist_elems = nc * nt * rscm::kSelBins;
    HIPCHK(rscm::dev_malloc(&s.d_rows, nc * sizeof(double*)));
    HIPCHK(rscm::dev_malloc(&s.d_q, (size_t)n_q * sizeof(double)));
    HIPCHK(rscm::dev_malloc(&s.d_hist, s.hist_elems * sizeof(int64_t)));
    HIPCHK(rscm::dev_malloc(&s.d_count, nc * sizeof(int64_t)));
    HIPCHK(rscm::dev_malloc(&s.d_prefix, nc * nt * sizeof(uint64_t)));
    HIPCHK(rscm::dev_malloc(&s.d_rank, nc * nt * sizeof(int64_t)));
    HIPCHK(rscm::dev_malloc(&s.d_out, nc * (size_t)(n_q + 1) * sizeof(double)));
    HIPCHK(hipMemcpyAsync(s.d_rows, rows.data(), nc * sizeof(double*), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s.d_q, q, (size_t)n_q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the host vectors go out of scope
    return RSCM_OK;
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
    const size_t elems = (size_t)s.n_comp * rscm::kSelBins * (s.pass == 0 ? 1 : (size_t)s.n_t);
    HIPCHK(rscm::launch_select_hist(s.d_rows, h->N, s.n_comp, s.pass, s.d_prefix, s.n_t, s.d_hist, elems, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    s.awaiting_commit = true;
    *done = 0;
    if (buf_dev) *buf_dev = s.d_hist;
    if (n) *n = (int64_t)elems;
    return RSCM_OK;
}

int select_commit(rscm_ens* h, SelectState& s)
{
    if (!s.awaiting_commit) return fail(RSCM_ERR_STATE, "select: no pass to commit");
    if (int rc = set_device(h)) return rc;
    HIPCHK(rscm::launch_select_commit(s.d_hist, s.pass, s.n_comp, s.n_t, s.d_q, s.d_count, s.d_prefix, s.d_rank, h->stream));
    s.awaiting_commit = false;
    if (++s.pass == rscm::kSelPasses)
        HIPCHK(rscm::launch_select_finish(s.d_count, s.d_prefix, s.n_comp, s.n_q, s.d_q, s.d_out, h->stream));
    return RSCM_OK;
}

int select_result(rscm_ens* h, SelectState& s, double* out, double* count)
{
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (s.n_comp > 0 && s.pass < rscm::kSelPasses)
        return fail(RSCM_ERR_STATE, "select: %d of %d passes are still to run", rscm::kSelPasses - s.pass, rscm::kSelPasses);
    std::vector<double> host((size_t)s.n_comp * (s.n_q + 1));
    if (s.n_comp > 0) {
        if (int rc = set_device(h)) return rc;
        HIPCHK(hipMemcpyAsync(host.data(), s.d_out, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    for (int32_t r = 0; r < s.n_rows; ++r) {
        const bool c = r < s.n_comp;
        if (count) count[r] = c ? host[(size_t)r * (s.n_q + 1)] : 0.0;
        for (int32_t k = 0; k < s.n_q; ++k)
            out[(size_t)r * s.n_q + k] = c ? host[(size_t)r * (s.n_q + 1) + 1 + k] : std::numeric_limits<double>::quiet_NaN();
    }
    return RSCM_OK;
}

}  // namespace

void select_release(rscm_ens* h)
{
    if (!h->select) return;
    h->select->release();
    delete h->select;
    h->select = nullptr;
}

extern "C" {

int rscm_ens_select_begin(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_q, const double* q)
{
    GUARD_BEGIN
    NEED(h);
    if (h->select) return fail(RSCM_ERR_STATE, "a select is already in flight on this handle: rscm_ens_select_end it first");
    auto* s = new SelectState();
    if (int rc = select_init(h, *s, var_id, t_begin, t_end, t_stride, n_q, q)) {
        s->release();
        delete s;
        return rc;
    }
    h->select = s;
    return RSCM_OK;
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
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    SelectState s;   // its own state: a staged select in flight on the handle is left alone
    int rc = select_init(h, s, var_id, t_begin, t_end, t_stride, n_q, q);
    int32_t done = 0;
    while (rc == RSCM_OK) {
        if ((rc = select_pass(h, s, &done, nullptr, nullptr)) != RSCM_OK || done) break;
        rc = select_commit(h, s);
    }
    if (rc == RSCM_OK) rc = select_result(h, s, out, count);
    if (s.d_rows) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
    }
    s.release();
    return rc;
    GUARD_END
}

}  // extern "C"
