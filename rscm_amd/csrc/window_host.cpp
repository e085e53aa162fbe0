// ---- windowed series (RSCM_FLAG_WINDOWED): d_series holds rows [win0, win0 + rows) of every series ----
#include "ens.hpp"

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
int window_seek(rscm_ens* h, int32_t k)
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
