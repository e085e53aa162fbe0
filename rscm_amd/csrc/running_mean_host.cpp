// Host side of the running-mean diagnostics (rscm_ens_define_running_mean, rscm_ens_diagnostic_running_mean; kernel in
// running_mean.hip): the mean of `window` rows of a variable, `step` time indices apart, as a diagnostic variable (the definition is
// stated in include/rscm_gpu.h).  It takes the slots, the ids, the store and the write epoch of the linear diagnostics
// (diagnostic_host.cpp) and is computed through rscm_ens_compute_diagnostic, which hands the call to running_mean_compute below.
//
// The source is a stored variable or a diagnostic defined earlier that is no running mean.  Its rows are resolved as every reader
// resolves them (period_rows: full storage, the window, the output store, a diagnostic's own store where it is current and holds
// exactly the row), all W + (R - 1) * m of them at spacing `step` in one walk, so nothing is launched on a row the host has not
// found.  No row is invented: an output whose window leaves the axis or the computed rows is refused.
#include "ens.hpp"
#include "running_mean.hpp"

static_assert(rscm::kRunMeanMaxWindow == RSCM_RUNMEAN_MAX_WINDOW, "the window limit in running_mean.hpp and rscm_gpu.h must agree");

namespace {

int32_t rows_back(const rscm_ens::Diagnostic& d) { return d.rm_align == RSCM_RUNMEAN_TRAILING ? d.rm_window - 1 : (d.rm_window - 1) / 2; }

}  // namespace

int running_mean_compute(rscm_ens* h, rscm_ens::Diagnostic& d, int32_t t_begin, int32_t t_end, int32_t t_stride)
{
    if (t_begin < 0 || t_end > h->T || t_begin >= t_end || t_stride < 1)
        return fail(RSCM_ERR_INVALID, "bad time range [%d, %d) stride %d (at least one row)", t_begin, t_end, t_stride);
    if (t_stride % d.rm_step != 0)
        return fail(RSCM_ERR_INVALID, "t_stride %d is no multiple of the running mean's step %d", t_stride, d.rm_step);
    const int64_t R = ((int64_t)t_end - 1 - t_begin) / t_stride + 1;
    const int64_t t_last = t_begin + (R - 1) * t_stride;
    const int64_t back = rows_back(d);
    const int64_t src_begin = (int64_t)t_begin - back * d.rm_step;
    const int64_t src_last = t_last + (d.rm_window - 1 - back) * d.rm_step;
    if (src_begin < 0 || src_last >= h->T)
        return fail(RSCM_ERR_INVALID, "rows [%d, %d) stride %d: their windows read the source rows %lld .. %lld, off the time axis [0, %d)", t_begin,
                    t_end, t_stride, (long long)src_begin, (long long)src_last, h->T);
    std::vector<const double*> rows;
    std::vector<double> times;
    if (int rc = period_rows(h, d.rm_source, (int32_t)src_begin, (int32_t)src_last + 1, d.rm_step, rows, times)) return rc;
    const int64_t m = t_stride / d.rm_step;
    if ((int64_t)rows.size() != (R - 1) * m + d.rm_window) return fail(RSCM_ERR_STATE, "the source rows of the running mean could not all be resolved");
    if (int rc = set_device(h)) return rc;
    const size_t need = (size_t)R * (size_t)h->N;
    if (d.d_rows.size() < need) {   // (as rscm_ens_compute_diagnostic: the old rows go first)
        HIPCHK(hipStreamSynchronize(h->stream));
        d.held = 0;
        HIPCHK(d.d_rows.reserve(need));
    }
    rscm::DevBuf<const double*> d_src;   // lives until the synchronise below
    if (int rc = upload_rows(h, rows, d_src)) return rc;
    rscm::RunningMeanArgs a{};
    a.d_rows = d_src.get();
    a.d_out = d.d_rows;
    a.N = h->N;
    a.n_rows = (int32_t)R;
    a.window = d.rm_window;
    a.m = (int32_t)m;
    d.held = 0;   // whatever fails from here on, the store no longer holds the old range
    HIPCHK(rscm::launch_running_mean(a, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    d.held = (int32_t)R;
    d.t_begin = t_begin;
    d.t_stride = t_stride;
    d.epoch = h->write_epoch;
    d.forcing_epoch = h->forcing_epoch;
    return RSCM_OK;
}

extern "C" {

int rscm_ens_define_running_mean(rscm_ens* h, int32_t source_var, int32_t window, int32_t align, int32_t step, int32_t* var_id_out)
{
    GUARD_BEGIN
    NEED(h);
    if (!var_id_out) return fail(RSCM_ERR_INVALID, "var_id_out is NULL");
    if (!h->has_rows(source_var))
        return fail(RSCM_ERR_INVALID, "source %d: a running mean averages a stored variable (1 .. %d) or a diagnostic defined before it (%d defined)",
                    source_var, h->V - 1, h->n_diag);
    const rscm_ens::Diagnostic* src = h->is_diagnostic(source_var) ? &h->diag[source_var - h->V] : nullptr;
    if (src && src->rm_source != 0) return fail(RSCM_ERR_INVALID, "source %d is a running mean itself", source_var);
    if (window < 2 || window > RSCM_RUNMEAN_MAX_WINDOW)
        return fail(RSCM_ERR_INVALID, "window %d: must be in [2, %d]", window, RSCM_RUNMEAN_MAX_WINDOW);
    if (align != RSCM_RUNMEAN_TRAILING && align != RSCM_RUNMEAN_CENTRED)
        return fail(RSCM_ERR_INVALID, "align %d: RSCM_RUNMEAN_TRAILING or RSCM_RUNMEAN_CENTRED", align);
    if (step < 1) return fail(RSCM_ERR_INVALID, "step %d: must be at least 1", step);
    if (h->n_diag == RSCM_DIAG_MAX) return fail(RSCM_ERR_INVALID, "this handle has its %d diagnostics: rscm_ens_clear_diagnostics first", RSCM_DIAG_MAX);
    if (int rc = no_select(h)) return rc;
    rscm_ens::Diagnostic& d = h->diag[h->n_diag];
    d.n_terms = 0;
    d.quantity = 0;
    d.budget_scale = 0.0;
    d.rm_source = source_var;
    d.rm_window = window;
    d.rm_align = align;
    d.rm_step = step;
    d.rm_forcing = src && src->reads_forcing();
    d.held = 0;
    *var_id_out = h->V + h->n_diag++;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_diagnostic_running_mean(rscm_ens* h, int32_t var_id, int32_t* source_var, int32_t* window, int32_t* align, int32_t* step)
{
    NEED(h);
    if (!h->is_diagnostic(var_id))
        return fail(RSCM_ERR_INVALID, "variable %d is no diagnostic of this handle (%d defined, ids from %d)", var_id, h->n_diag, h->V);
    const rscm_ens::Diagnostic& d = h->diag[var_id - h->V];
    const bool on = d.rm_source != 0;
    if (source_var) *source_var = d.rm_source;
    if (window) *window = on ? d.rm_window : 0;
    if (align) *align = on ? d.rm_align : 0;
    if (step) *step = on ? d.rm_step : 0;
    return RSCM_OK;
}

}  // extern "C"
