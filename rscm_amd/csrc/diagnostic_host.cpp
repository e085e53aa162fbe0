// Host side of the diagnostic variables (rscm_ens_define_diagnostic, rscm_ens_diagnostic, rscm_ens_compute_diagnostic,
// rscm_ens_clear_diagnostics; kernel in diagnostic.hip): per-member linear combinations of a handle's stored variables, kept as rows of
// their own that every reader of rows takes by variable id (rscm_ens::row_ptr, check_row_range; the definition is stated in
// include/rscm_gpu.h).
//
// The source rows are resolved as the per-member statistics resolve theirs (period_rows: full storage, the window, the output store;
// every row computed and resident).  The rows are a snapshot of the sources at the handle's write epoch (ens.hpp, rows_written): a
// reader that finds another epoch is told to compute again.  A staged select may be reading the rows, so nothing here runs while
// one is in flight.
//
// An energy-budget diagnostic (energy_budget_host.cpp) takes one of the same slots and is computed through the same entry point: its
// sources are the two state rows of the two-layer kind, its checks and its launch are budget_check and budget_launch.  So does a running
// mean (running_mean_host.cpp), whose whole compute is running_mean_compute.
#include <cmath>

#include "diagnostic.hpp"
#include "ens.hpp"

static_assert(rscm::kDiagMaxTerms == RSCM_DIAG_MAX_TERMS, "the term limit in diagnostic.hpp and rscm_gpu.h must agree");

namespace {

int check_is_diagnostic(const rscm_ens* h, int32_t var_id)
{
    if (!h->is_diagnostic(var_id))
        return fail(RSCM_ERR_INVALID, "variable %d is no diagnostic of this handle (%d defined, ids from %d)", var_id, h->n_diag, h->V);
    return RSCM_OK;
}

}  // namespace

int check_diagnostic_current(const rscm_ens* h, int32_t var_id)
{
    if (h->is_diagnostic(var_id) && h->diagnostic_stale(var_id)) return fail(RSCM_ERR_STATE, "diagnostic %d is stale: compute it again", var_id);
    return RSCM_OK;
}

extern "C" {

int rscm_ens_define_diagnostic(rscm_ens* h, int32_t n_terms, const int32_t* term_var, const int32_t* term_param_row, const double* term_scale,
                               int32_t* var_id_out)
{
    GUARD_BEGIN
    NEED(h);
    if (!var_id_out) return fail(RSCM_ERR_INVALID, "var_id_out is NULL");
    if (n_terms < 1 || n_terms > RSCM_DIAG_MAX_TERMS || !term_var || !term_param_row || !term_scale)
        return fail(RSCM_ERR_INVALID, "bad term list (1 to %d terms)", RSCM_DIAG_MAX_TERMS);
    for (int32_t k = 0; k < n_terms; ++k) {
        if (term_var[k] < 1 || term_var[k] >= h->V)
            return fail(RSCM_ERR_INVALID, "term %d: variable %d has no stored series (a diagnostic combines stored variables only)", k, term_var[k]);
        if (term_param_row[k] < -1 || term_param_row[k] >= h->P)
            return fail(RSCM_ERR_INVALID, "term %d: parameter row %d is outside [-1, %d)", k, term_param_row[k], h->P);
        if (!std::isfinite(term_scale[k])) return fail(RSCM_ERR_INVALID, "term %d: the scale is not finite", k);
    }
    if (h->n_diag == RSCM_DIAG_MAX) return fail(RSCM_ERR_INVALID, "this handle has its %d diagnostics: rscm_ens_clear_diagnostics first", RSCM_DIAG_MAX);
    if (int rc = no_select(h)) return rc;
    rscm_ens::Diagnostic& d = h->diag[h->n_diag];
    d.n_terms = n_terms;
    for (int32_t k = 0; k < n_terms; ++k) {
        d.var[k] = term_var[k];
        d.row[k] = term_param_row[k];
        d.scale[k] = term_scale[k];
    }
    d.quantity = 0;
    d.budget_scale = 0.0;
    d.held = 0;
    *var_id_out = h->V + h->n_diag++;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_diagnostic(rscm_ens* h, int32_t var_id, int32_t* n_terms, int32_t term_var[4], int32_t term_param_row[4], double term_scale[4],
                        int32_t* rows_held, int32_t* t_begin, int32_t* t_stride)
{
    NEED(h);
    if (int rc = check_is_diagnostic(h, var_id)) return rc;
    const rscm_ens::Diagnostic& d = h->diag[var_id - h->V];
    if (n_terms) *n_terms = d.n_terms;
    for (int32_t k = 0; k < RSCM_DIAG_MAX_TERMS; ++k) {
        const bool on = k < d.n_terms;
        if (term_var) term_var[k] = on ? d.var[k] : 0;
        if (term_param_row) term_param_row[k] = on ? d.row[k] : -1;
        if (term_scale) term_scale[k] = on ? d.scale[k] : 0.0;
    }
    const bool current = d.held > 0 && h->diagnostic_current(d);
    if (rows_held) *rows_held = current ? d.held : 0;
    if (t_begin) *t_begin = current ? d.t_begin : 0;
    if (t_stride) *t_stride = current ? d.t_stride : 1;
    return RSCM_OK;
}

int rscm_ens_compute_diagnostic(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = check_is_diagnostic(h, var_id)) return rc;
    if (int rc = no_select(h)) return rc;
    rscm_ens::Diagnostic& d = h->diag[var_id - h->V];
    if (d.rm_source != 0) return running_mean_compute(h, d, t_begin, t_end, t_stride);
    // the sources' rows, term after term: [K][R]
    std::vector<const double*> rows, term_rows;
    std::vector<double> times;
    const bool budget = d.quantity != 0;   // its sources: Ts, then Td
    const int32_t budget_var[2] = {RSCM_TL_VAR_TS, RSCM_TL_VAR_TD};
    for (int32_t k = 0; k < (budget ? 2 : d.n_terms); ++k) {
        term_rows.clear();
        times.clear();
        if (int rc = period_rows(h, budget ? budget_var[k] : d.var[k], t_begin, t_end, t_stride, term_rows, times)) return rc;
        rows.insert(rows.end(), term_rows.begin(), term_rows.end());
    }
    const size_t R = times.size();
    if (budget)
        if (int rc = budget_check(h, d, t_begin, t_stride, (int32_t)R)) return rc;
    bool reads_params = false;
    for (int32_t k = 0; k < d.n_terms; ++k) reads_params = reads_params || d.row[k] >= 0;
    if (reads_params && !h->params_set) return fail(RSCM_ERR_STATE, "parameters not set: a term's weight reads a parameter row");
    if (int rc = set_device(h)) return rc;
    const size_t need = R * (size_t)h->N;
    if (d.d_rows.size() < need) {   // allocated at first use, reused when large enough; nobody reads the old rows (no select in flight)
        HIPCHK(hipStreamSynchronize(h->stream));
        d.held = 0;   // too large to hold twice: the old rows go first, and a failed allocation leaves a store that serves none
        HIPCHK(d.d_rows.reserve(need));
    }
    rscm::DevBuf<const double*> d_src;   // lives until the synchronise below
    HIPCHK(d_src.alloc(rows.size()));
    HIPCHK(hipMemcpyAsync(d_src.get(), rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice, h->stream));
    if (budget) {
        d.held = 0;   // (as below)
        HIPCHK(budget_launch(h, d, d_src.get(), t_begin, t_stride, (int32_t)R));
        HIPCHK(hipStreamSynchronize(h->stream));
        d.held = (int32_t)R;
        d.t_begin = t_begin;
        d.t_stride = t_stride;
        d.epoch = h->write_epoch;
        d.forcing_epoch = h->forcing_epoch;
        return RSCM_OK;
    }
    rscm::DiagnosticArgs a{};
    a.d_rows = d_src.get();
    a.d_params = h->d_params;
    a.d_out = d.d_rows;
    a.N = h->N;
    a.n_rows = (int32_t)R;
    for (int32_t k = 0; k < d.n_terms; ++k) {
        a.param_row[k] = d.row[k];
        a.scale[k] = d.scale[k];
    }
    d.held = 0;   // whatever fails from here on, the store no longer holds the old range
    HIPCHK(rscm::launch_diagnostic(a, d.n_terms, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    d.held = (int32_t)R;
    d.t_begin = t_begin;
    d.t_stride = t_stride;
    d.epoch = h->write_epoch;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_clear_diagnostics(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = no_select(h)) return rc;
    if (h->n_diag > 0) {
        if (int rc = set_device(h)) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        for (rscm_ens::Diagnostic& d : h->diag) d = rscm_ens::Diagnostic();   // the stores go with their definitions
        h->n_diag = 0;
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
