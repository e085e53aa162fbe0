// Host side of the energy-budget diagnostics (rscm_ens_define_energy_budget, rscm_ens_diagnostic_quantity; kernels in
// energy_budget.hip): the forcing a two-layer member saw, its radiative response, its deep-ocean heat uptake and its top-of-atmosphere
// imbalance as diagnostic variables (the definition is stated in include/rscm_gpu.h).  They take the slots, the ids, the store and the
// write epoch of the linear diagnostics (diagnostic_host.cpp) and are computed through rscm_ens_compute_diagnostic, which resolves the
// two state rows as it resolves any source and calls budget_check and budget_launch below.
//
// The two quantities that read the forcing read it at index t + off of the forcing axis for row t (off: 0 for an exogenous source, 1
// for RSCM_SRC_UPSTREAM), the index the stepping kernel reads for the step out of row t.  Nothing is launched on an index the host
// has not proved in range: the rows come resolved, the forcing indices are checked here against the axis, the scenario ids were
// checked by rscm_ens_set_forcing (the one writer of d_scen) and the parameter rows against P.  A linked forcing is another
// ensemble's series, not a table: refused for those two quantities, at define time and again here should the link be made later.
#include <cmath>

#include "energy_budget.hpp"
#include "ens.hpp"

static_assert(rscm::kBudgetForcing == RSCM_BUDGET_FORCING && rscm::kBudgetResponse == RSCM_BUDGET_RESPONSE &&
                  rscm::kBudgetDeepUptake == RSCM_BUDGET_DEEP_UPTAKE && rscm::kBudgetImbalance == RSCM_BUDGET_IMBALANCE,
              "the quantities in energy_budget.hpp and rscm_gpu.h must agree");

namespace {

const char* quantity_name(int32_t q)
{
    switch (q) {
        case RSCM_BUDGET_FORCING: return "forcing";
        case RSCM_BUDGET_RESPONSE: return "radiative response";
        case RSCM_BUDGET_DEEP_UPTAKE: return "deep-ocean heat uptake";
        default: return "top-of-atmosphere imbalance";
    }
}

int32_t forcing_offset(const rscm_ens* h) { return h->source == RSCM_SRC_UPSTREAM ? 1 : 0; }

}  // namespace

int budget_check(const rscm_ens* h, const rscm_ens::Diagnostic& d, int32_t t_begin, int32_t t_stride, int32_t n_rows)
{
    if (!h->params_set) return fail(RSCM_ERR_STATE, "parameters not set: the %s reads the member's parameter rows", quantity_name(d.quantity));
    if (h->P < 6 + h->n_comp) return fail(RSCM_ERR_INVALID, "this handle has %d parameter rows, the energy budget reads %d", h->P, 6 + h->n_comp);
    if (!d.reads_forcing()) return RSCM_OK;
    if (h->n_linked > 0)
        return fail(RSCM_ERR_INVALID, "the forcing of this handle is linked (rscm_ens_link_input): the %s of a linked handle is not available",
                    quantity_name(d.quantity));
    if (!h->forcing_set || !h->d_forcing) return fail(RSCM_ERR_STATE, "forcing not set: the %s reads the member's forcing", quantity_name(d.quantity));
    if (h->noise_kind == rscm::kNoiseKindMembers && (h->noise_sigma_row() < 0 || h->noise_phi_row() + 1 > h->P))
        return fail(RSCM_ERR_INVALID, "per-member forcing noise without its parameter rows");
    const int32_t off = forcing_offset(h);
    for (int32_t r = 0; r < n_rows; ++r) {
        const int64_t t = (int64_t)t_begin + (int64_t)r * t_stride;
        if (t + off < 0 || t + off >= h->T)
            return fail(RSCM_ERR_INVALID, "row %lld: the step out of it reads forcing index %lld, past the end of the forcing axis [0, %d)", (long long)t,
                        (long long)(t + off), h->T);
    }
    return RSCM_OK;
}

hipError_t budget_launch(rscm_ens* h, rscm_ens::Diagnostic& d, const double* const* d_src, int32_t t_begin, int32_t t_stride, int32_t n_rows)
{
    rscm::EnergyBudgetArgs a{};
    a.d_rows = d_src;
    a.d_params = h->d_params;
    a.uniform_rows = h->uniform_rows;
    a.d_out = d.d_rows;
    a.N = h->N;
    a.n_rows = n_rows;
    a.quantity = d.quantity;
    a.scale = d.budget_scale;
    int32_t noise = rscm::kNoiseKindNone;
    if (d.reads_forcing()) {
        a.d_forcing = h->d_forcing;
        a.d_scen = h->d_scen;
        a.n_times = h->T;
        a.n_comp = h->n_comp;
        a.f0 = t_begin + forcing_offset(h);
        a.f_stride = t_stride;
        noise = h->noise_kind;
        a.noise_seed = h->noise_seed;
        a.noise_sigma = h->noise_sigma;
        a.noise_phi = h->noise_phi;
        a.noise_member0 = h->noise_offset;
        a.noise_sigma_row = h->noise_sigma_row();
        a.noise_phi_row = h->noise_phi_row();
    }
    return rscm::launch_energy_budget(a, noise, h->stream);
}

extern "C" {

int rscm_ens_define_energy_budget(rscm_ens* h, int32_t quantity, double scale, int32_t* var_id_out)
{
    GUARD_BEGIN
    NEED(h);
    if (!var_id_out) return fail(RSCM_ERR_INVALID, "var_id_out is NULL");
    if (h->kind != RSCM_KIND_TWO_LAYER)
        return fail(RSCM_ERR_INVALID, "the energy budget is defined for the two-layer kind only (RSCM_KIND_TWO_LAYER), this handle has kind %d", h->kind);
    if (quantity < RSCM_BUDGET_FORCING || quantity > RSCM_BUDGET_IMBALANCE)
        return fail(RSCM_ERR_INVALID, "unknown energy-budget quantity %d (RSCM_BUDGET_FORCING .. RSCM_BUDGET_IMBALANCE)", quantity);
    if (!std::isfinite(scale)) return fail(RSCM_ERR_INVALID, "the scale is not finite");
    if (h->n_linked > 0 && rscm::budget_reads_forcing(quantity))
        return fail(RSCM_ERR_INVALID, "the forcing of this handle is linked (rscm_ens_link_input): only the radiative response and the deep-ocean heat "
                                      "uptake are available");
    if (h->n_diag == RSCM_DIAG_MAX) return fail(RSCM_ERR_INVALID, "this handle has its %d diagnostics: rscm_ens_clear_diagnostics first", RSCM_DIAG_MAX);
    if (int rc = no_select(h)) return rc;
    rscm_ens::Diagnostic& d = h->diag[h->n_diag];
    d.n_terms = 0;
    d.quantity = quantity;
    d.budget_scale = scale;
    d.held = 0;
    *var_id_out = h->V + h->n_diag++;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_diagnostic_quantity(rscm_ens* h, int32_t var_id, int32_t* quantity, double* scale)
{
    NEED(h);
    if (!h->is_diagnostic(var_id))
        return fail(RSCM_ERR_INVALID, "variable %d is no diagnostic of this handle (%d defined, ids from %d)", var_id, h->n_diag, h->V);
    const rscm_ens::Diagnostic& d = h->diag[var_id - h->V];
    if (quantity) *quantity = d.quantity;
    if (scale) *scale = d.quantity ? d.budget_scale : 0.0;
    return RSCM_OK;
}

}  // extern "C"
