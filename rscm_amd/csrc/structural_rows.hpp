// The parameter rows from which the HOST derives state when a handle is configured (configure_kind, kind_config.cpp: ClimateUDEB's
// geometry tables and look-back windows, OceanCarbon's impulse-response table and mode fit, GhgForcing's method switch): marked [u] in
// rscm_gpu.h, listed here once.  Nothing that writes parameters on the device (the samplers' proposals, the Latin hypercube) may touch
// them -- the derived tables would silently stay those of the base value, where the reference rebuilds the component for every parameter
// vector (model_runner.rs:257-266) -- and the `uniform` ones must hold ONE value for all members.  Host only: no other include.
#pragma once

#include "../../include/rscm_gpu.h"

namespace rscm {

struct StructuralRow { int kind, row; const char* name; bool uniform; };
constexpr int kN2oDelayRow = 4;
constexpr StructuralRow kStructuralRows[] = {
    {RSCM_KIND_UDEB, RSCM_UD_P_N_LAYERS, "n_layers", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_MIXED_LAYER_DEPTH, "mixed_layer_depth", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_LAYER_THICKNESS, "layer_thickness", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_DEPTH_DEPENDENT_AREA, "depth_dependent_area", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_LAND_HC_ENABLED, "land_heat_capacity_enabled", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_EFFICACY_APPLY, "efficacy_apply", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_OCEAN_TEMP_PROFILE, "ocean_temp_profile", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_STEPS_PER_YEAR, "steps_per_year", true},
    {RSCM_KIND_UDEB, RSCM_UD_P_FEEDBACK_CUMT_PERIOD, "feedback_cumt_period", true},
    {RSCM_KIND_GHG_FORCING, RSCM_GH_P_METHOD, "method", true},
    {RSCM_KIND_OCEAN_CARBON, RSCM_OC_P_MODEL, "model", true},
    {RSCM_KIND_OCEAN_CARBON, RSCM_OC_P_IRF_SCALE, "irf_scale", true},
    {RSCM_KIND_OCEAN_CARBON, RSCM_OC_P_STEPS_PER_YEAR, "steps_per_year", true},
    {RSCM_KIND_OCEAN_CARBON, RSCM_OC_P_MAX_HISTORY_MONTHS, "max_history_months", true},
    {RSCM_KIND_OCEAN_CARBON, RSCM_OC_P_IRF_SWITCH_TIME, "irf_switch_time", true},
    // The N2O delay has a standing of its own: the samplers refuse it like the rows above, but it MAY vary over the members -- the host
    // derives only the look-back from it, sized for the largest value (n2o_lookback) -- so rscm_ens_sample_lhs lets low and high differ
    {RSCM_KIND_N2O_CHEMISTRY, kN2oDelayRow, "stratospheric delay (sets the look-back)", false},
};

}  // namespace rscm

// the row's name for the error text, or nullptr: what the samplers, the Latin hypercube and the gather ask
constexpr const char* structural_row(int kind, int row)
{
    for (const rscm::StructuralRow& s : rscm::kStructuralRows)
        if (s.kind == kind && s.row == row) return s.name;
    return nullptr;
}
