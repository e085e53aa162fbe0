// What the HOST needs to know about each kind of ensemble (RSCM_KIND_*, include/rscm_gpu.h), one row per kind in kind order: sizes,
// state variables, look-back, which launcher it goes through and how the lock-step scheduler treats it.  Host only: no kernel file
// includes this.  Behaviour that is particular to one kind (ClimateUDEB's and OceanCarbon's host-built tables, GhgForcing's method, the
// N2O delay, the aggregate's NaN block, the structural rows) stays where it is and names that kind.
#pragma once

#include "../../include/rscm_gpu.h"

#include <cstdint>

namespace rscm {

// whose argument struct and launcher a kind uses (rscm_device.hpp; launch_host.cpp has one builder per family)
enum class Family : uint8_t { TwoLayer, Coupled, Udeb, Ghg, Pointwise, Chem, Carbon, Ocean, Halo };

struct KindInfo {
    int32_t kind;
    const char* name;
    int32_t n_params;     // parameter rows (a mix handle adds its coefficient rows)
    int32_t n_vars;       // variable ids, the input block 0 included: the stored series are 1 .. n_vars - 1
    int32_t n_inputs;     // rows per scenario of the shared input block
    int32_t state_first, state_last;   // the state variables (they need an initial value), one contiguous range; 1, 0: none
    int32_t lookback;     // own rows before the current one that a step reads, as the handle starts out (N2O: refreshed by set_params)
    bool needs_bounds;    // the kernel uses the step length: the time bounds go to the device
    bool has_derived;     // member constants formed from the parameters by a kernel of their own (ensure_derived)
    bool reads_end;       // linked inputs are read at the end of the step (index n + 1) whatever `source` said
    Family family;
    bool fusable;         // its one-step launch can join a fused launch (csrc/group.hip); GhgForcing: with linked inputs only
    bool internal_state;  // its component keeps state besides the stored rows (the reference's ComponentState): internal_state.hpp
    int32_t op_cost;      // plan_split's estimate: one unit ~ a dependent round trip to memory plus a few dozen instructions; the
                          // chemistry's Prather passes, the forcing formulas' logarithms and the RK4 box models weigh by their
                          // instruction counts on top
};

// ClimateUDEB, OceanCarbon, HalocarbonChemistry and the fused coupled chain are heavy components: they keep their own launches.
constexpr KindInfo kKinds[] = {
    //  kind                        name                   P  V   in  states lb  bounds derive end   family         fusable state  cost
    {RSCM_KIND_TWO_LAYER,          "TwoLayer",             6,  3,  1, 1,  2, 0, false, false, false, Family::TwoLayer,  true,  false, 12},
    {RSCM_KIND_COUPLED,            "Coupled",             10,  8,  1, 1,  5, 0, false, false, false, Family::Coupled,   false, false, 1},
    {RSCM_KIND_UDEB,               "ClimateUDEB",         37,  8,  1, 1,  4, 0, true,  true,  true,  Family::Udeb,      false, true,  1},
    {RSCM_KIND_GHG_FORCING,        "GhgForcing",          21,  4,  3, 1,  0, 0, false, true,  false, Family::Ghg,       true,  false, 4},
    {RSCM_KIND_OZONE_FORCING,      "OzoneForcing",        13,  4,  6, 1,  0, 0, false, false, false, Family::Pointwise, true,  false, 2},
    {RSCM_KIND_AEROSOL_DIRECT,     "AerosolDirect",       27,  5,  4, 1,  0, 0, false, false, false, Family::Pointwise, true,  false, 2},
    {RSCM_KIND_AEROSOL_INDIRECT,   "AerosolIndirect",      9,  2,  2, 1,  0, 0, false, false, false, Family::Pointwise, true,  false, 1},
    {RSCM_KIND_CH4_CHEMISTRY,      "CH4Chemistry",        18,  3,  5, 1,  1, 1, false, false, false, Family::Chem,      true,  false, 6},   // previous()
    {RSCM_KIND_N2O_CHEMISTRY,      "N2OChemistry",         6,  3,  1, 1,  1, 2, true,  false, false, Family::Chem,      true,  false, 5},   // at_offset(-(strat_delay + 1))
    {RSCM_KIND_CO2_BUDGET,         "CO2Budget",            2,  4,  4, 1,  1, 0, true,  false, false, Family::Carbon,    true,  false, 1},
    {RSCM_KIND_TERRESTRIAL_CARBON, "TerrestrialCarbon",   20,  6,  3, 1,  4, 0, true,  true,  false, Family::Carbon,    true,  false, 4},
    {RSCM_KIND_OCEAN_CARBON,       "OceanCarbon",         24,  4,  2, 1,  2, 0, true,  false, false, Family::Ocean,     false, true,  1},
    {RSCM_KIND_HALOCARBON,         "HalocarbonChemistry", 293, 46, 41, 1, 41, 0, true,  false, false, Family::Halo,      false, false, 1},
    {RSCM_KIND_FOURBOX_OHU,        "FourBoxOHU",           4,  5,  1, 1,  0, 0, false, false, false, Family::Pointwise, true,  false, 1},
    {RSCM_KIND_OSPP,               "OSPP",                13,  2,  2, 1,  0, 0, false, false, false, Family::Pointwise, true,  false, 1},
    {RSCM_KIND_CARBON_CYCLE,       "CarbonCycle",          3,  4,  2, 1,  3, 0, false, false, false, Family::Carbon,    true,  false, 4},
    {RSCM_KIND_CO2_ERF,            "CO2ERF",               2,  2,  1, 1,  0, 0, false, false, false, Family::Pointwise, true,  false, 1},
    {RSCM_KIND_AGGREGATE,          "Aggregate",            9,  2,  8, 1,  0, 0, false, false, true,  Family::Pointwise, true,  false, 1},
};
constexpr int32_t kNumKinds = (int32_t)(sizeof kKinds / sizeof kKinds[0]);

// parameter and input rows as include/rscm_gpu.h states them, in kind order (it has no input count for the first four kinds)
constexpr int32_t kHeaderSizes[][2] = {
    {RSCM_TL_NPARAMS, 1}, {RSCM_CP_NPARAMS, 1}, {RSCM_UD_NPARAMS, 1}, {RSCM_GH_NPARAMS, 3}, {RSCM_OZ_NPARAMS, RSCM_OZ_NINPUTS},
    {RSCM_AD_NPARAMS, RSCM_AD_NINPUTS}, {RSCM_AI_NPARAMS, RSCM_AI_NINPUTS}, {RSCM_CH4_NPARAMS, RSCM_CH4_NINPUTS},
    {RSCM_N2O_NPARAMS, RSCM_N2O_NINPUTS}, {RSCM_CB_NPARAMS, RSCM_CB_NINPUTS}, {RSCM_TC_NPARAMS, RSCM_TC_NINPUTS},
    {RSCM_OC_NPARAMS, RSCM_OC_NINPUTS}, {RSCM_HC_NPARAMS, RSCM_HC_NINPUTS}, {RSCM_FB_NPARAMS, RSCM_FB_NINPUTS},
    {RSCM_SP_NPARAMS, RSCM_SP_NINPUTS}, {RSCM_CC_NPARAMS, RSCM_CC_NINPUTS}, {RSCM_CE_NPARAMS, RSCM_CE_NINPUTS},
    {RSCM_AG_NPARAMS, RSCM_AG_NINPUTS}};
constexpr bool kinds_match_header()
{
    for (int32_t k = 0; k < kNumKinds; ++k)
        if (kKinds[k].kind != k || kKinds[k].n_params != kHeaderSizes[k][0] || kKinds[k].n_inputs != kHeaderSizes[k][1] ||
            kKinds[k].state_last >= kKinds[k].n_vars)
            return false;
    return true;
}
static_assert(kNumKinds == RSCM_KIND_AGGREGATE + 1 && sizeof kHeaderSizes / sizeof kHeaderSizes[0] == kNumKinds, "one row per RSCM_KIND_*");
static_assert(kinds_match_header(), "row k describes kind k with the header's NPARAMS / NINPUTS, and its states are stored variables");
static_assert(kKinds[RSCM_KIND_HALOCARBON].state_last == RSCM_HC_NSPECIES && kKinds[RSCM_KIND_COUPLED].state_last == RSCM_CP_VAR_CUM_EMIS &&
                  kKinds[RSCM_KIND_UDEB].state_last == RSCM_UD_VAR_ST_SH_LAND && kKinds[RSCM_KIND_TWO_LAYER].state_last == RSCM_TL_VAR_TD,
              "the state ranges follow the header's variable ids");

}  // namespace rscm
