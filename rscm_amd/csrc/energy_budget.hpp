// What the host side of the energy-budget diagnostics (energy_budget_host.cpp) asks of their kernels (energy_budget.hip).  A header of
// its own, like diagnostic.hpp: the other kernel files include neither it nor anything it changes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rscm {

constexpr int kBudgetForcing = 1;      // RSCM_BUDGET_FORCING
constexpr int kBudgetResponse = 2;     // RSCM_BUDGET_RESPONSE
constexpr int kBudgetDeepUptake = 3;   // RSCM_BUDGET_DEEP_UPTAKE
constexpr int kBudgetImbalance = 4;    // RSCM_BUDGET_IMBALANCE
constexpr bool budget_reads_forcing(int quantity) { return quantity == kBudgetForcing || quantity == kBudgetImbalance; }

// d_out[r][i] = scale * q, q the quantity include/rscm_gpu.h states (energy-budget diagnostics) of member i at the source rows
// d_rows[r][i] (Ts) and d_rows[n_rows + r][i] (Td), r < n_rows.  Row r reads the forcing axis at index f0 + r * f_stride; the host has
// proved every such index in [0, n_times), every scenario id in [0, n_scen) and the parameter rows 0 .. 5 + n_comp (and the two noise
// rows of the per-member kind) inside the block.  The forcing fields are read only where budget_reads_forcing(quantity).
struct EnergyBudgetArgs {
    const double* const* d_rows;   // [2][n_rows] device addresses of N doubles each
    const double* d_params;        // [P][N]
    uint64_t uniform_rows;         // param_at
    double* d_out;                 // [n_rows][N]
    int64_t N;
    int32_t n_rows;
    int32_t quantity;              // kBudget*: wave-uniform
    double scale;
    const double* d_forcing;       // [S][T], a mix handle's [S][K][T]
    const int32_t* d_scen;         // [N] or null: every member reads scenario 0
    int32_t n_times;               // T
    int32_t n_comp;                // K of a mix handle, else 0
    int32_t f0, f_stride;
    uint64_t noise_seed;
    double noise_sigma, noise_phi;
    int64_t noise_member0;
    int32_t noise_sigma_row, noise_phi_row;   // the per-member kind's parameter rows
};
// noise_kind: kNoiseKind* of rscm_device.hpp; ignored (as is n_comp) where the quantity reads no forcing
hipError_t launch_energy_budget(const EnergyBudgetArgs& a, int32_t noise_kind, hipStream_t s);

}  // namespace rscm
