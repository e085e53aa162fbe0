// What the host side of the diagnostic variables (diagnostic_host.cpp) asks of their kernel (diagnostic.hip).  A header of its own: the
// other kernel files include neither it nor anything it changes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rscm {

constexpr int kDiagMaxTerms = 4;   // RSCM_DIAG_MAX_TERMS
constexpr int kDiagTile = 32;      // rows a block walks (grid y); a thread forms its weights once per tile
constexpr int kDiagBatch = 4;      // rows whose K loads a thread issues before it uses them

// d_out[r][i] = the combination include/rscm_gpu.h states (diagnostic variables) of the source rows d_rows[k * n_rows + r][i],
// k < n_terms, r < n_rows, with the weight scale[k] * d_params[param_row[k] * N + i] (param_row[k] >= 0) or scale[k] (-1)
struct DiagnosticArgs {
    const double* const* d_rows;   // [n_terms][n_rows] device addresses of N doubles each
    const double* d_params;        // [P][N]
    double* d_out;                 // [n_rows][N]
    int64_t N;
    int32_t n_rows;
    int32_t param_row[kDiagMaxTerms];
    double scale[kDiagMaxTerms];
};
hipError_t launch_diagnostic(const DiagnosticArgs& a, int32_t n_terms, hipStream_t s);

}  // namespace rscm
