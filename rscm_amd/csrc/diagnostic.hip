// Diagnostic variables: per-member linear combinations of a handle's stored rows, for gfx950 (MI355X).
//
// diagnostic_kernel<K>: one thread per member (x, 256 threads as variability.hip and indicators.hip) and one tile of kDiagTile rows per
// block (y).  The definition is the one include/rscm_gpu.h states under "diagnostic variables":
//   w_k = scale_k * p[row_k][i]  (row_k >= 0)  or  scale_k  (row_k == -1),   formed once per thread, multiplied even by 1.0
//   y   = w_0 * x_0;  y = y + w_k * x_k  for k = 1 .. K - 1 in order
// Every product and sum is one f64 operation rounded on its own (-ffp-contract=off: no FMA).  K is a template parameter, so the
// combination is unrolled and the row loop has no per-term branch.  The source rows come from a device array of row pointers [K][R]
// (full storage, the window or the output store, resolved by the host); lanes of a wave read consecutive members of one row, 8 B per
// lane, and write consecutive members of the contiguous destination.  The K loads of kDiagBatch rows are issued before the first is
// used.  No LDS, no scratch.  Traffic: (K + 1) x 8 x R x N bytes, plus 8 K N of weights per tile of rows.
#include <hip/hip_runtime.h>

#include "diagnostic.hpp"

namespace rscm {

namespace {

constexpr int kDiagThreads = 256;

template <int K>
__device__ __forceinline__ double combine(const double (&w)[K], const double (&x)[K])
{
    double y = w[0] * x[0];
#pragma unroll
    for (int k = 1; k < K; ++k) y = y + w[k] * x[k];
    return y;
}

template <int K>
__global__ __launch_bounds__(kDiagThreads) void diagnostic_kernel(DiagnosticArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kDiagThreads + threadIdx.x;
    if (i >= a.N) return;
    const int32_t r_end = min((int32_t)(blockIdx.y + 1) * kDiagTile, a.n_rows);
    int32_t r = (int32_t)blockIdx.y * kDiagTile;

    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double p = a.param_row[k] >= 0 ? a.d_params[(int64_t)a.param_row[k] * a.N + i] : 1.0;
        w[k] = a.param_row[k] >= 0 ? a.scale[k] * p : a.scale[k];
    }

    const double* const* __restrict__ rows = a.d_rows;
    double* __restrict__ out = a.d_out;
    for (; r + kDiagBatch <= r_end; r += kDiagBatch) {
        double x[kDiagBatch][K];
#pragma unroll
        for (int j = 0; j < kDiagBatch; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k) x[j][k] = rows[(int64_t)k * a.n_rows + r + j][i];
#pragma unroll
        for (int j = 0; j < kDiagBatch; ++j) out[(int64_t)(r + j) * a.N + i] = combine<K>(w, x[j]);
    }
    for (; r < r_end; ++r) {
        double x[K];
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = rows[(int64_t)k * a.n_rows + r][i];
        out[(int64_t)r * a.N + i] = combine<K>(w, x);
    }
}

}  // namespace

hipError_t launch_diagnostic(const DiagnosticArgs& a, int32_t n_terms, hipStream_t s)
{
    if (a.N <= 0 || a.n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.N + kDiagThreads - 1) / kDiagThreads), (unsigned)((a.n_rows + kDiagTile - 1) / kDiagTile));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    switch (n_terms) {
        case 1: hipLaunchKernelGGL(diagnostic_kernel<1>, grid, dim3(kDiagThreads), 0, s, a); break;
        case 2: hipLaunchKernelGGL(diagnostic_kernel<2>, grid, dim3(kDiagThreads), 0, s, a); break;
        case 3: hipLaunchKernelGGL(diagnostic_kernel<3>, grid, dim3(kDiagThreads), 0, s, a); break;
        case 4: hipLaunchKernelGGL(diagnostic_kernel<4>, grid, dim3(kDiagThreads), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rscm
