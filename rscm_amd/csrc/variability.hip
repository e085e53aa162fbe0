// Per-member variability statistics of a stored variable and the Gaussian likelihood over per-member vectors, for gfx950 (MI355X).
//
// variability_kernel: one thread per member walks the device array of row pointers the host resolves (as indicators_kernel,
// indicators.hip: full storage, the window, the output store; lanes of a wave read consecutive members of one row, so every load
// is coalesced) TWICE in one launch.  The statistic is the one include/rscm_gpu.h states under rscm_ens_member_variability:
// working series u_k = x_k (RSCM_VAR_MEAN, RSCM_VAR_LINEAR) or x_{k+1} - x_k (RSCM_VAR_DIFFERENCE), n terms;
//   pass 1  S = u_0 + u_1 + ...,  and with RSCM_VAR_LINEAR  Q = tau_0 u_0 + tau_1 u_1 + ...,  tau_k = (double)k - (n - 1) / 2
//           m = S / n,  b = Q / Stt (else +0.0)
//   pass 2  a_k = u_k - m  (RSCM_VAR_LINEAR: (u_k - m) - b tau_k),  C0 = a_0 a_0 + ...,  C1 = a_0 a_1 + a_1 a_2 + ...
//           variance = C0 / n,  sd = sqrt(variance),  r1 = C1 / C0
// Every operation is one f64 operation rounded on its own (-ffp-contract=off: no FMA), the sums run left to right; they start at
// -0.0, the additive identity, which is "starting from the first term" bit for bit.  Loads are issued kVarBatch rows at a time; the
// previous x (RSCM_VAR_DIFFERENCE) and the previous a (C1) are carried in registers across batches.  No per-member array, no
// scratch.  The second pass re-reads the rows: 2 x 8 B x R x N of traffic in all; a one-pass shifted formula would not be the
// definition that numpy restates bit for bit.  A member with a non-finite value in any row gets NaN in all five statistics.
//
// loglik_vectors_kernel: out[i] = (add ? add[i] : 0.0) + sum_j -0.5 ((value_j - v_j[i])^2 / sigma_j^2), the expressions of
// loglik_kernel (ensemble_ops.hip) with the vectors as one more variable group; -inf for a non-finite v_j[i] or add[i].  add may be
// out: a thread reads its own element before it writes it.
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"

namespace rscm {

namespace {

constexpr int kVarThreads = 256;
constexpr int kVarBatch = 8;   // rows whose loads a thread issues before it uses them (kIndBatch of indicators.hip)

// f(u_k, k) for k = 0 .. n - 1 in order, from member i's values in the rows; the rows are loaded kVarBatch at a time
template <int kMode, bool kCheck, class F>
__device__ __forceinline__ void walk_series(const double* const* __restrict__ rows, int32_t n_rows, int64_t i, bool& bad, F&& f)
{
    [[maybe_unused]] double x_prev = 0.0;
    auto step = [&](double x, int32_t r) {
        if constexpr (kCheck) bad = bad || !__builtin_isfinite(x);
        if constexpr (kMode == kVarDifference) {
            if (r > 0) f(x - x_prev, r - 1);
            x_prev = x;
        } else {
            f(x, r);
        }
    };
    int32_t r = 0;
    for (; r + kVarBatch <= n_rows; r += kVarBatch) {
        double x[kVarBatch];
#pragma unroll
        for (int j = 0; j < kVarBatch; ++j) x[j] = rows[r + j][i];
#pragma unroll
        for (int j = 0; j < kVarBatch; ++j) step(x[j], r + j);
    }
    for (; r < n_rows; ++r) step(rows[r][i], r);
}

template <int kMode>
__global__ __launch_bounds__(kVarThreads) void variability_kernel(const double* const* __restrict__ rows, int32_t n_rows, double stt, int64_t N,
                                                                   double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kVarThreads + threadIdx.x;
    if (i >= N) return;
    const int32_t n = kMode == kVarDifference ? n_rows - 1 : n_rows;
    const double dn = (double)n, h = (double)(n - 1) * 0.5;
    bool bad = false;

    double S = -0.0;
    [[maybe_unused]] double Q = -0.0;
    walk_series<kMode, true>(rows, n_rows, i, bad, [&](double u, int32_t k) {
        S = S + u;
        if constexpr (kMode == kVarLinear) {
            const double tau = (double)k - h;
            Q = Q + tau * u;
        }
    });
    const double m = S / dn;
    double b = 0.0;
    if constexpr (kMode == kVarLinear) b = Q / stt;

    double C0 = -0.0, C1 = -0.0, a_prev = 0.0;
    walk_series<kMode, false>(rows, n_rows, i, bad, [&](double u, int32_t k) {
        double a = u - m;
        if constexpr (kMode == kVarLinear) {
            const double tau = (double)k - h;
            a = a - b * tau;
        }
        C0 = C0 + a * a;
        if (k > 0) C1 = C1 + a_prev * a;
        a_prev = a;
    });
    const double variance = C0 / dn;
    const double qnan = __builtin_nan("");
    out[i] = bad ? qnan : m;
    out[N + i] = bad ? qnan : b;
    out[2 * N + i] = bad ? qnan : variance;
    out[3 * N + i] = bad ? qnan : sqrt(variance);
    out[4 * N + i] = bad ? qnan : C1 / C0;
}

__global__ __launch_bounds__(kVarThreads) void loglik_vectors_kernel(LoglikVectors v, int32_t n_vec, const double* add, int64_t N, double* out)
{
    const int64_t i = (int64_t)blockIdx.x * kVarThreads + threadIdx.x;
    if (i >= N) return;
    const double base = add ? add[i] : 0.0;
    bool bad = !__builtin_isfinite(base);
    double partial = 0.0;
    for (int32_t j = 0; j < n_vec; ++j) {
        const double m = v.vec[j][i];
        bad = bad || !__builtin_isfinite(m);
        const double sigma = v.sigma[j];
        const double residual = v.value[j] - m;
        const double chi = (residual * residual) / (sigma * sigma);
        partial += -0.5 * chi;
    }
    out[i] = bad ? -__builtin_inf() : base + partial;
}

}  // namespace

hipError_t launch_variability(const double* const* d_rows, int32_t n_rows, int32_t mode, double stt, int64_t N, double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const dim3 grid((unsigned)((N + kVarThreads - 1) / kVarThreads));
    if (mode == kVarMean)
        hipLaunchKernelGGL(variability_kernel<kVarMean>, grid, dim3(kVarThreads), 0, s, d_rows, n_rows, stt, N, d_out);
    else if (mode == kVarLinear)
        hipLaunchKernelGGL(variability_kernel<kVarLinear>, grid, dim3(kVarThreads), 0, s, d_rows, n_rows, stt, N, d_out);
    else if (mode == kVarDifference)
        hipLaunchKernelGGL(variability_kernel<kVarDifference>, grid, dim3(kVarThreads), 0, s, d_rows, n_rows, stt, N, d_out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_loglik_vectors(const LoglikVectors& v, int32_t n_vec, const double* d_add, int64_t N, double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const dim3 grid((unsigned)((N + kVarThreads - 1) / kVarThreads));
    hipLaunchKernelGGL(loglik_vectors_kernel, grid, dim3(kVarThreads), 0, s, v, n_vec, d_add, N, d_out);
    return hipGetLastError();
}

}  // namespace rscm
