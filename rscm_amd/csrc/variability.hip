// Per-member variability statistics of a stored variable and the Gaussian likelihood over per-member vectors, for gfx950 (MI355X).
//
// variability_kernel: one thread per member walks the rows TWICE in one launch.  Working series, walk, pass 1 and the residuals are
// those of series_walk.hpp; the statistic is the one include/rscm_gpu.h states under rscm_ens_member_variability:
//   pass 2  C0 = a_0 a_0 + ...,  C1 = a_0 a_1 + a_1 a_2 + ...;  variance = C0 / n,  sd = sqrt(variance),  r1 = C1 / C0
// with the previous a carried in a register.  The second pass re-reads the rows: 2 x 8 B x R x N of traffic in all; a one-pass shifted
// formula would not be the definition that numpy restates bit for bit.  A member with a non-finite value in any row gets NaN in all
// five statistics.
//
// loglik_vectors_kernel: out[i] = (add ? add[i] : 0.0) + sum_j -0.5 ((value_j - v_j[i])^2 / sigma_j^2), the expressions of
// loglik_kernel (ensemble_ops.hip) with the vectors as one more variable group; -inf for a non-finite v_j[i] or add[i].  add may be
// out: a thread reads its own element before it writes it.
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"
#include "series_walk.hpp"

namespace rscm {

namespace {

constexpr int kVarThreads = 256;
constexpr int kVarBatch = 8;   // terms whose loads a thread issues before it uses them (kIndBatch of indicators.hip)

template <int kMode>
__global__ __launch_bounds__(kVarThreads) void variability_kernel(const double* const* __restrict__ rows_x, int32_t n_rows, double stt, int64_t N,
                                                                   double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kVarThreads + threadIdx.x;
    if (i >= N) return;
    using S = Series<kMode>;
    const double* const* const rows[1] = {rows_x};
    const int32_t n = S::terms(n_rows);
    const double dn = (double)n;
    bool bad = false;
    const Detrend<1> d = detrend_pass<S, kVarBatch>(rows, n, stt, i, bad);

    double C0 = -0.0, C1 = -0.0, a_prev = 0.0;
    walk_terms<S, kVarBatch, false>(rows, n, i, bad, [&](const double (&u)[1], int32_t k, auto) {
        double a[1];
        residuals<S>(u, (double)k - d.h, d, a);
        C0 = C0 + a[0] * a[0];
        if (k > 0) C1 = C1 + a_prev * a[0];
        a_prev = a[0];
    });
    const double variance = C0 / dn;
    const double qnan = __builtin_nan("");
    out[i] = bad ? qnan : d.m[0];
    out[N + i] = bad ? qnan : d.b[0];
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
    return with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(variability_kernel<decltype(m)::value>, grid, dim3(kVarThreads), 0, s, d_rows, n_rows, stt, N, d_out);
        return hipGetLastError();
    });
}

hipError_t launch_loglik_vectors(const LoglikVectors& v, int32_t n_vec, const double* d_add, int64_t N, double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const dim3 grid((unsigned)((N + kVarThreads - 1) / kVarThreads));
    hipLaunchKernelGGL(loglik_vectors_kernel, grid, dim3(kVarThreads), 0, s, v, n_vec, d_add, N, d_out);
    return hipGetLastError();
}

}  // namespace rscm
