// Per-member covariability of two variables -- covariance, correlation, regression slope and the cross-correlation at up to
// kCovMaxLags leads and lags -- for gfx950 (MI355X).
//
// covariability_kernel: one thread per member walks TWO device arrays of row pointers the host resolves (as variability_kernel,
// variability.hip: lanes of a wave read consecutive members of one row, so every load is coalesced) TWICE in one launch.  The statistic
// is the one include/rscm_gpu.h states under rscm_ens_member_covariability; per variable the working series is
//   plain       u_k = x_k                      (neither mode is RSCM_VAR_DIFFERENCE), n = R
//   difference  u_k = x_{k+1} - x_k            (the variable's own mode is RSCM_VAR_DIFFERENCE), n = R - 1
//   midpoint    u_k = (x_k + x_{k+1}) * 0.5    (only the OTHER variable's mode is RSCM_VAR_DIFFERENCE), n = R - 1
// and tau_k, S, m, Q, b and the residuals are variability_kernel's, operation for operation, under the variable's own mode:
//   pass 1  Sx, Sy, with RSCM_VAR_LINEAR Qx, Qy, and the finite check on both variables
//   pass 2  a_k, c_k re-formed;  Cxx = a_0 a_0 + ...,  Cyy = c_0 c_0 + ...,  G_0 = a_0 c_0 + ...,
//           G_l = a_0 c_l + a_1 c_{l+1} + ...,  G_{-l} = a_l c_0 + a_{l+1} c_1 + ...,  l = 1 .. n_lags
// Every operation is one f64 operation rounded on its own (-ffp-contract=off: no FMA), the sums run left to right and start at -0.0,
// the additive identity.  Loads are issued kCovBatch rows of BOTH variables at a time; the previous raw values (difference, midpoint)
// and the last kCovMaxLags residuals of each series are carried in named registers across batches.  No LDS, no per-member array, no
// scratch.  n_lags is a wave-uniform bound (scalar branches around the lagged products): the nine instances are the mode pairs.
// Traffic is 2 x 2 x 8 B x R x N, that of two variability launches.
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"

namespace rscm {

namespace {

constexpr int kCovThreads = 256;
constexpr int kCovBatch = 4;   // rows of each variable whose loads a thread issues before it uses them: 2 x kCovBatch values in flight

constexpr int kCovPlain = 0, kCovDifference = 1, kCovMidpoint = 2;
constexpr int cov_series(int mode, int other) { return mode == kVarDifference ? kCovDifference : other == kVarDifference ? kCovMidpoint : kCovPlain; }

template <int kSeries>
__device__ __forceinline__ double cov_term(double prev, double cur)
{
    if constexpr (kSeries == kCovDifference)
        return cur - prev;
    else
        return (prev + cur) * 0.5;
}

// f(u_k, v_k, k) for k = 0 .. n - 1 in order, from member i's values in the rows of both variables, loaded kCovBatch rows at a time
template <int kSx, int kSy, bool kCheck, class F>
__device__ __forceinline__ void walk_pair(const double* const* __restrict__ rows_x, const double* const* __restrict__ rows_y, int32_t n_rows,
                                          int64_t i, bool& bad, F&& f)
{
    static_assert((kSx == kCovPlain) == (kSy == kCovPlain), "both series span two rows per term or neither does");
    [[maybe_unused]] double x_prev = 0.0, y_prev = 0.0;
    auto step = [&](double x, double y, int32_t r) {
        if constexpr (kCheck) bad = bad || !__builtin_isfinite(x) || !__builtin_isfinite(y);
        if constexpr (kSx != kCovPlain) {
            if (r > 0) f(cov_term<kSx>(x_prev, x), cov_term<kSy>(y_prev, y), r - 1);
            x_prev = x;
            y_prev = y;
        } else {
            f(x, y, r);
        }
    };
    int32_t r = 0;
    for (; r + kCovBatch <= n_rows; r += kCovBatch) {
        double x[kCovBatch], y[kCovBatch];
#pragma unroll
        for (int j = 0; j < kCovBatch; ++j) x[j] = rows_x[r + j][i];
#pragma unroll
        for (int j = 0; j < kCovBatch; ++j) y[j] = rows_y[r + j][i];
#pragma unroll
        for (int j = 0; j < kCovBatch; ++j) step(x[j], y[j], r + j);
    }
    for (; r < n_rows; ++r) step(rows_x[r][i], rows_y[r][i], r);
}

template <int kModeX, int kModeY>
__global__ __launch_bounds__(kCovThreads) void covariability_kernel(const double* const* __restrict__ rows_x, const double* const* __restrict__ rows_y,
                                                                     int32_t n_rows, int32_t n_lags, double stt, int64_t N, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kCovThreads + threadIdx.x;
    if (i >= N) return;
    constexpr int kSx = cov_series(kModeX, kModeY), kSy = cov_series(kModeY, kModeX);
    const int32_t n = kSx != kCovPlain ? n_rows - 1 : n_rows;
    const double dn = (double)n, h = (double)(n - 1) * 0.5;
    bool bad = false;

    double Sx = -0.0, Sy = -0.0;
    [[maybe_unused]] double Qx = -0.0, Qy = -0.0;
    walk_pair<kSx, kSy, true>(rows_x, rows_y, n_rows, i, bad, [&](double u, double v, int32_t k) {
        Sx = Sx + u;
        Sy = Sy + v;
        [[maybe_unused]] const double tau = (double)k - h;
        if constexpr (kModeX == kVarLinear) Qx = Qx + tau * u;
        if constexpr (kModeY == kVarLinear) Qy = Qy + tau * v;
    });
    const double mx = Sx / dn, my = Sy / dn;
    [[maybe_unused]] double bx = 0.0, by = 0.0;
    if constexpr (kModeX == kVarLinear) bx = Qx / stt;
    if constexpr (kModeY == kVarLinear) by = Qy / stt;

    static_assert(kCovMaxLags == 3, "the carried residuals below are named for three lags");
    double Cxx = -0.0, Cyy = -0.0, G0 = -0.0;
    double Gp1 = -0.0, Gp2 = -0.0, Gp3 = -0.0, Gm1 = -0.0, Gm2 = -0.0, Gm3 = -0.0;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;   // a_{k-1}, a_{k-2}, a_{k-3} and the same of c
    walk_pair<kSx, kSy, false>(rows_x, rows_y, n_rows, i, bad, [&](double u, double v, int32_t k) {
        double a = u - mx, c = v - my;
        [[maybe_unused]] const double tau = (double)k - h;
        if constexpr (kModeX == kVarLinear) a = a - bx * tau;
        if constexpr (kModeY == kVarLinear) c = c - by * tau;
        Cxx = Cxx + a * a;
        Cyy = Cyy + c * c;
        G0 = G0 + a * c;
        if (n_lags >= 1 && k >= 1) {
            Gp1 = Gp1 + a1 * c;
            Gm1 = Gm1 + a * c1;
        }
        if (n_lags >= 2 && k >= 2) {
            Gp2 = Gp2 + a2 * c;
            Gm2 = Gm2 + a * c2;
        }
        if (n_lags >= 3 && k >= 3) {
            Gp3 = Gp3 + a3 * c;
            Gm3 = Gm3 + a * c3;
        }
        a3 = a2;
        a2 = a1;
        a1 = a;
        c3 = c2;
        c2 = c1;
        c1 = c;
    });
    const double D = sqrt(Cxx) * sqrt(Cyy);
    const double qnan = __builtin_nan("");
    out[i] = bad ? qnan : Cxx / dn;
    out[N + i] = bad ? qnan : Cyy / dn;
    out[2 * N + i] = bad ? qnan : G0 / dn;
    out[3 * N + i] = bad ? qnan : G0 / D;
    out[4 * N + i] = bad ? qnan : G0 / Cxx;
    if (n_lags >= 1) {
        out[5 * N + i] = bad ? qnan : Gp1 / D;
        out[6 * N + i] = bad ? qnan : Gm1 / D;
    }
    if (n_lags >= 2) {
        out[7 * N + i] = bad ? qnan : Gp2 / D;
        out[8 * N + i] = bad ? qnan : Gm2 / D;
    }
    if (n_lags >= 3) {
        out[9 * N + i] = bad ? qnan : Gp3 / D;
        out[10 * N + i] = bad ? qnan : Gm3 / D;
    }
}

template <int kModeX>
hipError_t launch_mode_y(const dim3 grid, const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_y, int32_t n_lags,
                         double stt, int64_t N, double* d_out, hipStream_t s)
{
    if (mode_y == kVarMean)
        hipLaunchKernelGGL((covariability_kernel<kModeX, kVarMean>), grid, dim3(kCovThreads), 0, s, d_rows_x, d_rows_y, n_rows, n_lags, stt, N, d_out);
    else if (mode_y == kVarLinear)
        hipLaunchKernelGGL((covariability_kernel<kModeX, kVarLinear>), grid, dim3(kCovThreads), 0, s, d_rows_x, d_rows_y, n_rows, n_lags, stt, N, d_out);
    else if (mode_y == kVarDifference)
        hipLaunchKernelGGL((covariability_kernel<kModeX, kVarDifference>), grid, dim3(kCovThreads), 0, s, d_rows_x, d_rows_y, n_rows, n_lags, stt, N,
                           d_out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_covariability(const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_x, int32_t mode_y,
                                int32_t n_lags, double stt, int64_t N, double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (n_lags < 0 || n_lags > kCovMaxLags) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + kCovThreads - 1) / kCovThreads));
    if (mode_x == kVarMean) return launch_mode_y<kVarMean>(grid, d_rows_x, d_rows_y, n_rows, mode_y, n_lags, stt, N, d_out, s);
    if (mode_x == kVarLinear) return launch_mode_y<kVarLinear>(grid, d_rows_x, d_rows_y, n_rows, mode_y, n_lags, stt, N, d_out, s);
    if (mode_x == kVarDifference) return launch_mode_y<kVarDifference>(grid, d_rows_x, d_rows_y, n_rows, mode_y, n_lags, stt, N, d_out, s);
    return hipErrorInvalidValue;
}

}  // namespace rscm
