// Per-member covariability of two variables -- covariance, correlation, regression slope and the cross-correlation at up to
// kCovMaxLags leads and lags -- for gfx950 (MI355X).
//
// covariability_kernel: one thread per member walks the rows of BOTH variables TWICE in one launch.  Working series (plain,
// difference, midpoint), walk, pass 1 and the residuals a_k (of x) and c_k (of y) are those of series_walk.hpp; the statistic is the
// one include/rscm_gpu.h states under rscm_ens_member_covariability:
//   pass 2  Cxx = a_0 a_0 + ...,  Cyy = c_0 c_0 + ...,  G_0 = a_0 c_0 + ...,
//           G_l = a_0 c_l + a_1 c_{l+1} + ...,  G_{-l} = a_l c_0 + a_{l+1} c_1 + ...,  l = 1 .. n_lags
// The last kCovMaxLags residuals of each series are carried in named registers across batches.  n_lags is a wave-uniform bound
// (scalar branches around the lagged products): the nine instances are the mode pairs.  Traffic is 2 x 2 x 8 B x R x N, that of two
// variability launches.
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"
#include "series_walk.hpp"

namespace rscm {

namespace {

constexpr int kCovThreads = 256;
constexpr int kCovBatch = 4;   // terms of each variable whose loads a thread issues before it uses them: 2 x kCovBatch values in flight

template <int kModeX, int kModeY>
__global__ __launch_bounds__(kCovThreads) void covariability_kernel(const double* const* __restrict__ rows_x, const double* const* __restrict__ rows_y,
                                                                     int32_t n_rows, int32_t n_lags, double stt, int64_t N, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kCovThreads + threadIdx.x;
    if (i >= N) return;
    using S = Series<kModeX, kModeY>;
    const double* const* const rows[2] = {rows_x, rows_y};
    const int32_t n = S::terms(n_rows);
    const double dn = (double)n;
    bool bad = false;
    const Detrend<2> d = detrend_pass<S, kCovBatch>(rows, n, stt, i, bad);

    static_assert(kCovMaxLags == 3, "the carried residuals below are named for three lags");
    double Cxx = -0.0, Cyy = -0.0, G0 = -0.0;
    double Gp1 = -0.0, Gp2 = -0.0, Gp3 = -0.0, Gm1 = -0.0, Gm2 = -0.0, Gm3 = -0.0;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;   // a_{k-1}, a_{k-2}, a_{k-3} and the same of c
    walk_terms<S, kCovBatch, false>(rows, n, i, bad, [&](const double (&u)[2], int32_t k, auto) {
        double r[2];
        residuals<S>(u, (double)k - d.h, d, r);
        const double a = r[0], c = r[1];
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

}  // namespace

hipError_t launch_covariability(const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_x, int32_t mode_y,
                                int32_t n_lags, double stt, int64_t N, double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (n_lags < 0 || n_lags > kCovMaxLags) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + kCovThreads - 1) / kCovThreads));
    return with_mode(mode_x, [&](auto mx) {
        return with_mode(mode_y, [&](auto my) {
            hipLaunchKernelGGL((covariability_kernel<decltype(mx)::value, decltype(my)::value>), grid, dim3(kCovThreads), 0, s, d_rows_x, d_rows_y,
                               n_rows, n_lags, stt, N, d_out);
            return hipGetLastError();
        });
    });
}

}  // namespace rscm
