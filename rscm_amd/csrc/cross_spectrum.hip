// Per-member co-spectra, coherence and gain of two variables in frequency bands, for gfx950 (MI355X).
//
// cross_spectrum_kernel: one thread per member walks TWO device arrays of row pointers (as covariability_kernel, covariability.hip:
// lanes of a wave read consecutive members of one row, so every load is coalesced).  The statistic is the one include/rscm_gpu.h
// states under rscm_ens_member_cross_spectrum; rows, working series (plain, difference, midpoint), S, m, Q, b and the residuals a_k
// (of x) and c_k (of y) are rscm_ens_member_covariability's, operation for operation.  All passes run in one launch:
//   pass 1          Sx, Sy, with RSCM_VAR_LINEAR Qx, Qy, and the finite check on both variables (covariability's pass 1)
//   one pass per    tile of kXSpecF frequencies j0 .. j0 + kXSpecF - 1: the lane keeps s1, s2 (of a) and t1, t2 (of c) of Goertzel's
//   tile            recurrence for every frequency of the tile in registers (8 kXSpecF VGPRs), re-forms a_k and c_k from the rows --
//                   one expression each, residuals(), so their bits cannot depend on the tile -- and advances all 2 kXSpecF
//                   recurrences with them:
//                       s0 = (a_k + c2_j * s1) - s2;  s2 = s1;  s1 = s0        t0 = (c_k + c2_j * t1) - t2;  t2 = t1;  t1 = t0
//                   (the register sets exchange their names at every term, not their values: walk_pair_terms hands the parity on, as
//                   walk_terms of spectrum.hip does).  The first tile also forms Cxx = a_0 a_0 + ... and Cyy = c_0 c_0 + ...
//   after a tile    in ascending j, with h_j = c2_j * 0.5 and g_j the double nearest sin(2 pi j / n):
//                       Ixx = ((s1 s1 + s2 s2) - (c2_j s1) s2) / n           Iyy the same on t
//                       K   = ((s1 t1 + s2 t2) - h_j (s1 t2 + s2 t1)) / n    Q = (g_j (s2 t1 - s1 t2)) / n
//                   added to four running band sums, which are carried in registers across tiles; a band that ends at j is divided
//                   by its count and its coherence, gain and quadrature gain are stored
// Every operation is one f64 operation rounded on its own (-ffp-contract=off: no FMA); sums start at -0.0, the additive identity,
// which is "starting from the first term" bit for bit.  c2_j and g_j come from the tables the host uploads per call
// (rscm_gpu_spectrum_coefficients, rscm_gpu_spectrum_sines), each padded by kSpectrumTablePad zeros and followed in the same
// allocation by the band edges; all are read at wave-uniform addresses, so they travel as scalar loads.  Only the frequencies inside
// [edges[0], edges[n_bands]) are computed; the last tile may be partial, and its idle recurrences run on the padding.  Loads are
// issued kXSpecBatch rows of BOTH variables at a time; the previous raw value of each variable (difference, midpoint) is carried in a
// named register.  No per-member array indexed at run time, no scratch, no LDS.  Row traffic: 2 x 8 B x R x N x (1 + tiles).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rscm_device.hpp"

namespace rscm {

namespace {

constexpr int kXSpecThreads = 256;
constexpr int kXSpecBatch = 4;   // rows of each variable whose loads a thread issues before it uses them: 2 x kXSpecBatch values in flight
// Frequencies per tile.  The listing (make asm-cross-spectrum) decides: 8 kXSpecF VGPRs of recurrence state, 4 kXSpecBatch of rows in
// flight and about forty more.  8 is the widest tile that fits 128 VGPRs -- four waves per SIMD, which the kernel asks the compiler
// for -- without scratch (122-128 VGPRs over the nine instances); 10 spills in three instances, 12 in all nine, and so does a batch
// of 8 rows at a tile of 8.  profiles/cross_spectrum_bench.txt has the listing's figures.
constexpr int kXSpecF = 8;
static_assert(kXSpecF - 1 <= kSpectrumTablePad, "a tile reads up to kXSpecF - 1 table entries past the last frequency");

constexpr int kXPlain = 0, kXDifference = 1, kXMidpoint = 2;
constexpr int xspec_series(int mode, int other) { return mode == kVarDifference ? kXDifference : other == kVarDifference ? kXMidpoint : kXPlain; }

template <int kSeries>
__device__ __forceinline__ double xspec_term(double prev, double cur)
{
    if constexpr (kSeries == kXDifference)
        return cur - prev;
    else
        return (prev + cur) * 0.5;
}

// f(u_k, v_k, k, parity of k) for k = 0 .. n - 1 in order, from member i's values in the rows of both variables.  With a differenced
// variable both series span two rows per term: row 0 of each is loaded ahead into x_prev, y_prev, so that every batch holds
// kXSpecBatch terms in every mode pair.  The parity travels as a type: the recurrences write even terms into one register set and odd
// terms into the other, so no value moves between terms.  After the batches the rest goes in pairs, then a last single term.
using Even = std::integral_constant<bool, false>;
using Odd = std::integral_constant<bool, true>;
template <int kSx, int kSy, bool kCheck, class F>
__device__ __forceinline__ void walk_pair_terms(const double* const* __restrict__ rows_x, const double* const* __restrict__ rows_y, int32_t n,
                                                int64_t i, bool& bad, F&& f)
{
    static_assert((kSx == kXPlain) == (kSy == kXPlain), "both series span two rows per term or neither does");
    static_assert(kXSpecBatch % 2 == 0, "a batch keeps the parity");
    constexpr int kOff = kSx != kXPlain ? 1 : 0;   // the (later) row of term k is k + kOff
    [[maybe_unused]] double x_prev = 0.0, y_prev = 0.0;
    auto term_x = [&](double x) {
        if constexpr (kCheck) bad = bad || !__builtin_isfinite(x);
        if constexpr (kSx != kXPlain) {
            const double u = xspec_term<kSx>(x_prev, x);
            x_prev = x;
            return u;
        } else {
            return x;
        }
    };
    auto term_y = [&](double y) {
        if constexpr (kCheck) bad = bad || !__builtin_isfinite(y);
        if constexpr (kSy != kXPlain) {
            const double v = xspec_term<kSy>(y_prev, y);
            y_prev = y;
            return v;
        } else {
            return y;
        }
    };
    if constexpr (kSx != kXPlain) {
        x_prev = rows_x[0][i];
        y_prev = rows_y[0][i];
        if constexpr (kCheck) bad = bad || !__builtin_isfinite(x_prev) || !__builtin_isfinite(y_prev);
    }
    int32_t k = 0;
    for (; k + kXSpecBatch <= n; k += kXSpecBatch) {
        double x[kXSpecBatch], y[kXSpecBatch];
#pragma unroll
        for (int j = 0; j < kXSpecBatch; ++j) x[j] = rows_x[kOff + k + j][i];
#pragma unroll
        for (int j = 0; j < kXSpecBatch; ++j) y[j] = rows_y[kOff + k + j][i];
#pragma unroll
        for (int j = 0; j < kXSpecBatch; j += 2) {
            f(term_x(x[j]), term_y(y[j]), k + j, Even{});
            f(term_x(x[j + 1]), term_y(y[j + 1]), k + j + 1, Odd{});
        }
    }
    for (; k + 2 <= n; k += 2) {
        const double x0 = rows_x[kOff + k][i], x1 = rows_x[kOff + k + 1][i];
        const double y0 = rows_y[kOff + k][i], y1 = rows_y[kOff + k + 1][i];
        f(term_x(x0), term_y(y0), k, Even{});
        f(term_x(x1), term_y(y1), k + 1, Odd{});
    }
    if (k < n) {
        const double x0 = rows_x[kOff + k][i], y0 = rows_y[kOff + k][i];
        f(term_x(x0), term_y(y0), k, Even{});
    }
}

// a_k of u_k and c_k of v_k: the one expression each that every pass re-forms the residuals with.  tau_k = (double)k - h is carried
// as tau_{k-1} + 1.0: with n <= 4096 both are exact (multiples of 0.5 below 2^12), so these are the bits of the definition's.
template <int kModeX, int kModeY>
__device__ __forceinline__ void residuals(double u, double v, double& tau, double mx, double bx, double my, double by, double& a, double& c)
{
    a = u - mx;
    c = v - my;
    if constexpr (kModeX == kVarLinear) a = a - bx * tau;
    if constexpr (kModeY == kVarLinear) c = c - by * tau;
    if constexpr (kModeX == kVarLinear || kModeY == kVarLinear) tau = tau + 1.0;
}

struct Detrend {
    double mx, bx, my, by, h;
};

// One pass over the rows of both variables for the frequencies j0 .. j0 + kXSpecF - 1 (those past the last one idle on the table's
// padding); kFirst: Cxx, Cyy too.  On return s1, t1 hold the recurrences' last values and s2, t2 the ones before them.
template <int kModeX, int kModeY, bool kFirst>
__device__ __forceinline__ void tile_pass(const double* const* __restrict__ rows_x, const double* const* __restrict__ rows_y, int32_t n, int64_t i,
                                          const Detrend& d, const double* __restrict__ c2, int32_t j0, double (&cf)[kXSpecF],
                                          double (&s1)[kXSpecF], double (&s2)[kXSpecF], double (&t1)[kXSpecF], double (&t2)[kXSpecF],
                                          double& Cxx, double& Cyy)
{
    constexpr int kSx = xspec_series(kModeX, kModeY), kSy = xspec_series(kModeY, kModeX);
#pragma unroll
    for (int f = 0; f < kXSpecF; ++f) {
        cf[f] = c2[j0 + f - 1];   // wave-uniform: scalar loads; past the last frequency the table's padding (zeros)
        s1[f] = 0.0;
        s2[f] = 0.0;
        t1[f] = 0.0;
        t2[f] = 0.0;
    }
    bool unused = false;
    [[maybe_unused]] double tau = -d.h;
    walk_pair_terms<kSx, kSy, false>(rows_x, rows_y, n, i, unused, [&](double u, double v, int32_t, auto odd) {
        double a, c;
        residuals<kModeX, kModeY>(u, v, tau, d.mx, d.bx, d.my, d.by, a, c);
        if constexpr (kFirst) {
            Cxx = Cxx + a * a;
            Cyy = Cyy + c * c;
        }
#pragma unroll
        for (int f = 0; f < kXSpecF; ++f) {
            // s0 = (a + c2 s1) - s2; s2 = s1; s1 = s0 -- with the names of s1 and s2 exchanged at every odd term instead of their values
            if constexpr (!decltype(odd)::value) {
                s2[f] = (a + cf[f] * s1[f]) - s2[f];
                t2[f] = (c + cf[f] * t1[f]) - t2[f];
            } else {
                s1[f] = (a + cf[f] * s2[f]) - s1[f];
                t1[f] = (c + cf[f] * t2[f]) - t1[f];
            }
        }
    });
    if (n & 1) {   // the last term was an even one: its values sit in s2, t2
#pragma unroll
        for (int f = 0; f < kXSpecF; ++f) {
            const double s = s1[f], t = t1[f];
            s1[f] = s2[f];
            s2[f] = s;
            t1[f] = t2[f];
            t2[f] = t;
        }
    }
}

// c2, sn: [J] doubles each and kSpectrumTablePad more that may be read; edges: int32 [n_bands + 1], 1 <= edges[0] < ... <
// edges[n_bands] <= J + 1 and n_bands <= kMaxCrossSpectrumBands (checked by the host)
// (amdgpu_waves_per_eu(4): as spectrum_kernel, so that the compiler does not spend the room below its next occupancy step)
template <int kModeX, int kModeY>
__global__ __launch_bounds__(kXSpecThreads) __attribute__((amdgpu_waves_per_eu(4))) void cross_spectrum_kernel(
    const double* const* __restrict__ rows_x, const double* const* __restrict__ rows_y, int32_t n_rows, double stt, const double* __restrict__ c2,
    const double* __restrict__ sn, const int32_t* __restrict__ edges, int32_t n_bands, int64_t N, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kXSpecThreads + threadIdx.x;
    if (i >= N) return;
    constexpr int kSx = xspec_series(kModeX, kModeY), kSy = xspec_series(kModeY, kModeX);
    const int32_t n = kSx != kXPlain ? n_rows - 1 : n_rows;
    const double dn = (double)n;
    Detrend d{0.0, 0.0, 0.0, 0.0, (double)(n - 1) * 0.5};
    bool bad = false;

    double Sx = -0.0, Sy = -0.0;
    [[maybe_unused]] double Qx = -0.0, Qy = -0.0;
    walk_pair_terms<kSx, kSy, true>(rows_x, rows_y, n, i, bad, [&](double u, double v, int32_t k, auto) {
        Sx = Sx + u;
        Sy = Sy + v;
        [[maybe_unused]] const double tau = (double)k - d.h;
        if constexpr (kModeX == kVarLinear) Qx = Qx + tau * u;
        if constexpr (kModeY == kVarLinear) Qy = Qy + tau * v;
    });
    d.mx = Sx / dn;
    d.my = Sy / dn;
    if constexpr (kModeX == kVarLinear) d.bx = Qx / stt;
    if constexpr (kModeY == kVarLinear) d.by = Qy / stt;

    const double qnan = __builtin_nan("");
    const int32_t j_begin = edges[0], j_end = edges[n_bands];
    int32_t band = 0, band_begin = j_begin, band_end = edges[1];
    double Cxx = -0.0, Cyy = -0.0;
    double Axx = -0.0, Ayy = -0.0, AK = -0.0, AQ = -0.0;   // the running band sums of Ixx, Iyy, K, Q
    for (int32_t j0 = j_begin; j0 < j_end; j0 += kXSpecF) {
        double cf[kXSpecF], s1[kXSpecF], s2[kXSpecF], t1[kXSpecF], t2[kXSpecF];
        if (j0 == j_begin)
            tile_pass<kModeX, kModeY, true>(rows_x, rows_y, n, i, d, c2, j0, cf, s1, s2, t1, t2, Cxx, Cyy);
        else
            tile_pass<kModeX, kModeY, false>(rows_x, rows_y, n, i, d, c2, j0, cf, s1, s2, t1, t2, Cxx, Cyy);
#pragma unroll
        for (int f = 0; f < kXSpecF; ++f) {
            const int32_t j = j0 + f;
            if (f < j_end - j0) {
                const double g = sn[j - 1], hc = cf[f] * 0.5;   // wave-uniform: g arrives as a scalar load; the halving is exact
                const double Ixx = ((s1[f] * s1[f] + s2[f] * s2[f]) - (cf[f] * s1[f]) * s2[f]) / dn;
                const double Iyy = ((t1[f] * t1[f] + t2[f] * t2[f]) - (cf[f] * t1[f]) * t2[f]) / dn;
                const double K = ((s1[f] * t1[f] + s2[f] * t2[f]) - hc * (s1[f] * t2[f] + s2[f] * t1[f])) / dn;
                const double Q = (g * (s2[f] * t1[f] - s1[f] * t2[f])) / dn;
                Axx = Axx + Ixx;
                Ayy = Ayy + Iyy;
                AK = AK + K;
                AQ = AQ + Q;
                if (j + 1 == band_end) {       // wave-uniform; band < n_bands <= 3 here, so the stores stay inside [3 + kMaxThresholds][N]
                    const double mb = (double)(band_end - band_begin);
                    const double Pxx = Axx / mb, Pyy = Ayy / mb, Kb = AK / mb, Qb = AQ / mb;
                    const double D = sqrt(Pxx) * sqrt(Pyy);
                    const double kc = Kb / D, qc = Qb / D;
                    double* o = out + (int64_t)(2 + 3 * band) * N + i;
                    o[0] = bad ? qnan : kc * kc + qc * qc;
                    o[N] = bad ? qnan : Kb / Pxx;
                    o[2 * N] = bad ? qnan : Qb / Pxx;
                    Axx = -0.0;
                    Ayy = -0.0;
                    AK = -0.0;
                    AQ = -0.0;
                    ++band;
                    band_begin = band_end;
                    if (band < n_bands) band_end = edges[band + 1];
                }
            }
        }
    }
    out[i] = bad ? qnan : Cxx / dn;
    out[N + i] = bad ? qnan : Cyy / dn;
}

template <int kModeX>
hipError_t launch_mode_y(const dim3 grid, const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_y, double stt,
                         const double* d_c2, const double* d_sin, const int32_t* d_edges, int32_t n_bands, int64_t N, double* d_out, hipStream_t s)
{
    if (mode_y == kVarMean)
        hipLaunchKernelGGL((cross_spectrum_kernel<kModeX, kVarMean>), grid, dim3(kXSpecThreads), 0, s, d_rows_x, d_rows_y, n_rows, stt, d_c2, d_sin,
                           d_edges, n_bands, N, d_out);
    else if (mode_y == kVarLinear)
        hipLaunchKernelGGL((cross_spectrum_kernel<kModeX, kVarLinear>), grid, dim3(kXSpecThreads), 0, s, d_rows_x, d_rows_y, n_rows, stt, d_c2, d_sin,
                           d_edges, n_bands, N, d_out);
    else if (mode_y == kVarDifference)
        hipLaunchKernelGGL((cross_spectrum_kernel<kModeX, kVarDifference>), grid, dim3(kXSpecThreads), 0, s, d_rows_x, d_rows_y, n_rows, stt, d_c2,
                           d_sin, d_edges, n_bands, N, d_out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_cross_spectrum(const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_x, int32_t mode_y,
                                 double stt, const double* d_c2, const double* d_sin, const int32_t* d_edges, int32_t n_bands, int64_t N,
                                 double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (n_bands < 1 || n_bands > kMaxCrossSpectrumBands) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + kXSpecThreads - 1) / kXSpecThreads));
    if (mode_x == kVarMean) return launch_mode_y<kVarMean>(grid, d_rows_x, d_rows_y, n_rows, mode_y, stt, d_c2, d_sin, d_edges, n_bands, N, d_out, s);
    if (mode_x == kVarLinear)
        return launch_mode_y<kVarLinear>(grid, d_rows_x, d_rows_y, n_rows, mode_y, stt, d_c2, d_sin, d_edges, n_bands, N, d_out, s);
    if (mode_x == kVarDifference)
        return launch_mode_y<kVarDifference>(grid, d_rows_x, d_rows_y, n_rows, mode_y, stt, d_c2, d_sin, d_edges, n_bands, N, d_out, s);
    return hipErrorInvalidValue;
}

}  // namespace rscm
