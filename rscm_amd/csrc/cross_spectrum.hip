// Per-member co-spectra, coherence and gain of two variables in frequency bands, for gfx950 (MI355X).
//
// cross_spectrum_kernel: one thread per member over the rows of BOTH variables; working series (plain, difference, midpoint), walk,
// pass 1 and the residuals a_k (of x) and c_k (of y) are those of series_walk.hpp.  The statistic is the one include/rscm_gpu.h
// states under rscm_ens_member_cross_spectrum.  All passes run in one launch:
//   pass 1          m, b of both variables, and whether any row of either is non-finite
//   one pass per    tile of kXSpecF frequencies j0 .. j0 + kXSpecF - 1: the lane keeps s1, s2 (of a) and t1, t2 (of c) of Goertzel's
//   tile            recurrence for every frequency of the tile in registers (8 kXSpecF VGPRs), re-forms a_k and c_k from the rows
//                   and advances all 2 kXSpecF recurrences with them:
//                       s0 = (a_k + c2_j * s1) - s2;  s2 = s1;  s1 = s0        t0 = (c_k + c2_j * t1) - t2;  t2 = t1;  t1 = t0
//                   (the register sets exchange their names at every term, not their values: the walk hands the parity on).  The
//                   first tile also forms Cxx = a_0 a_0 + ... and Cyy = c_0 c_0 + ...
//   after a tile    in ascending j, with h_j = c2_j * 0.5 and g_j the double nearest sin(2 pi j / n):
//                       Ixx = ((s1 s1 + s2 s2) - (c2_j s1) s2) / n           Iyy the same on t
//                       K   = ((s1 t1 + s2 t2) - h_j (s1 t2 + s2 t1)) / n    Q = (g_j (s2 t1 - s1 t2)) / n
//                   added to four running band sums, which are carried in registers across tiles; a band that ends at j is divided
//                   by its count and its coherence, gain and quadrature gain are stored
// c2_j and g_j come from the tables the host uploads per call (rscm_gpu_spectrum_coefficients, rscm_gpu_spectrum_sines), each padded
// by kSpectrumTablePad zeros and followed in the same allocation by the band edges; all are read at wave-uniform addresses, so they
// travel as scalar loads.  Only the frequencies inside [edges[0], edges[n_bands]) are computed; the last tile may be partial, and its
// idle recurrences run on the padding.  Row traffic: 2 x 8 B x R x N x (1 + tiles).
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"
#include "series_walk.hpp"

namespace rscm {

namespace {

constexpr int kXSpecThreads = 256;
constexpr int kXSpecBatch = 4;   // terms of each variable whose loads a thread issues before it uses them: 2 x kXSpecBatch values in flight
// Frequencies per tile.  The listing (make asm-cross-spectrum) decides: 8 kXSpecF VGPRs of recurrence state, 4 kXSpecBatch of rows in
// flight and about forty more.  8 is the widest tile that fits 128 VGPRs -- four waves per SIMD, which the kernel asks the compiler
// for -- without scratch (122-128 VGPRs over the nine instances); 10 spills in three instances, 12 in all nine, and so does a batch
// of 8 rows at a tile of 8.  profiles/cross_spectrum_bench.txt has the listing's figures.
constexpr int kXSpecF = 8;
static_assert(kXSpecF - 1 <= kSpectrumTablePad, "a tile reads up to kXSpecF - 1 table entries past the last frequency");

// One pass over the rows of both variables for the frequencies j0 .. j0 + kXSpecF - 1 (those past the last one idle on the table's
// padding); kFirst: Cxx, Cyy too.  On return s1, t1 hold the recurrences' last values and s2, t2 the ones before them.
template <class S, bool kFirst>
__device__ __forceinline__ void tile_pass(const double* const* const (&rows)[2], int32_t n, int64_t i, const Detrend<2>& d,
                                          const double* __restrict__ c2, int32_t j0, double (&cf)[kXSpecF],
                                          double (&s1)[kXSpecF], double (&s2)[kXSpecF], double (&t1)[kXSpecF], double (&t2)[kXSpecF],
                                          double& Cxx, double& Cyy)
{
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
    walk_terms<S, kXSpecBatch, false>(rows, n, i, unused, [&](const double (&u)[2], int32_t, auto odd) {
        double r[2];
        residuals<S>(u, tau, d, r);
        if constexpr (S::any_linear) tau = tau + 1.0;
        const double a = r[0], c = r[1];
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
    using S = Series<kModeX, kModeY>;
    const double* const* const rows[2] = {rows_x, rows_y};
    const int32_t n = S::terms(n_rows);
    const double dn = (double)n;
    bool bad = false;
    const Detrend<2> d = detrend_pass<S, kXSpecBatch>(rows, n, stt, i, bad);

    const double qnan = __builtin_nan("");
    const int32_t j_begin = edges[0], j_end = edges[n_bands];
    int32_t band = 0, band_begin = j_begin, band_end = edges[1];
    double Cxx = -0.0, Cyy = -0.0;
    double Axx = -0.0, Ayy = -0.0, AK = -0.0, AQ = -0.0;   // the running band sums of Ixx, Iyy, K, Q
    for (int32_t j0 = j_begin; j0 < j_end; j0 += kXSpecF) {
        double cf[kXSpecF], s1[kXSpecF], s2[kXSpecF], t1[kXSpecF], t2[kXSpecF];
        if (j0 == j_begin)
            tile_pass<S, true>(rows, n, i, d, c2, j0, cf, s1, s2, t1, t2, Cxx, Cyy);
        else
            tile_pass<S, false>(rows, n, i, d, c2, j0, cf, s1, s2, t1, t2, Cxx, Cyy);
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

}  // namespace

hipError_t launch_cross_spectrum(const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_x, int32_t mode_y,
                                 double stt, const double* d_c2, const double* d_sin, const int32_t* d_edges, int32_t n_bands, int64_t N,
                                 double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (n_bands < 1 || n_bands > kMaxCrossSpectrumBands) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + kXSpecThreads - 1) / kXSpecThreads));
    return with_mode(mode_x, [&](auto mx) {
        return with_mode(mode_y, [&](auto my) {
            hipLaunchKernelGGL((cross_spectrum_kernel<decltype(mx)::value, decltype(my)::value>), grid, dim3(kXSpecThreads), 0, s, d_rows_x, d_rows_y,
                               n_rows, stt, d_c2, d_sin, d_edges, n_bands, N, d_out);
            return hipGetLastError();
        });
    });
}

}  // namespace rscm
