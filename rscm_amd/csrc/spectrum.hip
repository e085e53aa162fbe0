// Per-member power spectra of a stored variable in frequency bands, and the spectral likelihood over band powers, for gfx950 (MI355X).
//
// spectrum_kernel: one thread per member; working series, walk, pass 1 and the residuals a_k are those of series_walk.hpp.  The
// statistic is the one include/rscm_gpu.h states under rscm_ens_member_spectrum.  All passes run in one launch:
//   pass 1          m, b, and whether any row is non-finite
//   one pass per    tile of kSpecF frequencies j0 .. j0 + kSpecF - 1: the lane keeps s1, s2 of Goertzel's recurrence for every
//   tile            frequency of the tile in registers (4 kSpecF VGPRs), re-forms a_k from the rows and advances all kSpecF
//                   recurrences with it:
//                       s0 = (a_k + c2_j * s1) - s2;  s2 = s1;  s1 = s0
//                   (the two register sets exchange their names at every term, not their values: the walk hands the parity on)
//                   kSpecF independent dependency chains per lane, three f64 operations per term and frequency, no memory operand
//                   but the residual.  The first tile also forms C0 = a_0 a_0 + a_1 a_1 + ...
//   after a tile    I_j = ((s1 s1 + s2 s2) - (c2_j s1) s2) / n in ascending j, added to the running band sum, which is carried in a
//                   register across tiles; a band that ends at j is divided by its count and stored
// c2_j = 2 cos(2 pi j / n) comes from the table the host uploads per call (rscm_gpu_spectrum_coefficients), followed in the same
// allocation by the band edges; both are read at wave-uniform addresses, once per tile and per band, so they travel as scalar loads
// and the coefficients sit in SGPRs during the pass.  Only the frequencies inside [edges[0], edges[n_bands]) are computed; the last
// tile may be partial, and its idle recurrences run on the zeros the table is padded with.  Row traffic: 8 B x R x N x (1 + tiles).
//
// loglik_spectrum_kernel: out[i] = (add ? add[i] : 0.0) + sum_b m_b (ln P_b[i] - 2 ln(P_b[i] + I_b)) with log_f64 (rk4_device.hpp),
// the expressions of rscm_ens_loglik_spectrum_device; -inf where a P_b[i] is non-finite or <= 0 or add[i] is non-finite.  add may be
// out: a thread reads its own element before it writes it.
#include <hip/hip_runtime.h>

#include "rk4_device.hpp"
#include "rscm_device.hpp"
#include "series_walk.hpp"

namespace rscm {

namespace {

constexpr int kSpecThreads = 256;
constexpr int kSpecBatch = 8;   // terms whose loads a thread issues before it uses them
// Frequencies per tile.  The listing (make asm-spectrum) decides: 4 kSpecF VGPRs of recurrence state, 2 kSpecBatch of rows in flight
// and about forty more.  16 is the widest tile that fits 128 VGPRs -- four waves per SIMD, which the kernel asks the compiler for --
// without scratch (118 / 126 / 120 VGPRs by mode); 20 needs 152-168.  profiles/spectrum_bench.txt has the listing's figures.
constexpr int kSpecF = 16;
static_assert(kSpecF - 1 <= kSpectrumTablePad, "a tile reads up to kSpecF - 1 coefficients past the last frequency");

// One pass over the rows for the frequencies j0 .. j0 + kSpecF - 1 (those past the last one idle on the table's padding); kFirst: C0 too.  On return
// s1 holds the recurrence's last value and s2 the one before it.
template <class S, bool kFirst>
__device__ __forceinline__ void tile_pass(const double* const* const (&rows)[1], int32_t n, int64_t i, const Detrend<1>& d,
                                          const double* __restrict__ c2, int32_t j0, double (&c)[kSpecF], double (&s1)[kSpecF],
                                          double (&s2)[kSpecF], double& C0)
{
#pragma unroll
    for (int f = 0; f < kSpecF; ++f) {
        c[f] = c2[j0 + f - 1];   // wave-uniform: scalar loads; past the last frequency the table's padding (zeros)
        s1[f] = 0.0;
        s2[f] = 0.0;
    }
    bool unused = false;
    [[maybe_unused]] double tau = -d.h;
    walk_terms<S, kSpecBatch, false>(rows, n, i, unused, [&](const double (&u)[1], int32_t, auto odd) {
        double r[1];
        residuals<S>(u, tau, d, r);
        if constexpr (S::any_linear) tau = tau + 1.0;
        const double a = r[0];
        if constexpr (kFirst) C0 = C0 + a * a;
#pragma unroll
        for (int f = 0; f < kSpecF; ++f) {
            // s0 = (a + c2 s1) - s2; s2 = s1; s1 = s0 -- with the names of s1 and s2 exchanged at every odd term instead of their values
            if constexpr (!decltype(odd)::value)
                s2[f] = (a + c[f] * s1[f]) - s2[f];
            else
                s1[f] = (a + c[f] * s2[f]) - s1[f];
        }
    });
    if (n & 1) {   // the last term was an even one: its value sits in s2
#pragma unroll
        for (int f = 0; f < kSpecF; ++f) {
            const double t = s1[f];
            s1[f] = s2[f];
            s2[f] = t;
        }
    }
}

// c2: [J] doubles and kSpectrumTablePad more that may be read; edges: int32 [n_bands + 1], 1 <= edges[0] < ... < edges[n_bands] <= J + 1 (checked by the host)
// (amdgpu_waves_per_eu(4): left alone the compiler spends the room below its next occupancy step, 130-160 VGPRs and three waves)
template <int kMode>
__global__ __launch_bounds__(kSpecThreads) __attribute__((amdgpu_waves_per_eu(4))) void spectrum_kernel(
    const double* const* __restrict__ rows_x, int32_t n_rows, double stt, const double* __restrict__ c2, const int32_t* __restrict__ edges,
    int32_t n_bands, int64_t N, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kSpecThreads + threadIdx.x;
    if (i >= N) return;
    using S = Series<kMode>;
    const double* const* const rows[1] = {rows_x};
    const int32_t n = S::terms(n_rows);
    const double dn = (double)n;
    bool bad = false;
    const Detrend<1> d = detrend_pass<S, kSpecBatch>(rows, n, stt, i, bad);

    const double qnan = __builtin_nan("");
    const int32_t j_begin = edges[0], j_end = edges[n_bands];
    int32_t band = 0, band_begin = j_begin, band_end = edges[1];
    double C0 = -0.0, acc = -0.0;
    for (int32_t j0 = j_begin; j0 < j_end; j0 += kSpecF) {
        double c[kSpecF], s1[kSpecF], s2[kSpecF];
        if (j0 == j_begin)
            tile_pass<S, true>(rows, n, i, d, c2, j0, c, s1, s2, C0);
        else
            tile_pass<S, false>(rows, n, i, d, c2, j0, c, s1, s2, C0);
#pragma unroll
        for (int f = 0; f < kSpecF; ++f) {
            const int32_t j = j0 + f;
            if (f < j_end - j0) {
                const double I = ((s1[f] * s1[f] + s2[f] * s2[f]) - (c[f] * s1[f]) * s2[f]) / dn;
                acc = acc + I;
                if (j + 1 == band_end) {       // wave-uniform; band < n_bands here, so the store stays inside [3 + n_bands][N]
                    const double P = acc / (double)(band_end - band_begin);
                    out[(int64_t)(3 + band) * N + i] = bad ? qnan : P;
                    acc = -0.0;
                    ++band;
                    band_begin = band_end;
                    if (band < n_bands) band_end = edges[band + 1];
                }
            }
        }
    }
    out[i] = bad ? qnan : d.m[0];
    out[N + i] = bad ? qnan : d.b[0];
    out[2 * N + i] = bad ? qnan : C0 / dn;
}

__global__ __launch_bounds__(kSpecThreads) void loglik_spectrum_kernel(LoglikSpectrum v, int32_t n_vec, const double* add, int64_t N, double* out)
{
    const int64_t i = (int64_t)blockIdx.x * kSpecThreads + threadIdx.x;
    if (i >= N) return;
    const double base = add ? add[i] : 0.0;
    bool bad = !__builtin_isfinite(base);
    double partial = 0.0;
    for (int32_t j = 0; j < n_vec; ++j) {
        const double P = v.vec[j][i];
        bad = bad || !(__builtin_isfinite(P) && P > 0.0);
        const double t = P + v.record[j];
        const double term = v.count[j] * (log_f64(P) - 2.0 * log_f64(t));
        partial += term;
    }
    out[i] = bad ? -__builtin_inf() : base + partial;
}

}  // namespace

hipError_t launch_spectrum(const double* const* d_rows, int32_t n_rows, int32_t mode, double stt, const double* d_c2, const int32_t* d_edges,
                           int32_t n_bands, int64_t N, double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    if (n_bands < 1 || n_bands > kMaxSpectrumBands) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + kSpecThreads - 1) / kSpecThreads));
    return with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(spectrum_kernel<decltype(m)::value>, grid, dim3(kSpecThreads), 0, s, d_rows, n_rows, stt, d_c2, d_edges, n_bands, N, d_out);
        return hipGetLastError();
    });
}

hipError_t launch_loglik_spectrum(const LoglikSpectrum& v, int32_t n_vec, const double* d_add, int64_t N, double* d_out, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const dim3 grid((unsigned)((N + kSpecThreads - 1) / kSpecThreads));
    hipLaunchKernelGGL(loglik_spectrum_kernel, grid, dim3(kSpecThreads), 0, s, v, n_vec, d_add, N, d_out);
    return hipGetLastError();
}

}  // namespace rscm
