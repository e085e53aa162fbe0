// The working series of the per-member series statistics -- rscm_ens_member_variability, _spectrum, _covariability and
// _cross_spectrum (variability.hip, spectrum.hip, covariability.hip, cross_spectrum.hip) -- stated once: which series a variable's
// rows stand for, the one walk over the rows, pass 1 (m, b and the finite check), the residual expression and the dispatch from a
// runtime detrending mode to a template argument.  include/rscm_gpu.h defines the four statistics to share these "operation for
// operation"; here they share them in the source as well.
//
// One thread per member i reads the device arrays of row pointers the host resolves (one array per variable; full storage, the
// window, the output store): lanes of a wave read consecutive members of one row, so every load is coalesced.  Every operation is one
// f64 operation rounded on its own (-ffp-contract=off: no FMA); sums run left to right and start at -0.0, the additive identity,
// which is "starting from the first term" bit for bit.  Nothing here is indexed at run time: no per-member array, no scratch, no LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rscm_device.hpp"

namespace rscm {

// The kind of a variable's working series under the detrending modes of a call (one variable, or a pair):
//   plain       u_k = x_k                      no variable of the call has RSCM_VAR_DIFFERENCE; n = R
//   difference  u_k = x_{k+1} - x_k            the variable's own mode is RSCM_VAR_DIFFERENCE; n = R - 1
//   midpoint    u_k = (x_k + x_{k+1}) * 0.5    only its partner's mode is RSCM_VAR_DIFFERENCE; n = R - 1
// so all series of a call have one length n, and either every series spans two rows per term or none does.
template <int... kModes>
struct Series {
    static constexpr int K = sizeof...(kModes);
    static constexpr bool two_rows = ((kModes == kVarDifference) || ...);
    static constexpr bool any_linear = ((kModes == kVarLinear) || ...);
    // (v is a constant wherever these are called: the loops over the variables are unrolled)
    __host__ __device__ static constexpr int mode(int v)
    {
        const int m[K] = {kModes...};
        return m[v];
    }
    __host__ __device__ static constexpr bool linear(int v) { return mode(v) == kVarLinear; }
    __host__ __device__ static constexpr int32_t terms(int32_t n_rows) { return two_rows ? n_rows - 1 : n_rows; }
    // u_k of variable v from its rows k (prev) and k + 1 (cur)
    __device__ static __forceinline__ double term(int v, double prev, double cur)
    {
        return mode(v) == kVarDifference ? cur - prev : (prev + cur) * 0.5;
    }
};

// The parity of a term index, handed on as a type: Goertzel's recurrences write even terms into one register set and odd terms into
// the other, so no value moves between terms.  The other statistics ignore it.
using Even = std::integral_constant<bool, false>;
using Odd = std::integral_constant<bool, true>;

// f(u, k, parity of k) for k = 0 .. n - 1 in order, u[v] = term k of variable v from member i's values in rows[v].  Where the series
// span two rows per term, row 0 of each variable is loaded ahead, so that every batch holds kBatch terms under every mode.  A batch's
// loads are issued before its terms are used: all of variable 0, then all of variable 1.  After the batches the rest goes in pairs,
// then a last single term.  kCheck: bad becomes true if any raw value loaded is not finite.
template <class S, int kBatch, bool kCheck, class F>
__device__ __forceinline__ void walk_terms(const double* const* const (&rows)[S::K], int32_t n, int64_t i, bool& bad, F&& f)
{
    static_assert(kBatch % 2 == 0, "a batch keeps the parity");
    constexpr int K = S::K;
    constexpr int kOff = S::two_rows ? 1 : 0;   // the (later) row of term k is k + kOff
    [[maybe_unused]] double prev[K];
    auto term = [&](const double (&x)[K], int32_t k, auto parity) {
        double u[K];
#pragma unroll
        for (int v = 0; v < K; ++v) {
            if constexpr (kCheck) bad = bad || !__builtin_isfinite(x[v]);
            if constexpr (S::two_rows) {
                u[v] = S::term(v, prev[v], x[v]);
                prev[v] = x[v];
            } else {
                u[v] = x[v];
            }
        }
        f(u, k, parity);
    };
    if constexpr (S::two_rows) {
#pragma unroll
        for (int v = 0; v < K; ++v) {
            prev[v] = rows[v][0][i];
            if constexpr (kCheck) bad = bad || !__builtin_isfinite(prev[v]);
        }
    }
    int32_t k = 0;
    for (; k + kBatch <= n; k += kBatch) {
        double x[kBatch][K];
#pragma unroll
        for (int v = 0; v < K; ++v)
#pragma unroll
            for (int j = 0; j < kBatch; ++j) x[j][v] = rows[v][kOff + k + j][i];
#pragma unroll
        for (int j = 0; j < kBatch; j += 2) {
            term(x[j], k + j, Even{});
            term(x[j + 1], k + j + 1, Odd{});
        }
    }
    for (; k + 2 <= n; k += 2) {
        double x[2][K];
#pragma unroll
        for (int v = 0; v < K; ++v)
#pragma unroll
            for (int j = 0; j < 2; ++j) x[j][v] = rows[v][kOff + k + j][i];
        term(x[0], k, Even{});
        term(x[1], k + 1, Odd{});
    }
    if (k < n) {
        double x[K];
#pragma unroll
        for (int v = 0; v < K; ++v) x[v] = rows[v][kOff + k][i];
        term(x, k, Even{});
    }
}

// What pass 1 leaves of each variable: m = S / n, b = Q / Stt under RSCM_VAR_LINEAR (else +0.0), and h = (n - 1) / 2
template <int K>
struct Detrend {
    double m[K], b[K], h;
};

// Pass 1: S = u_0 + u_1 + ..., and per linear variable Q = tau_0 u_0 + tau_1 u_1 + ..., tau_k = (double)k - h; and whether any
// raw value of any variable is not finite
template <class S, int kBatch>
__device__ __forceinline__ Detrend<S::K> detrend_pass(const double* const* const (&rows)[S::K], int32_t n, double stt, int64_t i, bool& bad)
{
    constexpr int K = S::K;
    Detrend<K> d;
    d.h = (double)(n - 1) * 0.5;
    double sum[K];
    [[maybe_unused]] double Q[K];
#pragma unroll
    for (int v = 0; v < K; ++v) sum[v] = Q[v] = -0.0;
    walk_terms<S, kBatch, true>(rows, n, i, bad, [&](const double (&u)[K], int32_t k, auto) {
        [[maybe_unused]] const double tau = (double)k - d.h;
#pragma unroll
        for (int v = 0; v < K; ++v) {
            sum[v] = sum[v] + u[v];
            if constexpr (S::any_linear)
                if (S::linear(v)) Q[v] = Q[v] + tau * u[v];
        }
    });
#pragma unroll
    for (int v = 0; v < K; ++v) {
        d.m[v] = sum[v] / (double)n;
        d.b[v] = S::linear(v) ? Q[v] / stt : 0.0;
    }
    return d;
}

// The residuals a[v] of the terms u[v] at tau = tau_k: the one expression every later pass re-forms them with, so their bits cannot
// depend on the pass.  The caller obtains tau in its own way: as (double)k - h, or carried as tau_{k-1} + 1.0 from -h; with n <= 4096
// both are exact (multiples of 0.5 below 2^12), so the carried tau has the bits of the definition's.
template <class S>
__device__ __forceinline__ void residuals(const double (&u)[S::K], [[maybe_unused]] double tau, const Detrend<S::K>& d, double (&a)[S::K])
{
#pragma unroll
    for (int v = 0; v < S::K; ++v) {
        a[v] = u[v] - d.m[v];
        if (S::linear(v)) a[v] = a[v] - d.b[v] * tau;
    }
}

// f(the detrending mode as a std::integral_constant) for a valid runtime mode; hipErrorInvalidValue for any other
template <class F>
hipError_t with_mode(int32_t mode, F&& f)
{
    if (mode == kVarMean) return f(std::integral_constant<int, kVarMean>{});
    if (mode == kVarLinear) return f(std::integral_constant<int, kVarLinear>{});
    if (mode == kVarDifference) return f(std::integral_constant<int, kVarDifference>{});
    return hipErrorInvalidValue;
}

}  // namespace rscm
