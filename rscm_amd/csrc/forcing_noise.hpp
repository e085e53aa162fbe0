// The seeded forcing noise of a two-layer handle (include/rscm_gpu.h, rscm_ens_set_forcing_noise): a standard normal deviate that is
// a pure function of (seed, global member id g, forcing-axis index t) -- white in t, independent between members, no state.
//
//   Philox4x32-10, counter (lo32 g, hi32 g, t >> 1, RSCM_NOISE_STREAM_TAG), key (lo32 seed, hi32 seed); even t: words (0,1), odd: (2,3)
//   k = ((hi << 32) | lo) >> 12;  u = (2k + 1) 2^-53 in (0,1), symmetric about 1/2;  q = u - 1/2          (all exact)
//   z = AS241 PPND16(u) (Wichura 1988), Horner form
//
// Everything after the integer part is f64 + - * / and sqrt, each rounded on its own (the library is compiled with -ffp-contract=off
// and nothing here is written as an FMA), so tests/host_forcing_noise.py restates it in numpy with the same bits.  That is why the
// tails' logarithm is written out below instead of calling the device's log.
#pragma once

#include "philox.hpp"
#include "rscm_device.hpp"

namespace rscm {
namespace noise {

constexpr uint32_t kStreamTag = kNoiseStreamTag;   // RSCM_NOISE_STREAM_TAG; rscm_gpu.cpp static_asserts that the two agree

// ln(p) for a normal f64 p (used for p in [2^-53, 1/2]): p = m 2^e with m in (1/sqrt 2, sqrt 2], s = (m - 1)/(m + 1), w = s s,
// ln m = 2 atanh s = 2s + 2s w (1/3 + w/5 + ... + w^11/25), ln p = e ln 2 + ln m.  |s| <= 0.1716: the series' remainder is below
// 2^-64 relative; within 1 ulp of the correctly rounded logarithm on [2^-53, 0.075] (tests/test_forcing_noise_cpu.py).
__device__ __forceinline__ double ln_small(double p)
{
    const uint64_t bits = (uint64_t)__double_as_longlong(p);
    int32_t e = (int32_t)(bits >> 52) - 1023;
    double m = __longlong_as_double((long long)((bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull));
    const bool big = m > 1.4142135623730951;
    m = big ? m * 0.5 : m;
    e = big ? e + 1 : e;
    const double s = (m - 1.0) / (m + 1.0);
    const double w = s * s;
    double P = 1.0 / 25.0;
    P = P * w + 1.0 / 23.0;
    P = P * w + 1.0 / 21.0;
    P = P * w + 1.0 / 19.0;
    P = P * w + 1.0 / 17.0;
    P = P * w + 1.0 / 15.0;
    P = P * w + 1.0 / 13.0;
    P = P * w + 1.0 / 11.0;
    P = P * w + 1.0 / 9.0;
    P = P * w + 1.0 / 7.0;
    P = P * w + 1.0 / 5.0;
    P = P * w + 1.0 / 3.0;
    const double s2 = s + s;
    const double r = s2 + s2 * (w * P);
    return (double)e * 0.6931471805599453 + r;
}

// degree 7 in Horner form, highest coefficient first
__device__ __forceinline__ double poly7(double r, double c7, double c6, double c5, double c4, double c3, double c2, double c1, double c0)
{
    double p = c7 * r + c6;
    p = p * r + c5;
    p = p * r + c4;
    p = p * r + c3;
    p = p * r + c2;
    p = p * r + c1;
    return p * r + c0;
}

// Q(u): the standard normal quantile of a probability u in [2^-1022, 1 - 2^-53] (include/rscm_gpu.h, rscm_ens_sample_lhs_priors; the
// callers keep u inside: ln_small wants a normal f64).  q = u - 1/2 is one rounded subtraction (exact for u >= 1/4), 1 - u is exact
// for u >= 1/2.  The central branch (|q| <= 0.425, 85 % of uniform draws) and the near tail (r <= 5) are both computed and selected:
// with 15 % of lanes in the tail nearly every wavefront would run both anyway.  The far tail (p < e^-25, one uniform draw in 4e10; every
// lane of a prior truncated out there) is a real branch.
__device__ __forceinline__ double normal_from_p(double u)
{
    const double q = u - 0.5;
    const double aq = __builtin_fabs(q);
    // central: r = 0.180625 - q^2, z = q A(r) / B(r)
    const double rc = 0.180625 - q * q;
    const double num_c = poly7(rc, 2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                               1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0) * q;
    const double den_c = poly7(rc, 5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                               5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0);
    // tail: p = min(u, 1 - u) (exact), r = sqrt(-ln p)
    const double p = q < 0.0 ? u : 1.0 - u;
    const double rt = __builtin_sqrt(-ln_small(p));
    double num_t, den_t;
    if (__builtin_expect(rt > 5.0, 0)) {
        const double r = rt - 5.0;
        num_t = poly7(r, 2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0);
        den_t = poly7(r, 2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0);
    } else {
        const double r = rt - 1.6;
        num_t = poly7(r, 7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
                      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0);
        den_t = poly7(r, 1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                      6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0);
    }
    // one division serves both: x / y is the same IEEE operation whichever branch supplied x and y, and -(x / y) == (-x) / y
    const bool central = aq <= 0.425;
    const double num = central ? num_c : (q < 0.0 ? -num_t : num_t);
    const double den = central ? den_c : den_t;
    return num / den;
}

// The deviate of a 52-bit integer k: Q at u = (2k + 1) 2^-53, where q and 1 - u are exact
__device__ __forceinline__ double normal_from_k(uint64_t k)
{
    return normal_from_p((double)(2 * k + 1) * (1.0 / 9007199254740992.0));
}

// The Philox block of (seed, g, t >> 1): words (0,1) serve even t, words (2,3) odd t
__device__ __forceinline__ void block_of(uint64_t seed, uint64_t g, uint32_t t, uint32_t c[4])
{
    c[0] = (uint32_t)g;
    c[1] = (uint32_t)(g >> 32);
    c[2] = t >> 1;
    c[3] = kStreamTag;
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__device__ __forceinline__ uint64_t k_of(uint32_t lo, uint32_t hi) { return (((uint64_t)hi << 32) | lo) >> 12; }

// z(seed, g, t)
__device__ __forceinline__ double draw(uint64_t seed, uint64_t g, uint32_t t)
{
    uint32_t c[4];
    block_of(seed, g, t, c);
    return normal_from_k((t & 1u) ? k_of(c[2], c[3]) : k_of(c[0], c[1]));
}

}  // namespace noise
}  // namespace rscm
