// The finishing step of the cross-member moments (rscm_gpu_moment_finish, include/rscm_gpu.h): a block of 68 signed limbs with
// deferred carries and a count of non-finite terms becomes the one double RN(canonical value * 2^-1088 / divisor).  Integers only
// until the last line; no HIP, so a host compiler builds it alone (tests/c_abi/moments_finish_host.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace rscm {

constexpr int kMomentLimbs = 68;                 // limb k in units of 2^(32 k - 1088)
constexpr int kMomentBlock = kMomentLimbs + 1;   // the limbs, then the count of non-finite terms
constexpr int kMomentUnitExp = -1088;            // the unit of limb 0 (and of the canonical integer)
constexpr int64_t kMomentMaxTerms = int64_t(1) << 31;   // an int64 limb takes this many 32-bit digits before it can wrap

// One block.  The canonical integer V = sum limb_k 2^(32 k) is normalised into 70 digits of 32 bits (the 68 limbs are each below 2^63
// in magnitude, so V is below 2^(32 * 67 + 64)), divided by the divisor digit by digit from the top (the remainder is below 2^63, so
// remainder * 2^32 + digit fits 128 bits), and the integer quotient Q = floor(|V| / divisor), in units of 2^-1088, is rounded to
// the 53 bits -- fewer in the subnormal range -- of a double, with the division's remainder as one more sticky bit.  The finest
// double bit is 2^-1074 = 2^14 units, so Q always holds the rounding bit: nothing below the units is needed.
inline double moment_finish_block(const int64_t* block, int64_t divisor)
{
    constexpr int kDigits = kMomentLimbs + 2;
    if (block[kMomentLimbs] != 0 || divisor <= 0) return std::numeric_limits<double>::quiet_NaN();
    uint32_t dig[kDigits];
    __int128 carry = 0;
    for (int k = 0; k < kDigits; ++k) {
        const __int128 t = carry + (k < kMomentLimbs ? (__int128)block[k] : (__int128)0);
        dig[k] = (uint32_t)((unsigned __int128)t & 0xFFFFFFFFu);
        carry = (t - (__int128)dig[k]) / ((__int128)1 << 32);   // exact: t - dig is a multiple of 2^32
    }
    const bool neg = carry < 0;   // what is left is the sign: 0 or -1
    if (neg) {                    // two's complement over the digits
        uint64_t c = 1;
        for (int k = 0; k < kDigits; ++k) {
            c += (uint64_t)(uint32_t)~dig[k];
            dig[k] = (uint32_t)c;
            c >>= 32;
        }
    }
    uint32_t q[kDigits];
    unsigned __int128 rem = 0;
    const unsigned __int128 d = (unsigned __int128)(uint64_t)divisor;
    bool any = false;
    for (int k = kDigits - 1; k >= 0; --k) {
        any |= dig[k] != 0;
        rem = (rem << 32) | dig[k];
        q[k] = (uint32_t)(rem / d);
        rem %= d;
    }
    if (!any) return 0.0;   // a zero sum is +0.0
    bool sticky = rem != 0;
    int len = 0;            // bits of Q
    for (int k = kDigits - 1; k >= 0 && !len; --k)
        if (q[k]) len = 32 * k + 64 - __builtin_clzll((uint64_t)q[k]);
    auto bit = [&](int i) { return (q[i >> 5] >> (i & 31)) & 1u; };
    const int shift = len - 53 > 14 ? len - 53 : 14;   // normal: 53 bits kept; below 2^-1022: the grid of 2^-1074
    uint64_t mant = 0;
    for (int i = len - 1; i >= shift; --i) mant = (mant << 1) | bit(i);
    const bool half = len >= shift && bit(shift - 1);
    for (int i = 0; i < shift - 1 && i < len && !sticky; ++i) sticky = bit(i);
    if (half && (sticky || (mant & 1))) ++mant;          // ties to even; 2^53 is a double, and ldexp carries it on
    const double r = std::ldexp((double)mant, shift + kMomentUnitExp);   // exact, or +inf beyond the largest finite double
    return neg ? -r : r;
}

// out[b] of blocks[n_blocks][kMomentBlock] with divisor[b] each; 0, or 1 for arguments the contract refuses (a NULL, a negative
// divisor or number of blocks, n_terms outside [0, 2^31): more terms than that may have wrapped a limb)
inline int moment_finish(const int64_t* blocks, int32_t n_blocks, const int64_t* divisor, int64_t n_terms, double* out)
{
    if (n_blocks < 0 || n_terms < 0 || n_terms >= kMomentMaxTerms) return 1;
    if (n_blocks > 0 && (!blocks || !divisor || !out)) return 1;
    for (int32_t b = 0; b < n_blocks; ++b)
        if (divisor[b] < 0) return 1;
    for (int32_t b = 0; b < n_blocks; ++b) out[b] = moment_finish_block(blocks + (size_t)b * kMomentBlock, divisor[b]);
    return 0;
}

}  // namespace rscm
