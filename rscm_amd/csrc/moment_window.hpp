// The pure integer pieces of the moments of stored rows (moment_rows.hip; the definition is stated in include/rscm_gpu.h,
// rscm_ens_moment_rows_sums): a term as five 32-bit digits, a lane's private window of kMomWin limbs, and the fold of a window into
// the 68-limb block of moments_finish.hpp.  No HIP and no floating point: a host compiler builds it alone
// (tests/c_abi/moment_window_host.cpp), and the kernels include the very same functions (moments.hip those of the term alone).
//
// The window.  A term w * mantissa << pos (at most 106 + 31 bits above the limb boundary below pos) is five digits d_0 .. d_4, digit
// k in limb q + k with q = pos >> 5.  A lane keeps kMomWin = 8 consecutive limbs, base .. base + 7, as uint64 registers; a term with
// base <= q <= base + kMomWinSpan (= 3) lies inside and the lane adds it without leaving its registers: the five digits are moved
// up by off = q - base slots in two select stages (by 1, by 2) and each of the eight slots takes one 32-bit value.
// The sign costs no negation per slot: a negative term adds d ^ 0xFFFFFFFF = 0xFFFFFFFF - d to EVERY slot (0xFFFFFFFF where it has
// no digit) and the lane counts it; mom_window_settle then takes n_neg * 0xFFFFFFFF off every slot, which leaves -d.
//
// Why a fold is exact.  After settling, slot j of a lane holds, modulo 2^64, the signed sum of the digits the lane's terms have in
// limb base + j.  The sum of slot j over the 64 lanes is what moments.hip's lane-per-limb design would have added to that limb for
// the same terms; adding it to limb base + j of the block adds exactly those terms, because a block's value is linear in its limbs.
// Slots with base + j >= 68 (base reaches 62) hold zero and are left out: no finite double has a digit there (pos <= 2059, and
// the 106 bits above it end below bit 2176 = 68 * 32).
//
// Overflow.  Between two folds a lane adds fewer than 2^31 values below 2^32 to a slot (fewer than 2^31 members per handle), so a
// slot stays below 2^63 and cannot wrap before it is settled; the settled slot and the sum over the lanes are signed sums of fewer
// than 2^31 digits below 2^32, below 2^63 in magnitude: the bound N < 2^31 that moments.hip states is the one needed here.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSCM_MW_HD __host__ __device__ __forceinline__
#define RSCM_MW_UNROLL _Pragma("unroll")   // the slots are registers: every index must be a constant
#else
#define RSCM_MW_HD inline
#define RSCM_MW_UNROLL
#endif

namespace rscm {

constexpr int kMomWin = 8;                     // limbs of a lane's window: 16 VGPRs per sum
constexpr int kMomWinSpan = kMomWin - 5;       // a term lies inside when base <= q <= base + kMomWinSpan
constexpr int kMomWinLimbs = 68;               // kMomentLimbs of moments_finish.hpp (asserted where both are included)
constexpr uint32_t kMomDigitMask = 0xFFFFFFFFu;

RSCM_MW_HD bool mom_finite_bits(uint64_t bits) { return ((bits >> 52) & 0x7FFu) != 0x7FFu; }

// The raw fields of a double as the accumulator sees them: the mantissa (the fraction, with the hidden bit unless E == 0), the bit
// position of its lowest bit (max(E, 1) + 13) and the sign; false for a non-finite double (E == 0x7FF)
RSCM_MW_HD bool mom_fields(uint64_t bits, uint64_t& mant, uint32_t& pos, uint32_t& neg)
{
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7FFu;
    const uint64_t frac = bits & ((uint64_t(1) << 52) - 1);
    mant = e ? (frac | (uint64_t(1) << 52)) : frac;
    pos = (e ? e : 1u) + 13u;
    neg = (uint32_t)(bits >> 63);
    return e != 0x7FFu;
}

// w * mant as (hi : lo)
RSCM_MW_HD void mom_product(uint64_t w, uint64_t mant, uint64_t& lo, uint64_t& hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    lo = w * mant;
    hi = __umul64hi(w, mant);
#else
    const unsigned __int128 p = (unsigned __int128)w * mant;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// (hi : lo) << r, r = pos & 31, at most 137 bits, as five digits: digit k falls into limb (pos >> 5) + k
RSCM_MW_HD void mom_digits(uint64_t lo, uint64_t hi, uint32_t r, uint32_t (&d)[5])
{
    const uint64_t s0 = lo << r;
    const uint64_t s1 = (hi << r) | (r ? lo >> (64u - r) : 0ull);
    const uint64_t s2 = r ? hi >> (64u - r) : 0ull;
    d[0] = (uint32_t)s0;
    d[1] = (uint32_t)(s0 >> 32);
    d[2] = (uint32_t)s1;
    d[3] = (uint32_t)(s1 >> 32);
    d[4] = (uint32_t)s2;
}

// The base a window takes when it has to move: the largest term's limb two slots above it, one slot of headroom on top.  Every
// term within 64 bits below the largest one's lowest bit then lies inside (q >= qmax - 2).
RSCM_MW_HD int mom_window_base(int qmax) { return qmax > 2 ? qmax - 2 : 0; }
RSCM_MW_HD bool mom_window_holds(int base, int q) { return q >= base && q <= base + kMomWinSpan; }

// Adds the term (digits d, sign neg in {0, 1}) that lies off = q - base in [0, kMomWinSpan] slots above the window's base.  A lane
// that has no term in the window passes zero digits and neg = 0, which adds nothing.
RSCM_MW_HD void mom_window_add(uint64_t (&win)[kMomWin], uint32_t& n_neg, const uint32_t (&d)[5], uint32_t off, uint32_t neg)
{
    const uint32_t m = neg ? kMomDigitMask : 0u;
    uint32_t a[6], b[kMomWin];
    const bool by1 = (off & 1u) != 0u, by2 = (off & 2u) != 0u;
    RSCM_MW_UNROLL
    for (int j = 0; j < 6; ++j) {
        const uint32_t same = j < 5 ? (d[j < 5 ? j : 0] ^ m) : m;
        const uint32_t up = j >= 1 ? (d[j >= 1 ? j - 1 : 0] ^ m) : m;
        a[j] = by1 ? up : same;
    }
    RSCM_MW_UNROLL
    for (int j = 0; j < kMomWin; ++j) {
        const uint32_t same = j < 6 ? a[j < 6 ? j : 0] : m;
        const uint32_t up = j >= 2 ? a[j >= 2 ? j - 2 : 0] : m;
        b[j] = by2 ? up : same;
    }
    RSCM_MW_UNROLL
    for (int j = 0; j < kMomWin; ++j) win[j] += (uint64_t)b[j];
    n_neg += neg;
}

// Takes the negative terms' 0xFFFFFFFF off every slot: afterwards slot j is the signed sum of its digits modulo 2^64
RSCM_MW_HD void mom_window_settle(uint64_t (&win)[kMomWin], uint32_t n_neg)
{
    const uint64_t off = ((uint64_t)n_neg << 32) - (uint64_t)n_neg;   // n_neg * 0xFFFFFFFF
    RSCM_MW_UNROLL
    for (int j = 0; j < kMomWin; ++j) win[j] -= off;
}

// The fold as the host states it: slot_sum[j] = the sum over the lanes of their settled slot j goes into limb base + j
inline void mom_window_fold(const uint64_t (&slot_sum)[kMomWin], int base, int64_t* limbs)
{
    for (int j = 0; j < kMomWin; ++j)
        if (base + j < kMomWinLimbs) limbs[base + j] = (int64_t)((uint64_t)limbs[base + j] + slot_sum[j]);
}

// A term placed directly, digit by digit with its sign, as the serial walk does: the reference of the fold
inline void mom_place(const uint32_t (&d)[5], int q, uint32_t neg, int64_t* limbs)
{
    for (int k = 0; k < 5; ++k)
        if (q + k < kMomWinLimbs) limbs[q + k] += neg ? -(int64_t)d[k] : (int64_t)d[k];
}

}  // namespace rscm
