// n / d in two instructions for a divisor d that stays the same over many divisions (rk4_device.hpp, pair_div):
//     zh = RN(1/d)      zl = RN(1/d - zh) = RN(fma(-d, zh, 1) / d)           once per divisor
//     t  = n * zl       q  = fma(n, zh, t)                                    per division
// and, for one divisor, the verdict whether q equals the IEEE quotient RN(n/d) for EVERY numerator of pair_div's window.  One text for
// the host and the device: plain C++ on 64-bit integers and f64, every loop with a compile-time trip bound.  The device forms the
// constants per member (two_layer.hip, two_layer_pair_div_kernel); tests/c_abi/pair_div_host.cpp compiles this header on its own and
// tests/test_pair_div_verdict.py holds it to a big-integer restatement; scripts/pair_div_proof.py writes the argument out and checks it
// exhaustively at reduced precision.
//
// The argument, for d = Y 2^a and n = X 2^b with 53-bit integer significands X, Y in [2^52, 2^53) and everything normal (a power of
// two moves n, d, zh, zl, t and q exactly, so only X and Y matter):
//   * 1 - d zh is representable (a multiple of ulp(d) ulp(zh) below 2^-53 d), so zl is the correctly rounded 1/d - zh: with d in
//     [1, 2), |1/d - zh| <= 2^-54, |zl| <= 2^-54 and |1/d - zh - zl| <= 2^-107.  t rounds n zl: |t - n zl| <= 2^-53 |n| 2^-54.  The
//     sum n zh + t is formed exactly inside the fma, so it equals n/d + e with |e| <= |n| 2^-106.  With zl moved k ulps (an ulp of
//     zl is at most 2^-106) the same count gives |e| <= |n| 2^-106 (1 + k)(1 + 2^-53).
//   * q is the rounding of that sum, so q != RN(n/d) needs a rounding boundary -- a midpoint (2Q + 1) / 2^s of two neighbouring
//     doubles, s = 53 for X >= Y (quotient in [1, 2)), s = 54 for X < Y (quotient in (1/2, 1)) -- between n/d and the sum, or on the sum
//     (X/Y itself is never a midpoint: 2^s X = (2Q + 1) Y has no solution with 53-bit X, Y).  X/Y differs from that midpoint by
//     j / (2^s Y) with the non-zero integer j = 2^s X - (2Q + 1) Y, so a failure needs |j| <= 2^s Y X 2^-158 (1 + k)(1 + 2^-53) <
//     2^(s - 52) (1 + k): |j| <= 1 (s = 53) and 3 (s = 54) for the constants as defined, |j| <= 3 and 7 with zl's neighbours.
//   * kJ = 8 covers all of these.  For each s and j, 2^s X = j (mod Y) is a linear congruence in X.  With Y = 2^c Y', Y' odd: it needs
//     2^c | j (so c <= 3, and a divisor with four or more trailing zero bits in Y -- every power of two among them, where zl = 0 -- has
//     no candidate at all and is safe), and then X = (j / 2^c) inv(2^(s - c)) (mod Y'), up to 2^(c + 1) solutions in [2^52, 2^53).
//     Neither the cofactor's parity nor X >= Y is checked: a superset of candidates is harmless, since every one is simply tried,
//     at one exponent, against the compiler's IEEE division.
//   * inv(2^e) mod Y' is e halvings modulo Y' (h even: h/2, else (h + Y')/2; at most 54), j inv by repeated addition modulo Y'.
// The constants stored are the ones tried, bit for bit: the first of (zh, zl), (zh, zl + ulp), (zh, zl - ulp) that passes every
// candidate; a divisor where none does, or one outside the wide divisor box [2^kWideDivLo, 2^kWideDivHi), is marked by zh = 0.
#pragma once

#include <stdint.h>

#include "two_layer_chunk_box.hpp"

#if defined(__HIPCC__)
#define RSCM_PAIR_HD __host__ __device__ inline
#else
#define RSCM_PAIR_HD inline
#endif

namespace rscm {
namespace pairdiv {

// pair_div's numerator window for a divisor in the wide divisor box: +0, or 2^kNumLo <= |n| < 2^kNumHi.
// A non-zero zl is at least RN(2^-105 / d) >= 2^-105 2^-kWideDivHi = 2^-119 (1 - d zh is a non-zero multiple of 2^-105 for d scaled into
// [1, 2), and rounding is monotone), a neighbour of it at least 2^-120: n zl is normal from |n| = 2^(-1022 + 120) on.  zh <= 2^-kWideDivLo,
// so n zh, t and the quotient stay finite below the wide window's upper edge, and the quotient is normal above 2^(kNumLo - kWideDivHi).
// A divisor whose tried zl is not that small has a deeper window: n zl is normal from 2^(-1022 - exponent(zl)) on, and nothing else in
// the argument asks for more (n zh and the quotient are normal far below).  verdict() takes the lower edge it is to vouch for and marks
// a divisor whose zl is too small for it unsafe.  kSurfaceNumFloor is the edge the surface equation's numerators need: the chunk guard
// admits them down to 2^-946 (scripts/two_layer_box_proof.py, check_pair_window), the deep equation's stay above 2^kNumLo.  A heat
// capacity below 2^10 with |zl| < 2^-76 is a chance of about 2^-18 per member.
constexpr int kNumLo = -902, kNumHi = 760;
constexpr int kSurfaceNumFloor = -946;
static_assert(kSurfaceNumFloor >= tl::chunk::kWideNumLo && kSurfaceNumFloor - tl::chunk::kWideDivHi > -1022, "n zh and the quotient stay normal");
constexpr int kZlMinExp = -105 - tl::chunk::kWideDivHi - 1;   // a tried non-zero zl is at least 2^kZlMinExp in magnitude
static_assert(kNumLo == -1022 - kZlMinExp && kNumLo >= tl::chunk::kWideNumLo, "n zl must be normal, inside spec_div's wide window");
static_assert(kNumHi == tl::chunk::kWideNumHi && kNumHi - tl::chunk::kWideDivLo < 1023, "n zh must be finite, inside spec_div's wide window");

constexpr int kJ = 8;           // |j| up to which candidates are formed: covers zl and its two neighbours (above)
constexpr int kMaxTrailing = 3; // 2^c | j with |j| <= kJ
constexpr int kVariants = 3;    // zl, zl + ulp, zl - ulp (in magnitude)
constexpr int kMaxSolutions = (2 << kMaxTrailing) + 1;   // X0 + m Y' in [2^52, 2^53): m below 2^(c + 1) + 1

struct Constants {
    double zh, zl;     // zh = 0: no constants are safe for this divisor
    int32_t variant;   // which of the kVariants passed (0: as defined); -1: none, -2: the divisor is outside the box
};

RSCM_PAIR_HD uint64_t bits_of(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    return b;
}
RSCM_PAIR_HD double from_bits(uint64_t b)
{
    double x;
    __builtin_memcpy(&x, &b, sizeof x);
    return x;
}

// the quotient of rk4_device.hpp's pair_div, restated for host and device (the product rounded on its own)
RSCM_PAIR_HD double quotient(double n, double zh, double zl)
{
    const double t = n * zl;
    return __builtin_fma(n, zh, t);
}

RSCM_PAIR_HD bool divisor_in_box(double d)
{
    const uint64_t b = bits_of(d);
    const int32_t e = (int32_t)(b >> 52) - 1023;   // (the sign bit makes e large: negative divisors are outside)
    return e >= tl::chunk::kWideDivLo && e < tl::chunk::kWideDivHi;
}

// zh and zl as defined
RSCM_PAIR_HD void plain_constants(double d, double& zh, double& zl)
{
    zh = 1.0 / d;
    zl = __builtin_fma(-d, zh, 1.0) / d;
}

// num_lo: the lower edge of the numerator window the verdict is to hold for (kNumLo holds for every divisor of the box)
RSCM_PAIR_HD Constants verdict(double d, int num_lo = kNumLo)
{
    Constants c;
    c.zh = 0.0;
    c.zl = 0.0;
    c.variant = -2;
    if (!divisor_in_box(d)) return c;
    double zh, zl;
    plain_constants(d, zh, zl);
    const uint64_t db = bits_of(d);
    const uint64_t Y = (db & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull;
    // everything scaled so that the divisor is Y 2^-52 in [1, 2): zh and zl by the same power of two, exactly
    const double ds = from_bits((db & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    const double scale = from_bits(((db >> 52) & 0x7FFull) << 52);   // 2^exponent(d)
    double zhs = zh * scale, zls[kVariants];
    zls[0] = zl * scale;
    // the neighbours in magnitude (zl = 0 only where Y is a power of two, which has no candidate: the entries are never tried)
    zls[1] = from_bits(bits_of(zls[0]) + 1);
    zls[2] = from_bits(bits_of(zls[0]) - 1);
    // n zl must be normal at the window's lower edge: a non-zero zl of at least 2^(-1022 - num_lo), in d's own scale
    bool ok[kVariants];
    for (int v = 0; v < kVariants; ++v) {
        const int32_t ez = (int32_t)((bits_of(zls[v]) >> 52) & 0x7FFull) - (int32_t)((db >> 52) & 0x7FFull);   // exponent of the unscaled zl
        ok[v] = zls[0] == 0.0 || ez >= -1022 - num_lo;
    }

    int c2 = 0;   // trailing zero bits of Y, counted up to kMaxTrailing + 1
    for (int k = 0; k <= kMaxTrailing; ++k)
        if (c2 == k && ((Y >> k) & 1ull) == 0) c2 = k + 1;
    if (c2 <= kMaxTrailing) {
        const uint64_t Yo = Y >> c2;   // odd, in [2^49, 2^53)
        // h = inv(2^(53 - c2)) mod Yo, then inv(2^(54 - c2)) for the second pass
        uint64_t h = 1;
        for (int k = 0; k < 53; ++k)
            if (k < 53 - c2) h = (h & 1ull) ? (h + Yo) >> 1 : h >> 1;
        for (int s = 53; s <= 54; ++s) {
            if (s == 54) h = (h & 1ull) ? (h + Yo) >> 1 : h >> 1;
            uint64_t acc = 0;   // (j' h) mod Yo for j' = 1, 2, ...
            for (int jp = 1; jp <= kJ; ++jp) {
                acc += h;
                if (acc >= Yo) acc -= Yo;
                if ((jp << c2) > kJ) continue;   // j = j' 2^c2 beyond the bound
                for (int sign = 0; sign < 2; ++sign) {
                    uint64_t X = sign == 0 ? acc : (acc == 0 ? 0 : Yo - acc);   // +-j' inv (mod Yo), below Yo < 2^53
                    for (int m = 0; m < kMaxSolutions; ++m, X += Yo) {
                        if (X >= (1ull << 53)) break;
                        if (X < (1ull << 52)) continue;
                        const double n = from_bits((X & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);   // X 2^-52
                        const double ieee = n / ds;
                        for (int v = 0; v < kVariants; ++v) ok[v] = ok[v] && quotient(n, zhs, zls[v]) == ieee;
                    }
                }
            }
        }
    }
    c.variant = -1;
    for (int v = kVariants - 1; v >= 0; --v)
        if (ok[v]) c.variant = v;
    if (c.variant < 0) return c;
    // back to d's exponent: the stored constants are the tried ones times an exact power of two
    const double back = from_bits((uint64_t)(2046 - ((db >> 52) & 0x7FFull)) << 52);   // 2^-exponent(d)
    c.zh = zhs * back;
    c.zl = zls[c.variant] * back;
    return c;
}

}  // namespace pairdiv
}  // namespace rscm
