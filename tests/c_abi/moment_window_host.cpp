// The integer pieces of the moments of stored rows (rscm_amd/csrc/moment_window.hpp) on the host, alone: no HIP, no library of the
// project.  A wave of 64 lanes is played in plain C++: every lane owns a window, tiles of 64 terms arrive, the window's base follows
// the rule of moment_rows.hip (it moves when a term lies above it or every term of the tile below it; a move folds first), terms below
// the window are placed directly as the serial walk does.  After every sequence the fold's 68 limbs and the direct placement of the
// same terms (mom_place) must be the same canonical integer.  Built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_host_moment_window.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "moment_window.hpp"

namespace {

using namespace rscm;

struct Term {
    uint64_t bits, w;
};

uint64_t bits_of(double x)
{
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    return b;
}

// the canonical integer of 68 limbs as 70 digits of 32 bits, two's complement
void canonical(const int64_t* limbs, uint32_t (&dig)[70])
{
    __int128 carry = 0;
    for (int k = 0; k < 70; ++k) {
        const __int128 t = carry + (k < kMomWinLimbs ? (__int128)limbs[k] : (__int128)0);
        dig[k] = (uint32_t)((unsigned __int128)t & 0xFFFFFFFFu);
        carry = (t - (__int128)dig[k]) / ((__int128)1 << 32);
    }
}

struct Wave {
    uint64_t win[64][kMomWin] = {};
    uint32_t n_neg[64] = {};
    int base = -1;
    int64_t folded[kMomWinLimbs] = {};
    long n_window = 0, n_walked = 0, n_rebase = 0;

    void fold()
    {
        uint64_t slot_sum[kMomWin] = {};
        for (int l = 0; l < 64; ++l) {
            mom_window_settle(win[l], n_neg[l]);
            for (int j = 0; j < kMomWin; ++j) slot_sum[j] += win[l][j], win[l][j] = 0;
            n_neg[l] = 0;
        }
        mom_window_fold(slot_sum, base, folded);
    }

    // one tile: up to 64 terms, lane l takes term l
    void tile(const Term* t, int n, int64_t* direct)
    {
        uint64_t lo[64], hi[64];
        uint32_t pos[64], neg[64];
        bool valid[64];
        int qmax = -1;
        bool above = false, any_inside = false, any = false;
        for (int l = 0; l < n; ++l) {
            uint64_t mant;
            const bool finite = mom_fields(t[l].bits, mant, pos[l], neg[l]);
            mom_product(t[l].w, mant, lo[l], hi[l]);
            valid[l] = finite && (lo[l] | hi[l]) != 0;
            if (!valid[l]) continue;
            const int q = (int)(pos[l] >> 5);
            uint32_t d[5];
            mom_digits(lo[l], hi[l], pos[l] & 31u, d);
            mom_place(d, q, neg[l], direct);
            any = true;
            qmax = q > qmax ? q : qmax;
            above = above || q > base + kMomWinSpan;
            any_inside = any_inside || q >= base;
        }
        if (!any) return;
        if (base < 0 || above || !any_inside) {
            const int nb = mom_window_base(qmax);
            if (base >= 0 && nb != base) {
                fold();
                ++n_rebase;
            }
            base = nb;
        }
        for (int l = 0; l < n; ++l) {
            if (!valid[l]) continue;
            const int q = (int)(pos[l] >> 5);
            uint32_t d[5];
            mom_digits(lo[l], hi[l], pos[l] & 31u, d);
            if (mom_window_holds(base, q)) {
                mom_window_add(win[l], n_neg[l], d, (uint32_t)(q - base), neg[l]);
                ++n_window;
            } else if (q < base) {
                mom_place(d, q, neg[l], folded);   // the walk
                ++n_walked;
            } else {
                std::printf("a term above the window after the rebase: q %d base %d\n", q, base);
                ++n_window;   // counted, never added: the comparison fails
            }
        }
    }
};

int n_bad = 0, n_seq = 0;

// runs the terms through a wave in tiles of `tile` terms and compares; returns the wave for its counters
Wave run(const char* name, const std::vector<Term>& terms, int tile = 64)
{
    Wave w;
    std::vector<int64_t> direct(kMomWinLimbs, 0);
    for (size_t i = 0; i < terms.size(); i += (size_t)tile)
        w.tile(&terms[i], (int)(terms.size() - i < (size_t)tile ? terms.size() - i : (size_t)tile), direct.data());
    if (w.base >= 0) w.fold();
    uint32_t a[70], b[70];
    canonical(w.folded, a);
    canonical(direct.data(), b);
    if (std::memcmp(a, b, sizeof a) != 0) {
        std::printf("%s: the fold and the direct placement differ\n", name);
        ++n_bad;
    }
    ++n_seq;
    return w;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

double pow2(int e)   // 2^e for -1074 <= e <= 1023, from the fields
{
    const uint64_t b = e >= -1022 ? (uint64_t)(e + 1023) << 52 : uint64_t(1) << (e + 1074);
    double x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

}  // namespace

int main()
{
    const uint64_t w_max = (uint64_t(1) << 53) - 1;
    const double dbl_max = 1.7976931348623157e308, sub_min = 4.9406564584124654e-324;

    // one term at a time: every edge value, both signs, the smallest and the largest weight
    for (double x : {sub_min, 2.2250738585072009e-308 /* largest subnormal */, 2.2250738585072014e-308, 1.0, 1.5, 3.999999999999999, dbl_max,
                     pow2(-1074 + 17), pow2(-1022 + 18), pow2(0 - 13 + 32), pow2(1023)})
        for (int sign = 0; sign < 2; ++sign)
            for (uint64_t w : {uint64_t(1), uint64_t(3), w_max}) {
                std::vector<Term> t{{bits_of(sign ? -x : x), w}};
                const Wave r = run("single term", t);
                if (r.n_window != 1 || r.n_walked != 0) ++n_bad;
            }
    // q at both edges of the window and just outside: a first tile places the base at q0 - 2, the second brings one term each at
    // q = base - 1 (walked), base, base + 3 (inside) and base + 4 (the window moves)
    for (int q0 : {2, 3, 10, 34, 40, 62, 64}) {
        auto at_q = [](int q, int r, bool neg) {   // a double whose mantissa's lowest bit sits at accumulator bit 32 q + r
            const int e = 32 * q + r - 13;   // pos = E + 13 for 1 <= E <= 2046 (the callers keep to that)
            return ((uint64_t)e << 52) | 0xFFFFFFFFFFFFFull | ((uint64_t)neg << 63);
        };
        for (int r : {0, 1, 18, 31})
            for (int neg = 0; neg < 2; ++neg) {
                if (32 * q0 + r - 13 > 2046 || 32 * q0 + r < 14) continue;
                const int base = mom_window_base(q0);
                std::vector<Term> t(64, Term{at_q(q0, r, neg != 0), 5});
                std::vector<int> qs{base, base + kMomWinSpan};
                if (base >= 1) qs.push_back(base - 1);
                for (int q : qs)
                    if (32 * q + r >= 14 && 32 * q + r - 13 <= 2046) t.push_back(Term{at_q(q, r, neg == 0), w_max});
                const Wave a = run("window edges", t);
                if (a.n_rebase != 0 || (base >= 1 && 32 * (base - 1) + r >= 14 && a.n_walked != 1)) ++n_bad;
                if (32 * (base + kMomWinSpan + 1) + r - 13 <= 2046) {
                    t.resize(64);
                    t.push_back(Term{at_q(base + kMomWinSpan + 1, r, neg == 0), w_max});
                    const Wave b = run("just above the window", t);
                    if (b.n_rebase != 1 || b.n_walked != 0) ++n_bad;
                }
            }
    }
    // random terms over the whole range of doubles, random weights up to 2^53 - 1, tiles of several sizes: windows, walks and rebases mix
    for (int rep = 0; rep < 40; ++rep) {
        std::vector<Term> t;
        const int n = 64 * 3 + (int)(rnd() % 200);
        for (int i = 0; i < n; ++i) {
            uint64_t b = rnd();
            if (((b >> 52) & 0x7FF) == 0x7FF) b &= ~(uint64_t(1) << 62);        // finite
            if (rep % 4 == 1) b = (b & ~(uint64_t(0x7FF) << 52)) | (uint64_t(1020 + rnd() % 8) << 52);   // a narrow band: all inside
            if (rep % 4 == 2 && i % 7 == 0) b &= (uint64_t(1) << 63) | 0xFFFFFFFFFFFFFull;               // subnormals among them
            const uint64_t w = rep % 3 == 0 ? 1 : rep % 3 == 1 ? rnd() % 9 : rnd() & w_max;              // zero weights too
            t.push_back(Term{b, w});
        }
        const Wave r = run("random terms", t, rep % 5 == 0 ? 17 : 64);
        if (rep % 4 == 1 && r.n_walked != 0) {
            std::printf("a narrow band of exponents walked %ld terms\n", r.n_walked);
            ++n_bad;
        }
    }
    // a sequence that rebases up and down: tiles of 2^-1074, 1, 1e300-sized, 1, 2^-1000, each repeated, negative and positive mixed
    {
        std::vector<Term> t;
        const double levels[] = {sub_min, 1.0, pow2(996), 1.25, pow2(-1000), pow2(1023), sub_min};
        for (double x : levels)
            for (int i = 0; i < 128; ++i) t.push_back(Term{bits_of(i % 3 ? x : -x), (uint64_t)(1 + i % 8)});
        const Wave r = run("up and down", t);
        if (r.n_rebase != 6 || r.n_walked != 0 || r.n_window != (long)t.size()) {
            std::printf("up and down: %ld rebases, %ld walked, %ld in the window\n", r.n_rebase, r.n_walked, r.n_window);
            ++n_bad;
        }
        // the same levels mixed inside every tile: the window sits at the top, everything else walks
        std::vector<Term> m;
        for (int i = 0; i < 128; ++i)
            for (double x : levels) m.push_back(Term{bits_of(i % 2 ? x : -x), w_max});
        const Wave s = run("mixed levels", m);
        if (s.n_walked == 0 || s.n_window == 0) ++n_bad;
    }
    // many negative terms in one lane's slots: the deferred correction of the sign
    {
        std::vector<Term> t(64 * 50, Term{bits_of(-3.75), w_max});
        run("all negative", t);
    }
    if (n_bad) return 1;
    std::printf("moment_window ok (%d sequences)\n", n_seq);
    return 0;
}
