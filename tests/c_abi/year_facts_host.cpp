// rscm::tl::YearFacts (rscm_amd/csrc/two_layer_year_facts.hpp) on the host: the two facts an EXACT two-layer launch is told about its
// years, the common sub-step count and whether every forcing value it can read lies in the chunk guard's forcing box.  The header is
// host-only; nothing else of the project is compiled and no HIP library is linked.  Built with -fsanitize=address,undefined by
// tests/test_host_year_facts.py.  Exit status 0 and "year_facts ok" on stdout if every check holds, else the failed checks on stderr
// and exit status 1.
#include "two_layer_year_facts.hpp"

#include <cstdio>
#include <limits>
#include <vector>

namespace {

int g_failed = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

using rscm::tl::YearFacts;
namespace chunk = rscm::tl::chunk;

// the box's edges as the kernel's check draws them: the header's constants, nothing restated
const double kLo = std::ldexp(1.0, chunk::kForcingLo), kHi = std::ldexp(1.0, chunk::kForcingHi);

struct Edge {
    double value;
    bool inside;
};
std::vector<Edge> edges()
{
    const double inf = std::numeric_limits<double>::infinity();
    return {{0.0, true},
            {-0.0, false},
            {kHi, false},
            {-kHi, false},
            {std::nextafter(kHi, 0.0), true},
            {-std::nextafter(kHi, 0.0), true},
            {kLo, true},
            {-kLo, true},
            {std::nextafter(kLo, 0.0), false},
            {std::numeric_limits<double>::denorm_min(), false},
            {-std::numeric_limits<double>::denorm_min(), false},
            {std::numeric_limits<double>::min() / 2.0, false},
            {1e300, false},
            {-1e300, false},
            {inf, false},
            {-inf, false},
            {std::numeric_limits<double>::quiet_NaN(), false},
            {1.0, true},
            {-3.7, true}};
}

void schedule()
{
    YearFacts f;
    CHECK(f.nsub_uniform(0, 1) == 0);   // no schedule yet
    const std::vector<int32_t> annual(12, 10);
    f.set_schedule(annual.data(), annual.size());
    CHECK(f.nsub_uniform(0, 12) == 10);
    CHECK(f.nsub_uniform(0, 0) == 0 && f.nsub_uniform(5, 5) == 0 && f.nsub_uniform(12, 12) == 0);   // empty ranges
    CHECK(f.nsub_uniform(7, 3) == 0 && f.nsub_uniform(-1, 3) == 0 && f.nsub_uniform(0, 13) == 0);    // no range of the axis
    for (int32_t k = 0; k < 12; ++k) CHECK(f.nsub_uniform(k, k + 1) == 10);                           // one-step ranges

    // a differing count at the first position, the last position and one past the range
    for (int32_t at = 0; at < 12; ++at) {
        std::vector<int32_t> n(12, 10);
        n[(size_t)at] = 5;
        f.set_schedule(n.data(), n.size());
        for (int32_t b = 0; b < 12; ++b)
            for (int32_t e = b + 1; e <= 12; ++e) {
                const bool holds_it = at >= b && at < e;
                const int32_t want = !holds_it ? 10 : (e - b == 1 ? 5 : 0);
                CHECK(f.nsub_uniform(b, e) == want);
            }
    }
    {
        std::vector<int32_t> n(12, 10);
        n[3] = 5;
        f.set_schedule(n.data(), n.size());
        CHECK(f.nsub_uniform(3, 8) == 0);    // first position of the range
        CHECK(f.nsub_uniform(0, 4) == 0);    // last position
        CHECK(f.nsub_uniform(0, 3) == 10);   // one past the range
        CHECK(f.nsub_uniform(4, 12) == 10);  // one before it
    }
    // a uniform count other than the annual one is reported as it is; two values that alternate never are uniform over two steps
    const std::vector<int32_t> twenty(6, 20);
    f.set_schedule(twenty.data(), twenty.size());
    CHECK(f.nsub_uniform(0, 6) == 20 && f.nsub_uniform(2, 5) == 20);
    const std::vector<int32_t> alt = {10, 20, 10, 20, 10};
    f.set_schedule(alt.data(), alt.size());
    CHECK(f.nsub_uniform(0, 5) == 0 && f.nsub_uniform(1, 3) == 0 && f.nsub_uniform(0, 3) == 0 && f.nsub_uniform(2, 3) == 10);
    // a new schedule replaces the old one, a dropped one answers nothing
    f.set_schedule(annual.data(), annual.size());
    CHECK(f.nsub_uniform(0, 12) == 10);
    f.drop_schedule();
    CHECK(f.nsub_uniform(0, 12) == 0);
}

void forcing_values()
{
    for (const Edge& e : edges()) CHECK(rscm::tl::forcing_value_boxed(e.value) == e.inside);
}

void forcing_ranges()
{
    constexpr int32_t T = 13;   // 12 steps
    YearFacts f;
    CHECK(!f.forcing_boxed(0, 12, 0));   // no table yet
    std::vector<double> good((size_t)T);
    for (int32_t t = 0; t < T; ++t) good[(size_t)t] = t % 3 == 0 ? 0.0 : 0.25 * t - 1.0;
    good[4] = 0.0;   // (0.25 * 4 - 1 is +0 anyway)
    f.set_forcing(good.data(), 1, T);
    for (int32_t off = 0; off <= 1; ++off) {
        CHECK(f.forcing_boxed(0, 12, off));
        CHECK(!f.forcing_boxed(0, 0, off) && !f.forcing_boxed(12, 12, off) && !f.forcing_boxed(5, 4, off));   // empty ranges
        CHECK(!f.forcing_boxed(-1, 4, off));
        for (int32_t k = 0; k < 12; ++k) CHECK(f.forcing_boxed(k, k + 1, off));                               // one-step ranges
    }
    // an index past the table is never vouched for (index 12 is the table's last: a range may read it, none may read 13)
    CHECK(f.forcing_boxed(0, 13, 0) && !f.forcing_boxed(0, 13, 1) && !f.forcing_boxed(0, 12, 2) && !f.forcing_boxed(0, 14, 0));
    CHECK(!f.forcing_boxed(0, 12, -1));

    // every edge value at every index: a range is boxed exactly when it does not read that index -- indices
    // [begin + off, end - 1 + off], whose last is also what the look-ahead of the range's last year is clamped to
    for (const Edge& e : edges())
        for (int32_t at = 0; at < T; ++at) {
            std::vector<double> tab = good;
            tab[(size_t)at] = e.value;
            f.set_forcing(tab.data(), 1, T);
            for (int32_t off = 0; off <= 1; ++off)
                for (int32_t b = 0; b < 12; ++b)
                    for (int32_t en = b + 1; en <= 12; ++en) {
                        const bool reads_it = at >= b + off && at <= en - 1 + off;
                        CHECK(f.forcing_boxed(b, en, off) == (e.inside || !reads_it));
                    }
        }

    // a run in three pieces whose boundary falls on the bad index: with src_off 0 index 4 belongs to [4, 8) only; with src_off 1 it
    // is the last index [0, 4) reads (its look-ahead) and [4, 8) starts past it
    {
        std::vector<double> tab = good;
        tab[4] = -0.0;
        f.set_forcing(tab.data(), 1, T);
        CHECK(f.forcing_boxed(0, 4, 0) && !f.forcing_boxed(4, 8, 0) && f.forcing_boxed(8, 12, 0));
        CHECK(!f.forcing_boxed(0, 4, 1) && f.forcing_boxed(4, 8, 1) && f.forcing_boxed(8, 12, 1));
    }

    // several scenarios: one bad value in any row spoils its index for all
    for (int32_t row = 0; row < 3; ++row) {
        std::vector<double> tab;
        for (int32_t s = 0; s < 3; ++s) tab.insert(tab.end(), good.begin(), good.end());
        f.set_forcing(tab.data(), 3, T);
        CHECK(f.forcing_boxed(0, 12, 0) && f.forcing_boxed(0, 12, 1));
        tab[(size_t)row * T + 7] = std::numeric_limits<double>::quiet_NaN();
        f.set_forcing(tab.data(), 3, T);
        CHECK(!f.forcing_boxed(0, 12, 0) && !f.forcing_boxed(7, 8, 0) && !f.forcing_boxed(6, 7, 1));
        CHECK(f.forcing_boxed(0, 7, 0) && f.forcing_boxed(8, 12, 0) && f.forcing_boxed(7, 12, 1) && f.forcing_boxed(0, 6, 1));
    }

    // a new table replaces the verdict both ways, a dropped one answers nothing
    std::vector<double> bad = good;
    bad[0] = 1e300;
    f.set_forcing(good.data(), 1, T);
    CHECK(f.forcing_boxed(0, 12, 0));
    f.set_forcing(bad.data(), 1, T);
    CHECK(!f.forcing_boxed(0, 12, 0) && f.forcing_boxed(0, 12, 1));
    f.set_forcing(good.data(), 1, T);
    CHECK(f.forcing_boxed(0, 12, 0));
    f.drop_forcing();
    CHECK(!f.forcing_boxed(0, 12, 0) && !f.forcing_boxed(3, 4, 1));
    // a shorter table after a longer one
    f.set_forcing(good.data(), 1, 5);
    CHECK(f.forcing_boxed(0, 4, 0) && f.forcing_boxed(0, 4, 1) && !f.forcing_boxed(0, 5, 1) && !f.forcing_boxed(0, 12, 0));
}

}  // namespace

int main()
{
    schedule();
    forcing_values();
    forcing_ranges();
    if (g_failed) {
        std::fprintf(stderr, "year_facts: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("year_facts ok\n");
    return 0;
}
