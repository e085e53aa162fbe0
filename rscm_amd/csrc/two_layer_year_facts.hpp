// What the host proves once about the years of an EXACT two-layer launch, so that the kernel need not find it out per year
// (two_layer_body.hpp, the uniform year; TwoLayerArgs::year_facts, rscm_device.hpp):
//   nsub_uniform     the RK4 sub-step count that every step of [step_begin, step_end) has, 0 if they differ
//   forcing_boxed    every forcing value the launch can read -- all scenarios, forcing-axis indices step_begin + src_off through
//                    step_end - 1 + src_off, the look-ahead's clamp included -- is +0 or a magnitude in the chunk guard's forcing box
//                    (two_layer_chunk_box.hpp; the kernel's box::forcing_in with those edges).  -0, denormals, Inf and NaN are outside.
// Both are answered in O(1) from prefix counts: the schedule's when the schedule is built (kind_config.cpp, refresh_schedule), the table's
// when rscm_ens_set_forcing is handed the caller's array; the table's verdict is dropped before anything can change the table.
// Host only, no HIP: tests/c_abi/year_facts_host.cpp compiles this header on its own.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "two_layer_chunk_box.hpp"

namespace rscm {
namespace tl {

// +0, or a magnitude in the chunk forcing box [2^kForcingLo, 2^kForcingHi): the host's statement of box::forcing_in
inline bool forcing_value_boxed(double f)
{
    uint64_t bits;
    std::memcpy(&bits, &f, sizeof bits);
    if (bits == 0) return true;
    const double m = std::fabs(f);   // (NaN fails both comparisons)
    return m >= std::ldexp(1.0, chunk::kForcingLo) && m < std::ldexp(1.0, chunk::kForcingHi);
}

struct YearFacts {
    // breaks[k]: how many j in [1, k] have nsub[j] != nsub[j - 1]; empty: no schedule
    std::vector<int32_t> breaks;
    std::vector<int32_t> nsub;
    // outside[t]: how many forcing-axis indices below t hold a value outside the box in some scenario ([T + 1]); empty: no verdict
    std::vector<int32_t> outside;

    void set_schedule(const int32_t* sub_steps, size_t n)
    {
        nsub.assign(sub_steps, sub_steps + n);
        breaks.assign(n, 0);
        for (size_t k = 1; k < n; ++k) breaks[k] = breaks[k - 1] + (nsub[k] != nsub[k - 1] ? 1 : 0);
    }
    void drop_schedule()
    {
        nsub.clear();
        breaks.clear();
    }
    // a plain table [n_scen][n_times] as the caller passed it
    void set_forcing(const double* table, int32_t n_scen, int32_t n_times)
    {
        outside.assign((size_t)n_times + 1, 0);
        for (int32_t t = 0; t < n_times; ++t) {
            bool in = true;
            for (int32_t s = 0; s < n_scen && in; ++s) in = forcing_value_boxed(table[(size_t)s * n_times + t]);
            outside[(size_t)t + 1] = outside[(size_t)t] + (in ? 0 : 1);
        }
    }
    void drop_forcing() { outside.clear(); }

    int32_t nsub_uniform(int32_t step_begin, int32_t step_end) const
    {
        if (step_begin < 0 || step_end <= step_begin || (size_t)step_end > nsub.size()) return 0;
        if (breaks[(size_t)step_end - 1] != breaks[(size_t)step_begin]) return 0;
        return nsub[(size_t)step_begin] > 0 ? nsub[(size_t)step_begin] : 0;
    }
    bool forcing_boxed(int32_t step_begin, int32_t step_end, int32_t src_off) const
    {
        if (step_begin < 0 || step_end <= step_begin || src_off < 0) return false;
        const int64_t lo = (int64_t)step_begin + src_off, hi = (int64_t)step_end - 1 + src_off;
        if (outside.empty() || hi + 1 >= (int64_t)outside.size()) return false;
        return outside[(size_t)hi + 1] == outside[(size_t)lo];
    }
};

}  // namespace tl
}  // namespace rscm
