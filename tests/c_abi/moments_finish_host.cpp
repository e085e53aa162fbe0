// rscm::moment_finish (rscm_amd/csrc/moments_finish.hpp) on the host, alone: no HIP, no library of the project.  Reads the cases of
// tests/host_moments.finish_cases from the file named on the command line -- per line: divisor, n_terms, the expected return code,
// the expected double as 16 hex digits, then the 69 int64 of the block -- and compares bit for bit (any NaN for a NaN).  Built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_host_moments_finish.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "moments_finish.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n_cases = 0, n_bad = 0;
    for (;;) {
        long long divisor, n_terms;
        int want_rc;
        unsigned long long want_bits;
        if (std::fscanf(f, "%lld %lld %d %llx", &divisor, &n_terms, &want_rc, &want_bits) != 4) break;
        std::vector<int64_t> block(rscm::kMomentBlock);
        for (auto& x : block) {
            long long v;
            if (std::fscanf(f, "%lld", &v) != 1) return 2;
            x = v;
        }
        const int64_t d = divisor;
        double got = 0.0, want;
        const uint64_t wb = want_bits;
        std::memcpy(&want, &wb, sizeof want);
        const int rc = rscm::moment_finish(block.data(), 1, &d, n_terms, &got);
        uint64_t gb;
        std::memcpy(&gb, &got, sizeof gb);
        const bool same = rc == want_rc && (rc != 0 || gb == wb || (got != got && want != want));
        if (!same) {
            std::printf("case %d: rc %d (want %d), got %016" PRIx64 " want %016" PRIx64 "\n", n_cases, rc, want_rc, gb, wb);
            ++n_bad;
        }
        ++n_cases;
    }
    std::fclose(f);
    // several blocks in one call, each with its own divisor; and no block at all
    {
        std::vector<int64_t> blocks(3 * rscm::kMomentBlock, 0);
        blocks[0 * rscm::kMomentBlock + 34] = 3;    // 3 * 2^(32 * 34 - 1088) = 3
        blocks[1 * rscm::kMomentBlock + 34] = -1;
        blocks[2 * rscm::kMomentBlock + 34] = 1, blocks[2 * rscm::kMomentBlock + rscm::kMomentLimbs] = 1;
        const int64_t div[3] = {2, 4, 1};
        double out[3] = {0, 0, 0};
        if (rscm::moment_finish(blocks.data(), 3, div, 3, out) != 0 || out[0] != 1.5 || out[1] != -0.25 || out[2] == out[2]) {
            std::printf("three blocks: %g %g %g\n", out[0], out[1], out[2]);
            ++n_bad;
        }
        if (rscm::moment_finish(nullptr, 0, nullptr, 0, nullptr) != 0) ++n_bad;
        if (rscm::moment_finish(nullptr, 1, div, 0, out) != 1 || rscm::moment_finish(blocks.data(), -1, div, 0, out) != 1) ++n_bad;
    }
    if (n_bad || n_cases == 0) return 1;
    std::printf("moments_finish ok (%d cases)\n", n_cases);
    return 0;
}
