// rscm_amd/csrc/pair_div_verdict.hpp compiled on its own, as host code: reads divisors (raw little-endian doubles) from the file named
// by its argument and prints, per divisor, "<divisor bits> <zh bits> <zl bits> <variant>" in hexadecimal -- the constants and the verdict
// the device forms per member.  With a second argument "flags" (instead of "rows"): one line with one character per divisor, '1' safe
// and '0' not.  A third argument is the lower edge, as a binary exponent, of the numerator window the verdict is asked for.
// tests/test_pair_div_verdict.py compares the output with scripts/pair_div_proof.py's integer restatement and builds this file with
// AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pair_div_verdict.hpp"

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s FILE [rows|flags] [num_lo]\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<double> d;
    double buf[1024];
    for (size_t got; (got = std::fread(buf, sizeof(double), 1024, f)) > 0;) d.insert(d.end(), buf, buf + got);
    std::fclose(f);
    const bool flags = argc > 2 && std::strcmp(argv[2], "flags") == 0;
    const int num_lo = argc > 3 ? std::atoi(argv[3]) : rscm::pairdiv::kNumLo;
    std::string line;
    for (double x : d) {
        const rscm::pairdiv::Constants c = rscm::pairdiv::verdict(x, num_lo);
        if (flags) {
            line.push_back(c.zh != 0.0 ? '1' : '0');
            continue;
        }
        std::printf("%016llx %016llx %016llx %d\n", (unsigned long long)rscm::pairdiv::bits_of(x), (unsigned long long)rscm::pairdiv::bits_of(c.zh),
                    (unsigned long long)rscm::pairdiv::bits_of(c.zl), (int)c.variant);
    }
    if (flags) std::printf("%s\n", line.c_str());
    return 0;
}
