// The bin of a value among ascending edges (rscm_amd/csrc/histogram_bin.hpp) on the host: this program includes that header alone and
// links nothing of the project.  Built with -fsanitize=address,undefined by tests/test_histogram_cpu.py as a stand-alone program.
// For E = 2, 3, 9, 64, 65 and 1025 edges -- in heap arrays of exactly E doubles, so that a read past either end is caught -- it
// compares histogram_count_le and histogram_slot with a linear scan of the comparison definition (include/rscm_gpu.h) on every edge,
// its two neighbouring doubles, both zeros, both infinities, the largest and smallest finite doubles and random values.  Three edge
// tables per E: random edges around an edge at 0.0, neighbouring doubles (every gap one ulp), and equally spaced edges.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "histogram_bin.hpp"

namespace {

long long checked = 0;

// the comparison definition, edge by edge
int32_t scan_slot(const double* e, int32_t E, double v)
{
    const int32_t B = E - 1;
    int32_t k = 0;
    for (int32_t j = 0; j < E; ++j)
        if (e[j] <= v) ++k;
    if (k == 0) return B;
    if (k <= B) return k - 1;
    return v == e[B] ? B - 1 : B + 1;
}

bool check(const double* e, int32_t E, double v, const char* table)
{
    const int32_t top = rscm::histogram_top_stride(E);
    int32_t k = 0;
    for (int32_t j = 0; j < E; ++j)
        if (e[j] <= v) ++k;
    const int32_t got_k = rscm::histogram_count_le(e, E, top, v), got = rscm::histogram_slot(e, E, top, v), want = scan_slot(e, E, v);
    ++checked;
    if (got_k == k && got == want) return true;
    std::printf("E = %d (%s), v = %a: count %d, slot %d; the scan says %d, %d\n", E, table, v, got_k, got, k, want);
    return false;
}

bool check_table(const std::vector<double>& edges, const char* table, std::mt19937_64& rng)
{
    const int32_t E = (int32_t)edges.size();
    double* e = new double[(size_t)E];   // exactly E doubles on the heap
    for (int32_t j = 0; j < E; ++j) e[j] = edges[(size_t)j];
    const double inf = std::numeric_limits<double>::infinity(), big = std::numeric_limits<double>::max();
    bool ok = true;
    for (int32_t j = 0; j < E; ++j) {
        ok &= check(e, E, e[j], table);
        ok &= check(e, E, std::nextafter(e[j], -inf), table);
        ok &= check(e, E, std::nextafter(e[j], inf), table);
    }
    for (double v : {0.0, -0.0, inf, -inf, big, -big, std::numeric_limits<double>::denorm_min(), -std::numeric_limits<double>::denorm_min()})
        ok &= check(e, E, v, table);
    std::uniform_real_distribution<double> inside(e[0], e[E - 1]), around(2.0 * e[0] - e[E - 1], 2.0 * e[E - 1] - e[0]);
    for (int i = 0; i < 2000; ++i) {
        ok &= check(e, E, inside(rng), table);
        ok &= check(e, E, around(rng), table);
    }
    delete[] e;
    return ok;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20240611);
    bool ok = true;
    for (int32_t E : {2, 3, 9, 64, 65, 1025}) {
        if (rscm::histogram_top_stride(E) > E || 2 * rscm::histogram_top_stride(E) <= E) {
            std::printf("E = %d: top stride %d\n", E, rscm::histogram_top_stride(E));
            ok = false;
        }
        // random ascending edges with an edge at 0.0 in the middle
        std::vector<double> random_edges((size_t)E);
        std::uniform_real_distribution<double> gap(1e-3, 1.0);
        const int32_t mid = E / 2;
        random_edges[(size_t)mid] = 0.0;
        for (int32_t j = mid + 1; j < E; ++j) random_edges[(size_t)j] = random_edges[(size_t)j - 1] + gap(rng);
        for (int32_t j = mid - 1; j >= 0; --j) random_edges[(size_t)j] = random_edges[(size_t)j + 1] - gap(rng);
        ok &= check_table(random_edges, "random", rng);
        // neighbouring doubles: an edge's neighbour is the next edge
        std::vector<double> ulp_edges((size_t)E);
        ulp_edges[0] = 1.5;
        for (int32_t j = 1; j < E; ++j) ulp_edges[(size_t)j] = std::nextafter(ulp_edges[(size_t)j - 1], 4.0);
        ok &= check_table(ulp_edges, "one ulp apart", rng);
        // equally spaced
        std::vector<double> even_edges((size_t)E);
        for (int32_t j = 0; j < E; ++j) even_edges[(size_t)j] = -3.0 + 0.125 * j;
        ok &= check_table(even_edges, "equally spaced", rng);
    }
    if (!ok) return 1;
    std::printf("histogram_bin ok (%lld values)\n", checked);
    return 0;
}
