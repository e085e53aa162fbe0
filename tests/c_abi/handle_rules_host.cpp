// The two host-only descriptions a handle's rules read (rscm_amd/csrc): the table of structural parameter rows (structural_rows.hpp)
// and the internal component state as runs of rows (internal_state.hpp).  Nothing else of the project is compiled and no HIP library is
// linked.  Built with -fsanitize=address,undefined by tests/test_host_handle_rules.py, which compares the printed table ("<kind> <row>
// <name>" lines) with tests/param_rows.py.  Exit status 0 and "handle_rules ok" on stdout if every check holds, else the failed
// checks on stderr and exit status 1.
#include "internal_state.hpp"
#include "structural_rows.hpp"

#include <cstdio>
#include <set>
#include <utility>
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

using rscm::StateBuf;
using rscm::StateRuns;
using rscm::StateShape;

void structural_table()
{
    std::set<std::pair<int, int>> seen;
    int n2o = 0;
    for (const rscm::StructuralRow& s : rscm::kStructuralRows) {
        CHECK(s.kind >= 0 && s.kind < rscm::kNumKinds);
        CHECK(s.row >= 0 && s.row < rscm::kKinds[s.kind].n_params);
        CHECK(seen.insert({s.kind, s.row}).second);
        CHECK(s.name && s.name[0]);
        CHECK(structural_row(s.kind, s.row) == s.name);
        // the N2O delay is the one row that may vary over the members
        CHECK(s.uniform == (s.kind != RSCM_KIND_N2O_CHEMISTRY));
        n2o += s.kind == RSCM_KIND_N2O_CHEMISTRY;
        std::printf("%d %d %s\n", s.kind, s.row, s.name);
    }
    CHECK(n2o == 1);
    // nothing else is structural
    for (int kind = 0; kind < rscm::kNumKinds; ++kind)
        for (int row = 0; row < rscm::kKinds[kind].n_params; ++row)
            CHECK((structural_row(kind, row) != nullptr) == (seen.count({kind, row}) == 1));
    CHECK(structural_row(RSCM_KIND_UDEB, -1) == nullptr && structural_row(-1, 0) == nullptr && structural_row(rscm::kNumKinds, 0) == nullptr);
}

void udeb_state()
{
    const int32_t T = 40, scalars = 7;
    for (int32_t layers : {2, 50, 65})
        for (int32_t k : {0, 1, T - 1}) {
            const StateRuns r = rscm::internal_state_runs(RSCM_KIND_UDEB, k, StateShape{layers, scalars, 0, 0});
            CHECK(r.n == 3);
            CHECK(r.run[0].buf == StateBuf::UdebColumns && r.run[0].first == 0 && r.run[0].count == 2 * layers);
            CHECK(r.run[1].buf == StateBuf::UdebScalars && r.run[1].first == 0 && r.run[1].count == scalars);
            CHECK(r.run[2].buf == StateBuf::UdebHistory && r.run[2].first == 0 && r.run[2].count == k + 1);
            CHECK(r.rows() == 2 * layers + scalars + k + 1);
        }
    CHECK(rscm::internal_state_runs(RSCM_KIND_UDEB, 3, StateShape{0, scalars, 0, 0}).n == 0);   // no columns yet: no state
}

// the pulses still held, oldest first, one row at a time: the branch's formulation before the runs
std::vector<int64_t> ring_rows_one_by_one(int64_t total, int64_t R)
{
    const int64_t cnt = total < R ? total : R, first = cnt > 0 ? (total - cnt) % R : 0;
    std::vector<int64_t> rows;
    for (int64_t i = 0; i < cnt; ++i) rows.push_back((first + i) % R);
    return rows;
}

void ocean_ring()
{
    const int32_t steps = 12;
    const int64_t R = 72;
    struct Case { int64_t pulses; int32_t runs; };
    // nothing taken; the ring not yet full; exactly full; the first wrap; gone round many times
    for (const Case& c : {Case{0, 0}, Case{12, 1}, Case{R, 1}, Case{R + 12, 2}, Case{5 * R + 24, 2}}) {
        CHECK(c.pulses % steps == 0);
        const int32_t k = (int32_t)(c.pulses / steps);
        const StateRuns r = rscm::internal_state_runs(RSCM_KIND_OCEAN_CARBON, k, StateShape{0, 0, steps, R});
        CHECK(r.n == c.runs && r.n <= 2);
        std::vector<int64_t> rows;
        for (const rscm::StateRun& run : r) {
            CHECK(run.buf == StateBuf::OceanRing && run.count > 0 && run.first >= 0 && run.first + run.count <= R);
            for (int64_t i = 0; i < run.count; ++i) rows.push_back(run.first + i);
        }
        CHECK(rows == ring_rows_one_by_one(c.pulses, R));
        CHECK(r.rows() == (c.pulses < R ? c.pulses : R) && (int64_t)rows.size() == r.rows());
        CHECK(std::set<int64_t>(rows.begin(), rows.end()).size() == rows.size());
    }
    CHECK(rscm::internal_state_runs(RSCM_KIND_OCEAN_CARBON, 3, StateShape{0, 0, steps, 0}).n == 0);   // no ring yet: no state
}

void other_kinds()
{
    int with_state = 0;
    for (int kind = 0; kind < rscm::kNumKinds; ++kind) {
        const StateRuns r = rscm::internal_state_runs(kind, 5, StateShape{50, 7, 12, 72});
        CHECK((r.n > 0) == rscm::kKinds[kind].internal_state);
        CHECK(rscm::kKinds[kind].internal_state == (kind == RSCM_KIND_UDEB || kind == RSCM_KIND_OCEAN_CARBON));
        with_state += r.n > 0;
    }
    CHECK(with_state == 2);
    CHECK(rscm::internal_state_runs(-1, 5, StateShape{50, 7, 12, 72}).n == 0 && rscm::internal_state_runs(rscm::kNumKinds, 5, StateShape{50, 7, 12, 72}).n == 0);
}

}  // namespace

int main()
{
    structural_table();
    udeb_state();
    ocean_ring();
    other_kinds();
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("handle_rules ok\n");
    return 0;
}
