// The internal component state of the kinds that keep one (kinds.hpp, KindInfo::internal_state) at time index k, as runs of rows of the
// handle's buffers in the checkpoint's order: what the checkpoint and the branch copy (state_host.cpp).  Host only, every count an argument.
//   ClimateUDEB   the ocean columns (2 x layers rows), the scalars, the history rows 0 .. k
//   OceanCarbon   the flux pulses still held, oldest first: pulse j lives in row j mod ring, so the k x steps pulses taken so far -- the
//                 last `ring` of them once the ring has gone round -- unroll into at most two runs
#pragma once

#include "kinds.hpp"

namespace rscm {

enum class StateBuf : uint8_t { UdebColumns, UdebScalars, UdebHistory, OceanRing };
struct StateRun { StateBuf buf; int64_t first, count; };   // rows [first, first + count) of the buffer
// the sizes the handle's configuration fixed; 0 where it has not yet (then there is no state).  ocean_steps: pulses per model step
struct StateShape { int32_t udeb_layers, udeb_scalars, ocean_steps; int64_t ocean_ring; };
struct StateRuns {
    StateRun run[3];
    int32_t n = 0;
    const StateRun* begin() const { return run; }
    const StateRun* end() const { return run + n; }
    int64_t rows() const { int64_t total = 0; for (const StateRun& r : *this) total += r.count; return total; }
};

inline StateRuns internal_state_runs(int32_t kind, int32_t k, const StateShape& s)
{
    StateRuns r;
    if (kind < 0 || kind >= kNumKinds || !kKinds[kind].internal_state) return r;
    if (kind == RSCM_KIND_UDEB && s.udeb_layers > 0) {
        r.run[r.n++] = {StateBuf::UdebColumns, 0, (int64_t)2 * s.udeb_layers};
        r.run[r.n++] = {StateBuf::UdebScalars, 0, s.udeb_scalars};
        r.run[r.n++] = {StateBuf::UdebHistory, 0, (int64_t)k + 1};
    } else if (kind == RSCM_KIND_OCEAN_CARBON && s.ocean_ring > 0) {
        const int64_t taken = (int64_t)k * s.ocean_steps, held = taken < s.ocean_ring ? taken : s.ocean_ring;
        const int64_t first = (taken - held) % s.ocean_ring, head = held < s.ocean_ring - first ? held : s.ocean_ring - first;
        if (head > 0) r.run[r.n++] = {StateBuf::OceanRing, first, head};
        if (held > head) r.run[r.n++] = {StateBuf::OceanRing, 0, held - head};
    }
    return r;
}

}  // namespace rscm
