// The boxes inside which kChunkSubSteps consecutive EXACT two-layer RK4 sub-steps keep every numerator of their right-hand sides in
// spec_div's wide window: +0 or a magnitude in [2^kWideNumLo, 2^kWideNumHi), for heat capacities in [2^kWideDivLo, 2^kWideDivHi)
// (rk4_device.hpp, "the wide window"; DESIGN.md section 4.1, "Guarding chunks of sub-steps").  A box [lo, hi) is 2^lo <= |x| < 2^hi, in
// binary exponents.  scripts/two_layer_box_proof.py reads this file and checks the argument without re-boxing between the sub-steps;
// tests/test_two_layer_chunk_box.py fails if a constant here is moved past what the proof covers, and if an edge could be moved
// further out and still be proven.
//
// Every edge is the widest the checker proves with the others in place, except where the state guard's box (two_layer_box.hpp) ends
// first: a wavefront takes the chunk guard only if it also qualifies for the state guard, so the parameter boxes stop at the state
// guard's edges (lambda0, a and eta below, Cs above; Cd is the wide divisor box), and the forcing box's lower edge is held at the state
// guard's so that the chunk forcing box contains the state guard's -- a year whose forcing the state guard accepts is never replayed
// here.  The state box's upper edge (2^7 K) is the proof's limit: above
// it a year replays where the state guard would not, which no physical member reaches.
//
// Parameters and step: checked once per member, one ballot per wavefront picks the chunk guard.  Forcing: checked once per model year,
// +0 or a magnitude in its box.  State: a magnitude in its box at the start of every chunk.
#pragma once

namespace rscm {
namespace tl {
namespace chunk {

constexpr int kChunkSubSteps = 3;                   // sub-steps covered by one check of the state

constexpr int kLambda0Lo = -16, kLambda0Hi = 2;     // lambda0
constexpr int kALo = -64, kAHi = -3;                // a (or exactly +0)
constexpr int kEffEtaLo = -16, kEffEtaHi = 1;       // efficacy * eta, as the kernel rounds it
constexpr int kEtaLo = -16, kEtaHi = 2;             // eta
constexpr int kCsLo = 2, kCsHi = 10;                // heat capacity of the surface layer
constexpr int kCdLo = -2, kCdHi = 14;               // heat capacity of the deep ocean
constexpr int kHLo = -5, kHHi = -3;                 // h
constexpr int kHalfLo = -5, kHalfHi = -4;           // h / 2
constexpr int kSixthLo = -6, kSixthHi = -5;         // h / 6
constexpr int kForcingLo = -128, kForcingHi = 13;   // |forcing| (or exactly +0)
constexpr int kStateLo = -154, kStateHi = 7;        // |Ts|, |Td| at the start of a chunk: the upper edge is the proof's limit

// spec_div's wide numerator window, valid for divisors in the wide divisor box (rk4_device.hpp)
constexpr int kWideDivLo = -2, kWideDivHi = 14;
constexpr int kWideNumLo = -960, kWideNumHi = 760;

}  // namespace chunk
}  // namespace tl
}  // namespace rscm
