// The boxes inside which one EXACT two-layer RK4 sub-step is proven to keep every numerator of its four right-hand sides in
// spec_div's window (rk4_device.hpp): +0 or a biased exponent in [512, 1535].  A box [lo, hi) below is 2^lo <= |x| < 2^hi, in
// binary exponents.  scripts/two_layer_box_proof.py reads this file and checks the argument ("Guarding the
// states"); tests/test_two_layer_box.py fails if a constant here is moved past what the proof covers.
//
// Parameters (checked once per member; one ballot per wavefront picks the state-guarded year loop): all positive, a also +0.
// Forcing (checked once per model year): +0 (not -0), or a magnitude in its box, either sign.
// State (checked at the start of every sub-step): a magnitude in its box, either sign; zeros are outside.
#pragma once

namespace rscm {
namespace tl {
namespace box {

constexpr int kLambda0Lo = -16, kLambda0Hi = 6;     // lambda0
constexpr int kALo = -64, kAHi = 2;                  // a (or exactly +0)
constexpr int kEffEtaLo = -16, kEffEtaHi = 6;       // efficacy * eta, as the kernel rounds it
constexpr int kEtaLo = -16, kEtaHi = 6;             // eta
constexpr int kCsLo = -2, kCsHi = 10;               // heat capacity of the surface layer (inside the divisor window)
constexpr int kCdLo = -2, kCdHi = 14;               // heat capacity of the deep ocean (inside the divisor window)
constexpr int kHLo = -16, kHHi = 2;                 // h and h / 2
constexpr int kForcingLo = -128, kForcingHi = 12;   // |forcing| (or exactly +0)
constexpr int kStateLo = -128, kStateHi = 26;       // |Ts|, |Td| at the start of a sub-step: the upper edge is the proof's limit

}  // namespace box
}  // namespace tl
}  // namespace rscm
