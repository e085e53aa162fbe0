// Device code of the two-layer stepping kernel, shared by two_layer.hip (whole-axis launches) and
// group.hip (several linked components of one model step in one launch).  See two_layer.hip for what it
// replaces in the reference and why it is written this way.
#pragma once

#include <type_traits>

#include "forcing_noise.hpp"
#include "rk4_device.hpp"
#include "rscm_device.hpp"
#include "two_layer_box.hpp"
#include "two_layer_chunk_box.hpp"

namespace rscm {
namespace tl {

struct TLConst {
    double lambda0, a, eff_eta, eta, cs, cd, rcs, rcd;
};

// EXACT arithmetic, the reference's expression order, every product and sum rounded separately:
//   temperature_difference = ts - td
//   lambda_eff = lambda0 - a*ts
//   heat_exchange_surface = efficacy*eta*temperature_difference      ((efficacy*eta) first)
//   dts = (erf - lambda_eff*ts - heat_exchange_surface) / heat_capacity_surface
//   dtd = (eta*temperature_difference) / heat_capacity_deep
// SPEC: the three-instruction quotients; TAGS: with one window tag per numerator (the per-numerator guard).
// PAIR (with SPEC, without TAGS): the two quotients by pair_div with the member's constants *z, which the verdict of
// pair_div_verdict.hpp found safe for both divisors (the pair lane of the uniform year); every other statement is the same.
struct TLPair {
    double zsh = 0.0, zsl = 0.0, zdh = 0.0, zdl = 0.0;   // zh, zl for Cs and for Cd
};

template <bool SPEC, bool TAGS = SPEC, bool PAIR = false>
__device__ __forceinline__ void rhs_exact(const TLConst& p, double erf, double ts, double td,
                                          double& dts, double& dtd, int32_t& acc, [[maybe_unused]] const TLPair* z = nullptr)
{
    static_assert(!PAIR || (SPEC && !TAGS), "pair_div belongs to the guarded speculative year");
    const double diff = ts - td;
    const double lambda_eff = p.lambda0 - p.a * ts;
    const double hx_s = p.eff_eta * diff;
    const double num_s = erf - lambda_eff * ts - hx_s;
    const double num_d = p.eta * diff;
    if constexpr (PAIR) {
        dts = pair_div(num_s, z->zsh, z->zsl);
        dtd = pair_div(num_d, z->zdh, z->zdl);
    } else if constexpr (SPEC) {
        dts = spec_div(num_s, p.cs, p.rcs);
        dtd = spec_div(num_d, p.cd, p.rcd);
        if constexpr (TAGS) acc = max3_i32(acc, window_tag(num_s), window_tag(num_d));
    } else {
        dts = num_s / p.cs;
        dtd = num_d / p.cd;
    }
}

template <bool SPEC, bool TAGS = SPEC, bool PAIR = false>
__device__ __forceinline__ void rk4_step_exact(const TLConst& p, double erf, double h,
                                               double half_step, double sixth, double& ts,
                                               double& td, int32_t& acc, [[maybe_unused]] const TLPair* z = nullptr)
{
    double k1s, k1d, k2s, k2d, k3s, k3d, k4s, k4d;
    rhs_exact<SPEC, TAGS, PAIR>(p, erf, ts, td, k1s, k1d, acc, z);
    rhs_exact<SPEC, TAGS, PAIR>(p, erf, ts + k1s * half_step, td + k1d * half_step, k2s, k2d, acc, z);
    rhs_exact<SPEC, TAGS, PAIR>(p, erf, ts + k2s * half_step, td + k2d * half_step, k3s, k3d, acc, z);
    rhs_exact<SPEC, TAGS, PAIR>(p, erf, ts + k3s * h, td + k3d * h, k4s, k4d, acc, z);
    if constexpr (SPEC) {
        // (k1 + k2*2) + k3*2: the doubling is exact, so the fused form rounds identically
        ts = rk4_combine_fused2(ts, k1s, k2s, k3s, k4s, sixth);
        td = rk4_combine_fused2(td, k1d, k2d, k3d, k4d, sixth);
    } else {
        ts = rk4_combine(ts, k1s, k2s, k3s, k4s, sixth);
        td = rk4_combine(td, k1d, k2d, k3d, k4d, sixth);
    }
}

// The state guard ("Guarding the states").  A member whose parameters, step and forcing lie in the boxes
// of two_layer_box.hpp keeps every numerator of a sub-step in spec_div's window whenever |Ts| and |Td| at the sub-step's start lie
// in the state box -- proven by scripts/two_layer_box_proof.py for those constants (tests/test_two_layer_box.py).  So a speculative
// year needs one tag per state value and sub-step instead of one per numerator.
namespace box {

constexpr double pow2(int e)
{
    double r = 1.0;
    for (; e > 0; --e) r *= 2.0;
    for (; e < 0; ++e) r *= 0.5;
    return r;
}

static_assert(kCsLo >= -128 && kCsHi <= 129 && kCdLo >= -128 && kCdHi <= 129, "heat-capacity boxes must lie in the divisor window");

// box_tag's operands for a magnitude box [2^lo, 2^hi)
constexpr uint32_t neg_edge(int lo) { return 0u - ((uint32_t)(1023 + lo) << 21); }
constexpr uint32_t span(int lo, int hi) { return (uint32_t)(hi - lo) << 21; }

__device__ __forceinline__ bool positive_in(double x, int lo, int hi)
{
    return x >= pow2(lo) && x < pow2(hi);
}

// +0, or a magnitude in the forcing box [2^lo, 2^hi) (-0 is not: it would make a numerator -0)
template <int lo = kForcingLo, int hi = kForcingHi>
__device__ __forceinline__ bool forcing_in(double f)
{
    return (__double_as_longlong(f) == 0) | (box_tag(f, neg_edge(lo)) < span(lo, hi));  // no branch
}

__device__ __forceinline__ bool params_in(const TLConst& p, double h, double half_step)
{
    return positive_in(p.lambda0, kLambda0Lo, kLambda0Hi) &&
           (__double_as_longlong(p.a) == 0 || positive_in(p.a, kALo, kAHi)) &&
           positive_in(p.eff_eta, kEffEtaLo, kEffEtaHi) && positive_in(p.eta, kEtaLo, kEtaHi) &&
           positive_in(p.cs, kCsLo, kCsHi) && positive_in(p.cd, kCdLo, kCdHi) &&
           positive_in(h, kHLo, kHHi) && positive_in(half_step, kHLo, kHHi);
}

}  // namespace box

// The chunk guard ("Guarding chunks of sub-steps"): with the narrower boxes of two_layer_chunk_box.hpp every
// numerator of chunk::kChunkSubSteps consecutive sub-steps stays in spec_div's wide window once the state at the chunk's start is in
// the chunk's state box, so the state is tagged at every kChunkSubSteps-th sub-step only (scripts/two_layer_box_proof.py, prove_chunk).
namespace chunk {

static_assert(kWideDivLo >= box::kCsLo && kWideDivHi <= box::kCdHi && kCsLo >= kWideDivLo && kCsHi <= kWideDivHi &&
                  kCdLo >= kWideDivLo && kCdHi <= kWideDivHi,
              "the chunk's heat capacities must lie in the wide window's divisor box");

__device__ __forceinline__ bool params_in(const TLConst& p, double h, double half_step, double sixth)
{
    using box::positive_in;
    return positive_in(p.lambda0, kLambda0Lo, kLambda0Hi) &&
           (__double_as_longlong(p.a) == 0 || positive_in(p.a, kALo, kAHi)) &&
           positive_in(p.eff_eta, kEffEtaLo, kEffEtaHi) && positive_in(p.eta, kEtaLo, kEtaHi) &&
           positive_in(p.cs, kCsLo, kCsHi) && positive_in(p.cd, kCdLo, kCdHi) &&
           positive_in(h, kHLo, kHHi) && positive_in(half_step, kHalfLo, kHalfHi) && positive_in(sixth, kSixthLo, kSixthHi);
}

}  // namespace chunk

// the sub-step count of the annual axis (h = 0.1): its year body is unrolled
constexpr int32_t kUnrolledSubSteps = 10;

// How a wavefront's years run (two_layer_body): the guard, the two facts of the uniform year, and whether its quotients are pair_div's
template <int32_t GUARD, bool UNIFORM = false, bool BOXED = false, bool PAIR = false>
struct YearLane {
    static constexpr int32_t kGuard = GUARD;
    static constexpr bool kUniform = UNIFORM, kBoxed = BOXED, kPair = PAIR;
};

// Where the uniform year stores: the row the launch writes first, the same for the whole wavefront, and the member's index in it
struct UniformRows {
    double* ts = nullptr;
    double* td = nullptr;
    int64_t member = 0;
    TLPair z;   // the pair lane's constants (read by it alone)
};

struct TLFast {
    double l0, a, ee, ed;  // lambda0/Cs, a/Cs, efficacy*eta/Cs, eta/Cd
};

// FAST: the same algebra with the heat capacities folded into the coefficients, FMAs, and the temperature DIFFERENCE
// w = Ts - Td as the second unknown instead of Td:
//     Ts' = F/Cs - (l0 - a Ts) Ts - ee w          w' = Ts' - ed w
// Four fused operations per stage instead of five (the difference need not be formed), 30 per RK4 step instead of 34; the
// deep-ocean temperature is Ts - w at the end of the model step.  Within 1e-11 of the oracle on bounded members
// (tests/test_gpu_parity.py; measured 6e-14).  The statements below are held bit for bit, for every member (runaway, inf, NaN and
// the status byte included), to their restatement in numpy with an exact fma: tests/host_fast.py, tests/test_gpu_fast_bits.py.
// Domain: finite 1/Cs and eta/Cd (include/rscm_gpu.h, RSCM_MODE_FAST).
__device__ __forceinline__ void rhs_fast(const TLFast& p, double erf_cs, double ts, double w, double& dts, double& dw)
{
    const double q = __builtin_fma(p.a, ts, -p.l0);   // -(lambda0 - a Ts)/Cs
    const double t = __builtin_fma(q, ts, erf_cs);
    dts = __builtin_fma(-p.ee, w, t);
    dw = __builtin_fma(-p.ed, w, dts);
}

// The RK4 sub-steps of one model step: stages as FMAs, combination y + h/6*(k1+k4) + h/3*(k2+k3).  Shared by the two-layer kind
// and the FAST coupled chain (coupled.hip), so the chain assembled from linked components carries the fused kernel's bits in this
// mode too.
__device__ __forceinline__ void rk4_year_fast(const TLFast& p, double erf_cs, int32_t m, double h, double half_step, double third,
                                              double sixth, double& ts, double& td)
{
    double w = ts - td;
    for (int32_t s = 0; s < m; ++s) {
        double k1s, k1w, k2s, k2w, k3s, k3w, k4s, k4w;
        rhs_fast(p, erf_cs, ts, w, k1s, k1w);
        rhs_fast(p, erf_cs, __builtin_fma(k1s, half_step, ts), __builtin_fma(k1w, half_step, w), k2s, k2w);
        rhs_fast(p, erf_cs, __builtin_fma(k2s, half_step, ts), __builtin_fma(k2w, half_step, w), k3s, k3w);
        rhs_fast(p, erf_cs, __builtin_fma(k3s, h, ts), __builtin_fma(k3w, h, w), k4s, k4w);
        ts = __builtin_fma(k2s + k3s, third, __builtin_fma(k1s + k4s, sixth, ts));
        w = __builtin_fma(k2w + k3w, third, __builtin_fma(k1w + k4w, sixth, w));
    }
    td = ts - w;
}

// the folded coefficients of a member, formed the same way wherever FAST two-layer arithmetic runs
__device__ __forceinline__ TLFast make_fast(double lambda0, double a, double efficacy, double eta, double cs, double cd, double& inv_cs)
{
    inv_cs = 1.0 / cs;
    TLFast p;
    p.l0 = lambda0 * inv_cs;
    p.a = a * inv_cs;
    p.ee = efficacy * eta * inv_cs;
    p.ed = eta / cd;
    return p;
}

// Per-member Gaussian log-likelihood accumulated while stepping (STORE == false): same
// expression and summation order as loglik_kernel in ensemble_ops.hip -- per-variable partial
// sums in time order, then the total in the caller's group order (likelihood.rs:186-250).
struct LikAcc {
    double part_s = 0.0, part_d = 0.0;
    bool bad = false;
    int32_t oi = 0;
};

__device__ __forceinline__ void lik_consume(const TwoLayerArgs& a, LikAcc& L, int32_t row, double ts,
                                            double td)
{
    while (L.oi < a.n_obs && a.obs_tidx[L.oi] == row) {  // wave-uniform
        const bool deep = a.obs_is_deep[L.oi] != 0;
        const double m = deep ? td : ts;
        if (!is_finite(m)) L.bad = true;
        const double sigma = a.obs_sigma[L.oi];
        const double residual = a.obs_value[L.oi] - m;
        const double chi = (residual * residual) / (sigma * sigma);
        double l = -0.5 * chi;
        if (a.normalize) {
            l -= 0.5 * 1.8378770664093453;  // ln(2*pi)
            l -= log(sigma);
        }
        if (deep) L.part_d += l;
        else L.part_s += l;
        ++L.oi;
    }
}

// The same with reference periods (REF launches; DESIGN.md section 7, "Reference periods").  A variable with a period is scored as the
// anomaly from the member's own mean b over the reference rows.  The thread adds each reference row to the variable's sum as it passes
// it (the sum starts at -0.0, the additive identity: the bits of rscm_ens_set_baseline).  An observation of that variable at a row up
// to the period's last cannot be scored yet: its model value goes to the handle's scratch ([slot][N], one coalesced store).  When the
// last reference row is in, b = sum / count is formed and the waiting observations are scored in observation order (one coalesced load
// each); later ones are scored on the fly.  A variable's partial sum so sees the addends loglik_kernel (ensemble_ops.hip) gives it,
// in the same order: the two paths agree bit for bit.
struct LikRef {
    double sum_s = -0.0, sum_d = -0.0, b_s = 0.0, b_d = 0.0;
    bool have_s = false, have_d = false;
};

__device__ __forceinline__ double lik_term(const TwoLayerArgs& a, int32_t k, double m)
{
    const double sigma = a.obs_sigma[k];
    const double residual = a.obs_value[k] - m;
    const double chi = (residual * residual) / (sigma * sigma);
    double l = -0.5 * chi;
    if (a.normalize) {
        l -= 0.5 * 1.8378770664093453;  // ln(2*pi)
        l -= log(sigma);
    }
    return l;
}

// the last reference row of a variable is in: form b and score the observations that waited for it (all of the variable's so far)
__device__ __forceinline__ void lik_settle(const TwoLayerArgs& a, const TwoLayerRefArgs& r, LikAcc& L, bool deep, double sum, int32_t count,
                                           double& b, double& part, int64_t i, int64_t N)
{
    b = sum / (double)count;
    if (!is_finite(b)) L.bad = true;
    for (int32_t k = 0; k < L.oi; ++k) {  // wave-uniform
        const int32_t slot = r.obs_slot[k];
        if ((a.obs_is_deep[k] != 0) != deep || slot < 0) continue;
        part += lik_term(a, k, r.defer[(size_t)slot * N + i] - b);
    }
}

__device__ __forceinline__ void lik_consume_ref(const TwoLayerArgs& a, const TwoLayerRefArgs& r, LikAcc& L, LikRef& R, int32_t row,
                                                double ts, double td, int64_t i, int64_t N)
{
    auto reference_row = [&](int32_t v) {  // wave-uniform
        return r.on[v] && row >= r.begin[v] && row <= r.last[v] && (r.stride[v] == 1 || (row - r.begin[v]) % r.stride[v] == 0);
    };
    if (reference_row(0)) R.sum_s += ts;
    if (reference_row(1)) R.sum_d += td;
    while (L.oi < a.n_obs && a.obs_tidx[L.oi] == row) {  // wave-uniform
        const bool deep = a.obs_is_deep[L.oi] != 0;
        const double m = deep ? td : ts;
        if (!is_finite(m)) L.bad = true;
        const int32_t slot = r.obs_slot[L.oi];
        if (slot >= 0) {
            r.defer[(size_t)slot * N + i] = m;
        } else {
            const bool anomaly = deep ? r.on[1] != 0 : r.on[0] != 0;
            const double l = lik_term(a, L.oi, anomaly ? m - (deep ? R.b_d : R.b_s) : m);
            if (deep) L.part_d += l;
            else L.part_s += l;
        }
        ++L.oi;
    }
    if (r.on[0] && row == r.last[0]) {
        lik_settle(a, r, L, false, R.sum_s, r.count[0], R.b_s, L.part_s, i, N);
        R.have_s = true;
    }
    if (r.on[1] && row == r.last[1]) {
        lik_settle(a, r, L, true, R.sum_d, r.count[1], R.b_d, L.part_d, i, N);
        R.have_d = true;
    }
}

// Member i over the steps [a.step_begin, a.step_end).  LDS: the forcing slice staged by the caller in
// lds_forcing ([n_scen][len]); otherwise read through L2 (table or linked series).
// Cache: NoCache for the stand-alone kernels; the fused multi-step launch (group.hip) keeps parameters, the
// state and the linked forcing of the current step in LDS between its steps (rscm_device.hpp, LdsCache).
// Returns the guard of the wavefront's speculative years (EXACT; the same in every lane): kGuardNumerators, kGuardStates or
// kGuardChunks; -1 in FAST mode.
enum : int32_t { kGuardNumerators = 0, kGuardStates = 1, kGuardChunks = 2, kGuardKinds = 3 };
// ... with this bit on top where the wavefront's uniform years formed their quotients with pair_div (stand-alone stored launches only)
constexpr int32_t kPairLaneBit = 0x100;

// REF (with STORE == false): the fused likelihood with the reference periods of *ref (lik_consume_ref).
// MIX (a mix handle, a.n_comp = K in 1..kMaxForcingComponents; stand-alone launches only, never linked): the forcing of member i is
// formed per year from the K rows of its scenario, [S][K][T] (LDS: [S][K][len]), and the coefficients in parameter rows 6..6+K-1:
//     F = S_0[n] * c_0;   F = F + S_k[n] * c_k   for k = 1 .. K-1, in that order,
// every product and sum rounded on its own in BOTH arithmetic modes (the file is compiled with -ffp-contract=off and nothing here is
// written as an FMA).  NaN and Inf propagate, no row is skipped and none is padded with 0 * S (that would change -0.0, NaN and Inf):
// the loop below is unrolled to eight with a wave-uniform k < K around each term, so the coefficients stay in registers.
// NOISE != 0 (the launcher passes noise_kind(a.noise_on), rscm_device.hpp; stand-alone STORE launches only, never linked): the forcing
// read at forcing-axis index t = n + a.src_off -- the scenario value, or the mix sum formed first -- becomes, with NOISE == 1 (white),
//     F' = F + a.noise_sigma * z(a.noise_seed, a.noise_member0 + i, t),
// product and sum rounded on their own in BOTH modes, z the stateless deviate of forcing_noise.hpp.  forcing_at adds the term, so the
// draw for year n + 1 is made in the look-ahead slot of year n and the box guard and the replay see F' like any forcing.  A Philox
// block serves an even index and the odd one after it: the second pair of words waits in two registers for the next year (which
// index they serve is wave-uniform), so the ten rounds run every other year.
// NOISE == 2 (red): F' = F + e_t with e_0 = sigma z_0 and e_t = (phi e_{t-1}) + ((sigma sqrt(1 - phi phi)) z_t), each
// operation rounded on its own.  forcing_at is called once per index in ascending order, so e lives in a register and a year costs
// two multiplies and an add on top of the white draw.  Before the year loop e is brought to the index before the launch's first:
// loaded from a.noise_state (a.noise_on == kNoiseRedCached) or formed from index 0 on by the same statements as in the loop (a
// wave-uniform trip count; the bits of the per-index definition by construction).  The launch ends with one store of e, which then
// stands at the last index drawn, step_end - 1 + a.src_off.
// NOISE == 3 (per-member): the red statements with member i's own sigma_i and phi_i, parameter rows
// kTwoLayerCoeff0 + K and the next (K = a.n_comp of a mix handle, else 0), read once per launch like every other row -- a row that
// rscm_ens_set_params found uniform is one element for the wavefront.  sigma_i, phi_i and sigma_i sqrt(1 - phi_i phi_i) live in vector
// registers (four more than NOISE == 2, where they are kernel arguments: the EXACT plain kernel crosses the 168-register step).  Nothing validates the rows: NaN, Inf or |phi_i| > 1 make that
// lane's forcing NaN and leave every other lane alone; a lane whose forcing leaves the guard's box replays its year as with any forcing.
// ALONE: a stand-alone launch (two_layer.hip), whose a.year_facts the host has filled in; the fused launches (group.hip) pass none.
// PAIRS (stand-alone stored EXACT launches of the plain table): pair_div holds the members' constants of the two-instruction quotient,
// [4][N] with the rows' stride: zh, zl for Cs, then for Cd, zh = 0 where a divisor has no safe ones (two_layer.hip,
// two_layer_pair_div_kernel); member i's are at pair_div[i].  The other instantiations take no such pointer and have no pair lane.
template <int MODE, bool LDS, bool STORE, class Cache = NoCache, bool REF = false, bool MIX = false, int NOISE = 0, bool ALONE = false,
          bool PAIRS = false>
__device__ __forceinline__ int32_t two_layer_body(const TwoLayerArgs& a, const double* lds_forcing, int64_t i, int32_t step_begin,
                                               int32_t step_end, const Cache& cache = Cache(), const TwoLayerRefArgs* ref = nullptr,
                                               [[maybe_unused]] const double* pair_div = nullptr)
{
    static_assert(!PAIRS || (MODE == 0 && ALONE && STORE && !REF && !MIX && !NOISE && !Cache::kOn), "the pair lane belongs to the plain stored EXACT launch");
    static_assert(!(REF && STORE), "reference periods belong to the fused likelihood");
    static_assert(!NOISE || (STORE && !Cache::kOn), "forcing noise belongs to the stand-alone stored run");
    const int32_t len = step_end - step_begin;
    const int64_t N = a.row_stride;   // the rows' stride (the caller has checked i against a.n_members)

    const double lambda0 = cache.param(a.params, a.uniform_rows, 0, N, i);
    const double pa = cache.param(a.params, a.uniform_rows, 1, N, i);
    const double efficacy = cache.param(a.params, a.uniform_rows, 2, N, i);
    const double eta = cache.param(a.params, a.uniform_rows, 3, N, i);
    const double cs = cache.param(a.params, a.uniform_rows, 4, N, i);
    const double cd = cache.param(a.params, a.uniform_rows, 5, N, i);
    const int32_t scen = a.scen ? a.scen[i] : 0;
    // a linked forcing (rscm_ens_link_input, always the non-LDS variant) is another ensemble's
    // [T][N] series: coalesced, one stride of N per year
    const double* fglob = a.link ? a.link + (size_t)a.src_off * N + i : a.forcing + (size_t)scen * a.n_times + a.src_off;
    const size_t fstride = a.link ? (size_t)N : (size_t)1;
    const int32_t fl0 = scen * len - step_begin;  // lds_forcing[fl0 + n], n >= step_begin
    // MIX: the member's coefficients, read once, and where row 0 of its scenario's block starts (row k follows mix_row elements later)
    using mix_index = std::conditional_t<LDS, int32_t, int64_t>;   // (the staged table is indexed in 32 bits like lds_forcing[fl0 + n])
    [[maybe_unused]] double coeff[kMaxForcingComponents];
    [[maybe_unused]] const int32_t n_comp = MIX ? a.n_comp : 0;   // wave-uniform (kernarg)
    [[maybe_unused]] const mix_index mix_row = LDS ? len : a.n_times;
    [[maybe_unused]] const double* mix_base = LDS ? lds_forcing : a.forcing;
    [[maybe_unused]] mix_index mix0 = 0;   // mix_base[mix0 + n]: component 0 at model index n (n >= step_begin for the staged table)
    if constexpr (MIX) {
        static_assert(!Cache::kOn, "a mix handle is never part of a fused launch");
#pragma unroll
        for (int k = 0; k < kMaxForcingComponents; ++k)
            coeff[k] = k < n_comp ? cache.param(a.params, a.uniform_rows, kTwoLayerCoeff0 + k, N, i) : 0.0;
        if constexpr (LDS) mix0 = (mix_index)scen * n_comp * len - step_begin;
        else mix0 = (mix_index)scen * n_comp * a.n_times + a.src_off;
    }
    // NOISE: the member's id in the whole ensemble, and words (2,3) of the last even index's block with the (odd) index they serve
    [[maybe_unused]] const uint64_t noise_g = NOISE ? (uint64_t)(a.noise_member0 + i) : 0;
    [[maybe_unused]] uint32_t noise_lo = 0, noise_hi = 0;
    [[maybe_unused]] int32_t noise_t = -1;   // wave-uniform
    [[maybe_unused]] auto noise_z = [&](int32_t t) -> double {   // z(seed, g, t)
        uint32_t lo, hi;
        if (t == noise_t) {
            lo = noise_lo;
            hi = noise_hi;
        } else {
            uint32_t c[4];
            noise::block_of(a.noise_seed, noise_g, (uint32_t)t, c);
            if (t & 1) {
                lo = c[2];
                hi = c[3];
            } else {
                lo = c[0];
                hi = c[1];
                noise_lo = c[2];
                noise_hi = c[3];
                noise_t = t + 1;
            }
        }
        return noise::normal_from_k(noise::k_of(lo, hi));
    };
    // red noise: e at the last index drawn, and sigma sqrt(1 - phi^2) (three roundings, then the product)
    constexpr bool RED = NOISE >= 2;
    constexpr bool MEMBERS = NOISE == 3;   // sigma and phi are the member's own
    [[maybe_unused]] double red_e = 0.0;
    [[maybe_unused]] double mem_sigma = 0.0, mem_phi = 0.0;
    if constexpr (MEMBERS) {
        mem_sigma = cache.param(a.params, a.uniform_rows, kTwoLayerCoeff0 + n_comp, N, i);
        mem_phi = cache.param(a.params, a.uniform_rows, kTwoLayerCoeff0 + n_comp + 1, N, i);
    }
    [[maybe_unused]] const double red_se = MEMBERS ? mem_sigma * __builtin_sqrt(1.0 - mem_phi * mem_phi)
                                           : RED   ? a.noise_sigma * __builtin_sqrt(1.0 - a.noise_phi * a.noise_phi)
                                                   : 0.0;
    [[maybe_unused]] auto red_advance = [&](int32_t t) {   // e_{t-1} -> e_t
        const double z = noise_z(t);
        if constexpr (MEMBERS) red_e = t == 0 ? mem_sigma * z : (mem_phi * red_e) + (red_se * z);
        else red_e = t == 0 ? a.noise_sigma * z : (a.noise_phi * red_e) + (red_se * z);
    };
    if constexpr (RED) {
        if (a.noise_on == (MEMBERS ? kNoiseMembersCached : kNoiseRedCached)) red_e = a.noise_state[i];
        else
            for (int32_t t = 0, t0 = step_begin + a.src_off; t < t0; ++t) red_advance(t);
    }
    [[maybe_unused]] auto noisy = [&](int32_t n, double f) -> double {
        const int32_t t = n + a.src_off;
        if constexpr (RED) {
            red_advance(t);
            return f + red_e;
        } else {
            return f + a.noise_sigma * noise_z(t);
        }
    };
    auto forcing_at = [&](int32_t n) -> double {
        if constexpr (MIX) {
            const mix_index at = mix0 + n;
            double f = mix_base[at] * coeff[0];
#pragma unroll
            for (int k = 1; k < kMaxForcingComponents; ++k)
                if (k < n_comp) f = f + mix_base[at + (mix_index)k * mix_row] * coeff[k];
            if constexpr (NOISE) return noisy(n, f);
            else return f;
        } else if constexpr (NOISE) return noisy(n, LDS ? lds_forcing[fl0 + n] : fglob[(size_t)n * fstride]);
        else if constexpr (LDS) return lds_forcing[fl0 + n];
        else return fglob[(size_t)n * fstride];
    };
    // the year a fused launch is at: the linked forcing from the producer's LDS slot if it is kept there
    auto forcing_first = [&]() -> double {
        if constexpr (Cache::kOn) {
            if (a.link && cache.has_link(0)) return cache.link(0);
        }
        return forcing_at(step_begin);
    };
    // next year's forcing: a fused launch calls per year (n == last), there is no next year to fetch (nor, with NOISE, to draw for)
    auto forcing_ahead = [&](int32_t n, int32_t np, double current) -> double {
        if constexpr (Cache::kOn || NOISE) return n < np ? forcing_at(np) : current;
        else return forcing_at(np);
    };

    double ts = cache.state(0, a.ts + (size_t)step_begin * N + i);
    double td = cache.state(1, a.td + (size_t)step_begin * N + i);
    double* out_ts = a.ts + (size_t)(step_begin + 1) * N + i;
    double* out_td = a.td + (size_t)(step_begin + 1) * N + i;

    const double h = a.h;
    const double half_step = a.h_half;
    const double sixth = a.h_sixth;
    const int32_t last = step_end - 1;

    LikAcc lik;
    [[maybe_unused]] LikRef lik_ref;
    [[maybe_unused]] auto consume = [&](int32_t row) {
        if constexpr (REF) lik_consume_ref(a, *ref, lik, lik_ref, row, ts, td, i, N);
        else lik_consume(a, lik, row, ts, td);
    };
    if constexpr (!STORE) consume(step_begin);  // observations (and a reference row) of the start row

    // next year's forcing and sub-step count are fetched a year ahead of their use
    double erf_next = forcing_first();
    int32_t m_next = a.nsub[step_begin];

    int32_t guard = -1;
    if constexpr (MODE == 0) {
        TLConst p;
        p.lambda0 = lambda0;
        p.a = pa;
        p.eff_eta = efficacy * eta;
        p.eta = eta;
        p.cs = cs;
        p.cd = cd;
        const ConstDiv dcs = make_const_div(cs), dcd = make_const_div(cd);
        p.rcs = dcs.r;
        p.rcd = dcd.r;
        // 0 (never "all inside") when a heat capacity is outside the divisor window
        const int32_t acc0 = (dcs.ok && dcd.ok) ? (int32_t)0x80000000 : 0;
        // one decision per wavefront: every member in the boxes -> the state guard; in the chunk boxes as well -> the chunk guard
        const bool guard_states = __all(!a.numerator_guard && box::params_in(p, h, half_step));
        const bool guard_chunks = guard_states && __all(chunk::params_in(p, h, half_step, sixth));
        // The uniform year (TwoLayerArgs::year_facts, proved by the host: two_layer_year_facts.hpp): every step of the launch has
        // kUnrolledSubSteps sub-steps, so a wavefront under the chunk guard neither loads nor tests the count and the generic sub-step
        // loops are not part of its year loop; with the forcing proved inside the chunk's box as well, the year's check of it is left
        // out (it would have found acc = 0).  Same statements otherwise.  Kernel arguments: the choice is made once, outside the loop.
        // The instantiations of fused launches, mix handles and noise do not have the lane: they compile to what they were.
        constexpr bool kUniformLane = ALONE && !Cache::kOn && !MIX && !NOISE;
        // kGuard 0: a tag per numerator; 1: the state at every sub-step; kChunkSubSteps: the state at every kGuard-th sub-step
        // (out: read by the uniform year only, and a parameter on purpose -- what the lambda captures, and in which order, stays what it
        // was, and with it the code of the instantiations without the lane)
        auto years = [&](auto lane, [[maybe_unused]] UniformRows out) {
            constexpr int32_t kGuard = decltype(lane)::kGuard;
            constexpr bool kStates = kGuard > 0;
            constexpr bool kChunks = kGuard > 1;   // the chunk guard covers the unrolled 10-sub-step year only
            constexpr bool kUniform = decltype(lane)::kUniform;   // every year has kUnrolledSubSteps sub-steps
            constexpr bool kBoxed = decltype(lane)::kBoxed;       // ... and a forcing inside the chunk's box
            static_assert(!kUniform || (kChunks && kUniformLane), "the uniform year belongs to the chunk guard of a plain launch");
            static_assert(!kBoxed || kUniform, "the forcing's verdict is used by the uniform year only");
            constexpr bool kPair = decltype(lane)::kPair;         // ... and safe pair_div constants for every member of the wavefront
            static_assert(!kPair || (kUniform && PAIRS), "pair_div belongs to the uniform year of a launch that brings the constants");
            for (int32_t n = step_begin; n < step_end; ++n) {
                const double erf = erf_next;
                const int32_t m = kUniform ? kUnrolledSubSteps : m_next;
                const int32_t np = n < last ? n + 1 : n;
                erf_next = forcing_ahead(n, np, erf_next);
                if constexpr (!kUniform) m_next = a.nsub[np];
                const double ts0 = ts, td0 = td;
                bool replay;
                if constexpr (kStates) {
                    int32_t no_tags = 0;
                    auto sub_step = [&](uint32_t& acc, uint32_t edge, bool tag) {
                        if (tag) acc = max3_u32(acc, box_tag(ts, edge), box_tag(td, edge));
                        if constexpr (kPair) rk4_step_exact<true, false, true>(p, erf, h, half_step, sixth, ts, td, no_tags, &out.z);
                        else rk4_step_exact<true, false>(p, erf, h, half_step, sixth, ts, td, no_tags);
                    };
                    if (kChunks && (kUniform || m == kUnrolledSubSteps)) {
                        // the chunk guard: the state at every kGuard-th sub-step against the chunk's boxes
                        constexpr uint32_t kEdge = box::neg_edge(chunk::kStateLo), kSpan = box::span(chunk::kStateLo, chunk::kStateHi);
                        uint32_t acc = kBoxed ? 0u : box::forcing_in<chunk::kForcingLo, chunk::kForcingHi>(erf) ? 0u : ~0u;
#pragma unroll
                        for (int32_t s = 0; s < kUnrolledSubSteps; ++s) sub_step(acc, kEdge, s % kGuard == 0);
                        replay = acc >= kSpan;
                    } else {
                        // the state guard: the state at every sub-step against two_layer_box.hpp's boxes -- also the generic loop of a
                        // wavefront that takes the chunk guard, so that loop replays exactly where it did before the chunk guard
                        constexpr uint32_t kEdge = box::neg_edge(box::kStateLo), kSpan = box::span(box::kStateLo, box::kStateHi);
                        uint32_t acc = box::forcing_in(erf) ? 0u : ~0u;
                        if (m == kUnrolledSubSteps) {
#pragma unroll
                            for (int32_t s = 0; s < kUnrolledSubSteps; ++s) sub_step(acc, kEdge, true);
                        } else {
                            for (int32_t s = 0; s < m; ++s) sub_step(acc, kEdge, true);
                        }
                        replay = acc >= kSpan;
                    }
                } else {
                    int32_t acc = acc0;
                    for (int32_t s = 0; s < m; ++s) rk4_step_exact<true>(p, erf, h, half_step, sixth, ts, td, acc);
                    replay = acc >= 0;
                }
                // A NaN state at the start of the year makes every value of the year NaN on either
                // path; everything else must have stayed inside the window.
                const bool settled = (ts0 != ts0) || (td0 != td0);
                if (__builtin_expect(replay && !settled, 0)) {
                    ts = ts0;
                    td = td0;
                    int32_t unused = 0;
                    for (int32_t s = 0; s < m; ++s) rk4_step_exact<false>(p, erf, h, half_step, sixth, ts, td, unused);
                }
                if constexpr (STORE && !kUniform) {
                    *out_ts = ts;
                    *out_td = td;
                    cache.put(0, ts);
                    cache.put(1, td);
                    out_ts += N;
                    out_td += N;
                } else if constexpr (STORE) {   // a wave-uniform row and the member's index
                    out.ts[out.member] = ts;
                    out.td[out.member] = td;
                    out.ts += N;
                    out.td += N;
                } else {
                    consume(n + 1);
                }
            }
        };
        bool uniform_year = false;
        if constexpr (kUniformLane) uniform_year = guard_chunks && year_nsub_uniform(a.year_facts) == kUnrolledSubSteps;
        // The pair lane ("Dividing by a constant in two instructions"): the host says that pair_div holds the
        // members' constants as formed from the parameter rows that stand now, and every member of the wavefront has safe ones for both
        // heat capacities (zh = 0 marks a divisor without).  The chunk guard keeps every numerator inside pair_div's window as it does
        // inside spec_div's; a year that leaves it is replayed in IEEE arithmetic as before.
        [[maybe_unused]] bool pair_lane = false;
        if (uniform_year) {
            if constexpr (kUniformLane) {
                UniformRows rows{a.ts + (size_t)(step_begin + 1) * N, a.td + (size_t)(step_begin + 1) * N, i};
                if constexpr (PAIRS) {
                    if (year_pair_valid(a.year_facts)) {
                        const double* z = pair_div + i;
                        rows.z = TLPair{z[0], z[N], z[2 * N], z[3 * N]};
                        pair_lane = __all(rows.z.zsh != 0.0 && rows.z.zdh != 0.0);
                    }
                }
                const bool boxed = year_forcing_boxed(a.year_facts);
                if constexpr (PAIRS) {
                    if (pair_lane) {
                        if (boxed) years(YearLane<chunk::kChunkSubSteps, true, true, true>(), rows);
                        else years(YearLane<chunk::kChunkSubSteps, true, false, true>(), rows);
                    }
                }
                if (!pair_lane) {
                    if (boxed) years(YearLane<chunk::kChunkSubSteps, true, true>(), rows);
                    else years(YearLane<chunk::kChunkSubSteps, true, false>(), rows);
                }
            }
        } else if (guard_chunks) years(YearLane<chunk::kChunkSubSteps>(), UniformRows());
        else if (guard_states) years(YearLane<1>(), UniformRows());
        else years(YearLane<0>(), UniformRows());
        guard = guard_chunks ? kGuardChunks : guard_states ? kGuardStates : kGuardNumerators;
        if (pair_lane) guard |= kPairLaneBit;
    } else {
        double inv_cs;
        const TLFast p = make_fast(lambda0, pa, efficacy, eta, cs, cd, inv_cs);
        const double third = h / 3.0;
        for (int32_t n = step_begin; n < step_end; ++n) {
            const double erf = erf_next * inv_cs;
            const int32_t m = m_next;
            const int32_t np = n < last ? n + 1 : n;
            erf_next = forcing_ahead(n, np, erf_next);
            m_next = a.nsub[np];
            rk4_year_fast(p, erf, m, h, half_step, third, sixth, ts, td);
            if constexpr (STORE) {
                *out_ts = ts;
                *out_td = td;
                cache.put(0, ts);
                cache.put(1, td);
                out_ts += N;
                out_td += N;
            } else {
                consume(n + 1);
            }
        }
    }
    if (cache.last_step()) a.status[i] = (is_finite(ts) && is_finite(td)) ? 0 : 1;
    if constexpr (RED) a.noise_state[i] = red_e;
    if constexpr (!STORE) {
        // observations whose row is never reached were never computed -> member failure
        if (lik.oi < a.n_obs) lik.bad = true;
        if constexpr (REF) {  // ... and so is a period whose last row is never reached
            if ((ref->on[0] && !lik_ref.have_s) || (ref->on[1] && !lik_ref.have_d)) lik.bad = true;
        }
        const double total = a.first_is_deep ? (0.0 + lik.part_d) + lik.part_s
                                             : (0.0 + lik.part_s) + lik.part_d;
        a.loglik[i] = lik.bad ? -__builtin_inf() : total;
    }
    return guard;
}

}  // namespace tl
}  // namespace rscm
