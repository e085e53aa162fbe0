// Two-layer energy-balance ensemble kernel for gfx950 (MI355X).
//
// One thread per ensemble member; the model's whole time loop, the RK4 sub-steps and the
// TwoLayer right-hand side are fused in that thread, so per member-year the only HBM traffic is
// the two 8-byte state stores (16 B) that the reference's stepper also produces
// (crates/rscm-core/src/model/runtime.rs:480 writes outputs at index n+1).
//
// What it replaces, per step n (reference file:line):
//   Model::step_model_component      crates/rscm-core/src/model/runtime.rs:368-497
//   TwoLayer::solve                  crates/rscm-two-layer/src/component.rs:223-251
//   IVPBuilder::to_rk4 + Rk4 (10 sub-steps of h = 0.1 for an annual step)
//                                    crates/rscm-core/src/ivp/mod.rs:245-253
//   TwoLayer::calculate_dy_dt        crates/rscm-two-layer/src/component.rs:159-189
// The third integrand (heat content, component.rs:186-187) is integrated from 0 and dropped by
// the reference (:236,245-248); it cannot influence Ts/Td and is not computed here.
//
// Layout: params [6][N], state series [T][N] (member fastest => a wavefront stores 512
// contiguous bytes per variable per year), shared forcing [S][T] staged once per workgroup in
// LDS (751 x 8 B = 6 KB per scenario) and read as a broadcast (one scenario) or a per-lane
// gather (scenario_of_member).  No inter-workgroup communication, so the blockIdx -> XCD
// round-robin needs no remap: every workgroup streams its own column block and re-reads only
// the (L2-resident) forcing.
//
// The year loop issues no vector-memory LOAD: forcing comes from LDS (or is prefetched one year
// ahead on the L2 path) and the sub-step counts through the scalar cache, so no s_waitcnt vmcnt
// ever waits behind the previous year's stores -- that wait was 31 % of wave time at
// 1.5 waves/SIMD (profiles/r1_exact_1e5_v1_pmc.txt).
//
// EXACT mode, speculative year: the RK4 sub-steps of a year run branch-free with
//   * n/C as q = n*r; rem = fma(-C,q,n); fma(rem,r,q)   (rk4_device.hpp: identical to IEEE
//     division when the numerator's biased exponent is in [512,1535] and C's in [895,1151]),
//   * k1 + k2*2 as fma(k2, 2, k1)                        (identical while 2*k2 cannot overflow),
// while one integer max3 per right-hand side accumulates whether every numerator stayed inside
// the window.  If any did not (zeros in the first year, a member overflowing towards inf, ...)
// the year is recomputed for those lanes from the saved state with the compiler's full IEEE
// division and unfused doubling.  Either way the stored bits equal the reference's arithmetic.
#include "two_layer_body.hpp"

#include <type_traits>

#include "pair_div_verdict.hpp"

namespace rscm {

namespace {

// test hook (rscm_gpu_two_layer_guard_counts): per guard (tl::kGuardNumerators / kGuardStates / kGuardChunks), the wavefronts of the
// counting launches that took it
__device__ unsigned long long g_guard_counts[tl::kGuardKinds];
// ... and of those, the wavefronts whose uniform years took the pair lane (rscm_gpu_two_layer_pair_lanes)
__device__ unsigned long long g_pair_lanes;

// a wavefront's first lane reports what two_layer_body returned
__device__ __forceinline__ void count_guard(const TwoLayerArgs& a, int32_t guard)
{
    if (a.count_guards && (threadIdx.x & 63) == 0) {
        atomicAdd(&g_guard_counts[guard & ~tl::kPairLaneBit], 1ull);
        if (guard & tl::kPairLaneBit) atomicAdd(&g_pair_lanes, 1ull);
    }
}

// MIX: a mix handle's launch (a.n_comp >= 1): the staged table is [n_scen][n_comp][len], n_scen * n_comp rows laid out like scenarios
// NOISE: a launch with a.noise_on (stored runs only): the seeded term of forcing_noise.hpp on top of the staged or read forcing, of the
// kind noise_kind(a.noise_on): kNoiseKindWhite, kNoiseKindRed, or kNoiseKindMembers (red with per-member sigma and phi)
template <int MODE, bool LDS, bool STORE, bool MIX = false, int NOISE = 0>
__global__ __launch_bounds__(kBlock) void two_layer_kernel(TwoLayerArgs a)
{
    extern __shared__ double lds_forcing[];
    if constexpr (LDS) {
        const int32_t len = a.step_end - a.step_begin;
        const int32_t total = (MIX ? a.n_scen * a.n_comp : a.n_scen) * len;
        for (int32_t idx = threadIdx.x; idx < total; idx += kBlock) {
            const int32_t s = idx / len, k = idx - s * len;
            lds_forcing[idx] = a.forcing[(size_t)s * a.n_times + a.step_begin + a.src_off + k];
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_members) return;
    const int32_t guard = tl::two_layer_body<MODE, LDS, STORE, NoCache, false, MIX, NOISE, true>(a, lds_forcing, i, a.step_begin, a.step_end);
    if constexpr (MODE == 0) count_guard(a, guard);
}

// The plain stored EXACT launch with the members' pair_div constants beside its arguments (TwoLayerArgs is full): the kernel above, whose
// uniform years form their quotients in two instructions in every wavefront whose members all have safe constants.  A kernel of its
// own, so that the launches without the constants run the kernels they ran.  (The staging loop is two_layer_kernel's, restated: moved
// into a function shared by the three kernels it reorders the prologue of every LDS instantiation, the mix, noise and FAST ones
// included, which are to stay the instructions they were.)
template <bool LDS>
__global__ __launch_bounds__(kBlock) void two_layer_pair_kernel(TwoLayerArgs a, const double* pair_div)
{
    extern __shared__ double lds_forcing[];
    if constexpr (LDS) {
        const int32_t len = a.step_end - a.step_begin;
        const int32_t total = a.n_scen * len;
        for (int32_t idx = threadIdx.x; idx < total; idx += kBlock) {
            const int32_t s = idx / len, k = idx - s * len;
            lds_forcing[idx] = a.forcing[(size_t)s * a.n_times + a.step_begin + a.src_off + k];
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_members) return;
    count_guard(a, tl::two_layer_body<0, LDS, true, NoCache, false, false, 0, true, true>(a, lds_forcing, i, a.step_begin, a.step_end, NoCache(),
                                                                                      nullptr, pair_div));
}

// The member constants of pair_div (rk4_device.hpp) for the two heat capacities, parameter rows 4 and 5 read the way the stepping kernel
// reads them: out[0][i], out[1][i] = zh, zl for Cs (vouched for down to the surface equation's numerators, pairdiv::kSurfaceNumFloor),
// out[2][i], out[3][i] for Cd; the constants the verdict tried, bit for bit, zh = 0 where it found none (pair_div_verdict.hpp).
__global__ __launch_bounds__(kBlock) void two_layer_pair_div_kernel(const double* params, uint64_t uniform_rows, int64_t n, double* out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const pairdiv::Constants s = pairdiv::verdict(param_at(params, uniform_rows, 4, n, i), pairdiv::kSurfaceNumFloor);
    const pairdiv::Constants d = pairdiv::verdict(param_at(params, uniform_rows, 5, n, i));
    out[i] = s.zh;
    out[n + i] = s.zl;
    out[2 * n + i] = d.zh;
    out[3 * n + i] = d.zl;
}

// rscm_gpu_selftest_pair_div: per pair the IEEE quotient, pair_div with the constants as defined, pair_div with the verdict's constants
// (NaN where it has none), and the verdict's variant.  num_lo: the window edge the verdict is asked for
__global__ __launch_bounds__(kBlock) void pair_div_selftest_kernel(const double* num, const double* den, int64_t n, int32_t num_lo, double* ieee,
                                                                   double* plain, double* tried, int32_t* variant)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const double x = num[j], d = den[j];
    ieee[j] = x / d;
    double zh, zl;
    pairdiv::plain_constants(d, zh, zl);
    plain[j] = pair_div(x, zh, zl);
    const pairdiv::Constants c = pairdiv::verdict(d, num_lo);
    tried[j] = c.zh != 0.0 ? pair_div(x, c.zh, c.zl) : __builtin_nan("");
    variant[j] = c.variant;
}

// e_t for rows [t_begin, t_end) x n members: what a noise handle of kind KIND adds to its forcing (rscm_ens_forcing_noise_rows).  White:
// sigma * z, as written.  Red: e_t of two_layer_body.hpp, formed from index 0 on by the same statements and written from t_begin on;
// per-member: the same with sigma and phi member i's, read the way the stepping kernel reads them
template <int KIND>
__global__ __launch_bounds__(kBlock) void forcing_noise_rows_kernel(uint64_t seed, double sigma, double phi, const double* params,
                                                                    uint64_t uniform_rows, int32_t sigma_row, int32_t phi_row, int64_t member0,
                                                                    int64_t n, int32_t t_begin, int32_t t_end, double* out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = (uint64_t)(member0 + i);
    double* o = out + i;
    if constexpr (KIND == kNoiseKindWhite) {   // (not the recurrence with phi = 0: (0 * e) + (sigma * z) has another zero's sign, and NaN once e is not finite)
        for (int32_t t = t_begin; t < t_end; ++t, o += n) *o = sigma * noise::draw(seed, g, (uint32_t)t);
    } else {
        if constexpr (KIND == kNoiseKindMembers) {
            sigma = param_at(params, uniform_rows, sigma_row, n, i);
            phi = param_at(params, uniform_rows, phi_row, n, i);
        }
        const double se = sigma * __builtin_sqrt(1.0 - phi * phi);
        double e = 0.0;
        for (int32_t t = 0; t < t_end; ++t) {
            const double z = noise::draw(seed, g, (uint32_t)t);
            e = t == 0 ? sigma * z : (phi * e) + (se * z);
            if (t >= t_begin) {
                *o = e;
                o += n;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void normal_selftest_kernel(const uint64_t* k52, int64_t n, double* z)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) z[j] = noise::normal_from_k(k52[j] & 0x000FFFFFFFFFFFFFull);
}

// The fused likelihood with reference periods: an instantiation of its own, so that launches without a period run the kernels above
// unchanged.
template <int MODE, bool LDS, bool MIX = false>
__global__ __launch_bounds__(kBlock) void two_layer_ref_kernel(TwoLayerArgs a, TwoLayerRefArgs r)
{
    extern __shared__ double lds_forcing[];
    if constexpr (LDS) {
        const int32_t len = a.step_end - a.step_begin;
        const int32_t total = (MIX ? a.n_scen * a.n_comp : a.n_scen) * len;
        for (int32_t idx = threadIdx.x; idx < total; idx += kBlock) {
            const int32_t s = idx / len, k = idx - s * len;
            lds_forcing[idx] = a.forcing[(size_t)s * a.n_times + a.step_begin + a.src_off + k];
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_members) return;
    const int32_t guard = tl::two_layer_body<MODE, LDS, false, NoCache, true, MIX, 0, true>(a, lds_forcing, i, a.step_begin, a.step_end, NoCache(), &r);
    if constexpr (MODE == 0) count_guard(a, guard);
}

}  // namespace

// (Round 5 built ONE persistent launch with a dependency-ordered work queue here -- tasks = (64-member block, chunk of steps) claimed by
// resident wavefronts, a block's chunk waiting only for the same block's previous chunk, the state handed over through device-scope
// accesses -- bit-identical to the plain launch, and removed it again: it never beat the two-stream cut of rscm_gpu.cpp.  The premise
// was wrong: 1e5 members are 1563 independent chains for 1024 SIMDs, a SIMD needs two to be saturated, and ONE wavefront alone runs at
// 0.93 of a saturated SIMD's rate (65 536 members: 1.505 ms; 131 072: 2.807) -- the configuration's own bound is 2.21 ms per pass, the
// cut runs take 2.31, the queue 2.45 with one wavefront per SIMD and worse with more (fewer blocks than wavefronts: every task waits for
// its predecessor).  DESIGN.md section 4.1, profiles/r5_queue_experiment.txt, commit history of this file.)

namespace {

// The eight shapes of a two-layer kernel, told apart in this one place: f is called with (MODE, LDS, MIX) as integral constants
template <class F>
constexpr auto with_shape(int mode, bool lds, bool mix, F f)
{
    auto with_mix = [&](auto M, auto L) { return mix ? f(M, L, std::true_type{}) : f(M, L, std::false_type{}); };
    auto with_lds = [&](auto M) { return lds ? with_mix(M, std::true_type{}) : with_mix(M, std::false_type{}); };
    return mode == 0 ? with_lds(std::integral_constant<int, 0>{}) : with_lds(std::integral_constant<int, 1>{});
}

// The families: the stepping kernel per (STORE, NOISE), and the fused likelihood with reference periods
using StepKernel = void (*)(TwoLayerArgs);
using RefKernel = void (*)(TwoLayerArgs, TwoLayerRefArgs);
template <bool STORE, int NOISE>
constexpr StepKernel step_kernel(int mode, bool lds, bool mix)
{
    return with_shape(mode, lds, mix, [](auto M, auto L, auto X) -> StepKernel { return two_layer_kernel<M(), L(), STORE, X(), NOISE>; });
}
constexpr RefKernel ref_kernel(int mode, bool lds, bool mix)
{
    return with_shape(mode, lds, mix, [](auto M, auto L, auto X) -> RefKernel { return two_layer_ref_kernel<M(), L(), X()>; });
}
// (a transposed index fails the build here, not a run)
static_assert(step_kernel<true, kNoiseKindRed>(0, true, false) == two_layer_kernel<0, true, true, false, 2>);
static_assert(step_kernel<true, kNoiseKindMembers>(1, false, true) == two_layer_kernel<1, false, true, true, 3>);
static_assert(step_kernel<false, kNoiseKindNone>(1, true, false) == two_layer_kernel<1, true, false, false, 0>);
static_assert(ref_kernel(0, false, true) == two_layer_ref_kernel<0, false, true>);

}  // namespace

// What every two-layer launch is refused for: a component count out of range, a linked mix launch, a noise code that is none
// (rscm_device.hpp), noise that is linked, and noise that keeps state without the state
static bool args_ok(const TwoLayerArgs& a)
{
    if (a.n_comp < 0 || a.n_comp > kMaxForcingComponents || (a.n_comp > 0 && a.link)) return false;
    if (a.noise_on && (a.link || noise_kind(a.noise_on) == kNoiseKindNone)) return false;
    return !noise_keeps_state(a.noise_on) || a.noise_state;
}

// ... and how every one of them ends: `rest` is what the kernel takes after the arguments
template <class... Rest>
static hipError_t launch_shaped(void (*kern)(TwoLayerArgs, Rest...), const TwoLayerArgs& a, hipStream_t s, const Rest&... rest)
{
    const size_t lds = a.lds_forcing ? two_layer_lds_bytes(a.n_scen, a.n_comp, a.step_end - a.step_begin) : 0;
    const dim3 grid((unsigned)((a.n_members + kBlock - 1) / kBlock));
    if (lds > (size_t)kMaxStaticLds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, s, a, rest...);
    return hipGetLastError();
}

template <bool STORE>
static hipError_t launch_impl(const TwoLayerArgs& a, int mode, hipStream_t s)
{
    if (a.n_members <= 0) return hipSuccess;
    if (STORE && a.step_end <= a.step_begin) return hipSuccess;
    if (!args_ok(a) || (a.noise_on && !STORE)) return hipErrorInvalidValue;   // noise: the stored run of a handle that is not linked, only
    const bool lds = a.lds_forcing != 0, mix = a.n_comp > 0;
    StepKernel kern = step_kernel<STORE, kNoiseKindNone>(mode, lds, mix);
    if constexpr (STORE) {
        switch (noise_kind(a.noise_on)) {
            case kNoiseKindWhite: kern = step_kernel<true, kNoiseKindWhite>(mode, lds, mix); break;
            case kNoiseKindRed: kern = step_kernel<true, kNoiseKindRed>(mode, lds, mix); break;
            case kNoiseKindMembers: kern = step_kernel<true, kNoiseKindMembers>(mode, lds, mix); break;
        }
    }
    return launch_shaped(kern, a, s);
}

// pair_div: the members' quotient constants for a launch whose year_facts say kYearPairValid (first member's; rows a.row_stride apart)
hipError_t launch_two_layer(const TwoLayerArgs& a, int mode, hipStream_t s, const double* pair_div)
{
    if (!year_pair_valid(a.year_facts)) return launch_impl<true>(a, mode, s);
    if (!pair_div || mode != 0 || a.n_comp != 0 || a.noise_on || a.link || !args_ok(a)) return hipErrorInvalidValue;
    if (a.n_members <= 0 || a.step_end <= a.step_begin) return hipSuccess;
    return launch_shaped(a.lds_forcing ? two_layer_pair_kernel<true> : two_layer_pair_kernel<false>, a, s, pair_div);
}

hipError_t launch_two_layer_loglik(const TwoLayerArgs& a, int mode, hipStream_t s)
{
    return launch_impl<false>(a, mode, s);
}

hipError_t launch_forcing_noise_rows(int32_t kind, uint64_t seed, double sigma, double phi, const double* params, uint64_t uniform_rows,
                                     int32_t sigma_row, int32_t phi_row, int64_t member0, int64_t n_members, int32_t t_begin, int32_t t_end,
                                     double* out, hipStream_t s)
{
    if (n_members <= 0 || t_end <= t_begin) return hipSuccess;
    if (kind == kNoiseKindMembers && (!params || sigma_row < 0 || phi_row < 0)) return hipErrorInvalidValue;
    auto kern = forcing_noise_rows_kernel<kNoiseKindWhite>;
    if (kind == kNoiseKindRed) kern = forcing_noise_rows_kernel<kNoiseKindRed>;
    else if (kind == kNoiseKindMembers) kern = forcing_noise_rows_kernel<kNoiseKindMembers>;
    else if (kind != kNoiseKindWhite) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_members + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, seed, sigma, phi, params, uniform_rows,
                       sigma_row, phi_row, member0, n_members, t_begin, t_end, out);
    return hipGetLastError();
}

hipError_t launch_normal_selftest(const uint64_t* k52, int64_t n, double* z, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(normal_selftest_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, k52, n, z);
    return hipGetLastError();
}

hipError_t launch_two_layer_loglik_ref(const TwoLayerArgs& a, const TwoLayerRefArgs& r, int mode, hipStream_t s)
{
    if (a.n_members <= 0) return hipSuccess;
    if (!args_ok(a) || a.noise_on) return hipErrorInvalidValue;   // (the fused likelihood of a noise handle is refused at the entry points)
    return launch_shaped(ref_kernel(mode, a.lds_forcing != 0, a.n_comp > 0), a, s, r);
}

hipError_t launch_two_layer_pair_div(const double* params, uint64_t uniform_rows, int64_t n_members, double* out, hipStream_t s)
{
    if (n_members <= 0) return hipSuccess;
    hipLaunchKernelGGL(two_layer_pair_div_kernel, dim3((unsigned)((n_members + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, params, uniform_rows,
                       n_members, out);
    return hipGetLastError();
}

hipError_t launch_pair_div_selftest(const double* num, const double* den, int64_t n, int32_t num_lo, double* ieee, double* plain, double* tried,
                                    int32_t* variant, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pair_div_selftest_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, num, den, n, num_lo, ieee, plain,
                       tried, variant);
    return hipGetLastError();
}

// the wavefronts that took the pair lane in the counting launches since the last call; the count is reset
hipError_t two_layer_pair_lanes(int64_t* out)
{
    unsigned long long c = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(&c, HIP_SYMBOL(g_pair_lanes), sizeof c);
    if (e != hipSuccess) return e;
    if (out) *out = (int64_t)c;
    const unsigned long long zero = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_pair_lanes), &zero, sizeof zero);
}

hipError_t two_layer_guard_counts(int64_t* out)
{
    unsigned long long c[tl::kGuardKinds] = {};
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && out) e = hipMemcpyFromSymbol(c, HIP_SYMBOL(g_guard_counts), sizeof c);
    if (e != hipSuccess) return e;
    if (out)
        for (int k = 0; k < tl::kGuardKinds; ++k) out[k] = (int64_t)c[k];
    const unsigned long long zero[tl::kGuardKinds] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_guard_counts), zero, sizeof zero);
}

}  // namespace rscm
