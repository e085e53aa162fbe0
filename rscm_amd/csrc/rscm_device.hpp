// Internal launch interface between the C-ABI layer (rscm_gpu.cpp) and the gfx950 kernels.
// Not part of the public boundary (that is include/rscm_gpu.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rscm {

#ifndef RSCM_BLOCK
#define RSCM_BLOCK 256
#endif
// The RSCM_KIND_* values of include/rscm_gpu.h that the kernels dispatch on (the device code does not
// include the public header; rscm_gpu.cpp static_asserts that the two agree).
enum Kind : int {
    kKindOzoneForcing = 4, kKindAerosolDirect = 5, kKindAerosolIndirect = 6, kKindCh4Chemistry = 7, kKindN2oChemistry = 8,
    kKindCo2Budget = 9, kKindTerrestrialCarbon = 10, kKindFourBoxOhu = 13, kKindOspp = 14, kKindCarbonCycle = 15,
    kKindCo2Erf = 16, kKindAggregate = 17
};

constexpr int kBlock = RSCM_BLOCK;           // 256 = 4 wavefronts of 64: one per SIMD of a CU
constexpr int kMaxStaticLds = 64 * 1024;     // above this the launcher raises the dynamic limit
constexpr int kMaxLds = 160 * 1024;          // CDNA4: 160 KiB per CU
constexpr int kMaxForcingComponents = 8;     // RSCM_TL_MAX_COMPONENTS: forcing components of a two-layer mix handle
constexpr int kTwoLayerCoeff0 = 6;           // RSCM_TL_P_COEFF0: the parameter row of its first coefficient
constexpr uint32_t kNoiseStreamTag = 0x4E5Au;   // RSCM_NOISE_STREAM_TAG ("NZ"): the Philox stream of the forcing noise (forcing_noise.hpp)

// Linked inputs (rscm_ens_link_input): input row k of a member is read from the stored series of
// another ensemble of the same shape -- row[k] is that series, [T][N], off[k] the index offset of
// the reference's VariableSource (0: Exogenous / OwnState -> index n, 1: UpstreamOutput -> n+1).
// Where a fused multi-step launch (csrc/group.hip) keeps an op's per-member values between model steps: LDS
// slots (one double per thread each) instead of the round trip through HBM.  -1: not kept.
struct OpCache {
    int32_t series_slot;   // first slot of the latest row of the op's own series (its state, and what consumers read)
    int32_t param_slot;    // first slot of its parameter rows
    int32_t link_slot[8];  // per input row: the slot of the producer's value this link reads at the current step
    uint32_t link_warm;    // bit k: link k reads what its producer kept in the PREVIOUS step (feedback): not at a launch's first step
};

// A null row[k] leaves row k with the scenario table.  Passed by value: the kernels read it from
// the kernarg segment with scalar loads.
constexpr int kMaxLinks = 8;
struct InputLinks {
    const double* row[kMaxLinks];
    int32_t off[kMaxLinks];
};

#ifdef __HIPCC__
// Parameter j of member i from the [P][N] block.  Rows the host found to be the same for every member
// (bit j of `uniform`, rows 0..63) are read from element 0 by every lane: one 64-byte request per
// wavefront from a line that stays hot in L1/L2 instead of 512 coalesced bytes from HBM -- in a graph
// of linked ensembles most rows are uniform (a calibration varies a handful), and the light
// components' launches are bound by exactly this traffic.  The value read is the same either way.
__device__ __forceinline__ double param_at(const double* __restrict__ params, uint64_t uniform, int j, int64_t N, int64_t i)
{
    const bool u = j < 64 && ((uniform >> (j & 63)) & 1ull) != 0;
    return params[(size_t)j * N + (u ? (int64_t)0 : i)];
}

// The same value, with a uniform row read through the constant address space: s_load_dwordx2 into scalar
// registers -- no vector memory instruction, no address arithmetic per lane, and code that branches on the
// value (the aggregate's operation) branches uniformly.  For the light bodies only: in the register-bound
// kernels (ClimateUDEB, OceanCarbon) dozens of parameters in scalar registers spill.  The block is not
// written while a kernel that reads it runs.
__device__ __forceinline__ double param_at_scalar(const double* __restrict__ params, uint64_t uniform, int j, int64_t N, int64_t i)
{
    const bool u = j < 64 && ((uniform >> (j & 63)) & 1ull) != 0;  // wave-uniform: a scalar branch
    if (u) {
        typedef const __attribute__((address_space(4))) double* scalar_row;
        // (the row address is wave-uniform; saying so keeps the scalar load legal where register pressure has moved the
        // pointer into vector registers -- without it hipcc 7.2 emits an s_load with a VGPR address there and stops with
        // "Illegal instruction detected: Operand has incorrect register class"; a no-op when the address is scalar already)
        const uintptr_t p = (uintptr_t)(params + (size_t)j * N);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
        return *(scalar_row)(((uintptr_t)hi << 32) | lo);
    }
    return params[(size_t)j * N + i];
}

// All P parameter rows of a component at once.  Where every row is uniform (the usual case in a graph of linked ensembles:
// a calibration varies a handful of rows of a few components) these are P scalar loads issued back to back and awaited
// ONCE; asked for one by one through param_at_scalar each sits behind its own uniform-bit branch and is awaited before
// the next is issued -- 27 dependent trips through the scalar cache per model step for AerosolDirect, and the fused
// launches of the light components spend two thirds of their time in s_waitcnt (gpurun_out/r3e).
// Mixed blocks take the vector loads of param_at: no branches either, one wait.
template <int P>
__device__ __forceinline__ void params_block(const double* __restrict__ params, uint64_t uniform, int64_t N, int64_t i, double (&p)[P])
{
    constexpr uint64_t mask = P >= 64 ? ~0ull : ((1ull << P) - 1ull);
    if ((uniform & mask) == mask) {
        typedef const __attribute__((address_space(4))) double* scalar_row;
        const uintptr_t q = (uintptr_t)params;   // (wave-uniform; said so for the reason given in param_at_scalar)
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)q), hi = __builtin_amdgcn_readfirstlane((uint32_t)(q >> 32));
        const scalar_row row0 = (scalar_row)(((uintptr_t)hi << 32) | lo);
#pragma unroll
        for (int j = 0; j < P; ++j) p[j] = row0[(size_t)j * N];
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) p[j] = param_at(params, uniform, j, N, i);
    }
}

// How a body reads parameters, its own previous state and linked inputs, and where it leaves its results
// besides the series in HBM.  The stand-alone kernels use NoCache (everything compiles to the plain loads);
// the fused multi-step launch passes an LdsCache.
struct NoCache {
    static constexpr bool kOn = false;
    __device__ __forceinline__ double param(const double* __restrict__ params, uint64_t uniform, int j, int64_t N, int64_t i) const
    {
        return param_at(params, uniform, j, N, i);
    }
    __device__ __forceinline__ double param_scalar(const double* __restrict__ params, uint64_t uniform, int j, int64_t N, int64_t i) const
    {
        return param_at_scalar(params, uniform, j, N, i);
    }
    template <int P>
    __device__ __forceinline__ void params(const double* __restrict__ block, uint64_t uniform, int64_t N, int64_t i, double (&p)[P]) const
    {
        params_block<P>(block, uniform, N, i, p);
    }
    __device__ __forceinline__ double state(int, const double* p) const { return *p; }
    __device__ __forceinline__ void put(int, double) const {}
    __device__ __forceinline__ bool has_link(int) const { return false; }
    __device__ __forceinline__ double link(int) const { return 0.0; }
    __device__ __forceinline__ bool last_step() const { return true; }
};

// Thread-private columns of LDS: slot s of this thread at col[s * kCacheStride].  Every value is written and
// read by the same thread, in program order: no barrier.  WARM: not the first model step of the launch, so
// the slots hold what the previous step left (the launch runs its first step with the cold variant).  What comes out of a slot is the double that went in -- the
// same bits as the row in HBM, which is still written every step.
// STRIDE: threads per workgroup (the fused group kernel: kBlock; the whole-graph kernel: one wavefront).
template <bool WARM, int STRIDE = kBlock>
struct LdsCache {
    static constexpr bool kOn = true;
    static constexpr int kCacheStride = STRIDE;
    double* col;
    OpCache c;
    bool last;
    __device__ __forceinline__ double param(const double* __restrict__ params, uint64_t uniform, int j, int64_t N, int64_t i) const
    {
        const bool u = j < 64 && ((uniform >> (j & 63)) & 1ull) != 0;
        if (u || c.param_slot < 0) return param_at_scalar(params, uniform, j, N, i);  // a uniform row is one scalar load
        double* slot = col + (size_t)(c.param_slot + j) * kCacheStride;
        if constexpr (WARM) {
            return *slot;
        } else {
            const double v = params[(size_t)j * N + i];
            *slot = v;
            return v;
        }
    }
    __device__ __forceinline__ double param_scalar(const double* __restrict__ params, uint64_t uniform, int j, int64_t N, int64_t i) const
    {
        return param(params, uniform, j, N, i);
    }
    template <int P>
    __device__ __forceinline__ void params(const double* __restrict__ block, uint64_t uniform, int64_t N, int64_t i, double (&p)[P]) const
    {
        constexpr uint64_t mask = P >= 64 ? ~0ull : ((1ull << P) - 1ull);
        if ((uniform & mask) == mask) {   // nothing of this block lives in a slot
            params_block<P>(block, uniform, N, i, p);
            return;
        }
#pragma unroll
        for (int j = 0; j < P; ++j) p[j] = param(block, uniform, j, N, i);
    }
    __device__ __forceinline__ double state(int v, const double* p) const
    {
        if constexpr (WARM) {
            if (c.series_slot >= 0) return col[(size_t)(c.series_slot + v) * kCacheStride];
        }
        return *p;
    }
    __device__ __forceinline__ void put(int v, double x) const
    {
        if (c.series_slot >= 0) col[(size_t)(c.series_slot + v) * kCacheStride] = x;
    }
    __device__ __forceinline__ bool has_link(int k) const
    {
        return c.link_slot[k] >= 0 && (WARM || ((c.link_warm >> k) & 1u) == 0);
    }
    __device__ __forceinline__ double link(int k) const { return col[(size_t)c.link_slot[k] * kCacheStride]; }
    __device__ __forceinline__ bool last_step() const { return last; }
};

// The same interface with an op's parameters and its own latest row in REGISTERS for the whole launch (csrc/group.hip,
// group_seq_kernel: a kernel compiled for a sequence of kinds keeps one of these per op across its step loop).  The bodies are
// inlined into that loop; what they form from the parameters alone -- reciprocals of heat capacities and lifetimes, folded
// coefficients, h/3 -- is loop-invariant to the compiler and leaves the loop, the state needs no trip through LDS, and only what
// OTHER ops read goes through the LDS slots (put() writes both).  prm / st point at arrays in the kernel's frame; every index the
// bodies pass is a literal after inlining, so the arrays are registers.  What comes out is the double that went in: the same bits.
template <bool WARM, int STRIDE = kBlock>
struct RegCache {
    static constexpr bool kOn = true;
    static constexpr int kCacheStride = STRIDE;
    const double* prm;   // [P] this member's parameter values, loaded once per launch
    double* st;          // [V - 1] the op's latest row (its state for the next step)
    double* col;         // this thread's column of LDS slots
    OpCache c;
    bool last;
    __device__ __forceinline__ double param(const double* __restrict__, uint64_t, int j, int64_t, int64_t) const { return prm[j]; }
    __device__ __forceinline__ double param_scalar(const double* __restrict__, uint64_t, int j, int64_t, int64_t) const { return prm[j]; }
    template <int P>
    __device__ __forceinline__ void params(const double* __restrict__, uint64_t, int64_t, int64_t, double (&p)[P]) const
    {
#pragma unroll
        for (int j = 0; j < P; ++j) p[j] = prm[j];
    }
    __device__ __forceinline__ double state(int v, const double*) const { return st[v]; }
    __device__ __forceinline__ void put(int v, double x) const
    {
        st[v] = x;
        if (c.series_slot >= 0) col[(size_t)(c.series_slot + v) * kCacheStride] = x;
    }
    __device__ __forceinline__ bool has_link(int k) const
    {
        return c.link_slot[k] >= 0 && (WARM || ((c.link_warm >> k) & 1u) == 0);
    }
    __device__ __forceinline__ double link(int k) const { return col[(size_t)c.link_slot[k] * kCacheStride]; }
    __device__ __forceinline__ bool last_step() const { return last; }
};

// The NI input rows of member i.  SRC 0: one shared table [NI][T]; 1: per-member scenario of a
// table [S][NI][T]; 2: linked rows (coalesced [T][N] reads) mixed with table rows.  SRC < 2
// compiles to the plain table indexing the kernels had before links existed.
template <int SRC, int NI>
struct MemberInputs {
    const double* base;
    int32_t T;
    int64_t N, i;
    const InputLinks* links;
    __device__ __forceinline__ MemberInputs(const double* table, const int32_t* scen, const InputLinks& links_, int32_t n_times, int64_t N_,
                                            int64_t i_)
        : T(n_times), N(N_), i(i_), links(&links_)
    {
        static_assert(SRC != 2 || NI <= kMaxLinks, "more input rows than InputLinks holds");
        const size_t s = SRC == 0 ? (size_t)0 : (scen ? (size_t)scen[i_] : (size_t)0);
        base = table + s * NI * n_times;
    }
    // SRC 2: the address is formed where the value is wanted (wave-uniform row choice, a few scalar
    // instructions) -- in a fused launch most linked values come out of LDS and need none
    __device__ __forceinline__ double at(int k, int32_t n) const
    {
        if constexpr (SRC == 2) {
            const double* row = links->row[k];
            if (row) return row[(size_t)(links->off[k] + n) * N + i];
        }
        return base[(size_t)k * T + n];
    }
    // the value of the CURRENT model step (the one the fused launch is at): from the producer's LDS slot if kept there
    template <class Cache>
    __device__ __forceinline__ double at(int k, int32_t n, const Cache& cache) const
    {
        if constexpr (Cache::kOn && SRC == 2) {
            if (cache.has_link(k)) return cache.link(k);
        }
        return at(k, n);
    }
};

// The NI rows of one model step, asked for together.  The light bodies request the rows of their first step -- and their
// state -- before they do any arithmetic on their parameters, and in a launch over several steps the rows of step n + 1
// while step n is computed: a component's step is then ONE trip to memory (parameters, state and inputs in flight
// together) where it was two or three (parameters; the quotients formed from them; then state and inputs, behind the
// status byte's store, which may alias anything).  Fused launches of light components are bound by exactly these trips.
template <int NI>
struct StepRows {
    double v[NI];
};
template <int SRC, int NI>
__device__ __forceinline__ StepRows<NI> rows_at(const MemberInputs<SRC, NI>& in, int32_t n)
{
    StepRows<NI> r;
#pragma unroll
    for (int k = 0; k < NI; ++k) r.v[k] = in.at(k, n);
    return r;
}

// The same rows with every address formed once, up front (pointer + stride per row in vector registers):
// for kernels that read their inputs inside long multi-step loops and are short of SCALAR registers
// (OceanCarbon's convolution keeps a 47-entry window of the response table there).
template <int SRC, int NI>
struct MemberInputsEager {
    const double* base;
    int32_t T;
    const double* p[SRC == 2 ? NI : 1];
    size_t stride[SRC == 2 ? NI : 1];
    __device__ __forceinline__ MemberInputsEager(const double* table, const int32_t* scen, const InputLinks& links, int32_t n_times, int64_t N,
                                                 int64_t i)
        : T(n_times)
    {
        static_assert(SRC != 2 || NI <= kMaxLinks, "more input rows than InputLinks holds");
        const size_t s = SRC == 0 ? (size_t)0 : (scen ? (size_t)scen[i] : (size_t)0);
        base = table + s * NI * n_times;
        if constexpr (SRC == 2) {
#pragma unroll
            for (int k = 0; k < NI; ++k) {
                if (links.row[k]) {
                    p[k] = links.row[k] + (size_t)links.off[k] * N + i;
                    stride[k] = (size_t)N;
                } else {
                    p[k] = base + (size_t)k * n_times;
                    stride[k] = 1;
                }
            }
        }
    }
    __device__ __forceinline__ double at(int k, int32_t n) const
    {
        if constexpr (SRC == 2) return p[k][(size_t)n * stride[k]];
        else return base[(size_t)k * T + n];
    }
};

// kernel<0> / kernel<1> / kernel<2> by where the inputs come from
#define RSCM_LAUNCH_BY_SOURCE(KERNEL, args, grid, block, stream, ...)                                        \
    do {                                                                                                     \
        if ((args).linked) hipLaunchKernelGGL((KERNEL<2>), grid, block, 0, stream, __VA_ARGS__);             \
        else if ((args).scen) hipLaunchKernelGGL((KERNEL<1>), grid, block, 0, stream, __VA_ARGS__);          \
        else hipLaunchKernelGGL((KERNEL<0>), grid, block, 0, stream, __VA_ARGS__);                           \
    } while (0)
#endif

// Stand-alone two-layer run over steps [step_begin, step_end).
struct TwoLayerArgs {
    int64_t n_members;       // members this launch covers ...
    int64_t row_stride;      // ... of an ensemble of this many: the stride of the [rows][N] series and [P][N] parameter rows.  Equal
                             // unless the host launches a BLOCK of members (pointers moved to its first member; rscm_gpu.cpp, split runs)
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t n_scen;
    int32_t src_off;         // 0: Exogenous -> F[n]; 1: UpstreamOutput -> F[n+1]
    int32_t lds_forcing;     // 1: forcing slice staged in LDS ([S][max(n_comp, 1)][len]), 0: read through L2
    const double* params;    // [6][N] ([6 + n_comp][N] for a mix handle)
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* forcing;   // [S][T] ([S][n_comp][T] for a mix handle)
    const double* link;      // [T][N] linked forcing (InputLinks, one row) or nullptr
    const int32_t* scen;     // [N] or nullptr
    const int32_t* nsub;     // [T-1] RK4 sub-steps of step n = ceil((b[n+1]-b[n])/h)
    double h;                // RK4 step (reference: 0.1)
    double h_half, h_sixth;  // h / 2.0 and h / 6.0 as the host's IEEE division rounds them (= the device's): uniform
                             // values, but a per-lane division per launch -- per model step in a fused graph launch
    double* ts;              // [T][N]
    double* td;              // [T][N]
    uint8_t* status;         // [N]
    // Fused likelihood (launch_two_layer_loglik): no series rows beyond step_begin are written;
    // observations merged over both variables and sorted by time index.
    int32_t n_obs;
    int32_t normalize;
    int32_t first_is_deep;        // which variable's group comes first in the caller's order
    int32_t numerator_guard;      // EXACT: 1 forces the per-numerator guard of every speculative year (test hook,
                                  // rscm_gpu_set_two_layer_guard); 0 guards the sub-step states where the boxes allow it
    int32_t count_guards;         // EXACT stand-alone launches: 1 counts the guard each wavefront took (test hook,
                                  // rscm_gpu_two_layer_guard_counts); 0 counts nothing
    int32_t n_comp;               // 0: `forcing` is [S][T].  K in 1..kMaxForcingComponents (a mix handle, rscm_ens_create_mix): `forcing`
                                  // is [S][K][T], `params` has rows 6..6+K-1 and member i is forced by ((S_0 c_0 + S_1 c_1) + ...) + S_K-1 c_K-1,
                                  // every product and sum rounded on its own (the MIX instantiations; never linked).  Sits in what was
                                  // padding: the layout of the other fields is that of the plain launches
    const int32_t* obs_tidx;      // [n_obs] ascending
    const int32_t* obs_is_deep;   // [n_obs] 0: Surface Temperature, 1: Deep Ocean Temperature
    const double* obs_value;
    const double* obs_sigma;
    union {
        double* loglik;           // [N]
        double* noise_state;      // [N] the noise kinds that keep state (below): a stored run scores nothing and the fused likelihood carries no noise
    };
    // Forcing noise (rscm_ens_set_forcing_noise*; the NOISE instantiations: stand-alone stored runs, never linked).  noise_on is a
    // kNoise* code (below): which kind of noise, noise_kind(), and for the kinds that keep state whether e is cached.  Member i of this
    // launch is forced by F' = F + e_t at forcing-axis index t = n + src_off, z_t = z(noise_seed, noise_member0 + i, t) the stateless
    // deviate of forcing_noise.hpp and every operation rounded on its own:
    //   white    e_t = noise_sigma * z_t
    //   red      e_0 = noise_sigma * z_0,    e_t = noise_phi * e_{t-1} + (noise_sigma * sqrt(1 - noise_phi^2)) * z_t
    //   members  the red recurrence with member i's sigma_i and phi_i, read once per launch from parameter rows kTwoLayerCoeff0 + n_comp
    //            and the one after it through `params` and `uniform_rows` like every other row; noise_sigma and noise_phi are not read
    // noise_member0 is the id in the whole ensemble of the launch's first member: the handle's member_offset, plus the block's first
    // member where the host launches a block (block_of, launch_host.cpp).  The kinds that keep state (noise_keeps_state()): noise_state[i]
    // (above, in the place of the fused likelihood's result: the struct is full at the 240 bytes the op union allows) is member i's slot
    // of the handle's cache, moved with the block like noise_member0.  A spin-up code: the launch forms e up to the index before its
    // first from the draws (nothing to form when that first index is 0); a cached code: noise_state holds e there.  Either way the
    // launch leaves e at the last index it drew, step_end - 1 + src_off, in noise_state.  At the end: the other fields keep the offsets
    // of the launches without noise
    uint64_t noise_seed;
    double noise_sigma;
    int64_t noise_member0;
    int32_t noise_on;
    uint32_t year_facts;     // what the host has proved about the launch's years (year_facts_word below; two_layer_year_facts.hpp); 0: nothing.
                             // Sits in what was padding, like n_comp
    double noise_phi;
};
// TwoLayerArgs::year_facts: the low bits hold the sub-step count that every step of [step_begin, step_end) has (0: they differ, or
// nobody looked), the top bit says that every forcing value the launch can read is +0 or a magnitude in the chunk guard's forcing box
// (two_layer_chunk_box.hpp) -- set for a plain table only: no link, no mix, no noise.  The bit below it says that the launch comes with
// the member constants of the two-instruction quotient, formed from the parameter rows as they stand (launch_two_layer's pair_div:
// stored stand-alone launches of the plain table only; the same in every chunk of a cut run).  The struct is full, so the pointer
// travels beside it as a kernel argument of its own.  A fused launch passes 0.
constexpr uint32_t kYearForcingBoxed = 0x80000000u, kYearPairValid = 0x40000000u;
constexpr uint32_t year_facts_word(int32_t nsub_uniform, bool forcing_boxed, bool pair_valid = false)
{
    return (nsub_uniform > 0 ? (uint32_t)nsub_uniform : 0u) | (forcing_boxed ? kYearForcingBoxed : 0u) | (pair_valid ? kYearPairValid : 0u);
}
constexpr int32_t year_nsub_uniform(uint32_t facts) { return (int32_t)(facts & ~(kYearForcingBoxed | kYearPairValid)); }
constexpr bool year_forcing_boxed(uint32_t facts) { return (facts & kYearForcingBoxed) != 0; }
constexpr bool year_pair_valid(uint32_t facts) { return (facts & kYearPairValid) != 0; }
// The kinds of forcing noise: a handle's setting (rscm_ens::noise_kind) and the NOISE template value of the two-layer kernels
constexpr int32_t kNoiseKindNone = 0, kNoiseKindWhite = 1, kNoiseKindRed = 2, kNoiseKindMembers = 3;
// TwoLayerArgs::noise_on (0: no noise): a kind, and for red and members whether noise_state holds e at the index before the launch's
// first.  The kernels compare against these values and the ops of a fused launch are compared bytewise: the numbers are fixed.  What a
// code means is stated by the three functions below and nowhere else
constexpr int32_t kNoiseWhite = 1, kNoiseRedSpinUp = 2, kNoiseRedCached = 3, kNoiseMembersSpinUp = 4, kNoiseMembersCached = 5;
constexpr int32_t noise_kind(int32_t on)   // kNoiseKindNone for 0 and for a value that is no code
{
    return on == kNoiseWhite                                         ? kNoiseKindWhite
           : on == kNoiseRedSpinUp || on == kNoiseRedCached          ? kNoiseKindRed
           : on == kNoiseMembersSpinUp || on == kNoiseMembersCached  ? kNoiseKindMembers
                                                                     : kNoiseKindNone;
}
constexpr bool noise_kind_keeps_state(int32_t kind) { return kind == kNoiseKindRed || kind == kNoiseKindMembers; }
constexpr bool noise_keeps_state(int32_t on) { return noise_kind_keeps_state(noise_kind(on)); }   // the launch reads or writes noise_state
constexpr int32_t noise_code(int32_t kind, bool cached)
{
    return kind == kNoiseKindWhite     ? kNoiseWhite
           : kind == kNoiseKindRed     ? (cached ? kNoiseRedCached : kNoiseRedSpinUp)
           : kind == kNoiseKindMembers ? (cached ? kNoiseMembersCached : kNoiseMembersSpinUp)
                                       : 0;
}
static_assert(noise_code(kNoiseKindWhite, true) == kNoiseWhite && noise_kind(noise_code(kNoiseKindMembers, true)) == kNoiseKindMembers &&
                  noise_kind(noise_code(kNoiseKindRed, false)) == kNoiseKindRed && !noise_keeps_state(kNoiseWhite) && noise_kind(6) == kNoiseKindNone,
              "noise_kind, noise_keeps_state and noise_code must agree");
static_assert(sizeof(TwoLayerArgs) == 240, "TwoLayerArgs must not grow the fused launches' op union");

// Reference periods of the fused likelihood (launch_two_layer_loglik_ref; DESIGN.md section 7, "Reference periods"), index 0: Surface
// Temperature, 1: Deep Ocean Temperature.  A variable with on[v] is scored as the anomaly from the member's own mean b over the rows
// begin[v], begin[v] + stride[v], ... <= last[v]: the thread sums those rows while it steps; the model values of that variable's
// observations at rows <= last[v] wait in `defer` until the last reference row has formed b.
struct TwoLayerRefArgs {
    int32_t on[2];
    int32_t begin[2], last[2], stride[2], count[2];
    const int32_t* obs_slot;   // [n_obs] (the merged order of TwoLayerArgs::obs_tidx): row of `defer`, -1 for an observation scored on the fly
    double* defer;             // [n_deferred][N] handle-owned scratch
};

// Coupled chain CarbonCycle -> CO2ERF -> Sum -> TwoLayer over steps [step_begin, step_end).
struct CoupledArgs {
    int64_t n_members;
    int64_t row_stride;      // as in TwoLayerArgs
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t n_scen;
    int32_t lds_forcing;
    const double* params;     // [10][N]
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* emissions;  // [S][T]
    const int32_t* scen;
    const int32_t* nsub_tl;   // [T-1]
    const int32_t* nsub_cc;   // [T-1]
    double h_tl, h_cc;
    double* ts; double* td; double* conc; double* cum_uptake; double* cum_emis;
    double* erf_co2; double* erf_total;   // each [T][N]
    uint8_t* status;
};

// ClimateUDEB (rscm-magicc) over steps [step_begin, step_end).
constexpr int kUdebBlock = 64;  // one wavefront per workgroup: ~250 VGPRs per lane
constexpr int kUdebNParams = 37;
constexpr int kUdebScalars = 11;
constexpr int kUdebMaxOnChipLayers = 64;   // up to this many ocean layers a member's columns stay in registers + LDS (csrc/udeb.hip)
constexpr int kUdebMaxLdsLayers = 128;     // ... and up to this many with the Thomas sweep's c' array in LDS (a hemisphere per wavefront)
// The geometry table has two homes, and the unrolled sweeps read BOTH by their compiled CAPACITY, not by the layer count (rows past
// the count are zero rows: exact no-ops).  So each home must hold, zero-padded, as many rows as the largest capacity that reads it:
//   UdebArgs::tables (by value, kernarg)  <- every on-chip instance,        capacity <= kUdebArgTableRows
//   rscm_ens::d_udeb_tables (device)      <- the c'-in-LDS instance,        capacity <= kUdebDevTableRows
// udeb_body.hpp static_asserts each instantiation against its home; rscm_gpu.cpp allocates and zero-fills by these constants.
constexpr int kUdebArgTableRows = kUdebMaxOnChipLayers;
constexpr int kUdebDevTableRows = kUdebMaxLdsLayers;

struct UdebArgs {
    int64_t n_members;
    int64_t row_stride;     // as in TwoLayerArgs: the stride of every [..][N] array when a block of members is launched
    int64_t n_total;        // members of the whole ensemble (0: n_members): the kernel variant is chosen by this, so that the member
                            // blocks of one cut run take one kernel
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t n_scen;
    int32_t n_layers, steps_per_year, land_hc, efficacy_apply;  // uniform over the ensemble
    int32_t fast;           // RSCM_MODE_FAST: one refinement term of the row reciprocals instead of two
    const double* params;   // [37][N], ClimateUDEBParameters order (include/rscm_gpu.h)
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* erf;      // [S][T]
    const int32_t* scen;    // [N] or nullptr
    const double* link;     // [T][N] linked forcing or nullptr
    const double* bounds;   // [T+1] (device)
    const int32_t* win_kfull;  // [T] first history entry that enters the cumulative-T window whole
    const double* win_partw;   // [T] weight of entry win_kfull-1 (0: not in the window)
    // rows [NL][6] = {af_top, af_bot, af_diff, 1 - rel_depth, G_nh, G_sh}, NL = n_layers <= 64 (udeb_tables.hpp), zero rows after
    // them: passed BY VALUE so the kernel reads them from the kernarg segment with scalar loads (no VGPRs, no vmcnt)
    double tables[6 * kUdebArgTableRows];
    const double* derived;     // [kDerivedRows][N] member constants: the base LAMCALC solve (launch_udeb_derive; udeb_body.hpp)
    int32_t derived_uniform;   // every parameter row it is formed from is uniform: element 0 serves all members
    const double* tables_dev;  // the same rows in device memory, any NL: the columns-in-HBM kernel (udeb_any_body.hpp); else nullptr
    double* work;              // [NL][N] the Thomas sweep's c' array of that kernel; else nullptr
    double* ocean;          // [2][NL][N] layer temperatures
    double* scal;           // [10][N] upwelling, land, ground, alpha_eff, hemi exchange (x2 hemispheres)
    double* hist;           // [T][N] year-weighted global temperature history
    double* st0; double* st1; double* st2; double* st3;   // Surface Temperature boxes, [T][N] each
    double* heat_uptake; double* ohc; double* sst;        // [T][N]
    uint8_t* status;        // [N]
};

// GhgForcing: scenario table rows built by the host (rscm_gpu.cpp, ghg_tables), [S][kGhgRows][T]
enum GhgRow {
    kGhgCo2 = 0, kGhgLnCo2, kGhgSqrtCo2, kGhgSqrtCh4, kGhgSqrtN2o,
    kGhgCh4P75, kGhgCh4TimesP152,  // CH4^0.75, CH4 * CH4^1.52
    kGhgN2oP75, kGhgN2oP152,       // N2O^0.75, N2O^1.52
    kGhgRows
};

struct GhgArgs {
    int64_t n_members;
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t rows;            // stored rows per series (T)
    int32_t method;          // 0 = IPCCTAR, 1 = OLBL (uniform over the ensemble)
    const double* params;    // [21][N]
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* derived;   // [kDerivedRows][N] member constants (launch_derive); row layout in ghg_body.hpp
    int32_t derived_uniform; // every parameter row they are formed from is uniform: element 0 serves all members (scalar loads)
    const double* tables;    // [S][kGhgRows][T]
    const int32_t* scen;     // [N] or null
    const double* conc;      // [S][3][T] the concentrations themselves (linked launches)
    InputLinks links;        // used when linked != 0: concentrations per member, no tables
    int32_t linked;
    double* erf_co2; double* erf_ch4; double* erf_n2o;  // [T][N] each
    uint8_t* status;
};

// OzoneForcing / AerosolDirect / AerosolIndirect (csrc/pointwise.hip)
struct PointwiseArgs {
    int64_t n_members;
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t rows;            // stored rows per series (T)
    int32_t kind;            // RSCM_KIND_OZONE_FORCING / _AEROSOL_DIRECT / _AEROSOL_INDIRECT / ...
    const double* params;    // [P][N]
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* inputs;    // [S][n_inputs][T]
    const int32_t* scen;     // [N] or null
    InputLinks links;        // used when linked != 0
    int32_t linked;
    int32_t n_inputs_used;   // aggregate kind: 1 + the highest contributor row that is linked or was given a series (the rest is NaN)
    double* out;             // [n_outputs][rows][N]
    uint8_t* status;
};

// CH4Chemistry / N2OChemistry (csrc/chem.hip)
struct ChemArgs {
    int64_t n_members;
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t kind;            // RSCM_KIND_CH4_CHEMISTRY / RSCM_KIND_N2O_CHEMISTRY
    const double* params;    // [P][N]
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* inputs;    // [S][n_inputs][T]
    const int32_t* scen;     // [N] or null
    InputLinks links;        // used when linked != 0
    int32_t linked;
    const double* bounds;    // [T+1]
    double* conc;            // [T][N] state, row 0 = initial value
    double* lifetime;        // [T][N]
    uint8_t* status;
};

// CO2Budget / TerrestrialCarbon (csrc/carbon.hip)
struct CarbonArgs {
    int64_t n_members;
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t kind;            // RSCM_KIND_CO2_BUDGET / RSCM_KIND_TERRESTRIAL_CARBON
    const double* params;    // [P][N]
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* derived;   // TerrestrialCarbon: [kDerivedRows][N] member constants (launch_derive); row layout in carbon_body.hpp
    int32_t derived_uniform; // every parameter row they are formed from is uniform: element 0 serves all members
    const double* inputs;    // [S][n_inputs][T]
    const int32_t* scen;     // [N] or null
    InputLinks links;        // used when linked != 0
    int32_t linked;
    const double* bounds;    // [T+1]
    const int32_t* nsub;     // CarbonCycle: [T-1] RK4 sub-steps per model step
    double h;                // CarbonCycle: RK4 step
    double h_half, h_sixth;  // h / 2.0, h / 6.0 (see TwoLayerArgs)
    int32_t rows;            // stored rows per series (T, or the window length)
    double* series;          // [n_states + n_outputs][rows][N], states first
    uint8_t* status;
};

// OceanCarbon (csrc/ocean.hip): model steps per pass over the flux history
template <bool FUSED>
constexpr int kOceanTileYears = FUSED ? 4 : 3;
constexpr int kOceanSplitYears = 2;  // years of a tile that is split over one-step launches

// OceanCarbon, RSCM_MODE_FAST: the far part of the impulse response (lags >= near, all in the late
// exponential-sum regime) as a sum of decaying modes  r(lag) ~ sum_q c[q] d[q]^(lag - near)  fitted by the
// host (rscm_gpu.cpp, ocean_fit_modes).  Each mode carries one running sum per member:
//   S_q(m) = d[q] S_q(m-1) + f(m - near) - e[q] f(m - H),   e[q] = d[q]^(H - near)
// so a sub-step costs O(modes + near) instead of O(H) multiply-adds.  Modes are sorted by rate; only the
// first n_exit of them still have a non-negligible weight when a pulse leaves the H-month window.
constexpr int kOceanModes = 21;   // constant + five rates + their fifteen pairwise sums (six-term late forms)
struct OceanModes {
    double d[kOceanModes], c[kOceanModes], e[kOceanModes];
    int32_t n_modes, n_exit;
};

// OceanCarbon (csrc/ocean.hip)
struct OceanArgs {
    int64_t n_members;
    int32_t n_times;
    int32_t step_begin, step_end;
    int32_t steps;           // sub-steps per model step (12)
    int32_t fused;           // RSCM_MODE_FAST: fused multiply-add in the convolution
    int64_t max_hist;        // max_history_months
    const double* params;    // [24][N]
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* inputs;    // [S][2][T]: CO2, SST anomaly
    const int32_t* scen;     // [N] or null
    InputLinks links;        // used when linked != 0
    int32_t linked;
    const double* bounds;    // [T+1]
    const double* irf;       // [max(max_hist, 1)] scaled impulse response at lag k/12 yr
    double* hist;            // [hist_rows][N] flux history, ppm/month: a ring, pulse j in row j mod hist_rows
    int32_t hist_rows;       // min((T-1)*steps, max_hist + ring slack): the whole run's pulses, or the convolution window
    double* partial;         // [(tile years - 1) * steps][N] running sums parked between the launches of a split tile
    int32_t part;            // -1: whole tiles; p >= 0: year p of a tile split over one-step launches
    int32_t rows;            // stored rows per series (T, or the window length)
    int32_t recur;           // RSCM_MODE_FAST with fitted modes: the O(T) recurrence kernel (near = 60 or 120 lags explicit)
    int32_t near;
    int32_t rebuild;         // the mode sums do not stand at step_begin: re-form them from the flux history first
    double* mode_state;      // [kOceanModes][N] the running sums S_q between launches
    const double* mode_table; // [3][kOceanModes] on the device: d_q, c_q, e_q (read with scalar loads)
    OceanModes modes;        // the same by value (n_exit; the constants for host-side use)
    double* series;          // [3][rows][N]: pCO2, cumulative uptake, flux
    uint8_t* status;
};

// HalocarbonChemistry (csrc/halocarbon.hip)
struct HaloArgs {
    int64_t n_members;
    int32_t n_times;
    int32_t step_begin, step_end;
    const double* params;     // [293][N]
    uint64_t uniform_rows;   // bit j: parameter row j (< 64) holds one value for all members (param_at)
    const double* emissions;  // [S][41][T]
    const int32_t* scen;      // [N] or null
    const double* bounds;     // [T+1]
    int32_t rows;             // stored rows per series (T, or the window length)
    double* series;           // [41 + 4][rows][N]: concentrations, then total / F-gas / Montreal forcing, EESC
    uint8_t* status;
};

// device stretch-move sampler (csrc/sampler.hip); pos is [D][W], the per-half buffers [.][W/2]
struct SamplerArgs {
    int32_t n_walkers, n_dims, n_params;
    int32_t n_groups;    // independent ensembles of n_walkers / n_groups walkers each
    int32_t half;        // 0 / 1: the half (of every group) being updated
    int32_t k_offset;    // this rank's block of the half: half-walker indices [k_offset, k_offset + n_local)
    int32_t n_local;     // = members of the evaluating ensemble (n_walkers / 2 when not sharded)
    int32_t iteration;
    int32_t identity;    // score the walkers where they stand (initialisation)
    uint64_t seed;
    double stretch_a;
    const int32_t* param_rows;   // [D] evaluator parameter row of each sampled dimension
    const double* base_params;   // [P] values of the rows that are not sampled
    const int32_t* prior_kind;   // [D] 0 = Uniform(a, b), 1 = Normal(mean a, std b), 2 = LogNormal(mu a, sigma b)
    const double* prior_a;
    const double* prior_b;
    const double* prior_lo;      // [D] truncation (Bound), -inf / +inf when there is none
    const double* prior_hi;
    double* pos;         // [D][W]
    double* logp;        // [W]
    double* proposal;    // [D][n_local]
    double* z;           // [n_local]
    double* lp;          // [n_local] log prior of the proposals
    const double* loglik;  // [n_local] written by the evaluator's fused run+likelihood launch
    double* eval_params;   // [P][n_local] the evaluator's parameter block
    double* const* param_ptr;  // graph evaluator: [D] parameter row of each sampled dimension in its owning ensemble's block ([n_local] each); else null
    double* exchange;      // pack: [D + 1][n_local] out; unpack: [n_ranks][D + 1][n_local] in (positions, then log prob)
    int32_t n_ranks;
    int64_t* n_accepted;   // [W]
    int64_t* n_proposed;   // [W]
};

struct LoglikArgs {
    int64_t n_members;
    int32_t n_obs;
    int32_t normalize;
    const double* const* obs_series;  // [n_obs] device pointers to the [N] row of (var, tidx)
    const int32_t* obs_group;         // [n_obs] variable id, for the per-variable partial sums
    const double* obs_value;
    const double* obs_sigma;
    double* out;                      // [N]
    // reference periods: the observations of a group whose obs_ref is r >= 0 are scored as anomalies from
    // b = (the sum of the rows ref_rows[ref_off[r] .. ref_off[r + 1]) in that order) / their count
    const int32_t* obs_ref;           // [n_obs] reference entry of the observation's group, -1: none; null: no group has one
    const int32_t* ref_off;           // [n_ref + 1] offsets into ref_rows
    const double* const* ref_rows;    // device pointers to the [N] reference rows
};

// One component of a fused lock-step launch (csrc/group.hip): the arguments its own kernel would get;
// the step range comes with the launch.  The table of ops lives in device memory and is read with
// scalar loads.
struct GroupOp {
    int32_t kind;      // RSCM_KIND_* of a kind the group kernel knows, -1: not fusable
    int32_t variant;   // two-layer: arithmetic mode; GhgForcing: method
    union Args {
        TwoLayerArgs tl;
        GhgArgs ghg;
        PointwiseArgs pw;
        ChemArgs chem;
        CarbonArgs carbon;
        Args() : pw() {}
    } u;
    OpCache cache;     // LDS slots of a multi-step launch (all -1 otherwise)
    // One-step launches (csrc/group.hip): the op runs model step `step + step_off` of the launch -- 1 for the ops of the NEXT step's
    // first segment when the scheduler merges them with this step's last segment (csrc/lockstep.cpp, MERGED schedule).
    int32_t step_off;
    GroupOp() : kind(-1), variant(0), u(), cache(), step_off(0) {}
};
constexpr int kMaxGroupOps = 16;
// up to this many ops travel by value in the kernel-argument segment (4 KiB in all) instead of a device table: the eight light
// components of the MAGICC graph's first segment, or that segment merged with the three of the previous step's last one (eleven)
constexpr int kGroupTableOps = 12;
struct GroupTable {
    GroupOp ops[kGroupTableOps];
};
static_assert(sizeof(GroupOp) == 296, "GroupOp grew: twelve of them must fit the kernel-argument segment");
static_assert(sizeof(GroupTable) <= 3840, "the by-value op table must fit the kernel-argument segment beside the other arguments");
// all_small: every op is one of the kinds group_kind_is_small accepts (the low-register variant of the kernel)
bool group_kind_is_small(int32_t kind);
// cache_slots > 0 (all_small only): the ops carry LDS slots (OpCache), cache_slots doubles per thread in all.
// Exactly one of d_ops (device table) and table (host, passed by value, n_ops <= kGroupTableOps) is given.
hipError_t launch_group(const GroupOp* d_ops, const GroupTable* table, int32_t n_ops, int64_t n_members, int32_t step_begin, int32_t step_end,
                        bool all_small, int32_t cache_slots, hipStream_t s);

// One model step of a by-value table whose first n_first ops and next n_second ops have no edge between them (two wavefronts per 64
// members run them at the same time), the rest after a workgroup barrier (csrc/group.hip, group_split_kernel).
// own_kernel: use the kernel compiled for this sequence of kinds and this cut where one exists (group_split_seq_available), else the interpreter
hipError_t launch_group_split(const GroupTable& table, int32_t n_first, int32_t n_second, int32_t n_ops, int64_t n_members, int32_t step, bool all_small,
                              hipStream_t s, bool own_kernel = true);
bool group_split_seq_available(const GroupTable& table, int32_t n_first, int32_t n_second, int32_t n_ops);

// A multi-step launch of a light graph whose sequence of kinds has a kernel of its own (csrc/group.hip: the op table
// by value, the kinds compile-time): true if one was launched (*status: its launch status), false if the sequence has none.
bool group_seq_available(const int32_t* kinds, int32_t n_ops);
bool launch_group_seq(const GroupTable& table, int32_t n_ops, int64_t n_members, int32_t step_begin, int32_t step_end, int32_t cache_slots,
                      hipStream_t s, hipError_t* status);

// bytes of LDS a two-layer launch stages for `len` steps: [n_scen][max(n_comp, 1)][len] doubles.  The one place the size is formed:
// the launchers use it, and the host decides lds_forcing with it (two_layer_fits_lds) wherever it cuts a run
inline size_t two_layer_lds_bytes(int32_t n_scen, int32_t n_comp, int32_t len)
{
    return (size_t)n_scen * (size_t)(n_comp > 0 ? n_comp : 1) * (size_t)len * sizeof(double);
}
inline bool two_layer_fits_lds(int32_t n_scen, int32_t n_comp, int32_t len)
{
    return two_layer_lds_bytes(n_scen, n_comp, len) <= (size_t)kMaxLds - 1024;
}
hipError_t launch_two_layer(const TwoLayerArgs& a, int mode, hipStream_t s, const double* pair_div = nullptr);
// out[(t - t_begin) * n_members + i] = e_t(seed, member0 + i) for t in [t_begin, t_end): the term a noise handle of this kind (kNoiseKind*,
// not none) adds to its forcing (TwoLayerArgs).  White: sigma * z.  Red: formed from index 0 on and written from t_begin on.  Members:
// the same from sigma_i = row sigma_row and phi_i = row phi_row of the [P][n_members] block; sigma and phi are not read
hipError_t launch_forcing_noise_rows(int32_t kind, uint64_t seed, double sigma, double phi, const double* params, uint64_t uniform_rows,
                                     int32_t sigma_row, int32_t phi_row, int64_t member0, int64_t n_members, int32_t t_begin, int32_t t_end,
                                     double* out, hipStream_t stream);
// z[j] = the deviate of the 52-bit integer k52[j] (test hook, rscm_gpu_selftest_normal)
hipError_t launch_normal_selftest(const uint64_t* k52, int64_t n, double* z, hipStream_t s);
hipError_t launch_two_layer_loglik(const TwoLayerArgs& a, int mode, hipStream_t s);
hipError_t launch_two_layer_loglik_ref(const TwoLayerArgs& a, const TwoLayerRefArgs& r, int mode, hipStream_t s);
// the current device's wavefront counts per guard of the counting launches (TwoLayerArgs::count_guards) into out[3] (if not null),
// then zeroes them; waits for the device first
hipError_t two_layer_guard_counts(int64_t* out);
hipError_t two_layer_pair_lanes(int64_t* out);
hipError_t launch_two_layer_pair_div(const double* params, uint64_t uniform_rows, int64_t n_members, double* out, hipStream_t s);
hipError_t launch_pair_div_selftest(const double* num, const double* den, int64_t n, int32_t num_lo, double* ieee, double* plain, double* tried,
                                    int32_t* variant, hipStream_t s);
hipError_t launch_coupled(const CoupledArgs& a, int mode, hipStream_t s);
hipError_t launch_udeb(const UdebArgs& a, hipStream_t s);
bool udeb_layers_unrolled(int32_t n_layers);  // the layer counts whose columns stay on chip (2 .. kUdebMaxOnChipLayers)
bool udeb_layers_fixed(int32_t n_layers);     // ... with the count compiled into the instance (20 / 30 / 40 / 50)
void set_udeb_variant(int variant);            // which ClimateUDEB kernel the calling thread's launches take (udeb.hip; -1: by size)
hipError_t launch_ghg(const GhgArgs& a, hipStream_t s);
// Member constants: what a light component's body formed from its parameters alone at the top of EVERY one-step launch (GhgForcing:
// four powers, three logarithms, two square roots of the pre-industrial concentrations; TerrestrialCarbon: its four turnover times,
// seven divisions -- parameters/terrestrial_carbon.rs:103-168) is formed once per parameter set by these small kernels, by the same
// device functions, and stored beside the parameter block: out [kDerivedRows][N].  Which parameter rows they read: *_derive_sources.
constexpr int kDerivedRows = 8;
hipError_t launch_ghg_derive(const double* params, uint64_t uniform_rows, int32_t method, int64_t n_members, double* out, hipStream_t s);
hipError_t launch_terrestrial_derive(const double* params, uint64_t uniform_rows, int64_t n_members, double* out, hipStream_t s);
hipError_t launch_udeb_derive(const double* params, uint64_t uniform_rows, int64_t n_members, double* out, hipStream_t s);
uint64_t udeb_derive_sources();
uint64_t ghg_derive_sources(int32_t method);      // bit j: parameter row j enters the member constants
uint64_t terrestrial_derive_sources();
hipError_t launch_pointwise(const PointwiseArgs& a, hipStream_t s);
hipError_t launch_chem(const ChemArgs& a, hipStream_t s);
hipError_t launch_carbon(const CarbonArgs& a, int mode, hipStream_t s);   // mode: CarbonCycle only (the other two kinds have one arithmetic)
hipError_t launch_ocean(const OceanArgs& a, hipStream_t s);
hipError_t launch_halocarbon(const HaloArgs& a, hipStream_t s);
hipError_t launch_sampler_propose(const SamplerArgs& a, hipStream_t s);
hipError_t launch_sampler_accept(const SamplerArgs& a, hipStream_t s);
// sharded sampler: this rank's block of the updated half into a.exchange / every rank's block out of it
hipError_t launch_sampler_pack(const SamplerArgs& a, hipStream_t s);
hipError_t launch_sampler_unpack(const SamplerArgs& a, hipStream_t s);
hipError_t launch_loglik(const LoglikArgs& a, hipStream_t s);
hipError_t launch_fill(double* p, int64_t n, double v, hipStream_t s);
hipError_t launch_broadcast_row(double* row, int64_t n, const double* src, int64_t n_src,
                                hipStream_t s);
// windowed series buffers [n_vars][R][N] (RSCM_FLAG_WINDOWED): move rows [shift, shift+keep) to the
// front, fill rows [row_begin, R), copy one row of chosen variables into / out of a row store
hipError_t launch_slide_rows(double* buf, int64_t N, int32_t R, int32_t n_vars, int32_t shift, int32_t keep, hipStream_t s);
hipError_t launch_fill_rows(double* buf, int64_t N, int32_t R, int32_t n_vars, int32_t row_begin, double value, hipStream_t s);
hipError_t launch_gather_rows(const double* src, int64_t N, int32_t src_rows, int32_t src_row, const int32_t* vars, int32_t n_out,
                              double* dst, int32_t dst_rows, int32_t dst_row, hipStream_t s);
hipError_t launch_scatter_rows(double* src, int64_t N, int32_t src_rows, int32_t src_row, const int32_t* vars, int32_t n_out,
                               const double* dst, int32_t dst_rows, int32_t dst_row, hipStream_t s);
// The window upkeep of a lock-step graph (slides, NaN fills, output rows) batched: one launch over a table of up to
// kMaxWindowOps descriptors instead of one small launch per ensemble and event.  A descriptor is a row move (rows [shift, shift +
// keep) of every variable to the front; shift >= keep: source and destination rows are disjoint), a row copy into the output store,
// or a fill of rows [fill_from, R).  Moves and copies only read what neither of them writes and go in one launch; fills (which
// overwrite the rows the moves read) in a second one.
constexpr int kMaxWindowOps = 40;
struct WindowOp {
    double* buf;          // [n_vars][R][N]
    const int32_t* vars;  // copy: variable ids kept in the output store (null: every variable, in order)
    double* dst;          // copy: [n_out][dst_rows][N]
    int64_t N;
    int32_t R, n_vars;
    int32_t kind;         // 0: move, 1: copy, 2: fill
    int32_t shift, keep;  // move
    int32_t src_row, n_out, dst_rows, dst_row;  // copy
    int32_t fill_from;    // fill (with NaN)
};
struct WindowBatch {
    WindowOp ops[kMaxWindowOps];
};
hipError_t launch_window_batch(const WindowBatch& batch, int32_t n_ops, hipStream_t s);
// the most rows one launch indexes with blockIdx.y (HIP's limit on gridDim.y): the launchers that put rows there -- the summaries
// and the select's histograms -- go over a longer axis in slices of this many rows
constexpr int32_t kMaxGridY = 65535;
// per row of rows[n_rows][n]: partial[n_rows][n_blocks][4], then reduced into out[n_rows][4] = {count_finite, sum, min, max}
int32_t summary_blocks(int64_t n);
hipError_t launch_summary_rows(const double* rows, int64_t n, int32_t n_rows, double* partial, int32_t n_blocks,
                               double* out, hipStream_t s);
// multi-pass radix select (select.hip): 8-bit digits, eight passes; one histogram of kSelBins int64 counts per row in pass 0, per
// (row, target) later.  Unweighted, target 2k / 2k + 1 of a row is the lower / upper order statistic of quantile k; weighted
// (int64 member weights d_w[N], numpy's "inverted_cdf"), the histograms sum weights and there is one target per quantile.
// Targets are histogrammed kSelGroup per launch (LDS: kSelGroup x kSelBins 32-bit counts, or gn x kSelBins 64-bit weight sums).
constexpr int kSelBins = 256;
constexpr int kSelPasses = 8;
constexpr int kSelGroup = 16;
constexpr int kMaxMemberGroups = 64;
int32_t select_blocks_per_row(int64_t N, int32_t n_rows);
// zeroes d_hist[hist_elems], then adds this pass's counts of rows d_rows[n_rows][N] (device array of row pointers); d_w non-null:
// member i adds d_w[i]; d_base non-null: of the anomalies x - d_base[i] (d_w and d_base 16-byte aligned).  d_group non-null (the
// grouped select, 8-byte aligned): member i counts only into the histograms of group d_group[i] (-1: none), the buffer being
// [n_rows][n_groups][256] in pass 0 and [n_rows][n_groups][n_t][256] later, d_prefix [n_rows][n_groups][n_t]: (row, group) is a
// virtual row of the commit and finish launches
hipError_t launch_select_hist(const double* const* d_rows, const int64_t* d_w, const double* d_base, const int32_t* d_group,
                              int32_t n_groups, int64_t N, int32_t n_rows, int32_t pass, const uint64_t* d_prefix, int32_t n_t,
                              int64_t* d_hist, size_t hist_elems, hipStream_t s);
// *d_flag = 1 if any d_group[i] is outside [-1, n_groups) (the caller zeroes it)
hipError_t launch_groups_check(const int32_t* d_group, int64_t N, int32_t n_groups, int32_t* d_flag, hipStream_t s);
// consumes the (reduced) histograms of `pass`: per (row, target) the bucket of its remaining rank; pass 0 also sets d_count[row].
// d_over non-null: the weighted commit, where d_count is the row's weight W and a row with W > 2^53 sets *d_over and gets NaN
hipError_t launch_select_commit(const int64_t* d_hist, int32_t pass, int32_t n_rows, int32_t n_t, const double* d_q, int64_t* d_count,
                                uint64_t* d_prefix, int64_t* d_rank, int32_t* d_over, hipStream_t s);
// after the last commit: d_out[r] = {count (weighted: W), quantile q[0], ..., q[n_q-1]} from the selected keys: numpy's
// nanquantile, method "linear" (weighted: the values of the keys)
hipError_t launch_select_finish(const int64_t* d_count, const uint64_t* d_keys, int32_t n_rows, int32_t n_q, const double* d_q,
                                bool weighted, double* d_out, hipStream_t s);
// the member weights (weights.hip):
// *d_key = max(*d_key, order key of ll[i]) over members with status 0 and finite ll (the caller seeds it with the key of -inf)
hipError_t launch_loglik_max(const double* d_ll, const uint8_t* d_status, int64_t N, unsigned long long* d_key, hipStream_t s);
// d_w[i] = llround(exp(min(ll[i] - ll_max, 0)) * 2^bits) for status 0 and finite ll, else 0
hipError_t launch_weights_from_loglik(const double* d_ll, const uint8_t* d_status, int64_t N, double ll_max, int32_t bits, int64_t* d_w,
                                      hipStream_t s);
// *d_flag = 1 if any d_w[i] < 0; *d_total += the sum of the weights, saturated so that it never wraps and exceeds 2^53 iff
// the true sum does (the caller zeroes both)
hipError_t launch_weights_check(const int64_t* d_w, int64_t N, int32_t* d_flag, unsigned long long* d_total, hipStream_t s);
// posterior resampling (resample.hip):
// d_out[5] = {sum w, count w != 0, max w, sum w^2 low word, sum w^2 high word}, exact, through d_partial[5 * weights_stats_partials(N)]
int32_t weights_stats_partials(int64_t N);
hipError_t launch_weights_stats(const int64_t* d_w, int64_t N, unsigned long long* d_partial, unsigned long long* d_out, hipStream_t s);
// d_out[i] = d_in[0] + ... + d_in[i] (d_in == d_out allowed) in three launches per level over d_scratch[scan_scratch_elems(n)]; no
// workgroup waits on another
int64_t scan_scratch_elems(int64_t n);
hipError_t launch_inclusive_scan(const int64_t* d_in, int64_t* d_out, int64_t n, int64_t* d_scratch, hipStream_t s);
// d_anc[j] = the first member i with d_cum[i] > t_k - w_before, k = k_first + j, t_k = k q + floor((s0 + k r) / M), for j < count
hipError_t launch_ancestors(const int64_t* d_cum, int64_t N, int64_t k_first, int64_t count, uint64_t M, uint64_t q, uint64_t r, uint64_t s0,
                            uint64_t w_before, int64_t* d_anc, hipStream_t s);
// *d_flag = 1 if any d_anc[j] is outside [0, n_src) (the caller zeroes it)
hipError_t launch_ancestors_check(const int64_t* d_anc, int64_t count, int64_t n_src, int32_t* d_flag, hipStream_t s);
// The member gather of rscm_ens_gather_members: piece p copies rows r < rows of elements of elem_bytes (8: f64, 1: status byte),
// dst[r * dst_stride + j] = src[r * src_stride + d_anc[j]] for j < count (strides in elements; dst already points at the first
// destination member).  One launch over a table of up to kMaxGatherPieces pieces.
constexpr int kMaxGatherPieces = 48;
struct GatherPiece {
    const void* src;
    void* dst;
    int64_t src_stride, dst_stride;
    int32_t rows, elem_bytes;
};
struct GatherBatch {
    GatherPiece pieces[kMaxGatherPieces];
};
hipError_t launch_gather_members(const GatherBatch& batch, int32_t n_pieces, const int64_t* d_anc, int64_t count, int64_t n_src, hipStream_t s);
// per-member indicators (indicators.hip) over rows d_rows[n_rows][N] at times d_time[n_rows], of x or (d_base non-null) of
// x - d_base[i]: a member with a NaN value gets NaN everywhere, else out[0][i] = sum in row order / n_rows and, with all,
// out[1] = max, out[2] = time of the first row attaining it, out[3 + k] = time of the first row >= thr[k] (+inf: none)
constexpr int kMaxThresholds = 8;
struct Thresholds {
    double v[kMaxThresholds];
};
hipError_t launch_indicators(const double* const* d_rows, const double* d_time, int32_t n_rows, const double* d_base, int64_t N, bool all,
                             int32_t n_thr, const Thresholds& thr, double* d_out, hipStream_t s);
// d_acc[k] += number (d_w non-null: summed weight) of members with v[i] >= thr[k], k < n_thr; d_acc[n_thr] += the same over the
// non-NaN members.  int64 sums, one integer atomic per block and bin; the caller zeroes d_acc[n_thr + 1].
hipError_t launch_exceedance(const double* d_v, const int64_t* d_w, int64_t N, int32_t n_thr, const Thresholds& thr,
                             unsigned long long* d_acc, hipStream_t s);
// the same per group: d_acc[g][n_thr + 1] (hits, then the total) over the members with d_group[i] == g; the caller zeroes it
hipError_t launch_exceedance_grouped(const double* d_v, const int64_t* d_w, const int32_t* d_group, int32_t n_groups, int64_t N,
                                     int32_t n_thr, const Thresholds& thr, unsigned long long* d_acc, hipStream_t s);
// the exact moment sums across members (moments.hip; the definition is stated in include/rscm_gpu.h, rscm_ens_moment_sums) of the
// vectors d_vec[n_vec] (a device array of device addresses of N doubles): d_out[G][2 + n_sums * 69] += {n, W, the blocks} with
// G = n_groups when d_group is non-null, else 1, and n_sums = n_vec (order 1) or n_vec (n_vec + 1) / 2 (order 2, about
// d_centre[G][n_vec]); d_w non-null: the member weights.  The caller zeroes d_out; d_mask[(N + 63) / 64] is scratch.  N < 2^31.
// The grid is capped at kMomBlocks blocks in x, which take kMomentMembersPerPass members per pass of their grid-stride loop.
constexpr int kMaxMomentVectors = 8;
constexpr int kMomBlocks = 1024;
constexpr int64_t kMomentMembersPerPass = 262144;
hipError_t launch_moment_sums(const double* const* d_vec, int32_t n_vec, const int64_t* d_w, const int32_t* d_group, int32_t n_groups,
                              int32_t order, const double* d_centre, int64_t N, unsigned long long* d_mask, unsigned long long* d_out,
                              hipStream_t s);
// the exact moment sums of stored rows (moment_rows.hip; the definition is stated in include/rscm_gpu.h, rscm_ens_moment_rows_sums):
// out[n_rows][G][2 + B * 69] += {n, W, the blocks} of the rows `rows` (a device array of n_rows device addresses of N doubles), with
// G = n_groups when group is non-null, else 1, and B = moment_rows_blocks(n_vec, order): order 1 the sums of x and of the n_vec member
// vectors vec[k], order 2 those of xx, x v_k, v_k v_k about centre[n_rows][G][1 + n_vec].  w non-null: the member weights; base
// non-null: x is the row's value minus base[i].  The caller zeroes out and stats[3] (window terms, walked terms, rebases); g_chunk is
// the launcher's.  N < 2^31.  The grid is capped at kMomRowBlocks blocks in x, which take kMomentRowsMembersPerPass members per pass
// of their grid-stride loop; a block's LDS bins take at most kMomentRowsLdsBytes, beyond which the groups are split over grid z.
constexpr int kMaxMomentRowVectors = 4;
constexpr int kMomRowBlocks = 32;
constexpr int64_t kMomentRowsMembersPerPass = 8192;
constexpr int32_t kMomentRowsLdsBytes = 61440;
struct MomentRowsArgs {
    const double* const* rows;
    const double* vec[kMaxMomentRowVectors];
    const int64_t* w;
    const int32_t* group;
    const double *base, *centre;
    unsigned long long *out, *stats;
    int64_t N;
    int32_t n_rows, n_groups, g_chunk;
};
constexpr int32_t moment_rows_blocks(int32_t n_vec, int32_t order) { return order == 1 ? 1 + n_vec : 1 + 2 * n_vec; }
hipError_t launch_moment_rows(MomentRowsArgs a, int32_t n_vec, int32_t order, hipStream_t s);
// exceedance and rank sums of stored rows (exceedance_rows.hip; the definition is stated in include/rscm_gpu.h,
// rscm_ens_exceedance_rows): acc[n_rows][G][exceedance_rows_stride(n_thr, equal)] += {total, hits[n_thr], equal[n_thr] when asked} of the
// rows `rows` (a device array of n_rows device addresses of N doubles), with G = n_groups when group is non-null, else 1.  The
// thresholds are thr.v[n_thr] for every row, or thr_rows[n_rows][n_thr] (device) when that is non-null.  w non-null: the member
// weights; base non-null: the value is the row's minus base[i].  The caller zeroes acc.  The grid is capped at kExcRowsBlocks blocks
// in x, which take kExceedanceRowsMembersPerPass members per pass of their grid-stride loop: a destination collects at most that many adders.
constexpr int kExcRowsBlocks = 32;
constexpr int64_t kExceedanceRowsMembersPerPass = 8192;
struct ExceedanceRowsArgs {
    const double* const* rows;
    const double* thr_rows;
    const int64_t* w;
    const int32_t* group;
    const double* base;
    unsigned long long* acc;
    Thresholds thr;
    int64_t N;
    int32_t n_rows, n_groups, n_thr;
};
constexpr int32_t exceedance_rows_stride(int32_t n_thr, bool equal) { return 1 + (equal ? 2 : 1) * n_thr; }
hipError_t launch_exceedance_rows(const ExceedanceRowsArgs& a, bool equal, hipStream_t s);
// histograms of stored rows and of member vectors (histogram.hip; the definition is stated in include/rscm_gpu.h,
// rscm_ens_histogram_rows): acc[n_rows][G][B + 2] += {counts[B], below, above} of the rows `rows` (a device array of n_rows device
// addresses of N doubles) among the ascending edges edges[E] (edge_stride 0: the same for every row) or edges[n_rows][E] (edge_stride
// E), device memory, B = E - 1, with G = n_groups when group is non-null, else 1.  w non-null: the member weights; base non-null: the
// value is the row's minus base[i].  The two-dimensional form: acc[G][Bx * By + 1] += {counts[Bx][By], outside} of the member vectors
// x and y among edges[Ex] followed by edges[Ey].  The caller zeroes acc and has checked the edges and the slots, G (B + 2) or
// G (Bx By + 1), against kHistogramMaxSlots: a block keeps them in LDS beside the edges.  The grid is capped at kHistBlocks blocks in
// x, which take kHistogramMembersPerPass members per pass of their grid-stride loop: a destination collects at most that many adders.
constexpr int32_t kHistogramMaxEdges = 1025;
constexpr int32_t kHistogramMaxSlots = 8192;
constexpr int kHistBlocks = 32;
constexpr int64_t kHistogramMembersPerPass = 8192;
struct HistogramArgs {
    const double* const* rows;
    const double* edges;
    const int64_t* w;
    const int32_t* group;
    const double* base;
    unsigned long long* acc;
    int64_t N;
    int32_t n_rows, n_groups, n_edges, edge_stride;
};
struct Histogram2dArgs {
    const double *x, *y, *edges;
    const int64_t* w;
    const int32_t* group;
    unsigned long long* acc;
    int64_t N;
    int32_t n_groups, n_edges_x, n_edges_y;
};
hipError_t launch_histogram(const HistogramArgs& a, hipStream_t s);
hipError_t launch_histogram2d(const Histogram2dArgs& a, hipStream_t s);
// per-member variability statistics (variability.hip) over rows d_rows[n_rows][N]: d_out[5][N] = mean, slope, variance, sd, r1 of
// the working series (mode kVarMean / kVarLinear: the rows, kVarDifference: their first differences; the definition is stated in
// include/rscm_gpu.h, rscm_ens_member_variability); stt = n (n^2 - 1) / 12 of the working series' length n, formed by the caller
constexpr int kVarMean = 0, kVarLinear = 1, kVarDifference = 2;
hipError_t launch_variability(const double* const* d_rows, int32_t n_rows, int32_t mode, double stt, int64_t N, double* d_out, hipStream_t s);
// per-member covariability of two variables (covariability.hip) over rows d_rows_x[n_rows][N] and d_rows_y[n_rows][N]:
// d_out[5 + 2 n_lags][N] = var_x, var_y, cov, corr, slope, then r_{+1}, r_{-1}, ... r_{+n_lags}, r_{-n_lags} (the definition is stated
// in include/rscm_gpu.h, rscm_ens_member_covariability); the modes are launch_variability's, stt = n (n^2 - 1) / 12 of the working
// series' common length n (n_rows - 1 when either mode is kVarDifference), formed by the caller; 0 <= n_lags <= kCovMaxLags
constexpr int kCovMaxLags = 3;
static_assert(5 + 2 * kCovMaxLags <= 3 + kMaxThresholds, "the covariability statistics share the indicator slots: [3 + kMaxThresholds][N]");
hipError_t launch_covariability(const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_x, int32_t mode_y,
                                int32_t n_lags, double stt, int64_t N, double* d_out, hipStream_t s);
// d_out[i] = (d_add ? d_add[i] : 0.0) + sum over j < n_vec of -0.5 ((value[j] - vec[j][i])^2 / sigma[j]^2), -inf where a vec[j][i] or
// d_add[i] is not finite; d_add may be d_out
constexpr int kMaxLoglikVectors = 16;
struct LoglikVectors {
    const double* vec[kMaxLoglikVectors];
    double value[kMaxLoglikVectors], sigma[kMaxLoglikVectors];
};
hipError_t launch_loglik_vectors(const LoglikVectors& v, int32_t n_vec, const double* d_add, int64_t N, double* d_out, hipStream_t s);
// per-member band powers (spectrum.hip) over rows d_rows[n_rows][N], mode and stt as launch_variability: d_out[3 + n_bands][N] = mean,
// slope, variance, then the mean periodogram ordinate of each band (the definition is stated in include/rscm_gpu.h,
// rscm_ens_member_spectrum).  d_c2[J] = 2 cos(2 pi j / n), j = 1 .. J = (n - 1) / 2, of the working series' length n (d_c2[j - 1];
// rscm_gpu_spectrum_coefficients) followed by kSpectrumTablePad zeros, which the last tile of frequencies reads and does not use;
// d_edges[n_bands + 1] int32 with 1 <= d_edges[0] < ... < d_edges[n_bands] <= J + 1: the caller
// has checked them, the kernel reads d_c2 and writes d_out by them
constexpr int kMaxSpectrumBands = 8;
constexpr int kSpectrumTablePad = 32;
static_assert(kMaxSpectrumBands <= kMaxThresholds, "the band powers share the indicator slots: [3 + kMaxThresholds][N]");
hipError_t launch_spectrum(const double* const* d_rows, int32_t n_rows, int32_t mode, double stt, const double* d_c2, const int32_t* d_edges,
                           int32_t n_bands, int64_t N, double* d_out, hipStream_t s);
// per-member co-spectra of two variables in frequency bands (cross_spectrum.hip) over rows d_rows_x[n_rows][N] and d_rows_y[n_rows][N],
// modes and stt as launch_covariability: d_out[2 + 3 n_bands][N] = var_x, var_y, then per band the squared coherence, the gain of y on
// x and its quadrature part (the definition is stated in include/rscm_gpu.h, rscm_ens_member_cross_spectrum).  d_c2 as launch_spectrum's;
// d_sin[J] = sin(2 pi j / n) at d_sin[j - 1] (rscm_gpu_spectrum_sines), padded by kSpectrumTablePad zeros like d_c2; d_edges as
// launch_spectrum's with 1 <= n_bands <= kMaxCrossSpectrumBands: the caller has checked them
constexpr int kMaxCrossSpectrumBands = 3;
static_assert(2 + 3 * kMaxCrossSpectrumBands <= 3 + kMaxThresholds, "the cross-spectrum statistics share the indicator slots: [3 + kMaxThresholds][N]");
hipError_t launch_cross_spectrum(const double* const* d_rows_x, const double* const* d_rows_y, int32_t n_rows, int32_t mode_x, int32_t mode_y,
                                 double stt, const double* d_c2, const double* d_sin, const int32_t* d_edges, int32_t n_bands, int64_t N,
                                 double* d_out, hipStream_t s);
// d_out[i] = (d_add ? d_add[i] : 0.0) + sum over j < n_vec of count[j] (ln vec[j][i] - 2 ln(vec[j][i] + record[j])), -inf where a
// vec[j][i] is not finite or <= 0 or d_add[i] is not finite; d_add may be d_out.  count[j] is the band's number of ordinates as a double.
struct LoglikSpectrum {
    const double* vec[kMaxLoglikVectors];
    double record[kMaxLoglikVectors], count[kMaxLoglikVectors];
};
hipError_t launch_loglik_spectrum(const LoglikSpectrum& v, int32_t n_vec, const double* d_add, int64_t N, double* d_out, hipStream_t s);
hipError_t launch_lhs(double* params, int32_t n_params, int64_t n_local, uint64_t seed,
                      const double* low, const double* high, int64_t member_offset,
                      int64_t n_total, hipStream_t s);
// The hypercube of launch_lhs through each row's inverse CDF (rscm_ens_sample_lhs_priors in include/rscm_gpu.h states it): rows[n_params]
// on the device, one entry per parameter row with the seven values of the entry point's seven arrays; the caller has checked them.
// any_quantile: whether a row is not kPriorUniform (false selects the kernel instance without the quantile's registers).
// kind: RSCM_PRIOR_UNIFORM / _NORMAL / _LOGNORMAL, the last two with or without RSCM_PRIOR_REFLECT (rscm_gpu.cpp static_asserts the four)
constexpr int32_t kPriorUniform = 0, kPriorNormal = 1, kPriorLogNormal = 2, kPriorReflect = 0x100;
struct LhsPriorRow { double a, b, p0, p1, lo, hi; int32_t kind, pad; };
hipError_t launch_lhs_priors(double* params, int32_t n_params, int64_t n_local, uint64_t seed, const LhsPriorRow* rows, bool any_quantile,
                             int64_t member_offset, int64_t n_total, hipStream_t s);
// out[i] = a[i] / b[i] through (1) the compiler's IEEE division and (2) the hoisted-reciprocal
// path used by the kernels, for the parity test of the latter.
hipError_t launch_divtest(const double* num, const double* den, double* out_ref,
                          double* out_fast, uint8_t* used_fast, int64_t n, hipStream_t s);
// out[i] = op 0 log_f64(x[i]), 1 the device library's log, 2 its exp, 3 chem::pow_ratio(x[i], y[i]), 4 guarded_rcp(x[i]) (test hook,
// rscm_gpu_selftest_math); y is read by op 3 only
constexpr int32_t kMathTestOps = 5;
hipError_t launch_mathtest(int32_t op, const double* x, const double* y, double* out, int64_t n, hipStream_t s);

}  // namespace rscm
