// Exact weighted first and second moments ACROSS the members of an ensemble, for gfx950 (MI355X): the integer sums behind
// rscm_ens_moment_sums (the definition is stated in include/rscm_gpu.h).
//
// One sum -- S_a = sum w_i x_ia, or C_ab = sum w_i ((x_ia - c_a)(x_ib - c_b)) -- is a block of 68 signed int64 limbs, limb k in units
// of 2^(32 k - 1088), and a count of non-finite terms.  A term is the integer w * mantissa (at most 106 bits) placed at the bit the
// double's exponent names, cut into 32-bit digits at limb boundaries; every digit is added, with the term's sign, into its limb.
// Integer adds: exact, and the order does not matter.  moment_rows.hip uses the same term, so it is stated once: its fields, product
// and digits in moment_window.hpp (a host program checks them), the wave sum and the wave-uniform read of a term in moment_wave.hpp.
//
// moment_mask_kernel: per tile of 64 members one uint64 of the members that count (in a group, all n_vec values finite: listwise), and
// the counts n and weight sums W per group, as exceedance_grouped_kernel forms its totals.
// moment_sum_kernel: grid x over tiles (grid-stride, capped at kMomBlocks blocks of kMomWaves waves), y over the sums.  A wave loads a
// tile, one member per lane, and each lane forms its own member's term: sign, bit position, the 128-bit product.  Then the wave
// walks the members that have one: the term becomes wave-uniform (moment_wave.hpp; scalar shifts into five 32-bit digits) and LANE l
// adds the digit that falls into LIMB l to a private int64 register -- no atomics, no conflicts.  Limbs 64 .. 67 (a second
// register of lanes 0 .. 3) sit behind a wave-uniform branch that only terms of 2^959 and beyond take.  The registers hold the sums
// of one member group and are flushed into the block's LDS bins [G][69] when the walked member's group differs, and at the end;
// the bins go out with one int64 atomic per non-zero limb and block.  A lane adds fewer than 2^31 digits below 2^32 (the host
// refuses N >= 2^31), so no register, bin or result limb wraps.
#include <hip/hip_runtime.h>

#include "moment_wave.hpp"
#include "moment_window.hpp"
#include "moments_finish.hpp"
#include "rscm_device.hpp"

namespace rscm {
namespace {

constexpr int kMomThreads = 256;
constexpr int kMomWaves = kMomThreads / 64;
static_assert(kMomBlocks * kMomWaves * 64 == kMomentMembersPerPass, "rscm_device.hpp states the members of one pass of the grid");

template <bool kW, bool kG>
__global__ __launch_bounds__(kMomThreads) void moment_mask_kernel(const double* const* __restrict__ vec, int32_t n_vec,
                                                                   const int64_t* __restrict__ w, const int32_t* __restrict__ group,
                                                                   int32_t n_groups, int64_t N, unsigned long long* __restrict__ mask,
                                                                   unsigned long long* __restrict__ out, int64_t out_stride)
{
    __shared__ unsigned long long bins[kMaxMemberGroups * 2];
    for (int32_t i = (int32_t)threadIdx.x; i < n_groups * 2; i += kMomThreads) bins[i] = 0ull;
    __syncthreads();
    // the wave index is the same in all 64 lanes; saying so keeps the tile index, the mask word and the walk in scalar registers
    const int lane = (int)(threadIdx.x & 63u), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_tiles = (N + 63) / 64;
    unsigned long long cnt = 0ull, tot = 0ull;
    int32_t cur = kG ? -1 : 0;   // the group the registers hold sums of
    auto flush = [&]() {
        if (cur < 0) return;
        if (cnt) atomicAdd(&bins[cur * 2], cnt);
        if (tot) atomicAdd(&bins[cur * 2 + 1], tot);
        cnt = tot = 0ull;
    };
    for (int64_t t = (int64_t)blockIdx.x * kMomWaves + wave; t < n_tiles; t += (int64_t)gridDim.x * kMomWaves) {
        const int64_t i = t * 64 + lane;
        bool ok = i < N;
        int32_t g = 0;
        if (kG) {
            g = ok ? group[i] : -1;
            ok = g >= 0;
        }
        for (int32_t k = 0; k < n_vec; ++k) {
            const double* __restrict__ v = vec[k];
            if (ok) ok = mom_finite_bits((uint64_t)__double_as_longlong(v[i]));
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) mask[t] = m;
        if (!ok) continue;
        if (g != cur) {
            flush();
            cur = g;
        }
        cnt += 1ull;
        tot += kW ? (unsigned long long)w[i] : 1ull;
    }
    // whole waves arrive here together; a wave whose lanes hold one group adds its sums through one lane
    const unsigned long long have = __ballot(cur >= 0);
    if (have != 0ull) {
        const int32_t c0 = __shfl(cur, __ffsll(have) - 1, 64);
        if (__ballot(cur >= 0 && cur != c0) == 0ull) {
            if (cur < 0) cnt = tot = 0ull;
            cnt = mom_wave_sum(cnt);
            tot = mom_wave_sum(tot);
            cur = lane == 0 ? c0 : -1;
        }
        flush();
    }
    __syncthreads();
    for (int32_t i = (int32_t)threadIdx.x; i < n_groups * 2; i += kMomThreads)
        if (bins[i]) atomicAdd(&out[(int64_t)(i >> 1) * out_stride + (i & 1)], bins[i]);
}

// kOrder 1: the terms are x_a; 2: (x_a - c[g][a]) * (x_b - c[g][b]) for the pair (a, b) that blockIdx.y names
template <int kOrder, bool kW, bool kG>
__global__ __launch_bounds__(kMomThreads) void moment_sum_kernel(const double* const* __restrict__ vec, int32_t n_vec,
                                                                  const int64_t* __restrict__ w, const int32_t* __restrict__ group,
                                                                  int32_t n_groups, const double* __restrict__ centre,
                                                                  const unsigned long long* __restrict__ mask, int64_t N,
                                                                  unsigned long long* __restrict__ out, int64_t out_stride)
{
    extern __shared__ unsigned long long mom_bins[];   // [n_groups][kMomentBlock]
    for (int32_t i = (int32_t)threadIdx.x; i < n_groups * kMomentBlock; i += kMomThreads) mom_bins[i] = 0ull;
    __syncthreads();
    // the wave index is the same in all 64 lanes; saying so keeps the tile index, the mask word and the walk in scalar registers
    const int lane = (int)(threadIdx.x & 63u), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_tiles = (N + 63) / 64;
    int32_t a = (int32_t)blockIdx.y, b = a;
    if (kOrder == 2) {   // (0,0), (0,1), ..., (0,K-1), (1,1), ...
        int32_t rest = a;
        a = 0;
        while (rest >= n_vec - a) {
            rest -= n_vec - a;
            ++a;
        }
        b = a + rest;
    }
    const double* __restrict__ va = vec[a];
    const double* __restrict__ vb = vec[b];

    long long acc = 0, acc_hi = 0;   // limb `lane`, and limb 64 + lane in lanes 0 .. 3
    unsigned int n_bad = 0u;         // non-finite terms (wave-uniform)
    int32_t cur = kG ? -1 : 0;       // the group the registers hold sums of (wave-uniform)
    auto flush = [&]() {
        if (cur < 0) return;
        unsigned long long* bin = mom_bins + cur * kMomentBlock;
        if (acc) atomicAdd(&bin[lane], (unsigned long long)acc);
        if (lane < kMomentLimbs - 64 && acc_hi) atomicAdd(&bin[64 + lane], (unsigned long long)acc_hi);
        if (lane == 0 && n_bad) atomicAdd(&bin[kMomentLimbs], (unsigned long long)n_bad);
        acc = acc_hi = 0;
        n_bad = 0u;
    };

    for (int64_t t = (int64_t)blockIdx.x * kMomWaves + wave; t < n_tiles; t += (int64_t)gridDim.x * kMomWaves) {
        const unsigned long long m = mask[t];   // wave-uniform
        if (m == 0ull) continue;
        const bool in = (m >> lane) & 1ull;      // implies t * 64 + lane < N
        const int64_t i = t * 64 + lane;
        double p = 0.0;
        unsigned long long wt = 0ull;
        int32_t g = 0;
        if (in) {
            if (kG) g = group[i];
            wt = kW ? (unsigned long long)w[i] : 1ull;
            p = va[i];
            if (kOrder == 2) {
                const double da = p - centre[g * n_vec + a];
                const double db = vb[i] - centre[g * n_vec + b];
                p = __dmul_rn(da, db);
            }
        }
        uint64_t mant, lo, hi;
        uint32_t pos, neg;
        const bool finite = mom_fields((uint64_t)__double_as_longlong(p), mant, pos, neg);
        mom_product(wt, mant, lo, hi);
        const unsigned long long bad = __ballot(in && !finite);
        unsigned long long walk = __ballot(in && finite && (lo | hi) != 0ull) | bad;
        // info = bit position (12 bits: at most 2046 + 13) | sign << 12 | group << 13
        const MomLaneTerm term = mom_lane_term(lo, hi, pos | (neg << 12) | ((uint32_t)g << 13));
        while (walk) {
            const int j = __ffsll(walk) - 1;
            walk &= walk - 1ull;
            const uint32_t inf = mom_uniform_info(term, j);
            if (kG) {
                const int32_t gj = (int32_t)(inf >> 13);
                if (gj != cur) {
                    flush();
                    cur = gj;
                }
            }
            if ((bad >> j) & 1ull) {
                ++n_bad;
                continue;
            }
            const int q = (int)((inf & 0xFFFu) >> 5);
            uint64_t plo, phi;
            uint32_t d[5];   // digit k falls into limb q + k
            mom_uniform_product(term, j, plo, phi);
            mom_digits(plo, phi, inf & 31u, d);
            const long long sign = -(long long)((inf >> 12) & 1u);   // 0 or -1, wave-uniform
            // five independent selects and a conditional negation: no branch per lane
            auto digit = [&](int k) -> long long {
                const uint32_t mine = (k == 0 ? d[0] : 0u) | (k == 1 ? d[1] : 0u) | (k == 2 ? d[2] : 0u) | (k == 3 ? d[3] : 0u) | (k == 4 ? d[4] : 0u);
                return ((long long)mine ^ sign) - sign;
            };
            acc += digit(lane - q);
            if (q + 4 >= 64) acc_hi += digit(64 + lane - q);   // lanes beyond 3 hold no limb there: never flushed
        }
    }
    flush();
    __syncthreads();
    const int64_t col = 2 + (int64_t)blockIdx.y * kMomentBlock;
    for (int32_t i = (int32_t)threadIdx.x; i < n_groups * kMomentBlock; i += kMomThreads)
        if (mom_bins[i]) atomicAdd(&out[(int64_t)(i / kMomentBlock) * out_stride + col + i % kMomentBlock], mom_bins[i]);
}

template <int kOrder, bool kW>
void launch_sum(bool grouped, dim3 grid, size_t lds, hipStream_t s, const double* const* d_vec, int32_t n_vec, const int64_t* d_w,
                const int32_t* d_group, int32_t G, const double* d_centre, const unsigned long long* d_mask, int64_t N,
                unsigned long long* d_out, int64_t stride)
{
    if (grouped)
        hipLaunchKernelGGL((moment_sum_kernel<kOrder, kW, true>), grid, dim3(kMomThreads), lds, s, d_vec, n_vec, d_w, d_group, G, d_centre,
                           d_mask, N, d_out, stride);
    else
        hipLaunchKernelGGL((moment_sum_kernel<kOrder, kW, false>), grid, dim3(kMomThreads), lds, s, d_vec, n_vec, d_w, d_group, G, d_centre,
                           d_mask, N, d_out, stride);
}

}  // namespace

hipError_t launch_moment_sums(const double* const* d_vec, int32_t n_vec, const int64_t* d_w, const int32_t* d_group, int32_t n_groups,
                              int32_t order, const double* d_centre, int64_t N, unsigned long long* d_mask, unsigned long long* d_out,
                              hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const int32_t G = d_group ? n_groups : 1;
    const int32_t n_sums = order == 1 ? n_vec : n_vec * (n_vec + 1) / 2;
    const int64_t stride = 2 + (int64_t)n_sums * kMomentBlock;
    const int64_t need = ((N + 63) / 64 + kMomWaves - 1) / kMomWaves;
    const unsigned gx = (unsigned)(need < kMomBlocks ? need : kMomBlocks);
    if (d_group && d_w)
        hipLaunchKernelGGL((moment_mask_kernel<true, true>), dim3(gx), dim3(kMomThreads), 0, s, d_vec, n_vec, d_w, d_group, G, N, d_mask, d_out, stride);
    else if (d_group)
        hipLaunchKernelGGL((moment_mask_kernel<false, true>), dim3(gx), dim3(kMomThreads), 0, s, d_vec, n_vec, d_w, d_group, G, N, d_mask, d_out, stride);
    else if (d_w)
        hipLaunchKernelGGL((moment_mask_kernel<true, false>), dim3(gx), dim3(kMomThreads), 0, s, d_vec, n_vec, d_w, d_group, G, N, d_mask, d_out, stride);
    else
        hipLaunchKernelGGL((moment_mask_kernel<false, false>), dim3(gx), dim3(kMomThreads), 0, s, d_vec, n_vec, d_w, d_group, G, N, d_mask, d_out, stride);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const dim3 grid(gx, (unsigned)n_sums);
    const size_t lds = (size_t)G * kMomentBlock * sizeof(unsigned long long);
    if (order == 1 && d_w)
        launch_sum<1, true>(d_group != nullptr, grid, lds, s, d_vec, n_vec, d_w, d_group, G, d_centre, d_mask, N, d_out, stride);
    else if (order == 1)
        launch_sum<1, false>(d_group != nullptr, grid, lds, s, d_vec, n_vec, d_w, d_group, G, d_centre, d_mask, N, d_out, stride);
    else if (d_w)
        launch_sum<2, true>(d_group != nullptr, grid, lds, s, d_vec, n_vec, d_w, d_group, G, d_centre, d_mask, N, d_out, stride);
    else
        launch_sum<2, false>(d_group != nullptr, grid, lds, s, d_vec, n_vec, d_w, d_group, G, d_centre, d_mask, N, d_out, stride);
    return hipGetLastError();
}

}  // namespace rscm
