// Exact weighted first and second moments of STORED ROWS across the members of an ensemble, for gfx950 (MI355X): the integer sums
// behind rscm_ens_moment_rows_sums (the definition is stated in include/rscm_gpu.h).  The limb scheme is that of moments.hip -- a
// sum is a block of 68 signed int64 limbs and a count of non-finite terms, a term w * mantissa is placed by the exponent -- and both
// share the pure integer pieces (moment_window.hpp, which a host compiler builds alone) and the wave helpers (moment_wave.hpp).
//
// One launch per order for all rows.  Grid: x over member tiles (grid-stride, capped at kMomRowBlocks blocks of four waves), y over
// rows (a block works on one row at a time and strides over rows beyond 65535), z over chunks of member groups that fit the block's
// LDS bins [groups of the chunk][2 + S * 69] (one chunk unless S * G is large; a block counts the members of its own groups only).
// A wave loads a tile of 64 members once -- the row's value, the K vector values, weight, group and baseline, one member per lane --
// forms the mask inline (no pre-pass) and feeds all S sums of the order from that one load: order 1 S = 1 + K (x, v_k), order 2
// S = 1 + 2 K (xx, x v_k, v_k v_k).  n and W come from a ballot's population count and a lane-local integer sum.
//
// The in-window path.  For every sum a lane keeps a private window of kMomWin = 8 consecutive limbs as eight uint64 (16 VGPRs per
// sum: the nine sums of K = 4, order 2, hold 144 of that instance's 223 VGPRs, two waves per SIMD; K = 0 takes 64 VGPRs, seven
// waves; seven slots would be the least that spans 64 bits below the largest term), based at a wave-uniform limb `base`.  A
// lane whose term has its five digits inside the window (base <= q <= base + 3) adds them to its own registers with selects
// (mom_window_add): no v_readlane, no scalar walk, no atomics, 64 members at once.  base follows the tile's largest q (a wave max,
// taken only when two ballots say the window must move) and is sticky: it moves when a term lies above the window or every term
// of the tile below it, to qmax - 2, so that the window spans at least 64 bits below the tile's largest term and one limb above.
// Before it moves, when the wave's group changes and at the end of the wave's work on the row the window is FOLDED: each lane
// settles its slots (mom_window_settle), the wave sums each of the eight slots over its lanes -- a butterfly that halves the slots
// a lane carries at each of the first three steps, ten 64-bit exchanges instead of 48 -- and eight lanes add the eight sums to the
// block's LDS bins at limbs base .. base + 7.  Terms below the window take the serial walk of moments.hip: the term becomes
// wave-uniform (moment_wave.hpp; scalar shifts) and lanes 0 .. 4 add its five digits to the LDS bins.  Every digit of every term is
// added to its limb exactly once by integer adds, whichever path it took, so the canonical value does not depend on the path.
// Overflow: see moment_window.hpp; a bin takes fewer than 2^31 digits below 2^32 in magnitude (N < 2^31), as in moments.hip.
//
// Groups.  Contiguous groups are the fast case: a tile holds one group, and the wave folds when its group changes.  A tile that
// mixes groups (posterior()'s interleaved scenarios, i % 3) is processed once per group present, by ballot, each time with the
// lanes of that group alone -- exact like everything else, with a fold per change of group; it is measured separately
// (profiles/moment_rows_bench.txt).
//
// Output: the bins go out with one int64 atomic per non-zero entry and block.  d_stats[3] += the terms that went through the
// window, the terms that were walked, the rebases (moves of a window that had a base).
#include <hip/hip_runtime.h>

#include "moment_wave.hpp"
#include "moment_window.hpp"
#include "moments_finish.hpp"
#include "rscm_device.hpp"

namespace rscm {
namespace {

static_assert(kMomWinLimbs == kMomentLimbs, "moment_window.hpp restates the number of limbs");
constexpr int kMomRowThreads = 256;
constexpr int kMomRowWaves = kMomRowThreads / 64;
static_assert(kMomRowBlocks * kMomRowWaves * 64 == kMomentRowsMembersPerPass, "rscm_device.hpp states the members of one pass of the grid");

__device__ __forceinline__ unsigned long long mr_xor(unsigned long long v, int off) { return __shfl_xor(v, off, 64); }

__device__ __forceinline__ int mr_wave_max(int v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// The sum over the 64 lanes of each of the eight slots: afterwards lane l with (l & 7) == 0 holds the sum of slot l >> 3
__device__ __forceinline__ unsigned long long mr_fold_slots(const uint64_t (&win)[kMomWin], int lane)
{
    const bool h32 = lane & 32, h16 = lane & 16, h8 = lane & 8;
    unsigned long long r4[4], r2[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) r4[j] = (h32 ? win[j + 4] : win[j]) + mr_xor(h32 ? win[j] : win[j + 4], 32);
#pragma unroll
    for (int j = 0; j < 2; ++j) r2[j] = (h16 ? r4[j + 2] : r4[j]) + mr_xor(h16 ? r4[j] : r4[j + 2], 16);
    unsigned long long r = (h8 ? r2[1] : r2[0]) + mr_xor(h8 ? r2[0] : r2[1], 8);
    r += mr_xor(r, 4);
    r += mr_xor(r, 2);
    r += mr_xor(r, 1);
    return r;
}

template <int kOrder, int kK>
__global__ __launch_bounds__(kMomRowThreads) void moment_rows_kernel(MomentRowsArgs a)
{
    constexpr int S = kOrder == 1 ? 1 + kK : 1 + 2 * kK;
    constexpr int kStride = 2 + S * kMomentBlock;
    extern __shared__ unsigned long long mr_bins[];   // [groups of this chunk][kStride]: n, W, the S blocks
    const int lane = (int)(threadIdx.x & 63u), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool grouped = a.group != nullptr;
    const int32_t G = grouped ? a.n_groups : 1;
    const int32_t g0 = (int32_t)blockIdx.z * a.g_chunk;
    const int32_t gc = G - g0 < a.g_chunk ? G - g0 : a.g_chunk;
    const int64_t n_tiles = (a.N + 63) / 64;
    unsigned int st_win = 0u, st_walk = 0u, st_rebase = 0u;   // wave-uniform

    for (int32_t row = (int32_t)blockIdx.y; row < a.n_rows; row += (int32_t)gridDim.y) {
        for (int32_t i = (int32_t)threadIdx.x; i < gc * kStride; i += kMomRowThreads) mr_bins[i] = 0ull;
        __syncthreads();
        const double* __restrict__ x_row = a.rows[row];

        uint64_t win[S][kMomWin];
        uint32_t n_neg[S];
        int base[S];            // wave-uniform; -1: the window has not been placed yet
        unsigned int n_bad[S];  // wave-uniform
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int j = 0; j < kMomWin; ++j) win[s][j] = 0ull;
            n_neg[s] = 0u;
            base[s] = -1;
            n_bad[s] = 0u;
        }
        unsigned long long acc_w = 0ull;   // this lane's part of W
        unsigned int cnt = 0u;             // n (wave-uniform)
        int32_t cur = -1;                  // the group the registers hold sums of (wave-uniform)

        auto fold_sum = [&](int s, uint64_t (&w8)[kMomWin], uint32_t& nn) __attribute__((always_inline)) {
            mom_window_settle(w8, nn);
            const unsigned long long r = mr_fold_slots(w8, lane);
            const int limb = base[s] + (lane >> 3);
            if ((lane & 7) == 0 && limb < kMomentLimbs && r != 0ull)
                atomicAdd(&mr_bins[(cur - g0) * kStride + 2 + s * kMomentBlock + limb], r);
#pragma unroll
            for (int j = 0; j < kMomWin; ++j) w8[j] = 0ull;
            nn = 0u;
        };
        auto fold_all = [&]() __attribute__((always_inline)) {
            if (cur < 0) return;
            unsigned long long* bin = mr_bins + (cur - g0) * kStride;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (base[s] >= 0) fold_sum(s, win[s], n_neg[s]);
                if (lane == 0 && n_bad[s]) atomicAdd(&bin[2 + s * kMomentBlock + kMomentLimbs], (unsigned long long)n_bad[s]);
                n_bad[s] = 0u;
            }
            const unsigned long long wsum = mom_wave_sum(acc_w);
            if (lane == 0) {
                if (cnt) atomicAdd(&bin[0], (unsigned long long)cnt);
                if (wsum) atomicAdd(&bin[1], wsum);
            }
            acc_w = 0ull;
            cnt = 0u;
        };

        for (int64_t t = (int64_t)blockIdx.x * kMomRowWaves + wave; t < n_tiles; t += (int64_t)gridDim.x * kMomRowWaves) {
            const int64_t i = t * 64 + lane;
            bool ok = i < a.N;
            int32_t g = 0;
            if (grouped) {
                g = ok ? a.group[i] : -1;
                ok = g >= g0 && g < g0 + gc;
            }
            double x = 0.0, v[kK > 0 ? kK : 1] = {};
            unsigned long long wt = 0ull;
            if (ok) {
                x = x_row[i];
                if (a.base) x = x - a.base[i];   // one rounded subtraction: the bits the anomaly select sees
                ok = mom_finite_bits((uint64_t)__double_as_longlong(x));
#pragma unroll
                for (int k = 0; k < kK; ++k) {
                    v[k] = a.vec[k][i];
                    ok = ok && mom_finite_bits((uint64_t)__double_as_longlong(v[k]));
                }
                wt = a.w ? (unsigned long long)a.w[i] : 1ull;
            }
            unsigned long long rem = __ballot(ok);
            while (rem) {   // once per group present in the tile
                unsigned long long sel = rem;
                int32_t gj = 0;
                if (grouped) {
                    gj = (int32_t)mom_readlane((uint32_t)g, __ffsll(rem) - 1);
                    sel = __ballot(ok && g == gj);
                }
                rem &= ~sel;
                if (gj != cur) {
                    fold_all();
                    cur = gj;
                }
                const bool in = (sel >> lane) & 1ull;
                cnt += (unsigned int)__popcll(sel);
                acc_w += in ? wt : 0ull;
                double dx = x, dv[kK > 0 ? kK : 1] = {};
                if (kOrder == 2) {
                    const double* __restrict__ c = a.centre + ((int64_t)row * G + gj) * (1 + kK);
                    dx = x - c[0];
#pragma unroll
                    for (int k = 0; k < kK; ++k) dv[k] = v[k] - c[1 + k];
                } else {
#pragma unroll
                    for (int k = 0; k < kK; ++k) dv[k] = v[k];
                }

                auto add_term = [&](int s, double p, uint64_t (&w8)[kMomWin], uint32_t& nn) __attribute__((always_inline)) {
                    uint64_t mant, lo, hi;
                    uint32_t pos, neg;
                    const bool finite = mom_fields((uint64_t)__double_as_longlong(p), mant, pos, neg);
                    mom_product(wt, mant, lo, hi);
                    const bool valid = in && finite && (lo | hi) != 0ull;
                    const int q = (int)(pos >> 5);
                    n_bad[s] += (unsigned int)__popcll(__ballot(in && !finite));
                    const unsigned long long any = __ballot(valid);
                    if (any == 0ull) return;
                    int b = base[s];
                    // the window must move: it has no base, a term lies above it, or every term of the tile lies below it
                    if (b < 0 || __ballot(valid && q > b + kMomWinSpan) != 0ull || __ballot(valid && q >= b) == 0ull) {
                        const int nb = mom_window_base(mr_wave_max(valid ? q : -1));
                        if (b >= 0 && nb != b) {
                            fold_sum(s, w8, nn);
                            ++st_rebase;
                        }
                        base[s] = b = nb;
                    }
                    const bool inside = valid && q >= b;   // q <= b + kMomWinSpan holds for every term now
                    uint32_t d[5];
                    mom_digits(inside ? lo : 0ull, inside ? hi : 0ull, pos & 31u, d);
                    mom_window_add(w8, nn, d, inside ? (uint32_t)(q - b) : 0u, inside ? neg : 0u);
                    unsigned long long walk = __ballot(valid && q < b);
                    st_win += (unsigned int)__popcll(any & ~walk);
                    st_walk += (unsigned int)__popcll(walk);
                    if (walk == 0ull) return;
                    // the serial walk: the term becomes wave-uniform and lanes 0 .. 4 add its digits to the bins
                    const MomLaneTerm term = mom_lane_term(lo, hi, pos | (neg << 12));
                    unsigned long long* bin = mr_bins + (cur - g0) * kStride + 2 + s * kMomentBlock;
                    while (walk) {
                        const int j = __ffsll(walk) - 1;
                        walk &= walk - 1ull;
                        const uint32_t inf = mom_uniform_info(term, j);
                        uint64_t plo, phi;
                        mom_uniform_product(term, j, plo, phi);
                        uint32_t dj[5];
                        mom_digits(plo, phi, inf & 31u, dj);
                        const int qj = (int)((inf & 0xFFFu) >> 5);
                        const uint32_t mine = lane == 0 ? dj[0] : lane == 1 ? dj[1] : lane == 2 ? dj[2] : lane == 3 ? dj[3] : dj[4];
                        const long long sd = (inf >> 12) & 1u ? -(long long)mine : (long long)mine;
                        if (lane < 5 && qj + lane < kMomentLimbs && mine != 0u) atomicAdd(&bin[qj + lane], (unsigned long long)sd);
                    }
                };

                if (kOrder == 1) {
                    add_term(0, dx, win[0], n_neg[0]);
#pragma unroll
                    for (int k = 0; k < kK; ++k) add_term(1 + k, dv[k], win[1 + k], n_neg[1 + k]);
                } else {
                    add_term(0, __dmul_rn(dx, dx), win[0], n_neg[0]);
#pragma unroll
                    for (int k = 0; k < kK; ++k) add_term(1 + k, __dmul_rn(dx, dv[k]), win[1 + k], n_neg[1 + k]);
#pragma unroll
                    for (int k = 0; k < kK; ++k) add_term(1 + kK + k, __dmul_rn(dv[k], dv[k]), win[1 + kK + k], n_neg[1 + kK + k]);
                }
            }
        }
        fold_all();
        __syncthreads();
        unsigned long long* __restrict__ o = a.out + ((int64_t)row * G + g0) * kStride;
        for (int32_t i = (int32_t)threadIdx.x; i < gc * kStride; i += kMomRowThreads)
            if (mr_bins[i]) atomicAdd(&o[i], mr_bins[i]);
        __syncthreads();
    }
    if (lane == 0) {
        if (st_win) atomicAdd(&a.stats[0], (unsigned long long)st_win);
        if (st_walk) atomicAdd(&a.stats[1], (unsigned long long)st_walk);
        if (st_rebase) atomicAdd(&a.stats[2], (unsigned long long)st_rebase);
    }
}

template <int kOrder, int kK>
void launch_one(const MomentRowsArgs& a, dim3 grid, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL((moment_rows_kernel<kOrder, kK>), grid, dim3(kMomRowThreads), lds, s, a);
}

template <int kOrder>
void launch_order(int32_t K, const MomentRowsArgs& a, dim3 grid, size_t lds, hipStream_t s)
{
    switch (K) {
        case 0: launch_one<kOrder, 0>(a, grid, lds, s); break;
        case 1: launch_one<kOrder, 1>(a, grid, lds, s); break;
        case 2: launch_one<kOrder, 2>(a, grid, lds, s); break;
        case 3: launch_one<kOrder, 3>(a, grid, lds, s); break;
        default: launch_one<kOrder, 4>(a, grid, lds, s); break;
    }
}

}  // namespace

hipError_t launch_moment_rows(MomentRowsArgs a, int32_t n_vec, int32_t order, hipStream_t s)
{
    if (a.N <= 0 || a.n_rows <= 0) return hipSuccess;
    if (n_vec < 0 || n_vec > kMaxMomentRowVectors || (order != 1 && order != 2)) return hipErrorInvalidValue;
    const int32_t G = a.group ? a.n_groups : 1;
    const int32_t stride = 2 + moment_rows_blocks(n_vec, order) * kMomentBlock;
    int32_t chunk = kMomentRowsLdsBytes / (stride * (int32_t)sizeof(unsigned long long));   // at least 12: 9 blocks are 4984 bytes
    if (chunk > G) chunk = G;
    a.g_chunk = chunk;
    const int64_t need = ((a.N + 63) / 64 + kMomRowWaves - 1) / kMomRowWaves;
    const dim3 grid((unsigned)(need < kMomRowBlocks ? need : kMomRowBlocks), (unsigned)(a.n_rows < 65535 ? a.n_rows : 65535),
                    (unsigned)((G + chunk - 1) / chunk));
    const size_t lds = (size_t)chunk * stride * sizeof(unsigned long long);
    if (order == 1)
        launch_order<1>(n_vec, a, grid, lds, s);
    else
        launch_order<2>(n_vec, a, grid, lds, s);
    return hipGetLastError();
}

}  // namespace rscm
