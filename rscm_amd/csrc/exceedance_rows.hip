// Exceedance and rank sums of STORED ROWS across the members of an ensemble, for gfx950 (MI355X): the integer sums behind
// rscm_ens_exceedance_rows (the definition is stated in include/rscm_gpu.h).  Per row and member group: the summed weight of the
// members whose value is not NaN (total), of those at or above each of up to kMaxThresholds thresholds (hits) and, when asked, of
// those equal to it (equal).  The thresholds are the same for every row (a kernel argument) or one set per row (a device table).
//
// One launch for all rows.  Grid: x over member stretches (grid-stride, capped at kExcRowsBlocks blocks of four waves, so that a
// destination collects at most that many adders), y over rows (a block works on one row at a time and strides over rows beyond
// 65535).  A thread walks its members with the grid's stride, kExcRowsBatch loads in flight, lanes of a wave on consecutive members
// (every load coalesced), and keeps total, hits[K] and equal[K] in registers: uint32 counts when every weight is 1 (a thread meets
// fewer than 2^32 members), uint64 sums of the int64 member weights otherwise.  The row's thresholds are read once per block and
// row; a threshold beyond n_thr is NaN, which no value reaches.  At the end of the row one wave ladder sums the registers over the
// lanes, lane 0 adds the wave's sums to the block's LDS bins, and one integer atomic per non-zero bin and block goes to the
// accumulator [rows][G][total, hits[K], equal[K]].  Integer adds throughout: exact, and the order does not matter.  With the
// weights' bound (a handle's weights sum to at most 2^53, weights.hip) nothing wraps.
//
// Groups: the scheme of exceedance_grouped_kernel (indicators.hip).  A thread keeps the sums of ONE group -- that of the members it
// has met since its last flush -- and flushes them into the block's LDS bins [n_groups][1 + 2 kMaxThresholds] when it meets
// another; the last flush goes through the wave ladder when the whole wave holds one group.  Contiguous groups flush once or twice
// per thread and row; interleaved groups (posterior()'s i % 3) flush at nearly every member and are measured separately
// (profiles/exceedance_rows_bench.txt).
//
// The weights, the groups and the baseline are read again for every row; at 1e6 members they are 8 + 4 + 8 MB.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rscm_device.hpp"

namespace rscm {
namespace {

constexpr int kExcRowsThreads = 256;
constexpr int kExcRowsBatch = 4;                          // members whose loads a thread issues before it uses them
constexpr int kExcRowsSlots = 1 + 2 * kMaxThresholds;     // a group's LDS bins: total, hits[kMaxThresholds], equal[kMaxThresholds]
static_assert(kExcRowsBlocks * kExcRowsThreads == kExceedanceRowsMembersPerPass, "rscm_device.hpp states the members of one pass of the grid");

__device__ __forceinline__ unsigned long long er_wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <bool kW, bool kG, bool kEq>
__global__ __launch_bounds__(kExcRowsThreads) void exceedance_rows_kernel(ExceedanceRowsArgs a)
{
    using Sum = std::conditional_t<kW, unsigned long long, unsigned int>;
    __shared__ unsigned long long bins[(kG ? kMaxMemberGroups : 1) * kExcRowsSlots];
    const int32_t G = kG ? a.n_groups : 1, K = a.n_thr;
    const int32_t S = exceedance_rows_stride(K, kEq);
    const int64_t step = (int64_t)gridDim.x * kExcRowsThreads;
    const int64_t first = (int64_t)blockIdx.x * kExcRowsThreads + threadIdx.x;
    const double qnan = __builtin_nan("");

    for (int32_t row = (int32_t)blockIdx.y; row < a.n_rows; row += (int32_t)gridDim.y) {
        for (int32_t i = (int32_t)threadIdx.x; i < G * kExcRowsSlots; i += kExcRowsThreads) bins[i] = 0ull;
        __syncthreads();
        const double* __restrict__ x_row = a.rows[row];
        double th[kMaxThresholds];
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k)
            th[k] = k >= K ? qnan : a.thr_rows ? a.thr_rows[(int64_t)row * K + k] : a.thr.v[k];

        Sum tot = 0, hit[kMaxThresholds], eq[kMaxThresholds];
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k) hit[k] = eq[k] = 0;
        int32_t cur = kG ? -1 : 0;   // the group the registers hold sums of

        auto flush = [&]() __attribute__((always_inline)) {
            if (cur < 0) return;
            unsigned long long* bin = bins + cur * kExcRowsSlots;
            if (tot) atomicAdd(&bin[0], (unsigned long long)tot);
#pragma unroll
            for (int k = 0; k < kMaxThresholds; ++k) {
                if (k < K && hit[k]) atomicAdd(&bin[1 + k], (unsigned long long)hit[k]);
                if (kEq && k < K && eq[k]) atomicAdd(&bin[1 + kMaxThresholds + k], (unsigned long long)eq[k]);
                hit[k] = eq[k] = 0;
            }
            tot = 0;
        };

        for (int64_t i0 = first; i0 < a.N; i0 += kExcRowsBatch * step) {
            double x[kExcRowsBatch];
            Sum wt[kExcRowsBatch];
            int32_t g[kExcRowsBatch];
#pragma unroll
            for (int j = 0; j < kExcRowsBatch; ++j) {
                const int64_t i = i0 + j * step;
                const bool in = i < a.N;
                x[j] = in ? x_row[i] : qnan;
                if (a.base) x[j] = x[j] - (in ? a.base[i] : 0.0);   // one rounded subtraction: the bits the anomaly select sees
                wt[j] = kW ? (in ? (Sum)a.w[i] : (Sum)0) : (Sum)1;
                g[j] = kG ? (in ? a.group[i] : -1) : 0;
            }
#pragma unroll
            for (int j = 0; j < kExcRowsBatch; ++j) {
                const double v = x[j];
                if (kG) {
                    if ((uint32_t)g[j] >= (uint32_t)G || v != v) continue;   // in no group, or NaN: takes no part
                    if (g[j] != cur) {
                        flush();
                        cur = g[j];
                    }
                }
                tot += v == v ? wt[j] : (Sum)0;
#pragma unroll
                for (int k = 0; k < kMaxThresholds; ++k) {
                    if (k < K) {
                        hit[k] += v >= th[k] ? wt[j] : (Sum)0;
                        if (kEq) eq[k] += v == th[k] ? wt[j] : (Sum)0;
                    }
                }
            }
        }

        // whole waves arrive here together; lanes that met no member of a group hold zeros and take the wave's group
        bool ladder = true;
        int32_t c0 = 0;
        if (kG) {
            const unsigned long long have = __ballot(cur >= 0);
            c0 = have ? __shfl(cur, __ffsll(have) - 1, 64) : -1;
            ladder = have != 0ull && __ballot(cur >= 0 && cur != c0) == 0ull;
        }
        if (ladder) {
            unsigned long long t = er_wave_sum((unsigned long long)tot), hk[kMaxThresholds], ek[kMaxThresholds];
#pragma unroll
            for (int k = 0; k < kMaxThresholds; ++k) {
                hk[k] = k < K ? er_wave_sum((unsigned long long)hit[k]) : 0ull;
                ek[k] = kEq && k < K ? er_wave_sum((unsigned long long)eq[k]) : 0ull;
            }
            if ((threadIdx.x & 63u) == 0u) {
                unsigned long long* bin = bins + c0 * kExcRowsSlots;
                if (t) atomicAdd(&bin[0], t);
#pragma unroll
                for (int k = 0; k < kMaxThresholds; ++k) {
                    if (hk[k]) atomicAdd(&bin[1 + k], hk[k]);
                    if (ek[k]) atomicAdd(&bin[1 + kMaxThresholds + k], ek[k]);
                }
            }
        } else {
            flush();
        }
        __syncthreads();
        unsigned long long* __restrict__ o = a.acc + (int64_t)row * G * S;
        for (int32_t i = (int32_t)threadIdx.x; i < G * S; i += kExcRowsThreads) {
            const int32_t gi = i / S, j = i % S;
            const unsigned long long v = bins[gi * kExcRowsSlots + (j <= K ? j : 1 + kMaxThresholds + (j - 1 - K))];
            if (v) atomicAdd(&o[i], v);
        }
        __syncthreads();
    }
}

template <bool kW, bool kG>
void launch_eq(const ExceedanceRowsArgs& a, bool equal, dim3 grid, hipStream_t s)
{
    if (equal)
        hipLaunchKernelGGL((exceedance_rows_kernel<kW, kG, true>), grid, dim3(kExcRowsThreads), 0, s, a);
    else
        hipLaunchKernelGGL((exceedance_rows_kernel<kW, kG, false>), grid, dim3(kExcRowsThreads), 0, s, a);
}

}  // namespace

hipError_t launch_exceedance_rows(const ExceedanceRowsArgs& a, bool equal, hipStream_t s)
{
    if (a.N <= 0 || a.n_rows <= 0) return hipSuccess;
    if (a.n_thr < 1 || a.n_thr > kMaxThresholds || (a.group && (a.n_groups < 1 || a.n_groups > kMaxMemberGroups))) return hipErrorInvalidValue;
    const int64_t need = (a.N + kExcRowsThreads - 1) / kExcRowsThreads;
    const dim3 grid((unsigned)(need < kExcRowsBlocks ? need : kExcRowsBlocks), (unsigned)(a.n_rows < 65535 ? a.n_rows : 65535));
    if (a.w && a.group)
        launch_eq<true, true>(a, equal, grid, s);
    else if (a.w)
        launch_eq<true, false>(a, equal, grid, s);
    else if (a.group)
        launch_eq<false, true>(a, equal, grid, s);
    else
        launch_eq<false, false>(a, equal, grid, s);
    return hipGetLastError();
}

}  // namespace rscm
