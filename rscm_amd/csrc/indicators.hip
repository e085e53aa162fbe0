// Per-member indicators of an ensemble and exceedance counts, for gfx950 (MI355X).
//
// indicators_kernel: one thread per member walks a device array of row pointers (resolved by the host with rscm_ens::row_ptr,
// as the radix select's are: full storage, the window, the output store) and keeps, in registers, the sum in row order, the
// maximum and the time of the first row attaining it, and the time of the first row at or above each of up to kMaxThresholds
// thresholds.  Lanes of a wave read consecutive members of one row, so every load is coalesced; each row is read once.  The
// values are the member's x or its anomaly x - b[i] against the handle's baseline (one IEEE subtraction).  A NaN in any row makes
// every indicator of the member NaN.  Without the per-row extras (all == false) the same kernel forms the baseline itself: the
// mean over the reference rows.  The sum starts at -0.0, the additive identity, so it is numpy's rows[0] + rows[1] + ... exactly
// (-ffp-contract=off: no FMA), and the mean is one IEEE division.
//
// exceedance_kernel: per block, the counts (or the summed int64 member weights) of members at or above each threshold and of
// non-NaN members go into LDS int64 bins, then one integer atomic per bin.  No float atomics: the sums are exact and independent
// of the block count, and shards of one ensemble add them exactly.  With the weights' bound (a handle's weights sum to at most
// 2^53, weights.hip) nothing wraps.  exceedance_grouped_kernel: the same sums per member group (rscm_ens_set_member_groups).
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"

namespace rscm {

namespace {

constexpr int kIndThreads = 256;
constexpr int kIndBatch = 8;   // rows whose loads a thread issues before it uses them

template <bool kAnom, bool kAll>
__global__ __launch_bounds__(kIndThreads) void indicators_kernel(const double* const* __restrict__ rows, const double* __restrict__ time,
                                                                  int32_t n_rows, const double* __restrict__ base, int64_t N,
                                                                  int32_t n_thr, Thresholds thr, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kIndThreads + threadIdx.x;
    if (i >= N) return;
    const double b = kAnom ? base[i] : 0.0;
    double sum = -0.0, peak = -__builtin_inf(), peak_t = time[0];
    double cross[kMaxThresholds];
#pragma unroll
    for (int k = 0; k < kMaxThresholds; ++k) cross[k] = __builtin_inf();
    unsigned found = 0u;
    bool nan = false;

    auto take = [&](double x, double t) {
        if constexpr (kAnom) x = x - b;
        nan = nan || x != x;
        sum = sum + x;
        if constexpr (kAll) {
            if (x > peak) {
                peak = x;
                peak_t = t;
            }
#pragma unroll
            for (int k = 0; k < kMaxThresholds; ++k) {
                if (k < n_thr && !(found & (1u << k)) && x >= thr.v[k]) {
                    found |= 1u << k;
                    cross[k] = t;
                }
            }
        }
    };

    int32_t r = 0;
    for (; r + kIndBatch <= n_rows; r += kIndBatch) {
        double x[kIndBatch];
#pragma unroll
        for (int j = 0; j < kIndBatch; ++j) x[j] = rows[r + j][i];
#pragma unroll
        for (int j = 0; j < kIndBatch; ++j) take(x[j], kAll ? time[r + j] : 0.0);
    }
    for (; r < n_rows; ++r) take(rows[r][i], kAll ? time[r] : 0.0);

    const double qnan = __builtin_nan("");
    out[i] = nan ? qnan : sum / (double)n_rows;
    if constexpr (kAll) {
        out[N + i] = nan ? qnan : peak;
        out[2 * N + i] = nan ? qnan : peak_t;
        for (int32_t k = 0; k < n_thr; ++k) out[(3 + (int64_t)k) * N + i] = nan ? qnan : cross[k];
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

constexpr int kExcBlocks = 1024;

template <bool kW>
__global__ __launch_bounds__(kIndThreads) void exceedance_kernel(const double* __restrict__ v, const int64_t* __restrict__ w, int64_t N,
                                                                  int32_t n_thr, Thresholds thr, unsigned long long* __restrict__ acc)
{
    __shared__ unsigned long long bins[kMaxThresholds + 1];
    if (threadIdx.x <= kMaxThresholds) bins[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long hit[kMaxThresholds], tot = 0ull;
#pragma unroll
    for (int k = 0; k < kMaxThresholds; ++k) hit[k] = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * kIndThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kIndThreads) {
        const double x = v[i];
        const unsigned long long wt = kW ? (unsigned long long)w[i] : 1ull;
        if (x == x) {
            tot += wt;
#pragma unroll
            for (int k = 0; k < kMaxThresholds; ++k)
                if (k < n_thr && x >= thr.v[k]) hit[k] += wt;
        }
    }
    tot = wave_sum(tot);
#pragma unroll
    for (int k = 0; k < kMaxThresholds; ++k)
        if (k < n_thr) hit[k] = wave_sum(hit[k]);
    if ((threadIdx.x & 63) == 0) {
        if (tot) atomicAdd(&bins[kMaxThresholds], tot);
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k)
            if (k < n_thr && hit[k]) atomicAdd(&bins[k], hit[k]);
    }
    __syncthreads();
    if ((int32_t)threadIdx.x < n_thr && bins[threadIdx.x]) atomicAdd(&acc[threadIdx.x], bins[threadIdx.x]);
    if ((int32_t)threadIdx.x == n_thr && bins[kMaxThresholds]) atomicAdd(&acc[n_thr], bins[kMaxThresholds]);
}

// exceedance_kernel per member group: acc[g][n_thr + 1] (the hits, then the total) over the members with group[i] == g (-1:
// none).  A thread keeps the integer sums of ONE group in registers -- the group of the members it has met since its last flush --
// and flushes them into the block's LDS int64 bins [n_groups][kMaxThresholds + 1] when it meets another: with contiguous groups that
// is once or twice per thread.  The last flush goes through a wave ladder when the whole wave holds one group (one lane adds the
// wave's sums).  Then one integer atomic per non-zero bin and block: exact, and the order in which blocks finish does not matter.
template <bool kW>
__global__ __launch_bounds__(kIndThreads) void exceedance_grouped_kernel(const double* __restrict__ v, const int64_t* __restrict__ w,
                                                                          const int32_t* __restrict__ group, int32_t n_groups, int64_t N,
                                                                          int32_t n_thr, Thresholds thr, unsigned long long* __restrict__ acc)
{
    constexpr int kRow = kMaxThresholds + 1;
    __shared__ unsigned long long bins[kMaxMemberGroups * kRow];
    for (int32_t i = (int32_t)threadIdx.x; i < n_groups * kRow; i += kIndThreads) bins[i] = 0ull;
    __syncthreads();
    unsigned long long hit[kMaxThresholds], tot = 0ull;
#pragma unroll
    for (int k = 0; k < kMaxThresholds; ++k) hit[k] = 0ull;
    int32_t cur = -1;   // the group the registers hold sums of
    auto flush = [&]() {
        if (cur < 0) return;
        if (tot) atomicAdd(&bins[cur * kRow + kMaxThresholds], tot);
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k)
            if (k < n_thr && hit[k]) atomicAdd(&bins[cur * kRow + k], hit[k]);
        tot = 0ull;
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k) hit[k] = 0ull;
    };
    for (int64_t i = (int64_t)blockIdx.x * kIndThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kIndThreads) {
        const int32_t g = group[i];
        const double x = v[i];
        if (g < 0 || x != x) continue;
        if (g != cur) {
            flush();
            cur = g;
        }
        const unsigned long long wt = kW ? (unsigned long long)w[i] : 1ull;
        tot += wt;
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k)
            if (k < n_thr && x >= thr.v[k]) hit[k] += wt;
    }
    // whole waves arrive here together; lanes that met no member of a group hold zeros and take the wave's group
    const uint64_t have = __ballot(cur >= 0);
    if (have != 0) {
        const int32_t c0 = __shfl(cur, __ffsll((unsigned long long)have) - 1, 64);
        if (__ballot(cur >= 0 && cur != c0) == 0) {
            tot = wave_sum(tot);
#pragma unroll
            for (int k = 0; k < kMaxThresholds; ++k)
                if (k < n_thr) hit[k] = wave_sum(hit[k]);
            cur = (threadIdx.x & 63) == 0 ? c0 : -1;
        }
        flush();
    }
    __syncthreads();
    for (int32_t i = (int32_t)threadIdx.x; i < n_groups * kRow; i += kIndThreads) {
        const int32_t g = i / kRow, k = i % kRow;
        if (!bins[i] || (k >= n_thr && k != kMaxThresholds)) continue;
        atomicAdd(&acc[g * (n_thr + 1) + (k == kMaxThresholds ? n_thr : k)], bins[i]);
    }
}

}  // namespace

hipError_t launch_indicators(const double* const* d_rows, const double* d_time, int32_t n_rows, const double* d_base, int64_t N, bool all,
                             int32_t n_thr, const Thresholds& thr, double* d_out, hipStream_t s)
{
    if (N <= 0 || n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((N + kIndThreads - 1) / kIndThreads));
    if (d_base && all)
        hipLaunchKernelGGL((indicators_kernel<true, true>), grid, dim3(kIndThreads), 0, s, d_rows, d_time, n_rows, d_base, N, n_thr, thr, d_out);
    else if (d_base)
        hipLaunchKernelGGL((indicators_kernel<true, false>), grid, dim3(kIndThreads), 0, s, d_rows, d_time, n_rows, d_base, N, n_thr, thr, d_out);
    else if (all)
        hipLaunchKernelGGL((indicators_kernel<false, true>), grid, dim3(kIndThreads), 0, s, d_rows, d_time, n_rows, d_base, N, n_thr, thr, d_out);
    else
        hipLaunchKernelGGL((indicators_kernel<false, false>), grid, dim3(kIndThreads), 0, s, d_rows, d_time, n_rows, d_base, N, n_thr, thr, d_out);
    return hipGetLastError();
}

hipError_t launch_exceedance(const double* d_v, const int64_t* d_w, int64_t N, int32_t n_thr, const Thresholds& thr,
                             unsigned long long* d_acc, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const int64_t need = (N + kIndThreads - 1) / kIndThreads;
    const dim3 grid((unsigned)(need < kExcBlocks ? need : kExcBlocks));
    if (d_w)
        hipLaunchKernelGGL(exceedance_kernel<true>, grid, dim3(kIndThreads), 0, s, d_v, d_w, N, n_thr, thr, d_acc);
    else
        hipLaunchKernelGGL(exceedance_kernel<false>, grid, dim3(kIndThreads), 0, s, d_v, d_w, N, n_thr, thr, d_acc);
    return hipGetLastError();
}

hipError_t launch_exceedance_grouped(const double* d_v, const int64_t* d_w, const int32_t* d_group, int32_t n_groups, int64_t N,
                                     int32_t n_thr, const Thresholds& thr, unsigned long long* d_acc, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const int64_t need = (N + kIndThreads - 1) / kIndThreads;
    const dim3 grid((unsigned)(need < kExcBlocks ? need : kExcBlocks));
    if (d_w)
        hipLaunchKernelGGL(exceedance_grouped_kernel<true>, grid, dim3(kIndThreads), 0, s, d_v, d_w, d_group, n_groups, N, n_thr, thr, d_acc);
    else
        hipLaunchKernelGGL(exceedance_grouped_kernel<false>, grid, dim3(kIndThreads), 0, s, d_v, d_w, d_group, n_groups, N, n_thr, thr, d_acc);
    return hipGetLastError();
}

}  // namespace rscm
