// Exact ensemble quantiles by a multi-pass radix select over resident rows, for gfx950 (MI355X).
//
// numpy.nanquantile, method "linear", per row (rscm_ens_quantile_series, rscm_ens_quantile_rows and the staged
// select), reached without sorting and without member-sized scratch: every double maps to an order-preserving
// 64-bit key (-0.0 before +0.0, NaNs of either sign left out), and each target order statistic is found
// digit by digit from the top.  Pass p histograms digit p (8 bits) of the members whose key matches a
// target's prefix of p digits; a commit then picks, per (row, target), the bucket holding the target's
// remaining rank and extends the prefix.  Eight passes give the whole key.
//
// Signed zeros: the order of the keys (-0.0 first) makes the sign of a zero result a function of the member
// set alone, not of where the members sit, which is what lets shards combine.
//
// Everything summed across workgroups (and, by the caller, across ranks) is an int64 count or weight: integer
// sums are exact and independent of their order, so the result does not depend on the block count,
// the number of ranks or the order in which they add.  No float atomics.
//
// Rows reach the kernels through a device array of row pointers (the host resolves them with
// rscm_ens::row_ptr), so full storage, the window and the strided output store all work alike -- and so does any device
// vector of N doubles (rscm_ens_select_begin_vectors: indicators, parameter rows).  The histogram pass can count each
// member's anomaly x - b[i] against the handle's baseline instead of x (rscm_ens_set_baseline).
//
// The weighted select (kW) is numpy.nanquantile(row, q, weights=w, method="inverted_cdf") with integer member weights: per
// (row, q) the target is the smallest integer C* >= 1 with (double)C* / (double)W >= q, W the summed weight of the row's
// non-NaN members, and the result is the first key, in key order, at which the cumulative weight reaches C*.  It is the same
// select with every counted member adding its weight instead of 1: one target per quantile, no interpolation.  Weights are int64
// and W <= 2^53 (the handle refuses weights that sum to more; weights.hip), so every histogram sum -- across workgroups here and
// across ranks by the caller -- is exact and independent of its order, as the unweighted counts are.
//
// The grouped select (kG; rscm_ens_set_member_groups) gives every member a group and every (row, group) its
// own histograms, targets and result: the same select with (row, group) as the row of the commit and finish kernels and a
// histogram pass that counts a member only into the histograms of its own group.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rscm_device.hpp"
#include "select_keys.hpp"

namespace rscm {

namespace {

constexpr int kSelThreads = 256;
constexpr long long kWMax = 1ll << 53;   // the largest row weight W the weighted select accepts

// An LDS bin: a 32-bit count, or (kW) a 64-bit sum of weights
template <bool kW>
using SelBin = std::conditional_t<kW, unsigned long long, unsigned>;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Adds v to bin[b] for every lane with `valid` (kW: and v != 0); called by all 64 lanes of the wave together.  When every adding
// lane has the same bin (clustered members: the top digits of a variable's keys are mostly equal) one lane adds the wave's
// total -- the lane count, or (kW) a wave sum of the weights -- instead of up to 64 atomics on one LDS address.
template <bool kW>
__device__ __forceinline__ void lds_add(SelBin<kW>* bins, unsigned b, SelBin<kW> v, bool valid)
{
    if constexpr (kW) valid = valid && v != 0ull;
    const uint64_t m = __ballot(valid);
    if (m == 0) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const unsigned b0 = (unsigned)__shfl((int)b, lead, 64);
    if (__ballot(valid && b == b0) == m) {
        SelBin<kW> total;
        if constexpr (kW)
            total = wave_sum_u64(valid ? v : 0ull);
        else
            total = (unsigned)__popcll(m);
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&bins[b0], total);
    } else if (valid) {
        atomicAdd(&bins[b], v);
    }
}

// One pass over rows[r] (blockIdx.y) for the targets [g0, g0 + gn) of each row.  Pass 0 fills one
// histogram per row (all targets share the empty prefix): hist[r][256].  Later passes fill
// hist[r][n_t][256] for the targets of the group.  Blocks of one row split its members in pair-aligned
// chunks; each flushes its LDS bins with one integer atomic per non-zero bin.
//
// kW: member i adds w[i] instead of 1, zero weights skipped.  Its 64-bit bins are dynamic LDS, nh x kSelBins x 8 B: 2 KiB in
// pass 0, at most kSelGroup x 2 KiB = 32 KiB later; the unweighted bins are static, kSelGroup x kSelBins x 4 B.  w is
// hipMalloc'd, so its pairs are 16-byte aligned exactly when the row's are.  The unweighted instantiations never read w.
//
// kAnom: member i counts the key of its anomaly x - base[i] (one IEEE subtraction; a NaN anomaly is left out).  base is
// handle-owned, hence 16-byte aligned: its pairs line up with the row's only when the row has no unpaired head member.  The
// plain instantiations (kAnom false) never read base.
//
// kG (the grouped select): member i counts only into the histograms of its own group, group[i] (-1: none).  A row then has
// n_slots histograms -- slot g in pass 0, slot g * n_t + t later -- laid out [r][n_slots][256], and a launch fills the slots
// [g0, g0 + gn), gn <= kSelGroup, in LDS exactly as the ungrouped launch fills gn targets.  The group picks the LDS base: a
// member looks only at the targets of its own group that lie in the launch's slots (at most min(n_t, gn) comparisons, not one
// per slot), and lds_add gets the bin index within all gn histograms, so a wave whose members share group, target and digit --
// contiguous groups, clustered keys -- still adds once.  group is handle-owned (16-byte aligned): its ids are read as int2 pairs
// when the row has no unpaired head member, else one by one, as the weights' pairs are.  The ids are read first, and a lane whose
// two members belong to no group of the launch's slots does not load them: with contiguous groups the launches after the first
// skip the rows of the other groups.  The instantiations without kG never read group or n_slots.
template <bool kW, bool kAnom, bool kG = false>
__global__ __launch_bounds__(kSelThreads) void select_hist_kernel(const double* const* __restrict__ rows, const int64_t* __restrict__ w,
                                                                   const double* __restrict__ base, int64_t N, int32_t pass,
                                                                   const uint64_t* __restrict__ prefix, int32_t n_t, int32_t g0,
                                                                   int32_t gn, unsigned long long* __restrict__ hist,
                                                                   const int32_t* __restrict__ group, int32_t n_slots)
{
    using Bin = SelBin<kW>;
    Bin* bins;
    if constexpr (kW) {
        extern __shared__ unsigned long long wbins[];
        bins = wbins;
    } else {
        __shared__ unsigned cbins[kSelGroup * kSelBins];
        bins = cbins;
    }
    __shared__ uint64_t pre[kSelGroup];
    const int32_t r = (int32_t)blockIdx.y;
    const int32_t nh = kG ? gn : (pass == 0 ? 1 : gn);
    for (int32_t i = (int32_t)threadIdx.x; i < nh * kSelBins; i += kSelThreads) bins[i] = 0;
    if ((int32_t)threadIdx.x < nh && pass > 0) pre[threadIdx.x] = prefix[(size_t)r * (kG ? n_slots : n_t) + g0 + threadIdx.x];
    __syncthreads();
    // kG: the groups with a slot in this launch, and the targets of one group a member has to look at (the launch's slots lie in
    // one group: those; else all n_t)
    const int32_t per_g = pass == 0 ? 1 : n_t;
    const int32_t g_lo = kG ? g0 / per_g : 0, g_hi = kG ? (g0 + gn - 1) / per_g : 0;
    const int32_t t_lo = kG && g_lo == g_hi ? g0 - g_lo * per_g : 0, t_hi = kG && g_lo == g_hi ? t_lo + gn : n_t;

    const double* row = rows[r];
    // rows start 8-byte aligned (odd N): the first member goes alone, the rest as 16-byte pairs
    const int64_t head = ((uintptr_t)row & 15) ? 1 : 0;
    const int64_t pairs = (N - head) / 2;
    const int64_t per = (pairs + gridDim.x - 1) / gridDim.x;
    const int64_t pb = (int64_t)blockIdx.x * per, pe = pb + per < pairs ? pb + per : pairs;
    const int shift = 56 - 8 * pass;   // the digit of this pass: bits [shift, shift + 8)
    const double2* row2 = reinterpret_cast<const double2*>(row + head);
    const int64_t* wp = w + head;   // kW: the weights of the pairs
    const int32_t* gp = group + head;   // kG: the groups of the pairs

    auto count = [&](double x, Bin v, bool in, int32_t g) {
        const bool ok = in && x == x;
        const uint64_t k = order_key(x);
        const unsigned d = (unsigned)(k >> shift) & (kSelBins - 1);
        if constexpr (kG) {
            if (pass == 0) {
                const int32_t s = g - g0;
                const bool mine = ok && s >= 0 && s < gn;
                lds_add<kW>(bins, (unsigned)(mine ? s : 0) * kSelBins + d, v, mine);
                return;
            }
            const uint64_t top = k >> (shift + 8);
            const int32_t sb = g * n_t - g0;   // the member's first slot, relative to the launch's
            for (int32_t t = t_lo; t < t_hi; ++t) {
                const bool mine = ok && g >= g_lo && sb + t >= 0 && sb + t < gn;
                const int32_t s = mine ? sb + t : 0;
                lds_add<kW>(bins, (unsigned)s * kSelBins + d, v, mine && top == pre[s]);
            }
            return;
        }
        if (pass == 0) {
            lds_add<kW>(bins, d, v, ok);
            return;
        }
        const uint64_t top = k >> (shift + 8);
        for (int32_t t = 0; t < gn; ++t) lds_add<kW>(bins + t * kSelBins, d, v, ok && top == pre[t]);
    };

    for (int64_t c0 = pb; c0 < pe; c0 += kSelThreads) {   // uniform trip count: whole waves call lds_add
        const int64_t i = c0 + threadIdx.x;
        const bool in = i < pe;
        double2 v = make_double2(0.0, 0.0);
        Bin v0 = kW ? 0 : 1, v1 = v0;   // what each member of the pair adds
        int32_t ga = -1, gb = -1;
        bool ld = in;
        if constexpr (kG) {
            if (in) {
                if (head) {
                    ga = gp[2 * i];
                    gb = gp[2 * i + 1];
                } else {
                    const int2 p = reinterpret_cast<const int2*>(gp)[i];
                    ga = p.x;
                    gb = p.y;
                }
            }
            ld = (ga >= g_lo && ga <= g_hi) || (gb >= g_lo && gb <= g_hi);
        }
        if (ld) {
            v = row2[i];
            if constexpr (kAnom) {
                const double* bp = base + head + 2 * i;
                const double2 b = head ? make_double2(bp[0], bp[1]) : *reinterpret_cast<const double2*>(bp);
                v.x = v.x - b.x;
                v.y = v.y - b.y;
            }
            if constexpr (kW) {
                if (head) {
                    v0 = (Bin)wp[2 * i];
                    v1 = (Bin)wp[2 * i + 1];
                } else {
                    const longlong2 p = reinterpret_cast<const longlong2*>(wp)[i];
                    v0 = (Bin)p.x;
                    v1 = (Bin)p.y;
                }
            }
        }
        count(v.x, v0, in, ga);
        count(v.y, v1, in, gb);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {   // the unpaired head and tail members, one wave
        const bool in_head = head && threadIdx.x == 0;
        const bool in_tail = ((N - head) & 1) && threadIdx.x == 1;
        const bool in = in_head || in_tail;
        const int64_t m = in_head ? 0 : N - 1;
        double x = in ? row[m] : 0.0;
        if constexpr (kAnom) {
            if (in) x = x - base[m];
        }
        Bin v = 1;
        if constexpr (kW) v = in ? (Bin)w[m] : 0ull;
        int32_t g = -1;
        if constexpr (kG) g = in ? group[m] : -1;
        count(x, v, in, g);
    }
    __syncthreads();
    unsigned long long* out = hist + (kG ? ((size_t)r * n_slots + g0) * kSelBins
                                         : (pass == 0 ? (size_t)r * kSelBins : ((size_t)r * n_t + g0) * kSelBins));
    for (int32_t i = (int32_t)threadIdx.x; i < nh * kSelBins; i += kSelThreads)
        if (bins[i]) atomicAdd(out + i, (unsigned long long)bins[i]);
}

// The smallest integer C >= 1 with (double)C / (double)W >= q (IEEE division), 1 <= W <= 2^53: fl(C / W) is monotone in C, so
// a few steps from ceil(q W) reach it.
__device__ __forceinline__ int64_t weight_target(double q, int64_t W)
{
    const double dw = (double)W;
    double c = ceil(q * dw);
    if (c < 1.0) c = 1.0;
    if (c > dw) c = dw;
    int64_t C = (int64_t)c;
    while (C > 1 && (double)(C - 1) / dw >= q) --C;
    while (C < W && (double)C / dw < q) ++C;
    return C;
}

// One thread per (row, target).  Pass 0 gives each target the cumulative count it has to reach in its row: the 1-based rank of
// one of numpy's linear order statistics on the row's n non-NaN members, or (kW) the C* of weight_target on the row's weight W;
// n and W are sums of the reduced histograms, so global, and go to count[r].  rank < 0: the row has no member.  Every pass:
// the bucket in which the cumulative count reaches the remaining target, which then drops by the count below that bucket.
template <bool kW>
__global__ void select_commit_kernel(const long long* __restrict__ hist, int32_t pass, int32_t n_rows, int32_t n_t,
                                     const double* __restrict__ q, int64_t* __restrict__ count, uint64_t* __restrict__ prefix,
                                     int64_t* __restrict__ rank, int32_t* __restrict__ over)
{
    const int32_t idx = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= n_rows * n_t) return;
    const int32_t r = idx / n_t, t = idx % n_t;
    const long long* h;
    int64_t want;
    if (pass == 0) {
        h = hist + (size_t)r * kSelBins;
        if constexpr (kW) {   // W = the sum of the histogram; rows with W == 0 or W > 2^53 (flagged in *over) get rank -1
            long long W = 0;
            bool big = false;
            for (int b = 0; b < kSelBins; ++b) {   // a bin above 2^53 ends the sum, so W (<= 256 x 2^53) cannot wrap
                if (h[b] < 0 || h[b] > kWMax) big = true;
                W += big ? 0 : h[b];
            }
            big = big || W > kWMax;
            if (t == 0) {
                count[r] = big ? 0 : W;
                if (big) *over = 1;
            }
            if (big || W == 0) {
                prefix[idx] = 0;
                rank[idx] = -1;
                return;
            }
            want = weight_target(q[t], W);
        } else {   // n = the sum of the histogram; target t is order statistic ip (t even) or ip + 1 clipped (t odd) of q[t / 2]
            int64_t n = 0;
            for (int b = 0; b < kSelBins; ++b) n += h[b];
            if (t == 0) count[r] = n;
            if (n == 0) {
                prefix[idx] = 0;
                rank[idx] = -1;
                return;
            }
            const double vi = (double)(n - 1) * q[t / 2];   // numpy _compute_virtual_index for "linear"
            double prev = floor(vi);
            if (prev < 0.0) prev = 0.0;
            if (prev > (double)(n - 1)) prev = (double)(n - 1);
            const int64_t ip = (int64_t)prev;
            want = (t & 1) && ip + 1 < n ? ip + 2 : ip + 1;   // 1-based
        }
    } else {
        want = rank[idx];
        if (want < 0) return;
        h = hist + (size_t)idx * kSelBins;
    }
    int64_t below = 0;
    int b = 0;
    for (; b < kSelBins - 1; ++b) {
        if (want <= below + h[b]) break;
        below += h[b];
    }
    prefix[idx] = pass == 0 ? (uint64_t)b : (prefix[idx] << 8) | (uint64_t)b;
    rank[idx] = want - below;
}

// out[r][0] = count (kW: W), out[r][1 + k] = quantile q[k], NaN for a row without members.  kW: the value of the selected
// key.  Unweighted: the two order statistics a, b of numpy's virtual index (n - 1) q (_compute_virtual_index(n, q, 1, 1)) from
// their full keys, then numpy's _lerp (function_base.py) with its own roundings, so the result carries numpy's bits:
// a + (b - a) g, from b's side for g >= 0.5, and a itself where b - a == 0 (which also keeps inf - inf out).
template <bool kW>
__global__ void select_finish_kernel(const int64_t* __restrict__ count, const uint64_t* __restrict__ keys, int32_t n_rows, int32_t n_q,
                                     const double* __restrict__ q, double* __restrict__ out)
{
    const int32_t idx = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= n_rows * (n_q + 1)) return;
    const int32_t r = idx / (n_q + 1), k = idx % (n_q + 1);
    const int64_t n = count[r];
    if (k == 0) {
        out[idx] = (double)n;
        return;
    }
    if (n == 0) {
        out[idx] = __builtin_nan("");
        return;
    }
    if constexpr (kW) {
        out[idx] = key_value(keys[(size_t)r * n_q + (k - 1)]);
    } else {
        const double t = q[k - 1];
        const double vi = (double)(n - 1) * t;
        double prev = floor(vi);
        if (prev < 0.0) prev = 0.0;
        if (prev > (double)(n - 1)) prev = (double)(n - 1);
        const double g = vi - prev;
        const size_t s = (size_t)r * (2 * n_q) + 2 * (k - 1);
        const double a = key_value(keys[s]), b = key_value(keys[s + 1]);
        const double d = b - a;
        double v = a + d * g;
        if (g >= 0.5) v = b - d * (1.0 - g);
        if (d == 0.0) v = a;
        out[idx] = v;
    }
}

__global__ void groups_check_kernel(const int32_t* __restrict__ group, int64_t N, int32_t n_groups, int32_t* __restrict__ flag)
{
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
        bad = bad || group[i] < -1 || group[i] >= n_groups;
    if (bad) *flag = 1;
}

}  // namespace

int32_t select_blocks_per_row(int64_t N, int32_t n_rows)
{
    // enough workgroups to fill the chip (~8 per CU) but at least ~4096 members each, so that the flush
    // (one integer atomic per non-zero bin) stays small next to the members a block reads
    const int64_t by_size = (N + 4095) / 4096;
    const int64_t by_chip = (2048 + n_rows - 1) / n_rows;
    int64_t b = by_size < by_chip ? by_size : by_chip;
    if (b < 1) b = 1;
    if (b > 65535) b = 65535;
    return (int32_t)b;
}

hipError_t launch_select_hist(const double* const* d_rows, const int64_t* d_w, const double* d_base, const int32_t* d_group,
                              int32_t n_groups, int64_t N, int32_t n_rows, int32_t pass, const uint64_t* d_prefix, int32_t n_t,
                              int64_t* d_hist, size_t hist_elems, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(d_hist, 0, hist_elems * sizeof(int64_t), s);
    if (e != hipSuccess || n_rows <= 0 || N <= 0) return e;
    const unsigned bpr = (unsigned)select_blocks_per_row(N, n_rows);
    if (d_group) {   // the grouped select: n_slots histograms per row, kSelGroup of them per launch
        const auto gkernel = d_w ? (d_base ? select_hist_kernel<true, true, true> : select_hist_kernel<true, false, true>)
                                 : (d_base ? select_hist_kernel<false, true, true> : select_hist_kernel<false, false, true>);
        const int32_t n_slots = pass == 0 ? n_groups : n_groups * n_t;
        for (int32_t r0 = 0; r0 < n_rows; r0 += kMaxGridY) {
            const int32_t nr = n_rows - r0 < kMaxGridY ? n_rows - r0 : kMaxGridY;
            auto* h = reinterpret_cast<unsigned long long*>(d_hist) + (size_t)r0 * n_slots * kSelBins;
            const uint64_t* pre = d_prefix + (size_t)r0 * n_groups * n_t;
            for (int32_t s0 = 0; s0 < n_slots; s0 += kSelGroup) {
                const int32_t sn = n_slots - s0 < kSelGroup ? n_slots - s0 : kSelGroup;
                const size_t lds = d_w ? (size_t)sn * kSelBins * sizeof(unsigned long long) : 0;
                hipLaunchKernelGGL(gkernel, dim3(bpr, (unsigned)nr), dim3(kSelThreads), lds, s, d_rows + r0, d_w, d_base, N, pass, pre, n_t,
                                   s0, sn, h, d_group, n_slots);
                if ((e = hipGetLastError()) != hipSuccess) return e;
            }
        }
        return hipSuccess;
    }
    const auto kernel = d_w ? (d_base ? select_hist_kernel<true, true> : select_hist_kernel<true, false>)
                            : (d_base ? select_hist_kernel<false, true> : select_hist_kernel<false, false>);
    for (int32_t r0 = 0; r0 < n_rows; r0 += kMaxGridY) {   // rows in slices the grid's y dimension can index
        const int32_t nr = n_rows - r0 < kMaxGridY ? n_rows - r0 : kMaxGridY;
        const size_t row_elems = (size_t)kSelBins * (pass == 0 ? 1 : (size_t)n_t);
        auto* h = reinterpret_cast<unsigned long long*>(d_hist) + (size_t)r0 * row_elems;
        const uint64_t* pre = d_prefix + (size_t)r0 * n_t;
        for (int32_t g0 = 0; g0 < (pass == 0 ? 1 : n_t); g0 += kSelGroup) {
            const int32_t gn = pass == 0 ? 1 : (n_t - g0 < kSelGroup ? n_t - g0 : kSelGroup);
            const size_t lds = d_w ? (size_t)gn * kSelBins * sizeof(unsigned long long) : 0;   // the weighted bins
            hipLaunchKernelGGL(kernel, dim3(bpr, (unsigned)nr), dim3(kSelThreads), lds, s, d_rows + r0, d_w, d_base, N, pass, pre, n_t, g0,
                               gn, h, nullptr, 0);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_groups_check(const int32_t* d_group, int64_t N, int32_t n_groups, int32_t* d_flag, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const int64_t need = (N + 255) / 256;
    hipLaunchKernelGGL(groups_check_kernel, dim3((unsigned)(need < 1024 ? need : 1024)), dim3(256), 0, s, d_group, N, n_groups, d_flag);
    return hipGetLastError();
}

hipError_t launch_select_commit(const int64_t* d_hist, int32_t pass, int32_t n_rows, int32_t n_t, const double* d_q, int64_t* d_count,
                                uint64_t* d_prefix, int64_t* d_rank, int32_t* d_over, hipStream_t s)
{
    const int64_t threads = (int64_t)n_rows * n_t;
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(d_over ? select_commit_kernel<true> : select_commit_kernel<false>, dim3((unsigned)((threads + 255) / 256)), dim3(256),
                       0, s, reinterpret_cast<const long long*>(d_hist), pass, n_rows, n_t, d_q, d_count, d_prefix, d_rank, d_over);
    return hipGetLastError();
}

hipError_t launch_select_finish(const int64_t* d_count, const uint64_t* d_keys, int32_t n_rows, int32_t n_q, const double* d_q,
                                bool weighted, double* d_out, hipStream_t s)
{
    const int64_t threads = (int64_t)n_rows * (n_q + 1);
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(weighted ? select_finish_kernel<true> : select_finish_kernel<false>, dim3((unsigned)((threads + 255) / 256)),
                       dim3(256), 0, s, d_count, d_keys, n_rows, n_q, d_q, d_out);
    return hipGetLastError();
}

}  // namespace rscm
