// Likelihood-weighted ensemble quantiles by the radix select of select.hip, for gfx950 (MI355X).
//
// numpy.nanquantile(row, q, weights=w, method="inverted_cdf") with integer member weights: per (row, q) the target is the
// smallest integer C* >= 1 with (double)C* / (double)W >= q, W the summed weight of the row's non-NaN members, and the result
// is the first key, in key order, at which the cumulative weight reaches C*.  The select is the unweighted one with every
// counted member adding its weight instead of 1 and the commit walking "remaining weight" instead of "remaining rank"; one
// target per quantile, no interpolation.  Weights are int64 and W <= 2^53, so every histogram sum -- across workgroups here
// and across ranks by the caller -- is exact and independent of its order, as the unweighted counts are.
//
// Also here: the two kernels that turn a per-member log-likelihood into such weights (the max over finite, ok members, and
// the quantisation w = llround(exp(min(ll - ll_max, 0)) * 2^bits)), and the check of a weight vector before a handle takes it:
// no negative weight, and a total of at most 2^53.  That bound on every handle is what keeps every sum above from wrapping: a
// bin of one handle holds at most 2^53, and a SUM over up to 2^10 handles (ranks) stays below 2^63, where the commit's check
// against 2^53 still sees it.
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"
#include "select_keys.hpp"

namespace rscm {

namespace {

constexpr int kWSelThreads = 256;
constexpr long long kWMax = 1ll << 53;   // the largest row weight W the select accepts

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Adds w to bin[b] for every lane with `valid` (and w != 0); called by all 64 lanes of the wave together.  When every adding
// lane has the same bin, a wave sum of the weights and one atomic replace up to 64 atomics on one LDS address.
__device__ __forceinline__ void lds_wadd(unsigned long long* bins, unsigned b, unsigned long long w, bool valid)
{
    valid = valid && w != 0ull;
    const uint64_t m = __ballot(valid);
    if (m == 0) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const unsigned b0 = (unsigned)__shfl((int)b, lead, 64);
    if (__ballot(valid && b == b0) == m) {
        const unsigned long long s = wave_sum_u64(valid ? w : 0ull);
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&bins[b0], s);
    } else if (valid) {
        atomicAdd(&bins[b], w);
    }
}

// select_hist_kernel (select.hip) with member i adding w[i]: the same row split, pair loads, head and tail.  The 64-bit LDS
// bins are dynamic shared memory, nh x kSelBins x 8 B: 2 KiB in pass 0, at most kSelGroup x 2 KiB = 32 KiB later.
// kAnom: the key of x - base[i], as select_hist_kernel<true> (base handle-owned, 16-byte aligned like w).
template <bool kAnom>
__global__ __launch_bounds__(kWSelThreads) void wselect_hist_kernel(const double* const* __restrict__ rows, const int64_t* __restrict__ w,
                                                                     const double* __restrict__ base, int64_t N, int32_t pass,
                                                                     const uint64_t* __restrict__ prefix, int32_t n_t, int32_t g0,
                                                                     int32_t gn, unsigned long long* __restrict__ hist)
{
    extern __shared__ unsigned long long wbins[];
    __shared__ uint64_t pre[kSelGroup];
    const int32_t r = (int32_t)blockIdx.y;
    const int32_t nh = pass == 0 ? 1 : gn;
    for (int32_t i = (int32_t)threadIdx.x; i < nh * kSelBins; i += kWSelThreads) wbins[i] = 0ull;
    if ((int32_t)threadIdx.x < nh && pass > 0) pre[threadIdx.x] = prefix[(size_t)r * n_t + g0 + threadIdx.x];
    __syncthreads();

    const double* row = rows[r];
    const int64_t head = ((uintptr_t)row & 15) ? 1 : 0;
    const int64_t pairs = (N - head) / 2;
    const int64_t per = (pairs + gridDim.x - 1) / gridDim.x;
    const int64_t pb = (int64_t)blockIdx.x * per, pe = pb + per < pairs ? pb + per : pairs;
    const int shift = 56 - 8 * pass;
    const double2* row2 = reinterpret_cast<const double2*>(row + head);
    const int64_t* wp = w + head;   // the weights of the pairs: 16-byte aligned iff the row is (hipMalloc'd weights)

    auto count = [&](double x, unsigned long long wt, bool in) {
        const bool ok = in && x == x;
        const uint64_t k = order_key(x);
        const unsigned d = (unsigned)(k >> shift) & (kSelBins - 1);
        if (pass == 0) {
            lds_wadd(wbins, d, wt, ok);
            return;
        }
        const uint64_t top = k >> (shift + 8);
        for (int32_t t = 0; t < gn; ++t) lds_wadd(wbins + t * kSelBins, d, wt, ok && top == pre[t]);
    };

    for (int64_t c0 = pb; c0 < pe; c0 += kWSelThreads) {   // uniform trip count: whole waves call lds_wadd
        const int64_t i = c0 + threadIdx.x;
        const bool in = i < pe;
        double2 v = make_double2(0.0, 0.0);
        unsigned long long w0 = 0ull, w1 = 0ull;
        if (in) {
            v = row2[i];
            if constexpr (kAnom) {
                const double* bp = base + head + 2 * i;
                const double2 b = head ? make_double2(bp[0], bp[1]) : *reinterpret_cast<const double2*>(bp);
                v.x = v.x - b.x;
                v.y = v.y - b.y;
            }
            if (head) {
                w0 = (unsigned long long)wp[2 * i];
                w1 = (unsigned long long)wp[2 * i + 1];
            } else {
                const longlong2 p = reinterpret_cast<const longlong2*>(wp)[i];
                w0 = (unsigned long long)p.x;
                w1 = (unsigned long long)p.y;
            }
        }
        count(v.x, w0, in);
        count(v.y, w1, in);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {   // the unpaired head and tail members, one wave
        const bool in_head = head && threadIdx.x == 0;
        const bool in_tail = ((N - head) & 1) && threadIdx.x == 1;
        const int64_t m = in_head ? 0 : N - 1;
        double x = (in_head || in_tail) ? row[m] : 0.0;
        if constexpr (kAnom) {
            if (in_head || in_tail) x = x - base[m];
        }
        const unsigned long long wt = (in_head || in_tail) ? (unsigned long long)w[m] : 0ull;
        count(x, wt, in_head || in_tail);
    }
    __syncthreads();
    unsigned long long* out = hist + (pass == 0 ? (size_t)r * kSelBins : ((size_t)r * n_t + g0) * kSelBins);
    for (int32_t i = (int32_t)threadIdx.x; i < nh * kSelBins; i += kWSelThreads)
        if (wbins[i]) atomicAdd(out + i, wbins[i]);
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

// One thread per (row, quantile).  Pass 0: W = the sum of the (reduced) histogram, stored as the row's count; rows with
// W == 0, or W > 2^53 (flagged in *over), get rank -1.  Every pass: the bucket in which the cumulative weight reaches the
// remaining target, which then drops by the weight below that bucket.
__global__ void wselect_commit_kernel(const long long* __restrict__ hist, int32_t pass, int32_t n_rows, int32_t n_t,
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

// out[r][0] = W, out[r][1 + k] = the value of the selected key of quantile k (NaN where W == 0).
__global__ void wselect_finish_kernel(const int64_t* __restrict__ count, const uint64_t* __restrict__ keys, int32_t n_rows,
                                      int32_t n_q, double* __restrict__ out)
{
    const int32_t idx = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= n_rows * (n_q + 1)) return;
    const int32_t r = idx / (n_q + 1), k = idx % (n_q + 1);
    const int64_t W = count[r];
    if (k == 0)
        out[idx] = (double)W;
    else
        out[idx] = W == 0 ? __builtin_nan("") : key_value(keys[(size_t)r * n_q + (k - 1)]);
}

// *out_key = max(order_key(ll[i])) over members with status 0 and a finite ll; *out_key starts as order_key(-inf)
__global__ __launch_bounds__(kWSelThreads) void loglik_max_kernel(const double* __restrict__ ll, const uint8_t* __restrict__ status,
                                                                   int64_t N, unsigned long long* __restrict__ out_key)
{
    unsigned long long m = order_key(-__builtin_inf());
    for (int64_t i = (int64_t)blockIdx.x * kWSelThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kWSelThreads) {
        const double x = ll[i];
        if (status[i] == 0 && isfinite(x)) {
            const unsigned long long k = order_key(x);
            m = k > m ? k : m;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out_key, m);
}

__global__ __launch_bounds__(kWSelThreads) void weights_from_loglik_kernel(const double* __restrict__ ll, const uint8_t* __restrict__ status,
                                                                            int64_t N, double ll_max, int32_t bits, int64_t* __restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * kWSelThreads + threadIdx.x;
    if (i >= N) return;
    const double x = ll[i];
    if (status[i] != 0 || !isfinite(x)) {
        w[i] = 0;
        return;
    }
    double d = x - ll_max;
    if (!(d < 0.0)) d = 0.0;   // ll above the given max: clamped to weight 2^bits
    w[i] = (int64_t)llround(ldexp(exp(d), bits));
}

// *flag = 1 if any w[i] < 0; *total += this block's sum of the weights, saturated at 2^53 + 1.  At most kCheckBlocks blocks, so
// *total <= kCheckBlocks x (2^53 + 1) < 2^64 never wraps, and *total > 2^53 iff the true total is.
constexpr int kCheckBlocks = 1024;
constexpr unsigned long long kSat = (1ull << 53) + 1ull;

__device__ __forceinline__ unsigned long long sat_add(unsigned long long a, unsigned long long b)
{
    return a >= kSat || b >= kSat || a + b >= kSat ? kSat : a + b;
}

__global__ __launch_bounds__(kWSelThreads) void weights_check_kernel(const int64_t* __restrict__ w, int64_t N, int32_t* __restrict__ flag,
                                                                      unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long part[kWSelThreads / 64];
    unsigned long long s = 0ull;
    bool neg = false;
    for (int64_t i = (int64_t)blockIdx.x * kWSelThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kWSelThreads) {
        const int64_t x = w[i];
        neg = neg || x < 0;
        s = sat_add(s, x < 0 ? 0ull : (unsigned long long)x);
    }
    if (neg) *flag = 1;
    for (int off = 32; off > 0; off >>= 1) s = sat_add(s, __shfl_xor(s, off, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0ull;
        for (int k = 0; k < kWSelThreads / 64; ++k) b = sat_add(b, part[k]);
        if (b) atomicAdd(total, b);
    }
}

unsigned grid_of(int64_t n) { return (unsigned)((n + kWSelThreads - 1) / kWSelThreads); }

}  // namespace

hipError_t launch_wselect_hist(const double* const* d_rows, const int64_t* d_w, const double* d_base, int64_t N, int32_t n_rows,
                               int32_t pass, const uint64_t* d_prefix, int32_t n_t, int64_t* d_hist, size_t hist_elems, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(d_hist, 0, hist_elems * sizeof(int64_t), s);
    if (e != hipSuccess || n_rows <= 0 || N <= 0) return e;
    const unsigned bpr = (unsigned)select_blocks_per_row(N, n_rows);
    constexpr int32_t kMaxGridY = 65535;
    for (int32_t r0 = 0; r0 < n_rows; r0 += kMaxGridY) {
        const int32_t nr = n_rows - r0 < kMaxGridY ? n_rows - r0 : kMaxGridY;
        const size_t row_elems = (size_t)kSelBins * (pass == 0 ? 1 : (size_t)n_t);
        auto* h = reinterpret_cast<unsigned long long*>(d_hist) + (size_t)r0 * row_elems;
        const uint64_t* pre = d_prefix + (size_t)r0 * n_t;
        for (int32_t g0 = 0; g0 < (pass == 0 ? 1 : n_t); g0 += kSelGroup) {
            const int32_t gn = pass == 0 ? 1 : (n_t - g0 < kSelGroup ? n_t - g0 : kSelGroup);
            const size_t lds = (size_t)gn * kSelBins * sizeof(unsigned long long);
            if (d_base)
                hipLaunchKernelGGL(wselect_hist_kernel<true>, dim3(bpr, (unsigned)nr), dim3(kWSelThreads), lds, s, d_rows + r0, d_w, d_base, N,
                                   pass, pre, n_t, g0, gn, h);
            else
                hipLaunchKernelGGL(wselect_hist_kernel<false>, dim3(bpr, (unsigned)nr), dim3(kWSelThreads), lds, s, d_rows + r0, d_w, d_base,
                                   N, pass, pre, n_t, g0, gn, h);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_wselect_commit(const int64_t* d_hist, int32_t pass, int32_t n_rows, int32_t n_t, const double* d_q, int64_t* d_count,
                                 uint64_t* d_prefix, int64_t* d_rank, int32_t* d_over, hipStream_t s)
{
    const int64_t threads = (int64_t)n_rows * n_t;
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(wselect_commit_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const long long*>(d_hist), pass, n_rows, n_t, d_q, d_count, d_prefix, d_rank, d_over);
    return hipGetLastError();
}

hipError_t launch_wselect_finish(const int64_t* d_count, const uint64_t* d_keys, int32_t n_rows, int32_t n_q, double* d_out, hipStream_t s)
{
    const int64_t threads = (int64_t)n_rows * (n_q + 1);
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(wselect_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, d_count, d_keys, n_rows, n_q, d_out);
    return hipGetLastError();
}

hipError_t launch_loglik_max(const double* d_ll, const uint8_t* d_status, int64_t N, unsigned long long* d_key, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const unsigned blocks = grid_of(N) < 1024u ? grid_of(N) : 1024u;
    hipLaunchKernelGGL(loglik_max_kernel, dim3(blocks), dim3(kWSelThreads), 0, s, d_ll, d_status, N, d_key);
    return hipGetLastError();
}

hipError_t launch_weights_from_loglik(const double* d_ll, const uint8_t* d_status, int64_t N, double ll_max, int32_t bits, int64_t* d_w,
                                      hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(weights_from_loglik_kernel, dim3(grid_of(N)), dim3(kWSelThreads), 0, s, d_ll, d_status, N, ll_max, bits, d_w);
    return hipGetLastError();
}

hipError_t launch_weights_check(const int64_t* d_w, int64_t N, int32_t* d_flag, unsigned long long* d_total, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const unsigned blocks = grid_of(N) < (unsigned)kCheckBlocks ? grid_of(N) : (unsigned)kCheckBlocks;
    hipLaunchKernelGGL(weights_check_kernel, dim3(blocks), dim3(kWSelThreads), 0, s, d_w, N, d_flag, d_total);
    return hipGetLastError();
}

}  // namespace rscm
