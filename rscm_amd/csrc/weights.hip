// The member weights of the weighted select (select.hip), for gfx950 (MI355X): the two kernels that turn a per-member
// log-likelihood into integer weights (the max over finite, ok members, and the quantisation
// w = llround(exp(min(ll - ll_max, 0)) * 2^bits)), and the check of a weight vector before a handle takes it: no negative weight,
// and a total of at most 2^53.  That bound on every handle is what keeps every histogram sum of the weighted select from
// wrapping: a bin of one handle holds at most 2^53, and a SUM over up to 2^10 handles (ranks) stays below 2^63, where the
// commit's check against 2^53 still sees it.
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"
#include "select_keys.hpp"

namespace rscm {

namespace {

constexpr int kWThreads = 256;

// *out_key = max(order_key(ll[i])) over members with status 0 and a finite ll; *out_key starts as order_key(-inf)
__global__ __launch_bounds__(kWThreads) void loglik_max_kernel(const double* __restrict__ ll, const uint8_t* __restrict__ status,
                                                                int64_t N, unsigned long long* __restrict__ out_key)
{
    unsigned long long m = order_key(-__builtin_inf());
    for (int64_t i = (int64_t)blockIdx.x * kWThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kWThreads) {
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

__global__ __launch_bounds__(kWThreads) void weights_from_loglik_kernel(const double* __restrict__ ll, const uint8_t* __restrict__ status,
                                                                         int64_t N, double ll_max, int32_t bits, int64_t* __restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * kWThreads + threadIdx.x;
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

__global__ __launch_bounds__(kWThreads) void weights_check_kernel(const int64_t* __restrict__ w, int64_t N, int32_t* __restrict__ flag,
                                                                   unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long part[kWThreads / 64];
    unsigned long long s = 0ull;
    bool neg = false;
    for (int64_t i = (int64_t)blockIdx.x * kWThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kWThreads) {
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
        for (int k = 0; k < kWThreads / 64; ++k) b = sat_add(b, part[k]);
        if (b) atomicAdd(total, b);
    }
}

unsigned grid_of(int64_t n) { return (unsigned)((n + kWThreads - 1) / kWThreads); }

}  // namespace

hipError_t launch_loglik_max(const double* d_ll, const uint8_t* d_status, int64_t N, unsigned long long* d_key, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const unsigned blocks = grid_of(N) < 1024u ? grid_of(N) : 1024u;
    hipLaunchKernelGGL(loglik_max_kernel, dim3(blocks), dim3(kWThreads), 0, s, d_ll, d_status, N, d_key);
    return hipGetLastError();
}

hipError_t launch_weights_from_loglik(const double* d_ll, const uint8_t* d_status, int64_t N, double ll_max, int32_t bits, int64_t* d_w,
                                      hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(weights_from_loglik_kernel, dim3(grid_of(N)), dim3(kWThreads), 0, s, d_ll, d_status, N, ll_max, bits, d_w);
    return hipGetLastError();
}

hipError_t launch_weights_check(const int64_t* d_w, int64_t N, int32_t* d_flag, unsigned long long* d_total, hipStream_t s)
{
    if (N <= 0) return hipSuccess;
    const unsigned blocks = grid_of(N) < (unsigned)kCheckBlocks ? grid_of(N) : (unsigned)kCheckBlocks;
    hipLaunchKernelGGL(weights_check_kernel, dim3(blocks), dim3(kWThreads), 0, s, d_w, N, d_flag, d_total);
    return hipGetLastError();
}

}  // namespace rscm
