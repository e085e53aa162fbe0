// The order-preserving 64-bit image of a double shared by the radix select (select.hip) and the log-likelihood maximum
// (weights.hip, select_host.cpp): -0.0 orders before +0.0 and NaNs of either sign fall outside the order (callers leave them out).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rscm {

// The device keeps HIP's bit casts: the same casts with __builtin_bit_cast inline earlier and change the kernels' code.
__host__ __device__ __forceinline__ uint64_t order_key(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    const uint64_t u = (uint64_t)__double_as_longlong(x);
#else
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
#endif
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__host__ __device__ __forceinline__ double key_value(uint64_t k)
{
    const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
#ifdef __HIP_DEVICE_COMPILE__
    return __longlong_as_double((long long)u);
#else
    return __builtin_bit_cast(double, u);
#endif
}

}  // namespace rscm
