// The order-preserving 64-bit image of a double shared by the radix selects (select.hip, wselect.hip): -0.0 orders before
// +0.0 and NaNs of either sign fall outside the order (callers leave them out).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rscm {

__device__ __forceinline__ uint64_t order_key(double x)
{
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double key_value(uint64_t k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

}  // namespace rscm
