// The wave-level pieces the two moment kernels share (moments.hip, moment_rows.hip): the integer sum over the 64 lanes, and the
// read that makes one lane's term wave-uniform for the serial walk.  Device only; the pure integer pieces of a term -- its fields,
// product and digits -- are in moment_window.hpp, which a host compiler builds alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rscm {

__device__ __forceinline__ unsigned long long mom_wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ uint32_t mom_readlane(uint32_t v, int j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, j); }

// A lane's term as the serial walk reads it: the product (hi : lo) in 32-bit halves, and an info word -- the bit position in bits
// 0 .. 11, the sign in bit 12, whatever else the kernel keeps above.  Formed once per tile, ahead of the walk.
struct MomLaneTerm { uint32_t lo0, lo1, hi0, hi1, info; };

__device__ __forceinline__ MomLaneTerm mom_lane_term(uint64_t lo, uint64_t hi, uint32_t info)
{
    return {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), info};
}

// Lane j's term in scalar registers (j wave-uniform): the info word by one v_readlane, the product (phi : plo) by four.  Two reads,
// so that a walk which decides on the info word alone (a non-finite term, a change of group) does so ahead of the other four
__device__ __forceinline__ uint32_t mom_uniform_info(const MomLaneTerm& t, int j) { return mom_readlane(t.info, j); }

__device__ __forceinline__ void mom_uniform_product(const MomLaneTerm& t, int j, uint64_t& plo, uint64_t& phi)
{
    plo = (uint64_t)mom_readlane(t.lo0, j) | ((uint64_t)mom_readlane(t.lo1, j) << 32);
    phi = (uint64_t)mom_readlane(t.hi0, j) | ((uint64_t)mom_readlane(t.hi1, j) << 32);
}

}  // namespace rscm
