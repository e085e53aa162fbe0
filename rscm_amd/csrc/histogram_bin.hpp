// The bin of a value among ascending edges (the definition is stated in include/rscm_gpu.h, rscm_ens_histogram_rows): what the
// histogram kernels (histogram.hip) apply to every member, and what a host program can check against a linear scan
// (tests/test_histogram_cpu.py compiles one).  Nothing here needs the device: plain comparisons of doubles.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSCM_HIST_HD __host__ __device__
#else
#define RSCM_HIST_HD
#endif

namespace rscm {

// the largest power of two that is at most n (n >= 1): the first stride of histogram_count_le's search
RSCM_HIST_HD inline int32_t histogram_top_stride(int32_t n)
{
    int32_t top = 1;
    while (top <= n / 2) top *= 2;
    return top;
}

// The number of edges with e[j] <= v, for e[0] < e[1] < ... < e[E-1] and a v that is not NaN; top = histogram_top_stride(E).
// "e[k-1] <= v" holds for every k up to that number and for none beyond, so the strides top, top / 2, ... 1 build the number bit by
// bit: floor(log2 E) + 1 reads of e, the same for every v (lanes of a wave stay together).  IEEE comparisons: -0 equals +0, and an
// infinite v compares like any other.
RSCM_HIST_HD inline int32_t histogram_count_le(const double* e, int32_t E, int32_t top, double v)
{
    int32_t k = 0;
    for (int32_t stride = top; stride > 0; stride >>= 1) {
        const int32_t to = k + stride;
        if (to <= E && e[to - 1] <= v) k = to;
    }
    return k;
}

// The slot of v among a histogram's B + 2 = E + 1 slots [counts[B], below, above]: bin k - 1 for k = histogram_count_le in [1, B];
// k == 0 is below (slot B); k == E is the last bin when v sits on the last edge, else above (slot B + 1).
RSCM_HIST_HD inline int32_t histogram_slot(const double* e, int32_t E, int32_t top, double v)
{
    const int32_t B = E - 1, k = histogram_count_le(e, E, top, v);
    if (k == 0) return B;
    if (k <= B) return k - 1;
    return v == e[B] ? B - 1 : B + 1;
}

}  // namespace rscm
