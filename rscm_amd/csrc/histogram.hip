// Histograms of STORED ROWS and of member vectors across the members of an ensemble, for gfx950 (MI355X): the integer sums behind
// rscm_ens_histogram_rows, rscm_ens_histogram_vectors and rscm_ens_histogram2d (the definition is stated in include/rscm_gpu.h, the
// bin of a value in histogram_bin.hpp).  Per row and member group: the summed weight of the members in each of B = E - 1 bins between
// ascending edges, below the first edge and above the last; for two vectors, in each of Bx x By cells and outside them.
//
// One launch for all rows.  Grid: x over member stretches (grid-stride, capped at kHistBlocks blocks of four waves, so that a
// destination collects at most that many adders), y over rows (a block works on one row at a time and strides over rows beyond
// 65535).  A thread walks its members with the grid's stride, kHistBatch loads in flight, lanes of a wave on consecutive members
// (every load coalesced).  The weights, the groups and the baseline are read again for every row, as exceedance_rows.hip reads them.
//
// LDS, sized to the call (dynamic): the row's edges, then the block's slots [G][B + 2] (counts, below, above; two dimensions:
// [G][Bx By + 1]) as uint64.  A member's bin is found by histogram_slot's search over the edges in LDS: floor(log2 E) + 1 reads, the
// same number for every lane.  Every add is a 64-bit integer add: ds_add_u64 into the slots, and at the end of the row one global
// atomic per non-zero slot and block into the zeroed accumulator.  Exact, and the order does not matter.
//
// Contention.  A plume puts most members of a wave into the same few bins, and lanes that add to one LDS address take turns.  Two
// measures, both on (DESIGN 8aa has the figures):
//   * each wave adds to slots of its own while four copies and the edges stay within kHistFullOccupancyLds, the LDS at which eight
//     blocks still share a CU; the copies are summed at the end of the row;
//   * before a wave adds, it merges crowded slots: it takes the slot of its first unserved lane and ballots the lanes that hold the
//     same slot; when there are at least kHistMergeMin of them (kHistMergeMinWeighted with weights), one lane adds their sum -- a
//     popcount without weights, a wave ladder with them -- and the wave looks at the next unserved lane.  The first slot that is not
//     crowded ends the merging, and the lanes left over add for themselves.  Members spread over many bins pay one ballot; members
//     in one bin pay one add per wave instead of 64 turns.  A few lanes on one address are cheaper served by the LDS than merged.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "histogram_bin.hpp"
#include "rscm_device.hpp"

namespace rscm {
namespace {

constexpr int kHistThreads = 256;
constexpr int kHistWaves = kHistThreads / 64;
constexpr int kHistBatch = 4;                       // members whose loads a thread issues before it uses them
constexpr int kHistMergeMin = 16;                   // lanes on one slot from which one merged add (a popcount) replaces their turns
constexpr int kHistMergeMinWeighted = 32;           // the same where the merged add costs a wave ladder of 64-bit sums (measured: DESIGN 8aa)
constexpr size_t kHistFullOccupancyLds = 20480;     // 160 KiB of a CU over the eight blocks that fill its 32 waves
constexpr size_t kHistDefaultLdsLimit = 65536;      // dynamic LDS beyond this needs the function attribute
static_assert(kHistBlocks * kHistThreads == kHistogramMembersPerPass, "rscm_device.hpp states the members of one pass of the grid");

extern __shared__ unsigned long long hist_lds[];    // the edges (as doubles), then copies x slots

__device__ __forceinline__ unsigned long long hist_wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the wave's adds of weight w to hist[slot] for the lanes with `take`; every lane of the wave calls it
template <bool kW, class Sum>
__device__ __forceinline__ void hist_add(unsigned long long* hist, int32_t slot, bool take, Sum w)
{
    constexpr int kMin = kW ? kHistMergeMinWeighted : kHistMergeMin;
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long rem = __ballot(take);
#pragma unroll
    for (int p = 0; p < 64 / kMin; ++p) {                 // (no more slots than that can hold kMin lanes each)
        if (__popcll(rem) < kMin) break;
        const int lead = __ffsll(rem) - 1;
        const int32_t s0 = __shfl(slot, lead, 64);
        const bool match = take && slot == s0;
        const unsigned long long same = __ballot(match);
        const int n = __popcll(same);
        if (n < kMin) break;                              // the first lane's slot is not crowded: take the wave for spread out
        rem &= ~same;
        const unsigned long long sum = kW ? hist_wave_sum(match ? (unsigned long long)w : 0ull) : (unsigned long long)n;
        if (lane == lead && sum) atomicAdd(&hist[s0], sum);
        take = take && !match;
    }
    if (take) atomicAdd(&hist[slot], (unsigned long long)w);
}

__device__ __forceinline__ void hist_zero(unsigned long long* bins, int32_t n)
{
    for (int32_t i = (int32_t)threadIdx.x; i < n; i += kHistThreads) bins[i] = 0ull;
}

// the block's slots, summed over the waves' copies, into the accumulator record o[slots]
__device__ __forceinline__ void hist_flush(const unsigned long long* bins, int32_t slots, int32_t copies, unsigned long long* __restrict__ o)
{
    for (int32_t i = (int32_t)threadIdx.x; i < slots; i += kHistThreads) {
        unsigned long long v = 0ull;
        for (int32_t c = 0; c < copies; ++c) v += bins[c * slots + i];
        if (v) atomicAdd(&o[i], v);
    }
}

template <bool kW, bool kG>
__global__ __launch_bounds__(kHistThreads) void histogram_kernel(HistogramArgs a, int32_t copies)
{
    using Sum = std::conditional_t<kW, unsigned long long, unsigned int>;
    const int32_t E = a.n_edges, S = E + 1, G = kG ? a.n_groups : 1, slots = G * S;
    const int32_t top = histogram_top_stride(E);
    double* edges = reinterpret_cast<double*>(hist_lds);
    unsigned long long* bins = hist_lds + E;
    unsigned long long* mine = bins + (copies > 1 ? (int32_t)(threadIdx.x >> 6) * slots : 0);
    const int64_t step = (int64_t)gridDim.x * kHistThreads;
    const int64_t first = (int64_t)blockIdx.x * kHistThreads + threadIdx.x;
    const int64_t lane = (int64_t)(threadIdx.x & 63u);
    const double qnan = __builtin_nan("");

    for (int32_t row = (int32_t)blockIdx.y; row < a.n_rows; row += (int32_t)gridDim.y) {
        hist_zero(bins, copies * slots);
        if (row == (int32_t)blockIdx.y || a.edge_stride) {
            const double* __restrict__ e_row = a.edges + (int64_t)row * a.edge_stride;
            for (int32_t i = (int32_t)threadIdx.x; i < E; i += kHistThreads) edges[i] = e_row[i];
        }
        __syncthreads();
        const double* __restrict__ x_row = a.rows[row];

        for (int64_t i0 = first; i0 - lane < a.N; i0 += kHistBatch * step) {   // by the wave's first member: its lanes stay together
            double x[kHistBatch];
            Sum wt[kHistBatch];
            int32_t g[kHistBatch];
#pragma unroll
            for (int j = 0; j < kHistBatch; ++j) {
                const int64_t i = i0 + j * step;
                const bool in = i < a.N;
                x[j] = in ? x_row[i] : qnan;
                if (a.base) x[j] = x[j] - (in ? a.base[i] : 0.0);   // one rounded subtraction: the bits the anomaly select sees
                wt[j] = kW ? (in ? (Sum)a.w[i] : (Sum)0) : (Sum)1;
                g[j] = kG ? (in ? a.group[i] : -1) : 0;
            }
#pragma unroll
            for (int j = 0; j < kHistBatch; ++j) {
                const double v = x[j];
                const bool take = v == v && (uint32_t)g[j] < (uint32_t)G;   // NaN (a member beyond N reads as one), or in no group: no part
                const int32_t slot = (take ? g[j] * S : 0) + histogram_slot(edges, E, top, v);
                hist_add<kW>(mine, slot, take, wt[j]);
            }
        }
        __syncthreads();
        hist_flush(bins, slots, copies, a.acc + (int64_t)row * slots);
        __syncthreads();
    }
}

template <bool kW, bool kG>
__global__ __launch_bounds__(kHistThreads) void histogram2d_kernel(Histogram2dArgs a, int32_t copies)
{
    using Sum = std::conditional_t<kW, unsigned long long, unsigned int>;
    const int32_t Ex = a.n_edges_x, Ey = a.n_edges_y, Bx = Ex - 1, By = Ey - 1, S = Bx * By + 1, G = kG ? a.n_groups : 1, slots = G * S;
    const int32_t top_x = histogram_top_stride(Ex), top_y = histogram_top_stride(Ey);
    double* edges_x = reinterpret_cast<double*>(hist_lds);
    double* edges_y = edges_x + Ex;
    unsigned long long* bins = hist_lds + Ex + Ey;
    unsigned long long* mine = bins + (copies > 1 ? (int32_t)(threadIdx.x >> 6) * slots : 0);
    const int64_t step = (int64_t)gridDim.x * kHistThreads;
    const int64_t first = (int64_t)blockIdx.x * kHistThreads + threadIdx.x;
    const int64_t lane = (int64_t)(threadIdx.x & 63u);
    const double qnan = __builtin_nan("");

    hist_zero(bins, copies * slots);
    for (int32_t i = (int32_t)threadIdx.x; i < Ex + Ey; i += kHistThreads) edges_x[i] = a.edges[i];
    __syncthreads();

    for (int64_t i0 = first; i0 - lane < a.N; i0 += kHistBatch * step) {   // by the wave's first member: its lanes stay together
        double x[kHistBatch], y[kHistBatch];
        Sum wt[kHistBatch];
        int32_t g[kHistBatch];
#pragma unroll
        for (int j = 0; j < kHistBatch; ++j) {
            const int64_t i = i0 + j * step;
            const bool in = i < a.N;
            x[j] = in ? a.x[i] : qnan;
            y[j] = in ? a.y[i] : qnan;
            wt[j] = kW ? (in ? (Sum)a.w[i] : (Sum)0) : (Sum)1;
            g[j] = kG ? (in ? a.group[i] : -1) : 0;
        }
#pragma unroll
        for (int j = 0; j < kHistBatch; ++j) {
            const bool take = x[j] == x[j] && y[j] == y[j] && (uint32_t)g[j] < (uint32_t)G;
            const int32_t sx = histogram_slot(edges_x, Ex, top_x, x[j]), sy = histogram_slot(edges_y, Ey, top_y, y[j]);
            const int32_t cell = sx < Bx && sy < By ? sx * By + sy : Bx * By;   // below or above in either direction: outside
            hist_add<kW>(mine, (take ? g[j] * S : 0) + cell, take, wt[j]);
        }
    }
    __syncthreads();
    hist_flush(bins, slots, copies, a.acc);
}

// the waves' own copies of the slots while they and the edges leave the CU its eight blocks
int32_t hist_copies(size_t edge_doubles, size_t slots)
{
    return (edge_doubles + kHistWaves * slots) * sizeof(unsigned long long) <= kHistFullOccupancyLds ? kHistWaves : 1;
}

template <class Kernel, class Args>
hipError_t hist_launch(Kernel kernel, const Args& a, size_t edge_doubles, size_t slots, dim3 grid, hipStream_t s)
{
    const int32_t copies = hist_copies(edge_doubles, slots);
    const size_t lds = (edge_doubles + (size_t)copies * slots) * sizeof(unsigned long long);
    if (lds > kHistDefaultLdsLimit)
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(kHistThreads), lds, s, a, copies);
    return hipGetLastError();
}

unsigned hist_grid_x(int64_t N)
{
    const int64_t need = (N + kHistThreads - 1) / kHistThreads;
    return (unsigned)(need < kHistBlocks ? need : kHistBlocks);
}

bool hist_edges_ok(int32_t E) { return E >= 2 && E <= kHistogramMaxEdges; }

}  // namespace

hipError_t launch_histogram(const HistogramArgs& a, hipStream_t s)
{
    if (a.N <= 0 || a.n_rows <= 0) return hipSuccess;
    const int32_t G = a.group ? a.n_groups : 1;
    if (!hist_edges_ok(a.n_edges) || G < 1 || G > kMaxMemberGroups || (int64_t)G * (a.n_edges + 1) > kHistogramMaxSlots ||
        (a.edge_stride != 0 && a.edge_stride != a.n_edges))
        return hipErrorInvalidValue;
    const size_t slots = (size_t)G * (a.n_edges + 1);
    const dim3 grid(hist_grid_x(a.N), (unsigned)(a.n_rows < 65535 ? a.n_rows : 65535));
    if (a.w && a.group) return hist_launch(histogram_kernel<true, true>, a, (size_t)a.n_edges, slots, grid, s);
    if (a.w) return hist_launch(histogram_kernel<true, false>, a, (size_t)a.n_edges, slots, grid, s);
    if (a.group) return hist_launch(histogram_kernel<false, true>, a, (size_t)a.n_edges, slots, grid, s);
    return hist_launch(histogram_kernel<false, false>, a, (size_t)a.n_edges, slots, grid, s);
}

hipError_t launch_histogram2d(const Histogram2dArgs& a, hipStream_t s)
{
    if (a.N <= 0) return hipSuccess;
    const int32_t G = a.group ? a.n_groups : 1;
    if (!hist_edges_ok(a.n_edges_x) || !hist_edges_ok(a.n_edges_y) || G < 1 || G > kMaxMemberGroups ||
        (int64_t)G * ((int64_t)(a.n_edges_x - 1) * (a.n_edges_y - 1) + 1) > kHistogramMaxSlots)
        return hipErrorInvalidValue;
    const size_t slots = (size_t)G * ((size_t)(a.n_edges_x - 1) * (a.n_edges_y - 1) + 1), edge_doubles = (size_t)a.n_edges_x + a.n_edges_y;
    const dim3 grid(hist_grid_x(a.N), 1u);
    if (a.w && a.group) return hist_launch(histogram2d_kernel<true, true>, a, edge_doubles, slots, grid, s);
    if (a.w) return hist_launch(histogram2d_kernel<true, false>, a, edge_doubles, slots, grid, s);
    if (a.group) return hist_launch(histogram2d_kernel<false, true>, a, edge_doubles, slots, grid, s);
    return hist_launch(histogram2d_kernel<false, false>, a, edge_doubles, slots, grid, s);
}

}  // namespace rscm
