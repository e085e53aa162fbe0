// Posterior resampling on the device, for gfx950 (MI355X): exact statistics of the integer member weights, systematic
// resampling in integer form (an inclusive running sum of the weights and one binary search per draw), and the gather that
// copies drawn members' rows from one handle to another.  Everything that decides WHO is drawn is 64-bit integer arithmetic,
// so a draw is the same bits on one handle, on any split of it into handles and at any number of ranks.
//
// No workgroup waits on another anywhere in this file: the scan is the three-launch form (scan every tile and keep its total,
// scan the totals, add them back), recursive over the totals, and the statistics go through per-block partials that a second
// launch reduces.  Inside a block the scans are __shfl_up ladders over the 64 lanes of a wavefront and a four-entry LDS hop
// between the block's four wavefronts.
#include <hip/hip_runtime.h>

#include "rscm_device.hpp"

namespace rscm {

namespace {

constexpr int kRThreads = 256;
constexpr int kRWaves = kRThreads / 64;
constexpr int kScanItems = 4;
constexpr int kScanTile = kRThreads * kScanItems;   // weights per block of the scan
constexpr int kStatBlocks = 1024;

// ---- weight statistics ----------------------------------------------------------------------------------------------
// One partial per block: {sum w, count w != 0, max w, sum w^2 low word, sum w^2 high word}.  w <= 2^53 (the bound of
// rscm_ens_set_member_weights), so w^2 < 2^106 is formed as (__umul64hi, low product) and added with the carry.
struct U128 { unsigned long long lo, hi; };

__device__ __forceinline__ void add128(U128& a, unsigned long long lo, unsigned long long hi)
{
    const unsigned long long s = a.lo + lo;
    a.hi += hi + (s < a.lo ? 1ull : 0ull);
    a.lo = s;
}

struct WStat {
    unsigned long long total, nonzero, wmax;
    U128 sq;
};

__device__ __forceinline__ void wstat_merge(WStat& a, unsigned long long total, unsigned long long nonzero, unsigned long long wmax,
                                            unsigned long long lo, unsigned long long hi)
{
    a.total += total;
    a.nonzero += nonzero;
    a.wmax = wmax > a.wmax ? wmax : a.wmax;
    add128(a.sq, lo, hi);
}

// the block's merged statistics, valid in thread 0
__device__ __forceinline__ WStat wstat_block_reduce(WStat v)
{
    __shared__ unsigned long long part[kRWaves][5];
    for (int off = 32; off > 0; off >>= 1)
        wstat_merge(v, __shfl_xor(v.total, off, 64), __shfl_xor(v.nonzero, off, 64), __shfl_xor(v.wmax, off, 64),
                    __shfl_xor(v.sq.lo, off, 64), __shfl_xor(v.sq.hi, off, 64));
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* p = part[threadIdx.x / 64];
        p[0] = v.total; p[1] = v.nonzero; p[2] = v.wmax; p[3] = v.sq.lo; p[4] = v.sq.hi;
    }
    __syncthreads();
    WStat b{0ull, 0ull, 0ull, {0ull, 0ull}};
    if (threadIdx.x == 0)
        for (int k = 0; k < kRWaves; ++k) wstat_merge(b, part[k][0], part[k][1], part[k][2], part[k][3], part[k][4]);
    return b;
}

__global__ __launch_bounds__(kRThreads) void weights_stats_kernel(const int64_t* __restrict__ w, int64_t N,
                                                                   unsigned long long* __restrict__ partial)
{
    WStat v{0ull, 0ull, 0ull, {0ull, 0ull}};
    for (int64_t i = (int64_t)blockIdx.x * kRThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kRThreads) {
        const unsigned long long x = (unsigned long long)w[i];
        wstat_merge(v, x, x != 0ull ? 1ull : 0ull, x, x * x, __umul64hi(x, x));
    }
    const WStat b = wstat_block_reduce(v);
    if (threadIdx.x == 0) {
        unsigned long long* p = partial + (size_t)blockIdx.x * 5;
        p[0] = b.total; p[1] = b.nonzero; p[2] = b.wmax; p[3] = b.sq.lo; p[4] = b.sq.hi;
    }
}

// one block: out[5] = the partials merged
__global__ __launch_bounds__(kRThreads) void weights_stats_final_kernel(const unsigned long long* __restrict__ partial, int32_t n_partial,
                                                                         unsigned long long* __restrict__ out)
{
    WStat v{0ull, 0ull, 0ull, {0ull, 0ull}};
    for (int32_t k = threadIdx.x; k < n_partial; k += kRThreads) {
        const unsigned long long* p = partial + (size_t)k * 5;
        wstat_merge(v, p[0], p[1], p[2], p[3], p[4]);
    }
    const WStat b = wstat_block_reduce(v);
    if (threadIdx.x == 0) {
        out[0] = b.total; out[1] = b.nonzero; out[2] = b.wmax; out[3] = b.sq.lo; out[4] = b.sq.hi;
    }
}

// ---- inclusive scan -------------------------------------------------------------------------------------------------
// out[i] = in[base] + ... + in[i] within the block's tile of kScanTile values, sums[block] = the tile's total.  in == out is
// allowed: a thread has read its four values before it writes them and no thread reads another's.
__global__ __launch_bounds__(kRThreads) void scan_tile_kernel(const int64_t* in, int64_t* out, int64_t n, int64_t* __restrict__ sums)
{
    __shared__ int64_t wave_total[kRWaves];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int64_t x[kScanItems];
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) x[j] = base + j < n ? in[base + j] : 0;
#pragma unroll
    for (int j = 1; j < kScanItems; ++j) x[j] += x[j - 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t incl = x[kScanItems - 1];
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int64_t before = incl - x[kScanItems - 1];   // what the lanes below hold
    for (int k = 0; k < wave; ++k) before += wave_total[k];
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (base + j < n) out[base + j] = x[j] + before;
    if (threadIdx.x == kRThreads - 1) sums[blockIdx.x] = before + x[kScanItems - 1];
}

// tile b > 0 of out takes the running total of the tiles before it
__global__ __launch_bounds__(kRThreads) void scan_add_kernel(int64_t* __restrict__ out, int64_t n, const int64_t* __restrict__ scanned_sums)
{
    const int64_t tile = (int64_t)blockIdx.x + 1;
    const int64_t add = scanned_sums[tile - 1];
    const int64_t base = tile * kScanTile + (int64_t)threadIdx.x * kScanItems;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (base + j < n) out[base + j] += add;
}

// ---- ancestors ------------------------------------------------------------------------------------------------------
// Draw k sits at t_k = k q + floor((s + k r) / M), W = q M + r: with r < M <= 2^31, k < M and s < W < 2^63 the sum s + k r stays
// below 2^64 and k q <= W, so nothing leaves 64 bits and no 128-bit division is needed.  Its ancestor is the first member whose
// inclusive running sum C exceeds t_k - w_before (a zero-weight member repeats the sum before it and is never first).
__global__ __launch_bounds__(kRThreads) void ancestors_kernel(const int64_t* __restrict__ C, int64_t N, int64_t k_first, int64_t count,
                                                               unsigned long long M, unsigned long long q, unsigned long long r,
                                                               unsigned long long s, unsigned long long w_before, int64_t* __restrict__ anc)
{
    const int64_t j = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (j >= count) return;
    const unsigned long long k = (unsigned long long)(k_first + j);
    const int64_t t = (int64_t)(k * q + (s + k * r) / M - w_before);
    int64_t lo = 0, hi = N - 1;   // C[N - 1] = W_local > t: the answer exists
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (C[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    anc[j] = lo;
}

// ---- gather of members between handles ------------------------------------------------------------------------------
__global__ __launch_bounds__(kRThreads) void ancestors_check_kernel(const int64_t* __restrict__ anc, int64_t count, int64_t n_src,
                                                                     int32_t* __restrict__ flag)
{
    const int64_t j = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (j >= count) return;
    const int64_t a = anc[j];
    if (a < 0 || a >= n_src) *flag = 1;
}

// grid.x: blocks of destination members, grid.y: strides over the rows of all pieces
__global__ __launch_bounds__(kRThreads) void gather_members_kernel(GatherBatch batch, int32_t n_pieces, int32_t total_rows,
                                                                    const int64_t* __restrict__ anc, int64_t count, int64_t n_src)
{
    const int64_t j = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (j >= count) return;
    const int64_t a = anc[j];
    if (a < 0 || a >= n_src) return;   // refused by the check before this launch; never read out of bounds
    for (int32_t row = blockIdx.y; row < total_rows; row += gridDim.y) {
        int32_t p = 0, first = 0;
        while (p + 1 < n_pieces && row >= first + batch.pieces[p].rows) first += batch.pieces[p++].rows;
        const GatherPiece& g = batch.pieces[p];
        const int64_t r = row - first;
        if (g.elem_bytes == 8)
            reinterpret_cast<double*>(g.dst)[r * g.dst_stride + j] = reinterpret_cast<const double*>(g.src)[r * g.src_stride + a];
        else
            reinterpret_cast<uint8_t*>(g.dst)[r * g.dst_stride + j] = reinterpret_cast<const uint8_t*>(g.src)[r * g.src_stride + a];
    }
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + kRThreads - 1) / kRThreads); }

}  // namespace

int32_t weights_stats_partials(int64_t N)
{
    const unsigned b = blocks_of(N);
    return (int32_t)(b < (unsigned)kStatBlocks ? b : (unsigned)kStatBlocks);
}

hipError_t launch_weights_stats(const int64_t* d_w, int64_t N, unsigned long long* d_partial, unsigned long long* d_out, hipStream_t s)
{
    const int32_t blocks = weights_stats_partials(N);
    hipLaunchKernelGGL(weights_stats_kernel, dim3(blocks), dim3(kRThreads), 0, s, d_w, N, d_partial);
    hipLaunchKernelGGL(weights_stats_final_kernel, dim3(1), dim3(kRThreads), 0, s, d_partial, blocks, d_out);
    return hipGetLastError();
}

int64_t scan_scratch_elems(int64_t n)
{
    int64_t total = 0;
    while (n > 1) {
        n = (n + kScanTile - 1) / kScanTile;
        total += n;
    }
    return total > 0 ? total : 1;
}

hipError_t launch_inclusive_scan(const int64_t* d_in, int64_t* d_out, int64_t n, int64_t* d_scratch, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int64_t tiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(scan_tile_kernel, dim3((unsigned)tiles), dim3(kRThreads), 0, s, d_in, d_out, n, d_scratch);
    if (tiles > 1) {
        const hipError_t e = launch_inclusive_scan(d_scratch, d_scratch, tiles, d_scratch + tiles, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)(tiles - 1)), dim3(kRThreads), 0, s, d_out, n, d_scratch);
    }
    return hipGetLastError();
}

hipError_t launch_ancestors(const int64_t* d_cum, int64_t N, int64_t k_first, int64_t count, uint64_t M, uint64_t q, uint64_t r, uint64_t s0,
                            uint64_t w_before, int64_t* d_anc, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ancestors_kernel, dim3(blocks_of(count)), dim3(kRThreads), 0, s, d_cum, N, k_first, count, (unsigned long long)M,
                       (unsigned long long)q, (unsigned long long)r, (unsigned long long)s0, (unsigned long long)w_before, d_anc);
    return hipGetLastError();
}

hipError_t launch_ancestors_check(const int64_t* d_anc, int64_t count, int64_t n_src, int32_t* d_flag, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ancestors_check_kernel, dim3(blocks_of(count)), dim3(kRThreads), 0, s, d_anc, count, n_src, d_flag);
    return hipGetLastError();
}

hipError_t launch_gather_members(const GatherBatch& batch, int32_t n_pieces, const int64_t* d_anc, int64_t count, int64_t n_src, hipStream_t s)
{
    if (count <= 0 || n_pieces <= 0) return hipSuccess;
    int32_t total_rows = 0;
    for (int32_t p = 0; p < n_pieces; ++p) total_rows += batch.pieces[p].rows;
    if (total_rows <= 0) return hipSuccess;
    const unsigned gy = (unsigned)(total_rows < 128 ? total_rows : 128);
    hipLaunchKernelGGL(gather_members_kernel, dim3(blocks_of(count), gy), dim3(kRThreads), 0, s, batch, n_pieces, total_rows, d_anc, count,
                       n_src);
    return hipGetLastError();
}

}  // namespace rscm
