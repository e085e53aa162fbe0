// Running means of a variable's rows over the time axis, per member, for gfx950 (MI355X).
//
// running_mean_kernel<kSlots>: one thread per member (x, 256 threads as diagnostic.hip) and one tile of `tile` output rows per block
// (y).  The definition is the one include/rscm_gpu.h states under "running means": with W = window and the source rows x_0 .. x_{W-1}
// of an output in time order,
//   s = x_0;  s = s + x_j  for j = 1 .. W - 1 in that order;  y = s / (double)W
// Every add and the division is one f64 operation rounded on its own (no FMA to contract, no reciprocal, no tree), and an output is
// formed from its own W terms and nothing else: there is no sliding update, so a non-finite source value reaches the outputs whose
// window holds it and no other.
//
// Source row q of a tile (output r of the launch reads the rows r * m .. r * m + W - 1 of d_rows, m = t_stride / step) is loaded from
// global memory once, 8 B per lane and consecutive members per wave, and parked in slot q mod kSlots of an LDS ring
// ring[kSlots][256]: a lane reads and writes its own column only, so there is no barrier in the kernel, and the 64 lanes of a
// ds_read_b64 / ds_write_b64 hit 64 consecutive doubles -- conflict-free.  The W terms of a sum come from the ring.  Outputs are
// formed in groups of `group`: the rows the group adds to the ring (group * m of them where windows overlap, W where m >= W and
// group is 1) are loaded kRunMeanBatch at a time into registers, all of a batch's loads issued before the first is parked, then the
// group's sums are formed.  m >= W, disjoint period means, is the same code: the rows between two windows are never loaded.
//
// Where windows overlap most -- m = 1, W >= kRunMeanBatch, a full group -- the group's kRunMeanBatch sums are formed together
// (shared_sums): row r of the group is a term of every output whose window holds it, so it is read from the ring once and added to
// each of those sums, which are independent dependency chains.  One eighth of the LDS reads, and eight adds in flight where one
// output at a time leaves a lone chain of W dependent adds behind each read (measured: profiles/running_mean_bench.txt).  Every sum
// still adds its own W terms in time order.  Any other shape (m > 1, W < kRunMeanBatch, a tile's short last group) forms one output
// at a time from the ring, kRunMeanReads slots read ahead of their adds.
//
// The ring.  It must hold W + (group - 1) * m rows, and LDS is what bounds the occupancy: 2 KiB per slot and block, 160 KiB per CU,
// so the blocks per CU are 160 / (2 kSlots).  kSlots is therefore the largest ring at each block count -- 16, 20, 26, 40 slots for 5,
// 4, 3, 2 blocks per CU -- and 72 (144 KiB, one block) beyond; running_mean_shape takes the smallest that holds W + kRunMeanSpare rows
// (W where m >= W) and lets the group fill what is left, at most kRunMeanBatch outputs.  kRunMeanSpare is kRunMeanBatch - 1, so that
// at m = 1 a group is full.  W = 20 at m = 1: 40 slots, two blocks (8 waves) per CU.  W = 64: a ring of exactly 64 slots would not
// buy a second block either (128 KiB) and would leave each output's one new row as a lone load; with 72 slots 8 rows are in flight
// per wave where only four waves share a CU.  Narrower blocks do not help: the ring costs 512 B per slot and wave whatever the
// block's shape.
//
// The tile (running_mean_tile).  A tile of L outputs reads L * m + W - m source rows where m < W: overlap (L m + W - m) / (L m).  The
// host takes L = n_rows / (kRunMeanMinBlocks / blocks in x), so that 1e5 members still give the 256 CUs some thousand blocks, but
// no shorter than kRunMeanMaxOverlap * (W - m) / m (overlap at most 1.25), and rounds it up to a multiple of kRunMeanBatch.  At 1e6
// members (3907 blocks in x) a centred 20-term mean over 171 rows is one tile, overlap 1.11; at 1e5 x 751 it is 6 tiles of 128, 1.15.
//
// No scratch (make check-running-mean-scratch).  Traffic: 8 N bytes per source row and tile, 8 N per output.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "running_mean.hpp"

namespace rscm {

namespace {

// s + p[0] + p[kRunMeanThreads] + ... (n terms of one lane's column, consecutive slots), added in that order; the reads of kRunMeanReads
// slots are issued before the first is added
__device__ __forceinline__ double add_slots(double s, const double* p, int32_t n)
{
    int32_t t = 0;
    for (; t + kRunMeanReads <= n; t += kRunMeanReads) {
        double y[kRunMeanReads];
#pragma unroll
        for (int u = 0; u < kRunMeanReads; ++u) y[u] = p[(t + u) * kRunMeanThreads];
#pragma unroll
        for (int u = 0; u < kRunMeanReads; ++u) s = s + y[u];
    }
    for (; t < n; ++t) s = s + p[t * kRunMeanThreads];
    return s;
}

// The sums of kRunMeanBatch consecutive outputs at m = 1, W >= kRunMeanBatch: row r of the group (slot first + r of the ring) is term
// r - j of output j, so each slot is read once for all of them and the sums are kRunMeanBatch independent chains -- each still its own
// W terms in time order.  Rows 0 .. B - 1 open the sums one after the other, rows B .. W - 1 continue all, rows W .. W + B - 2 the later ones.
template <int kSlots>
__device__ __forceinline__ void shared_sums(const double* col, int32_t first, int32_t W, double (&s)[kRunMeanBatch])
{
    int32_t slot = first;
    auto next = [&]() {
        const double x = col[slot * kRunMeanThreads];
        slot = slot + 1 == kSlots ? 0 : slot + 1;
        return x;
    };
#pragma unroll
    for (int r = 0; r < kRunMeanBatch; ++r) {
        const double x = next();
#pragma unroll
        for (int j = 0; j < r; ++j) s[j] = s[j] + x;
        s[r] = x;
    }
    int32_t r = kRunMeanBatch;
    for (; r + 4 <= W; r += 4) {   // four slots read before the first is added
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = next();
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < kRunMeanBatch; ++j) s[j] = s[j] + x[u];
    }
    for (; r < W; ++r) {
        const double x = next();
#pragma unroll
        for (int j = 0; j < kRunMeanBatch; ++j) s[j] = s[j] + x;
    }
#pragma unroll
    for (int u = 0; u < kRunMeanBatch - 1; ++u) {   // row W + u: past the sums 0 .. u
        const double x = next();
#pragma unroll
        for (int j = u + 1; j < kRunMeanBatch; ++j) s[j] = s[j] + x;
    }
}

template <int kSlots>
__global__ __launch_bounds__(kRunMeanThreads) void running_mean_kernel(RunningMeanArgs a)
{
    __shared__ double ring[kSlots][kRunMeanThreads];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kRunMeanThreads + lane;
    if (i >= a.N) return;   // (no barrier below)
    const int32_t r0 = (int32_t)blockIdx.y * a.tile;
    const int32_t n_out = min(a.tile, a.n_rows - r0);
    const int32_t W = a.window, m = a.m;
    const double w = (double)W;
    const double* const* __restrict__ rows = a.d_rows + (int64_t)r0 * m;   // the tile's row q is rows[q]
    double* __restrict__ out = a.d_out + (int64_t)r0 * a.N + i;
    double* col = &ring[0][lane];   // slot s of this lane: col[s * kRunMeanThreads]

    int32_t parked = 0;   // the tile's rows [.., parked) have been through the ring
    for (int32_t k = 0; k < n_out; k += a.group) {
        const int32_t g = min(a.group, n_out - k);
        const int32_t need = (k + g - 1) * m + W;   // at most kSlots rows from the group's first, k * m, on (running_mean_shape)
        // the rows [q, need) in batches; a short last batch repeats row need - 1 (the same value into the same slot) and keeps its shape
        for (int32_t q = max(parked, k * m); q < need; q += kRunMeanBatch) {
            double x[kRunMeanBatch];
#pragma unroll
            for (int j = 0; j < kRunMeanBatch; ++j) x[j] = rows[min(q + j, need - 1)][i];
#pragma unroll
            for (int j = 0; j < kRunMeanBatch; ++j) col[((uint32_t)min(q + j, need - 1) % kSlots) * kRunMeanThreads] = x[j];
        }
        parked = need;
        if (m == 1 && g == kRunMeanBatch && W >= kRunMeanBatch) {
            double s[kRunMeanBatch];
            shared_sums<kSlots>(col, (int32_t)((uint32_t)k % kSlots), W, s);
#pragma unroll
            for (int j = 0; j < kRunMeanBatch; ++j) out[(int64_t)(k + j) * a.N] = s[j] / w;
            continue;
        }
        for (int32_t j = 0; j < g; ++j) {
            const int32_t first = (int32_t)((uint32_t)((k + j) * m) % kSlots);
            const int32_t n_first = min(W, kSlots - first);   // the window's terms before the ring wraps
            double s = col[first * kRunMeanThreads];
            s = add_slots(s, col + (first + 1) * kRunMeanThreads, n_first - 1);
            s = add_slots(s, col, W - n_first);
            out[(int64_t)(k + j) * a.N] = s / w;
        }
    }
}

}  // namespace

void running_mean_shape(int32_t window, int32_t m, int32_t* slots, int32_t* group)
{
    const int32_t want = m < window ? window + kRunMeanSpare : window;   // <= 64 + 7
    const int32_t n = want <= 16 ? 16 : want <= 20 ? 20 : want <= 26 ? 26 : want <= 40 ? 40 : 72;
    *slots = n;
    *group = m < window ? std::max(1, std::min(kRunMeanBatch, 1 + (n - window) / m)) : 1;
}

int32_t running_mean_tile(int32_t n_rows, int32_t window, int32_t m, int64_t N)
{
    const int64_t blocks_x = (N + kRunMeanThreads - 1) / kRunMeanThreads;
    const int64_t tiles = (kRunMeanMinBlocks + blocks_x - 1) / blocks_x;
    int64_t L = (n_rows + tiles - 1) / tiles;
    if (m < window) L = std::max<int64_t>(L, ((int64_t)kRunMeanMaxOverlap * (window - m) + m - 1) / m);
    L = std::max<int64_t>(L, 1);
    return (int32_t)((L + kRunMeanBatch - 1) / kRunMeanBatch * kRunMeanBatch);
}

hipError_t launch_running_mean(const RunningMeanArgs& args, hipStream_t s)
{
    RunningMeanArgs a = args;
    if (a.N <= 0 || a.n_rows <= 0) return hipSuccess;
    if (a.window < 2 || a.window > kRunMeanMaxWindow || a.m < 1) return hipErrorInvalidValue;
    int32_t slots = 0;
    running_mean_shape(a.window, a.m, &slots, &a.group);
    a.tile = running_mean_tile(a.n_rows, a.window, a.m, a.N);
    const dim3 grid((unsigned)((a.N + kRunMeanThreads - 1) / kRunMeanThreads), (unsigned)((a.n_rows + a.tile - 1) / a.tile));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    switch (slots) {
        case 16: hipLaunchKernelGGL(running_mean_kernel<16>, grid, dim3(kRunMeanThreads), 0, s, a); break;
        case 20: hipLaunchKernelGGL(running_mean_kernel<20>, grid, dim3(kRunMeanThreads), 0, s, a); break;
        case 26: hipLaunchKernelGGL(running_mean_kernel<26>, grid, dim3(kRunMeanThreads), 0, s, a); break;
        case 40: hipLaunchKernelGGL(running_mean_kernel<40>, grid, dim3(kRunMeanThreads), 0, s, a); break;
        default: hipLaunchKernelGGL(running_mean_kernel<72>, grid, dim3(kRunMeanThreads), 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace rscm
