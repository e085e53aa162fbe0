// What the host side of the running-mean diagnostics (running_mean_host.cpp) asks of their kernel (running_mean.hip).  A header of its
// own, as diagnostic.hpp: the other kernel files include neither it nor anything it changes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rscm {

constexpr int kRunMeanMaxWindow = 64;   // RSCM_RUNMEAN_MAX_WINDOW
constexpr int kRunMeanThreads = 256;    // members per block (x)
constexpr int kRunMeanBatch = 8;        // source rows whose loads a thread issues before it uses the first
constexpr int kRunMeanReads = 8;        // ring slots a thread reads before it adds the first
constexpr int kRunMeanSpare = kRunMeanBatch - 1;   // ring slots beyond the window where windows overlap: at m = 1 a group is kRunMeanBatch outputs
constexpr int kRunMeanMinBlocks = 2048; // blocks the host asks for before it lets a tile grow past its shortest (running_mean_tile)
constexpr int kRunMeanMaxOverlap = 4;   // a tile of L outputs re-reads W - m rows: L * m >= kRunMeanMaxOverlap * (W - m), overlap <= 1.25

// d_out[r][i] = the running mean include/rscm_gpu.h states (running means) of the source rows d_rows[r * m + j][i], j < window, in that
// order, divided by (double)window: r < n_rows, and d_rows holds (n_rows - 1) * m + window device addresses of N doubles each
struct RunningMeanArgs {
    const double* const* d_rows;
    double* d_out;   // [n_rows][N]
    int64_t N;
    int32_t n_rows;
    int32_t window;  // W, 2 .. kRunMeanMaxWindow
    int32_t m;       // source rows from one output to the next (t_stride / step), >= 1
    int32_t tile;    // outputs per block (y): running_mean_tile          } both set by launch_running_mean,
    int32_t group;   // outputs whose new rows are loaded together         } whatever the caller put there
};
// The ring's slots and the group for (window, m): the smallest ring of running_mean.hip (16, 20, 26, 40, 72 slots) that holds
// window + kRunMeanSpare rows where m < window (the rows of several outputs overlap), `window` rows else; and the outputs per group,
// min(kRunMeanBatch, 1 + (slots - window) / m) where m < window, 1 else: window + (group - 1) * m <= slots
void running_mean_shape(int32_t window, int32_t m, int32_t* slots, int32_t* group);
// Outputs per block: a multiple of kRunMeanBatch, see the head of running_mean.hip
int32_t running_mean_tile(int32_t n_rows, int32_t window, int32_t m, int64_t N);
hipError_t launch_running_mean(const RunningMeanArgs& a, hipStream_t s);

}  // namespace rscm
