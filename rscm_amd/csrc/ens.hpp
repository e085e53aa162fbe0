// Host-side internals shared by the translation units of librscm_gpu.so (rscm_gpu.cpp: handles, parameters, forcing, links,
// marshalling; kind_config.cpp: what the host builds from a kind's parameters and time axis; state_host.cpp: a handle's state in time
// -- initial values, time index, checkpoint, branch, rewind; window_host.cpp: the windowed storage; noise_host.cpp: the forcing-noise
// setting; selftest_host.cpp: the device self-tests; launch_host.cpp: one launch range of one handle; lockstep.cpp: the lock-step
// scheduler of component graphs; loglik_host.cpp: the likelihoods).  Not part of the boundary (include/rscm_gpu.h) and not visible
// outside the library (-fvisibility=hidden).
// Device allocation -- rscm::dev_malloc and rscm::DevBuf, the owner of every device buffer of the host layer, a call's
// temporaries and the d_* members of the handle, the sampler and the lock-step plan alike -- lives in dev_buf.hpp, which this
// header includes.  Nothing here frees device memory by hand: `delete` of a handle is its whole teardown.
#pragma once

#include "../../include/rscm_gpu.h"
#include "../../include/rscm_gpu_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <cstdlib>
#include <string>
#include <vector>

#include "dev_buf.hpp"
#include "internal_state.hpp"
#include "kinds.hpp"
#include "rscm_device.hpp"
#include "structural_rows.hpp"
#include "two_layer_year_facts.hpp"

// thread-local error text behind rscm_gpu_last_error(); returns `code`
int fail(int code, const char* fmt, ...);

inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? RSCM_ERR_NOMEM : RSCM_ERR_DEVICE; }
#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(hip_code(e_), "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

// n fresh elements in buf (grow: room for n, what it holds kept where that is enough -- DevBuf::reserve), or the failure under the
// caller's words for what could not be had: "<what>: out of memory" (rscm_gpu.cpp)
__attribute__((format(printf, 4, 5))) int alloc_or_fail(rscm::DevBuf<double>& buf, size_t n, bool grow, const char* what, ...);

#define GUARD_BEGIN try {
#define GUARD_END                                                                          \
    }                                                                                      \
    catch (const std::bad_alloc&) { return fail(RSCM_ERR_NOMEM, "host allocation failed"); } \
    catch (...) { return fail(RSCM_ERR_INVALID, "unexpected C++ exception"); }

#define NEED(h) \
    if (!(h)) return fail(RSCM_ERR_INVALID, "handle is NULL")

// Window upkeep of the handles of a lock-step run, collected while a model step (or a chunk of steps) is enqueued and issued as
// one or two launches at its end (rscm_device.hpp, WindowBatch).  first: moves and output-row copies; second: fills; then the
// windows' new first rows take effect on the host side.
struct WindowDeferral {
    std::vector<rscm::WindowOp> first, second;
    std::vector<std::pair<rscm_ens*, int32_t>> new_win0;
};

// Cached state of rscm_ens_run_lockstep for one list of handles (kept by the first of them): the device
// table of fused-launch operations (csrc/group.hip) and what it currently holds.
struct LockstepPlan {
    std::vector<rscm_ens*> handles;
    rscm::DevBuf<rscm::GroupOp> d_ops;       // [handles.size()]
    std::vector<rscm::GroupOp> cached;       // the table's contents (step fields zeroed)
    std::vector<uint8_t> valid;
    rscm::GroupOp* staging = nullptr;        // page-locked ring the uploads are sourced from
    int32_t ring_pos = 0;
    static constexpr int32_t kRing = 128;
    ~LockstepPlan() { if (staging) (void)hipHostFree(staging); }   // (d_ops makes the plan move-only)
};

// A staged quantile select in flight on a handle (rscm_ens_select_begin .. _end, rscm_gpu.cpp)
struct SelectState;

// The queue side of a handle: its stream, the timing events and what a two-stream cut run adds.  A base of rscm_ens, so that it
// is destroyed after every member of the handle -- the order teardown relies on (below).
struct EnsQueues {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // whole-axis runs as two member blocks on two streams in chunks of model steps (launch_host.cpp, plan_member_split): the second stream
    // and the fork / join events, created with the first such run
    hipStream_t split_stream = nullptr;
    hipEvent_t split_fork = nullptr, split_join = nullptr;
    ~EnsQueues()
    {
        if (split_stream) (void)hipStreamDestroy(split_stream);
        if (split_fork) (void)hipEventDestroy(split_fork);
        if (split_join) (void)hipEventDestroy(split_join);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

// Teardown is `delete h` and nothing else, in this order: ~rscm_ens() synchronises the stream and lets go of what is not device
// memory (the link reference counts, the staged select, the lock-step plan with its page-locked ring); then the members go, every
// d_* buffer among them (rscm::DevBuf); then the base, EnsQueues, destroys the events and the stream the handle owns.  So no
// buffer is freed under work in flight, and none outlives its stream.  The caller has made the handle's device current.
struct rscm_ens : EnsQueues {
    ~rscm_ens();   // rscm_gpu.cpp
    int32_t kind = 0;
    int64_t N = 0;
    int32_t T = 0;
    int32_t rows = 0;  // stored rows per series: T, or 1 with RSCM_FLAG_NO_SERIES
    int32_t device = 0;
    int32_t P = 0, V = 0;
    int32_t mode = RSCM_MODE_EXACT;
    std::vector<double> bounds;
    double h_tl = 0.1, h_cc = 0.1;
    bool schedule_dirty = true;
    std::vector<int32_t> nsub_tl, nsub_cc;
    rscm::DevBuf<int32_t> d_nsub_tl;
    rscm::DevBuf<int32_t> d_nsub_cc;
    // two-layer kind: what is proved once about the schedule and the forcing table for the uniform year (two_layer_year_facts.hpp).
    // The schedule's part is rebuilt with nsub_tl (refresh_schedule) and not read while schedule_dirty; the table's part is formed by
    // rscm_ens_set_forcing from the caller's array -- the only writer of d_forcing -- and dropped there before the table is touched
    rscm::tl::YearFacts year_facts;

    rscm::DevBuf<double> d_params;  // [P][N]
    int32_t ag_rows_set = 0;     // aggregate kind: 1 + the highest contributor row rscm_ens_set_forcing has ever been given data for
    uint64_t uniform_rows = 0;   // bit j: parameter row j (< 64) holds one value for every member (the kernels then read element 0: param_at)
    int32_t last_blocks = 1, last_chunks = 1;   // how the last run was cut (rscm_ens_last_run_plan; the second stream: EnsQueues)
    // member constants of the kinds that have them (GhgForcing, TerrestrialCarbon; rscm_device.hpp, launch_*_derive): [kDerivedRows][N],
    // re-formed by ensure_derived() at the next run after anything wrote the parameter block
    rscm::DevBuf<double> d_derived;
    bool derived_dirty = true;
    bool params_exposed = false; // rscm_ens_params_devptr handed the block out: uniform_rows stays 0 for the life of the handle
    bool derived_hold = false;   // inside one rscm_ens_run_lockstep call: the member constants were formed at its start and serve all its steps
    rscm::DevBuf<double> d_series;  // [(V-1)][T][N], variable v at slot v-1
    rscm::DevBuf<double> d_forcing; // [S][n_inputs][T]
    int32_t n_inputs = 1;        // rows per scenario of the shared input block
    // The forcing-noise setting (set_noise, noise_host.cpp, behind rscm_ens_set_forcing_noise* and rscm_ens_clear_forcing_noise): member i
    // is forced by F + e_t(noise_seed, noise_offset + i) of the kind noise_kind (rscm::kNoiseKind*; TwoLayerArgs, rscm_device.hpp).
    // noise_sigma: white and red (0 otherwise); noise_phi: red (0 otherwise); the per-member kind reads both from parameter rows.
    // The kinds that keep state (noise_red()): e is a pure function of (seed, sigma, phi, member id, t), and d_noise_state [N] caches
    // every member's e at forcing-axis index noise_state_index (-1: nothing cached); allocated by the first such setting.  step_launch
    // drops the index before a run's first launch and sets it after the whole run was issued; set_noise drops it.  A launch that does
    // not find the index before its first re-forms e from the draws
    int32_t noise_kind = rscm::kNoiseKindNone;
    uint64_t noise_seed = 0;
    double noise_sigma = 0.0;
    double noise_phi = 0.0;
    int64_t noise_offset = 0;
    rscm::DevBuf<double> d_noise_state;
    int32_t noise_state_index = -1;
    int32_t n_comp = 0;          // rscm_ens_create_mix: forcing components K (then n_inputs == K and P == 6 + K), 0 for every other handle
    // RSCM_FLAG_NOISE_PARAMS: the handle has the parameter rows noise_sigma_row() and noise_phi_row() -- a fact of its shape, whatever
    // the setting.  The per-member kind forms e from those rows as they stand at launch, so the cache is only as good as the rows.
    // A run leaves its index behind only where nobody can write the rows unseen: never once rscm_ens_params_devptr has handed the
    // block out (noise_cache_kept()); whatever writes a parameter row from the host drops it (params_written(), below).
    bool noise_rows = false;
    int32_t noise_sigma_row() const { return noise_rows ? 6 + n_comp : -1; }
    int32_t noise_phi_row() const { return noise_rows ? 6 + n_comp + 1 : -1; }
    bool noise_red() const { return rscm::noise_kind_keeps_state(noise_kind); }   // the settings that cache e
    bool noise_cache_kept() const { return !(noise_kind == rscm::kNoiseKindMembers && params_exposed); }
    // The rules that drop what the handle has cached about its parameter block and about where it stands.  Nothing outside them assigns
    // uniform_rows, derived_dirty or time_index but ensure_derived and step_finish (launch_host.cpp) and a fused launch's provisional index.
    // The parameter block was written from the host and these rows hold one value for every member -- none once the block has been
    // handed out: rscm_ens_set_params[_aos] (a restore goes through it), rscm_ens_sample_lhs[_priors], rscm_ens_gather_members into the handle
    void params_written(uint64_t uniform) { uniform_rows = params_exposed ? 0 : uniform; params_may_change(); rows_written(); }
    // A kernel is about to write these rows (~0: any), the samplers' proposals; the diagnostics' epoch moves with the run that follows
    void params_kernel_writes(uint64_t rows) { uniform_rows &= ~rows; if (rows) derived_dirty = true; }
    // rscm_ens_params_devptr: the writes it makes possible are the caller's to follow (no epoch moves)
    void expose_params() { params_exposed = true; uniform_rows = 0; params_may_change(); }
    void params_may_change() { derived_dirty = true; if (noise_kind == rscm::kNoiseKindMembers) noise_state_index = -1; }
    // The stepper was put at index k from outside: rscm_ens_set_time_index, _set_internal_state, _rewind, _clear_series, the gather, the samplers' resets
    void put_at(int32_t k) { time_index = k; rows_written(); ocean_forget_partial_sums(); }
    // rscm_ens_set_initial, the one entry point that moves the index (to 0) and keeps OceanCarbon's sums.  The next launch starts at step 0
    // (step_check), where ocean_advance (launch_host.cpp) never continues a parked tile -- only at a step after the tile's first -- so `part`
    // is the same either way; but mode sums standing at 0 (after an empty run [0, 0)) are served, where put_at(0) would set `rebuild`.  Kept
    void initial_written() { time_index = 0; rows_written(); }
    // Diagnostic variables (diagnostic_host.cpp; kernel in diagnostic.hip): per-member linear combinations of the stored variables with
    // ids V, V + 1, ..., their rows [held][N] for t_begin, t_begin + t_stride, ... in a store of their own.  The rows are a snapshot:
    // write_epoch moves with everything that can change a stored row, a parameter row or the time index (rows_written(): step_finish
    // for every run, params_written(), launch_loglik for the fused runs, set_noise, put_at() / initial_written() and the entry points
    // that write a state), and a store serves its rows only at the epoch it was computed at.
    // An energy-budget diagnostic (energy_budget_host.cpp; kernels in energy_budget.hip) takes one of the same slots: quantity is its
    // RSCM_BUDGET_* (0: a linear combination), budget_scale its scale, n_terms 0.  The two quantities that read the forcing are a
    // snapshot of it as well: forcing_epoch moves with whatever replaces the forcing table, the scenario assignment or the source
    // (rscm_ens_set_forcing, a mix handle's included) and with a link made or dropped, and their rows serve only at the forcing epoch
    // they were computed at.  The linear diagnostics and the two forcing-free quantities do not look at it.
    // A running mean (running_mean_host.cpp; kernel in running_mean.hip) takes a slot as well: rm_source is the variable it averages
    // (0: no running mean) -- a stored variable or a diagnostic of a lower slot that is no running mean itself -- over rm_window terms
    // rm_step time indices apart, aligned rm_align (RSCM_RUNMEAN_*); n_terms and quantity are 0.  rm_forcing: its source reads the
    // forcing, so its rows go stale with the forcing epoch too.  Once formed, its rows do not depend on the source's store.
    struct Diagnostic {
        int32_t n_terms = 0;
        int32_t var[RSCM_DIAG_MAX_TERMS] = {}, row[RSCM_DIAG_MAX_TERMS] = {};
        double scale[RSCM_DIAG_MAX_TERMS] = {};
        int32_t quantity = 0;
        double budget_scale = 0.0;
        int32_t rm_source = 0, rm_window = 0, rm_align = 0, rm_step = 1;
        bool rm_forcing = false;
        rscm::DevBuf<double> d_rows;   // [size() / N][N]: room for at least `held` rows
        int32_t held = 0, t_begin = 0, t_stride = 1;
        uint64_t epoch = 0, forcing_epoch = 0;
        bool reads_forcing() const { return quantity == RSCM_BUDGET_FORCING || quantity == RSCM_BUDGET_IMBALANCE || rm_forcing; }
    };
    Diagnostic diag[RSCM_DIAG_MAX];
    int32_t n_diag = 0;
    uint64_t write_epoch = 1, forcing_epoch = 1;
    void rows_written() { ++write_epoch; }
    void forcing_replaced() { ++forcing_epoch; }
    bool is_diagnostic(int32_t var) const { return var >= V && var < V + n_diag; }
    bool has_rows(int32_t var) const { return var >= 1 && var < V + n_diag; }   // a stored variable or a diagnostic
    bool diagnostic_current(const Diagnostic& d) const { return d.epoch == write_epoch && (!d.reads_forcing() || d.forcing_epoch == forcing_epoch); }
    bool diagnostic_stale(int32_t var) const { return diag[var - V].held > 0 && !diagnostic_current(diag[var - V]); }
    const double* diagnostic_row(int32_t var, int32_t t) const
    {
        if (!is_diagnostic(var)) return nullptr;
        const Diagnostic& d = diag[var - V];
        if (!diagnostic_current(d) || t < d.t_begin || (t - d.t_begin) % d.t_stride != 0) return nullptr;
        const int32_t r = (t - d.t_begin) / d.t_stride;
        return r < d.held ? d.d_rows + (size_t)r * N : nullptr;
    }
    rscm::DevBuf<double> d_ghg_tables;  // GhgForcing: [S][kGhgRows][T] derived scenario rows
    int32_t ghg_method = 1;
    // OceanCarbon: flux history (internal state) and the tabulated impulse response
    rscm::DevBuf<double> d_ocean_hist;  // [ocean_hist_rows][N]: a ring, pulse j in row j mod ocean_hist_rows
    int64_t ocean_hist_rows = 0;     // min((T-1)*12, max_hist + slack): the convolution never looks further back
    rscm::DevBuf<double> d_ocean_irf;   // [max(max_hist, 1)]
    rscm::DevBuf<double> d_ocean_partial;  // [(tile years - 1) * steps][N] split-tile running sums (one-step launches)
    int32_t ocean_tile_base = -1;       // first step of the split tile d_ocean_partial belongs to, -1: none
    int32_t ocean_tile_years = 0;       // its length (depends on the arithmetic mode it was started in)
    int32_t ocean_steps = 0;
    int64_t ocean_max_hist = 0;
    bool ocean_ready = false;
    // RSCM_MODE_FAST: the far response as decaying modes (ocean_fit_modes) and their running sums
    rscm::OceanModes ocean_modes{};
    bool ocean_recur_ok = false;
    int32_t ocean_near = 0;
    double ocean_fit_error = 0.0;
    rscm::DevBuf<double> d_ocean_mode_state;  // [kOceanModes][N]
    rscm::DevBuf<double> d_ocean_mode_table;  // [3][kOceanModes]: d_q, c_q, e_q
    int32_t ocean_modes_at = -1;           // time index the running sums stand at (-1: re-form them from the history)
    rscm::DevBuf<int32_t> d_scen;   // [N] or null
    int32_t n_scen = 0;
    int32_t source = RSCM_SRC_EXOGENOUS;
    rscm::DevBuf<uint8_t> d_status;

    // ClimateUDEB internal state
    rscm::DevBuf<double> d_ocean;    // [2][NL][N], room for size() / (2 N) layers
    rscm::DevBuf<double> d_udeb_work;   // [NL][N]  the any-layer-count kernel's c' array (udeb_any_body.hpp)
    rscm::DevBuf<double> d_udeb_tables; // [max(NL, kUdebDevTableRows)][6]  its geometry table
    int32_t udeb_work_layers() const { return (int32_t)(d_udeb_work.size() / (size_t)N); }   // layers d_udeb_work has room for
    rscm::DevBuf<double> d_scal;     // [kUdebScalars][N]
    rscm::DevBuf<double> d_hist;     // [T][N]
    rscm::DevBuf<double> d_bounds;   // [T+1]
    rscm::DevBuf<int32_t> d_win_kfull;  // [T]
    rscm::DevBuf<double> d_win_partw;   // [T]
    int32_t udeb_n_layers = 0, udeb_steps = 0, udeb_land_hc = 0, udeb_efficacy = 0;
    bool udeb_ready = false;
    std::vector<double> udeb_tables;

    rscm::DevBuf<double> d_partial;  // summary scratch
    rscm::DevBuf<double> d_out4;
    rscm::DevBuf<double> d_loglik;   // [N]
    // observations prepared for the fused run+likelihood kernel (prepare_obs)
    rscm::DevBuf<unsigned char> d_obs;   // (grows: prepare_obs)
    int32_t obs_n = 0, obs_normalize = 0, obs_first_is_deep = 0;
    int32_t obs_last_tidx = 0;        // the latest time index any prepared observation refers to
    bool loglik_stop_at_last_obs = false;  // fused run+likelihood launches end there (the device sampler: only ln L is used)
    // reference periods of the prepared observations (prepare_ref; cleared by prepare_obs)
    std::vector<int32_t> obs_merged_tidx, obs_merged_deep;   // host copy of the merged observation order
    bool ref_active = false;
    rscm::TwoLayerRefArgs ref{};
    int32_t ref_last_row = 0;         // the latest reference row of any period
    rscm::DevBuf<int32_t> d_ref_slot;    // [obs_n]
    rscm::DevBuf<double> d_defer;        // [n_deferred][N] model values waiting for their variable's b; room for size() / N rows

    bool timed = false;

    // linked inputs (rscm_ens_link_input)
    struct Link { rscm_ens* src = nullptr; int32_t var = 0; int32_t off = 0; };
    Link links[rscm::kMaxLinks];
    int32_t n_linked = 0;
    bool link_order_check = true;
    int32_t link_refs = 0;  // links of other ensembles into this one's series

    SelectState* select = nullptr;  // rscm_ens_select_begin .. rscm_ens_select_end
    rscm::DevBuf<int64_t> d_weights;   // [N] member weights of the weighted select (rscm_ens_set_member_weights)
    // posterior resampling (resample_host.cpp): the running sum of the weights with its scan scratch, and the ancestors of the last draw
    rscm::DevBuf<int64_t> d_cumw;      // [N + scan_scratch_elems(N)], allocated at the first rscm_ens_resample
    rscm::DevBuf<int64_t> d_anc;       // [size()] local member indices (rscm_ens_resample hands this out)
    // a destination of rscm_ens_gather_members: the time index its members were gathered at (-1: never a destination) and element 0 of
    // every parameter row of the source that configured it
    int32_t gather_k = -1;
    std::vector<double> gather_p0;
    rscm::DevBuf<int32_t> d_groups;    // [N] member groups of the grouped select and exceedance (rscm_ens_set_member_groups), -1: none
    int32_t n_groups = 0;
    rscm::DevBuf<double> d_base;       // [N] baseline of the anomaly select and indicators (rscm_ens_set_baseline)
    static constexpr int32_t kIndSlots = 4;
    rscm::DevBuf<double> d_ind[kIndSlots];  // [3 + kMaxThresholds][N] per slot of rscm_ens_member_indicators, allocated at first use
    LockstepPlan* plan = nullptr;  // rscm_ens_run_lockstep with this handle first
    WindowDeferral* defer = nullptr;  // set while rscm_ens_run_lockstep collects this handle's window upkeep (lockstep.cpp)

    int32_t time_index = 0;
    bool params_set = false, forcing_set = false;
    std::vector<uint8_t> initial_set;  // per variable id

    // Windowed storage (RSCM_FLAG_WINDOWED): d_series holds rows [win0, win0 + rows) of every series.
    bool windowed = false;
    int32_t win0 = 0;            // absolute time index of the first stored row
    int32_t lookback = 0;        // own rows before the current one that a step reads (chemistry kinds)
    bool read_ahead = false;     // a linked consumer may read index n+1 before this producer wrote it: rows after a slide must be NaN
    rscm::DevBuf<double> d_row0;    // [V-1][N] the initial rows, saved when step 0 starts (rewind restores them)
    bool row0_saved = false;
    int32_t out_stride = 0;      // > 0: every out_stride-th row of the output variables is kept in d_out
    int32_t n_out = 0, out_rows = 0;
    std::vector<int32_t> out_vars;      // variable ids kept
    std::vector<int32_t> out_slot;      // per variable id: slot in d_out or -1
    rscm::DevBuf<int32_t> d_out_vars;
    rscm::DevBuf<double> d_out;     // [n_out][out_rows][N]
    int32_t keep_rows() const { return std::max(lookback + 1, 2); }

    // Base of series[var] such that row t lives at base + t * N (for a windowed handle the address of
    // the virtual row 0: only rows [win0, win0 + rows) exist).
    double* series(int32_t var) const
    {
        return d_series + ((int64_t)(var - 1) * (int64_t)rows - (int64_t)win0) * N;
    }
    // Device address of row t of a stored variable where it is resident: the output store (every
    // out_stride-th row of the output variables, up to the current index), else the window; nullptr
    // if the row is not held any more.  Of a diagnostic: its own store, where it holds the row and is not stale.
    const double* row_ptr(int32_t var, int32_t t) const
    {
        if (var >= V) return diagnostic_row(var, t);   // (before the window: out_slot has no entry for a diagnostic)
        if (!windowed) return (rows == T || t == 0) ? series(var) + (size_t)t * N : nullptr;
        if (t >= win0 && t < win0 + rows) return series(var) + (size_t)t * N;  // the window is the live copy
        if (out_stride > 0 && out_slot[var] >= 0 && t % out_stride == 0 && t <= time_index)
            return d_out + ((size_t)out_slot[var] * out_rows + (size_t)(t / out_stride)) * N;
        return nullptr;
    }
    const rscm::KindInfo& info() const { return rscm::kKinds[kind]; }
    bool is_state(int32_t var) const { return var >= info().state_first && var <= info().state_last; }
    // a checkpoint, a gathered member or a time index set from outside carries its own state rows
    void mark_states_set() { std::fill(initial_set.begin() + info().state_first, initial_set.begin() + info().state_last + 1, (uint8_t)1); }
    // whether a linked input is read at index n + 1 of its source
    bool reads_end(const Link& l) const { return info().reads_end || l.off == 1; }
    // OceanCarbon: the sums parked for a split tile and the running mode sums no longer belong to where the handle stands
    void ocean_forget_partial_sums() { ocean_tile_base = -1; ocean_modes_at = -1; }
    // The internal component state at index k (internal_state.hpp; none while the columns or the ring do not exist), the buffers of its
    // runs, and whether the configuration it belongs to stands
    rscm::StateRuns state_runs(int32_t k) const { return rscm::internal_state_runs(kind, k, {d_ocean ? udeb_n_layers : 0, rscm::kUdebScalars, ocean_steps, d_ocean_hist ? ocean_hist_rows : 0}); }
    double* state_buf(rscm::StateBuf b) const { return b == rscm::StateBuf::UdebColumns ? d_ocean : b == rscm::StateBuf::UdebScalars ? d_scal : b == rscm::StateBuf::UdebHistory ? d_hist : d_ocean_hist; }
    bool internal_ready() const { return kind == RSCM_KIND_UDEB ? udeb_ready : kind == RSCM_KIND_OCEAN_CARBON ? ocean_ready : true; }
};

inline int set_device(const rscm_ens* h)
{
    HIPCHK(hipSetDevice(h->device));
    return RSCM_OK;
}

// One launch range of one handle, in pieces (launch_host.cpp); rscm_ens_run_lockstep (lockstep.cpp) fuses the
// launches of several handles out of the same pieces.
extern "C" {
int step_check(rscm_ens* h, int32_t step_begin, int32_t step_end, bool derive = true);
void set_two_layer_pair_lane(int32_t mode);     // A/B hook: -1 default, 0 never the two-instruction quotients, 1 whatever the run's length (calling thread)
void set_two_layer_guard(int32_t numerators);  // test hook: 1 forces the EXACT two-layer per-numerator guard (calling thread)
void set_run_plan(int32_t mode);          // A/B hook: -1 default, 0 one plain launch, 1 the two-stream cut where it applies (calling thread)
void set_fail_chunk_launch(int32_t k);   // test hook: the k-th chunk launch of the calling thread's next cut run fails (0: off)
int64_t take_derive_launches();           // test hook: member-constant kernels launched by the calling thread since the last call
int ensure_derived(rscm_ens* h);   // (every run starts with current member constants: run_range after its first event, rscm_ens_run_lockstep once per call)
int step_window_pre(rscm_ens* h, int32_t step_begin, int32_t step_end);
int step_links(rscm_ens* h, int32_t step_begin, int32_t step_end, rscm::InputLinks& links, int32_t& linked_out);
// op_out (zeroed by the caller): nothing is launched, the arguments go into a fused launch's table with a step range of [0, 0) -- the
// range is an argument of the fused launch.  RSCM_ERR_STATE for a handle that cannot be fused (can_fuse).
int step_launch(rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::GroupOp* op_out);
int step_finish(rscm_ens* h, int32_t step_begin, int32_t step_end);
int run_range(rscm_ens* h, int32_t step_begin, int32_t step_end, bool timed);
// what every two-layer launch takes from the handle: step_launch and the fused run + likelihood (loglik_host.cpp)
rscm::TwoLayerArgs two_layer_args(const rscm_ens* h, int32_t step_begin, int32_t step_end);
}
// Whether the handle's one-step launch can join a fused launch (kinds.hpp; GhgForcing's table path uses host-built rows)
inline bool can_fuse(const rscm_ens* h) { return h->info().fusable && (h->kind != RSCM_KIND_GHG_FORCING || h->n_linked > 0); }
// frees the staged select in flight on h, if any (select_host.cpp)
void select_release(rscm_ens* h);
// the rows t_begin, t_begin + t_stride, ... < t_end of var_id that this model instance has computed (t <= time_index), as device
// addresses (rscm_ens::row_ptr); *n_range = the rows of the whole range.  RSCM_ERR_STATE if a computed row is not resident.  The
// caller has checked var_id and the range (select_host.cpp).  The two checks that come first: var_id has a stored series and the range
// lies on the axis (empty ranges refused with at_least_one); a handle that stores only its initial row serves no range past it.
int check_row_range(const rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, bool at_least_one);
int check_series_stored(const rscm_ens* h, int32_t t_end);
// RSCM_OK for a stored variable and for a diagnostic whose rows are current; RSCM_ERR_STATE "diagnostic N is stale: compute it again"
// (diagnostic_host.cpp).  What every reader of a diagnostic's rows asks before it resolves them.
int check_diagnostic_current(const rscm_ens* h, int32_t var_id);
// An energy-budget diagnostic inside rscm_ens_compute_diagnostic (energy_budget_host.cpp).  budget_check: what the host proves before
// anything is launched for the rows t_begin + r * t_stride, r < n_rows -- parameters set, and for the quantities that read the forcing:
// no linked input, forcing set, every forcing-axis index on the axis.  budget_launch: the kernel over the uploaded source rows
// d_src [2][n_rows] (Ts, Td) into d.d_rows, enqueued on the handle's stream.
int budget_check(const rscm_ens* h, const rscm_ens::Diagnostic& d, int32_t t_begin, int32_t t_stride, int32_t n_rows);
hipError_t budget_launch(rscm_ens* h, rscm_ens::Diagnostic& d, const double* const* d_src, int32_t t_begin, int32_t t_stride, int32_t n_rows);
// A running-mean diagnostic inside rscm_ens_compute_diagnostic (running_mean_host.cpp): every check of the range and of the source's
// rows, the launch and the bookkeeping of the store.  A refusal leaves the rows held before in place.
int running_mean_compute(rscm_ens* h, rscm_ens::Diagnostic& d, int32_t t_begin, int32_t t_end, int32_t t_stride);
int resolve_rows(const rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, std::vector<const double*>& rows,
                 int32_t* n_range);
// resolve_rows with its checks for a range every row of which must be computed (RSCM_ERR_STATE else), and the rows' times
// (indicators_host.cpp): what the per-member statistics and the diagnostics' sources go through
int period_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, std::vector<const double*>& rows,
                std::vector<double>& times);
// What the readers of such rows share besides (indicators_host.cpp): RSCM_ERR_STATE while a staged select is in flight; the device
// array of the row pointers, enqueued on the handle's stream (rows must live until the caller has synchronised it); the check of an
// indicator slot, and the slot's buffer d_ind[slot], allocated at first use
int no_select(const rscm_ens* h);
int upload_rows(rscm_ens* h, const std::vector<const double*>& rows, rscm::DevBuf<const double*>& d_rows);
int check_slot(int32_t slot);
int slot_buffer(rscm_ens* h, int32_t slot);
// RSCM_OK if p is device memory on h's device holding at least N doubles from p on, else RSCM_ERR_INVALID (select_host.cpp)
int check_member_vector(const rscm_ens* h, const double* p, const char* what);
// RSCM_OK if p is device memory on h's device holding at least n int64 from p on, else RSCM_ERR_INVALID: the `out` of the moment sums
// when it is on the device (moments_host.cpp)
int check_device_out(const rscm_ens* h, const int64_t* p, size_t n);
// What rscm_ens_moment_sums and rscm_ens_moment_rows_sums share besides (moments_host.cpp).  Their refusals, in this order: flags
// outside `allowed`, the order, order 2 without a centre, the vector list, a NULL out, a flag whose member weights, groups or
// baseline the handle lacks, 2^31 members or more; then, on the handle's device, check_member_vector of every vector
int check_moment_call(const rscm_ens* h, int32_t flags, int32_t allowed, int32_t order, const double* center, int32_t n_vec,
                      const double* const* vec_dev, int32_t min_vec, int32_t max_vec, const int64_t* out);
int check_member_vectors(const rscm_ens* h, int32_t n_vec, const double* const* vec_dev);
// The centre on the device, enqueued on the handle's stream (none, for order 1: nothing): n records of `width` doubles, a record with a
// non-finite entry all NaN, so that every term about it is counted as non-finite.  c, the host copy, lives until the stream is synchronised
int upload_moment_centre(rscm_ens* h, const double* center, size_t n, size_t width, std::vector<double>& c, rscm::DevBuf<double>& d_centre);
// The device array of `total` int64 the sums land in, zeroed on the handle's stream: the caller's `out` when it is on the device
// (check_device_out first), else the temporary, which end_moment_out copies to `out` before it ends the call with its one synchronise
int begin_moment_out(rscm_ens* h, int64_t* out, size_t total, int32_t on_device, rscm::DevBuf<unsigned long long>& d_tmp,
                     unsigned long long** d_out);
int end_moment_out(rscm_ens* h, int64_t* out, const unsigned long long* d_out, size_t total, int32_t on_device);
// sums [RG][2 + B * 69] (n, W, B blocks) as out[RG][B], every block over its record's W, and n[RG], weight[RG] unless NULL
int finish_moment_sums(const int64_t* sums, size_t RG, int32_t B, double* out, int64_t* n, int64_t* weight);
// issue what a WindowDeferral holds on `stream` and make the new windows current (window_host.cpp)
int window_flush(WindowDeferral* d, hipStream_t stream);
// the handle's own window (window_host.cpp)
int window_reset(rscm_ens* h, bool clear);
int window_slide(rscm_ens* h, int32_t new_win0);
int window_seek(rscm_ens* h, int32_t k);
int window_store_row(rscm_ens* h, int32_t t);

// What the host builds from parameters and time axis (kind_config.cpp): the RK4 sub-step tables, GhgForcing's rows [S][kGhgRows][T] of conc [S][3][T] ...
int refresh_schedule(rscm_ens* h);
std::vector<double> ghg_tables(const double* conc, int32_t n_scen, int32_t T);
// ... and the configuration derived from a parameter vector's structural rows (structural_rows.hpp): ClimateUDEB's tables and windows,
// OceanCarbon's response table, ring and mode fit, GhgForcing's method.  Members 0 .. n_check - 1 are checked for uniformity: a block
// [P][N] is {soa, N, 1, N}, one vector {p, 1, 0, 1}.  state_replaced: a branch is about to replace the internal state, so a change of its shape is no error
struct ParamView {
    const double* base; int64_t row_stride, member_stride, n_check;
    double at(int32_t j, int64_t i = 0) const { return base[(size_t)j * row_stride + (size_t)i * member_stride]; }
};
int configure_kind(rscm_ens* h, const ParamView& p, bool state_replaced = false);
// N2O: the rows the stratospheric delay looks back (n2o.rs:203-218).  Two callers: rscm_ens_set_params with the largest member value,
// rscm_ens_sample_lhs with `high` of the delay's row
inline int32_t n2o_lookback(double largest_delay) { return (int32_t)std::min(std::max(1.0, largest_delay), 1e6) + 1; }

// An observation list and its reference periods as the boundary passes them.  owner: the handle of a list that each entry refers
// to (the graph sampler), null: all refer to the first.
struct ObsList {
    int32_t n;
    const int32_t *owner, *var, *tidx;
    const double *value, *sigma;
    int32_t normalize;
};
struct RefList {
    int32_t n;
    const int32_t *owner, *var, *begin, *end, *stride;
};
// ... resolved to the device rows the stored-series likelihood reads (loglik_kernel, ensemble_ops.hip)
struct LoglikRows {
    std::vector<const double*> obs_rows, ref_rows;   // observation j's row; entry e averages ref_rows[ref_off[e] .. ref_off[e + 1])
    std::vector<int32_t> grp, obs_ref, ref_off;      // observation j's group and its group's reference entry (-1: none)
    int32_t last_row = 0;      // the last row any of them reads
    bool uncomputed = false;   // a row beyond its handle's time index is read: every member scores -inf, no row is resolved
    std::vector<unsigned char> staging;   // upload_loglik's host copy of the table, the source of its asynchronous copy
};
// the likelihood's host side (loglik_host.cpp), shared with the sampler (sampler_host.cpp)
extern "C" {
// Validates the lists against the handles and resolves the rows.  whole_series: the samplers' evaluators, which store their whole series
// and are run afresh for every score (rows at series(var) + t * N, the time index does not matter); else a handle's own likelihood (rows
// where they are resident, rscm_ens::row_ptr; RSCM_ERR_STATE if one is not).
int resolve_loglik_rows(rscm_ens* const* handles, int32_t n_handles, bool whole_series, const ObsList& o, const RefList& r, LoglikRows* out);
// Lays rows, values, sigmas, groups and reference tables out in one device allocation, d_blob, and points *args into it: ready for
// launch_loglik on `stream`.  The copy is enqueued on `stream` from rows.staging: rows must live until the caller has synchronised
// that stream.
int upload_loglik(LoglikRows& rows, const ObsList& o, int64_t n_members, double* out, hipStream_t stream, rscm::DevBuf<unsigned char>& d_blob,
                  rscm::LoglikArgs* args);
int prepare_obs(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx, const double* obs_value, const double* obs_sigma,
                int32_t normalize);
// reference periods for the observations prepare_obs holds (n_ref == 0: none): validates, lays out the deferred observations' scratch
int prepare_ref(rscm_ens* h, int32_t n_ref, const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end, const int32_t* ref_stride);
// shapes of a reference-period list on an axis of T rows: ranges as rscm_ens_set_baseline, each variable at most once
// (per owner where ref_owner is given: the graph sampler)
int check_reference(int32_t T, int32_t n_ref, const int32_t* ref_owner, const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end,
                    const int32_t* ref_stride);
int check_loglik_ready(rscm_ens* h);
hipError_t launch_loglik(rscm_ens* h);   // asynchronous, with the prepared observations; fills h->d_loglik
}
