// One launch range of one handle, in pieces: what must hold before anything is enqueued (step_check), the handle's own window
// (step_window_pre), the producers' series (step_links), the launch (step_launch) and the bookkeeping after it (step_finish).
// run_range strings them together for a stand-alone run; rscm_ens_run_lockstep (lockstep.cpp) fuses the launches of several handles
// out of the same pieces.  Each family of kinds (kinds.hpp) has one function that builds its argument struct from the handle.
#include "ens.hpp"
#include "experiment_env.hpp"

extern "C" {

// ---- (1) what must hold before anything is enqueued ----
// The member constants of GhgForcing, TerrestrialCarbon and ClimateUDEB (what their bodies used to form from the parameters alone at the
// top of every launch; ClimateUDEB: the base LAMCALC solve): one small kernel whenever the parameter block has been written since the last one -- rscm_ens_set_params*,
// rscm_ens_sample_lhs, a checkpoint restore, a sampler's proposals -- and before EVERY run of a handle whose block the caller may
// write directly (rscm_ens_params_devptr).
// (test hook: derive launches issued by the calling thread, rscm_gpu_derive_launches)
static thread_local int64_t t_derive_launches = 0;
int64_t take_derive_launches()
{
    const int64_t n = t_derive_launches;
    t_derive_launches = 0;
    return n;
}

int ensure_derived(rscm_ens* h)
{
    if (!h->info().has_derived || !h->params_set) return RSCM_OK;
    if (!h->derived_dirty && !h->params_exposed && h->d_derived) return RSCM_OK;
    // a block the caller may write directly is re-derived before every run -- once per API call: the steps of one
    // rscm_ens_run_lockstep call share the constants formed at its start (a one-step launch per model step used to pay the
    // derive kernel, ClimateUDEB's secant solve, every step)
    if (h->derived_hold && !h->derived_dirty && h->d_derived) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    if (int rc = alloc_or_fail(h->d_derived, (size_t)rscm::kDerivedRows * h->N, true, "member constants of %lld members", (long long)h->N)) return rc;
    switch (h->info().family) {
        case rscm::Family::Ghg: HIPCHK(rscm::launch_ghg_derive(h->d_params, h->uniform_rows, h->ghg_method, h->N, h->d_derived, h->stream)); break;
        case rscm::Family::Udeb: HIPCHK(rscm::launch_udeb_derive(h->d_params, h->uniform_rows, h->N, h->d_derived, h->stream)); break;
        default: HIPCHK(rscm::launch_terrestrial_derive(h->d_params, h->uniform_rows, h->N, h->d_derived, h->stream)); break;
    }
    ++t_derive_launches;
    h->derived_dirty = false;
    return RSCM_OK;
}

// The two-layer kind's member constants: zh, zl of the two-instruction quotient for both heat capacities ([4][N]; two_layer.hip,
// two_layer_pair_div_kernel), held under the same rule -- dirty after anything that can write a parameter row, re-formed before every
// run while the block is exposed -- but formed only on behalf of a run that will use them (pair_lane_wanted below): the samplers and
// the fused likelihood change the parameters with every evaluation and never pay for them.
static int ensure_pair_constants(rscm_ens* h)
{
    if (!h->derived_dirty && !h->params_exposed && h->d_derived) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    if (int rc = alloc_or_fail(h->d_derived, (size_t)4 * h->N, true, "quotient constants of %lld members", (long long)h->N)) return rc;
    HIPCHK(rscm::launch_two_layer_pair_div(h->d_params, h->uniform_rows, h->N, h->d_derived, h->stream));
    h->derived_dirty = false;
    return RSCM_OK;
}

int step_check(rscm_ens* h, int32_t step_begin, int32_t step_end, bool derive)
{
    NEED(h);
    if (step_begin < 0 || step_end > h->T - 1 || step_begin > step_end)
        return fail(RSCM_ERR_STATE, "steps [%d, %d) outside [0, %d] (Model::step asserts time_index < len-1)",
                    step_begin, step_end, h->T - 1);
    if (step_begin != h->time_index)
        return fail(RSCM_ERR_STATE, "step_begin %d != current time index %d", step_begin, h->time_index);
    if (!h->windowed && h->rows != h->T && step_end > step_begin)
        return fail(RSCM_ERR_STATE, "this handle stores no series (RSCM_FLAG_NO_SERIES): use rscm_ens_run_loglik");
    const int32_t keep = h->keep_rows();
    if (h->windowed && step_end > step_begin) {
        if (h->rows < 2 * keep)
            return fail(RSCM_ERR_STATE, "a window of %d rows is too short for a component that reads %d of its own earlier rows (need >= %d)",
                        h->rows, h->lookback, 2 * keep);
        if (step_end - step_begin + keep > h->rows)
            return fail(RSCM_ERR_STATE, "steps [%d, %d) do not fit a window of %d rows (%d are kept for look-back): step in shorter ranges",
                        step_begin, step_end, h->rows, keep);
        // the rows the first step looks back at must be resident (they are after any slide made with this
        // look-back; not after the look-back was raised on a window that had already moved)
        if (std::max(0, step_begin - h->lookback) < h->win0)
            return fail(RSCM_ERR_STATE, "step %d reads row %d of its own series, the window starts at row %d", step_begin,
                        std::max(0, step_begin - h->lookback), h->win0);
    }
    if (!h->params_set) return fail(RSCM_ERR_STATE, "parameters not set");
    if (!h->forcing_set && h->n_linked < h->n_inputs) return fail(RSCM_ERR_STATE, "shared input series not set");
    for (int32_t v = 1; v < h->V; ++v)
        if (h->is_state(v) && !h->initial_set[v])  // builder.rs:704-717 MissingInitialValue
            return fail(RSCM_ERR_STATE, "state variable %d has no initial value (MissingInitialValue)", v);
    return derive ? ensure_derived(h) : RSCM_OK;
}

// ---- (2) schedule tables and the handle's own window: room for the rows this range writes ----
int step_window_pre(rscm_ens* h, int32_t step_begin, int32_t step_end)
{
    const int32_t keep = h->keep_rows();
    if (int rc = set_device(h)) return rc;
    if (int rc = refresh_schedule(h)) return rc;
    if (h->windowed && step_end > step_begin) {
        // room for the rows this range writes must exist before its launch is enqueued: nothing here is left to a later flush
        struct Immediate {
            rscm_ens* h; WindowDeferral* d;
            explicit Immediate(rscm_ens* x) : h(x), d(x->defer) { h->defer = nullptr; }
            ~Immediate() { h->defer = d; }
        } now(h);
        if (step_begin == 0) {
            if (h->win0 != 0)
                if (int rc = window_reset(h, false)) return rc;
            if (!h->row0_saved) {  // the initial rows, for rewind
                HIPCHK(rscm::launch_gather_rows(h->d_series, h->N, h->rows, 0, nullptr, h->V - 1, h->d_row0, 1, 0, h->stream));
                h->row0_saved = true;
            }
            if (int rc = window_store_row(h, 0)) return rc;
        }
        if (step_end >= h->win0 + h->rows)
            if (int rc = window_slide(h, step_begin - keep + 1)) return rc;
        // the links of h were resolved against the producers' windows above; h's own base moved with the slide
    }

    return RSCM_OK;
}

// ---- (3) the producing ensembles' series as they stand now (after every window of the graph has been moved) ----
int step_links(rscm_ens* h, int32_t step_begin, int32_t step_end, rscm::InputLinks& links, int32_t& linked_out)
{
    // linked inputs: the producing ensembles' series, in launch order on one stream
    links = rscm::InputLinks{};
    linked_out = h->n_linked > 0 ? 1 : 0;
    for (int32_t k = 0; k < rscm::kMaxLinks && k < h->n_inputs; ++k) {
        const auto& l = h->links[k];
        if (!l.src) continue;
        if (l.src->stream != h->stream)
            return fail(RSCM_ERR_STATE, "input row %d is linked to an ensemble on another stream (rscm_ens_set_stream both to the same one)", k);
        // ClimateUDEB reads at_start / at_end, the aggregate at_end: index n+1 whatever `source` said
        const int32_t off = h->reads_end(l) ? 1 : 0;
        const int32_t need = step_end - 1 + off;
        if (h->link_order_check && step_end > step_begin && l.src->time_index < need)
            return fail(RSCM_ERR_STATE, "input row %d reads index %d of its source, which has only been stepped to %d", k, need,
                        l.src->time_index);
        if (l.src->windowed && step_end > step_begin) {  // the rows this launch reads must be resident in the producer's window
            const int32_t lo = step_begin + (h->kind == RSCM_KIND_UDEB ? 0 : off), hi = need;
            if (lo < l.src->win0 || hi >= l.src->win0 + l.src->rows)
                return fail(RSCM_ERR_STATE, "input row %d reads indices [%d, %d] of its source, whose window holds [%d, %d): step the graph in lock-step",
                            k, lo, hi, l.src->win0, l.src->win0 + l.src->rows);
        }
        links.row[k] = l.src->series(l.var);
        links.off[k] = h->info().reads_end ? 0 : l.off;   // (such a kernel goes to index n + 1 by itself)
    }
    return RSCM_OK;
}

// ---- (4) the launch itself ----
// Whole-axis launches of the two-layer and the coupled kind as TWO member blocks on two streams, each in chunks of model steps issued
// in turn.  One launch of 1e5 members is 1564 wavefronts on 1024 SIMDs: the SIMDs that got two take twice as long as those that got one,
// and the launch takes the time of two (issue utilisation 0.66).  Cut into a block that fills the chip once
// (65 536 members) and the rest, each block on its own stream and in chunks of ~64 model steps, the same kernels resume from the rows they
// stored (as rscm_ens_run in pieces always could), a block's next chunk is dispatched while the other block's is still running, and the
// hardware's dispatcher evens out the SIMDs over the chunks: 2.86 -> 2.36 ms at 1e5 members x 750 years, 1.1-1.36x at every size between
// 1e5 and 3e5, 1.05x at 1e6, never slower with three chunks or more (scripts/multi_stream_two_layer.py).  Same kernels on the same
// operands: the same bits.  The caller's stream forks into the helper stream and joins it again with events: to the caller this is one
// asynchronous run on its stream, as before.  RSCM_SPLIT_RUNS=0 turns it off (A/B).
// A/B and test hook (include/rscm_gpu_internal.h, rscm_gpu_set_run_plan): how the calling thread's whole-axis runs go out --
// -1 by the environment and the sizes (default), 0 always one plain launch, 1 the two-stream cut where it applies.
static thread_local int32_t t_run_plan = -1;
void set_run_plan(int32_t mode) { t_run_plan = mode; }
// Test hook (rscm_gpu_set_two_layer_guard): 1 makes the calling thread's EXACT two-layer launches guard every numerator.
static thread_local int32_t t_tl_numerator_guard = 0;
void set_two_layer_guard(int32_t numerators) { t_tl_numerator_guard = numerators; }
// A/B and test hook (rscm_gpu_set_two_layer_pair_lane): the two-instruction quotients of the calling thread's stand-alone stored EXACT
// two-layer runs of the plain table with ten sub-steps everywhere -- -1 from kPairLaneMinSteps steps on (default), 0 never, 1 whatever
// the run's length.
static thread_local int32_t t_tl_pair_lane = -1;
void set_two_layer_pair_lane(int32_t mode) { t_tl_pair_lane = mode; }
// The run must earn back the kernel that forms the constants, even if it is the only run of its parameter set: that kernel takes 72 us
// at 1e5 members and the lane saves 0.17 us per model step there (profiles/two_layer_pair_div.txt: 0.126 ms per 750 steps), which
// breaks even at about 430 steps.  Both scale with the wavefronts per SIMD, so the count holds for other sizes.
constexpr int32_t kPairLaneMinSteps = 512;
// Test hook (rscm_gpu_two_layer_guard_counts): 1 makes the calling thread's stand-alone EXACT two-layer launches count their guards.
static thread_local int32_t t_tl_count_guards = 0;
int rscm_gpu_two_layer_guard_counts(int32_t device_id, int32_t enable, int64_t* counts)
{
    GUARD_BEGIN
    if (enable != 0 && enable != 1) return fail(RSCM_ERR_INVALID, "guard counting %d (0 off, 1 on)", enable);
    HIPCHK(hipSetDevice(device_id));
    hipError_t e = rscm::two_layer_guard_counts(counts);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "two_layer_guard_counts: %s", hipGetErrorString(e));
    t_tl_count_guards = enable;
    return RSCM_OK;
    GUARD_END
}
int rscm_gpu_two_layer_pair_lanes(int32_t device_id, int64_t* count)
{
    GUARD_BEGIN
    HIPCHK(hipSetDevice(device_id));
    hipError_t e = rscm::two_layer_pair_lanes(count);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "two_layer_pair_lanes: %s", hipGetErrorString(e));
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"

namespace {

struct MemberSplit {
    bool on = false;
    int64_t first = 0;     // members of the first block
    int32_t chunk = 0;     // model steps per launch
};
MemberSplit plan_member_split(rscm_ens* h, int32_t step_begin, int32_t step_end, bool linked, bool halves)
{
    static const bool enabled = [] { const char* e = getenv("RSCM_SPLIT_RUNS"); return !e || atoi(e) != 0; }();
    // (tuning knobs of the experiments build only, experiment_env.hpp: model steps per chunk, members of the first block)
    static const int32_t chunk_env = (int32_t)rscm::experiment_env("RSCM_SPLIT_CHUNK", 0);
    static const int64_t first_env = (int64_t)rscm::experiment_env("RSCM_SPLIT_FIRST", 0);
    MemberSplit m;
    // two-layer / coupled: 32-64 steps per chunk 2.30 ms at 1e5 members, 96: 2.32, 192: 2.37 (scripts/sweep_split.sh); ClimateUDEB reloads
    // and stores its columns with every chunk: 96 (88 ms at 1e5 members against 90 with 64)
    const int32_t kChunk = chunk_env > 0 ? chunk_env : (halves ? 96 : 64);
    const int32_t len = step_end - step_begin;
    if ((t_run_plan >= 0 ? t_run_plan != 1 : !enabled) || linked || h->windowed || h->rows != h->T || len < 3 * kChunk) return m;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus <= 0) return m;
    const int64_t per_round = (int64_t)cus * 4 * 64;   // one wavefront on every SIMD: 65 536 members on an MI355X
    if (h->N <= per_round) return m;                   // every wavefront has a SIMD to itself already
    m.first = halves ? (h->N / 2 + 63) / 64 * 64 : std::max(per_round, (h->N / 2) / per_round * per_round);
    if (first_env > 0) {   // (experiment knob) rounded up to whole wavefronts; ignored unless both blocks keep members
        const int64_t want = (first_env + 63) / 64 * 64;
        if (want > 0 && want < h->N) m.first = want;
    }
    if (!(m.first > 0 && m.first < h->N)) return m;   // never a block that reaches past the ensemble
    const int32_t n_chunks = (len + kChunk - 1) / kChunk;
    m.chunk = (len + n_chunks - 1) / n_chunks;
    m.on = true;
    return m;
}
int member_split_streams(rscm_ens* h)
{
    if (!h->split_stream) HIPCHK(hipStreamCreateWithFlags(&h->split_stream, hipStreamNonBlocking));
    if (!h->split_fork) HIPCHK(hipEventCreateWithFlags(&h->split_fork, hipEventDisableTiming));
    if (!h->split_join) HIPCHK(hipEventCreateWithFlags(&h->split_join, hipEventDisableTiming));
    return RSCM_OK;
}
// Test hook (include/rscm_gpu_internal.h, rscm_gpu_fail_chunk_launch): the k-th chunk launch of the calling thread's next cut run
// reports a launch failure instead of being issued -- the only way to execute the join-after-failure path below.
thread_local int32_t t_fail_chunk = 0;

// issue(begin, end, first_member, count, stream) launches one chunk of one block; the fork and the join around all of them
template <class Issue>
int run_member_split(rscm_ens* h, const MemberSplit& m, int32_t step_begin, int32_t step_end, Issue issue)
{
    // (test hook) a cut run consumes it, whether k was reached or not and however the run ends: it never outlives the run it was set for
    int32_t fail_at = t_fail_chunk;
    t_fail_chunk = 0;
    if (int rc = member_split_streams(h)) return rc;
    h->last_blocks = 2;
    h->last_chunks = (step_end - step_begin + m.chunk - 1) / m.chunk;
    HIPCHK(hipEventRecord(h->split_fork, h->stream));
    HIPCHK(hipStreamWaitEvent(h->split_stream, h->split_fork, 0));
    // (experiments: RSCM_SPLIT_CHUNK2 gives the second block its own chunk length; the block that is behind is issued next)
    static const int32_t chunk2_env = (int32_t)rscm::experiment_env("RSCM_SPLIT_CHUNK2", 0);
    const int32_t c0 = m.chunk, c1 = chunk2_env > 0 ? chunk2_env : m.chunk;
    hipError_t err = hipSuccess;
    auto guarded = [&](int32_t b, int32_t e, int64_t m0, int64_t cnt, hipStream_t st) -> hipError_t {
        if (fail_at > 0 && --fail_at == 0) return hipErrorLaunchFailure;   // (test hook)
        return issue(b, e, m0, cnt, st);
    };
    for (int32_t b0 = step_begin, b1 = step_begin; err == hipSuccess && (b0 < step_end || b1 < step_end);) {
        if (b0 < step_end && (b0 <= b1 || b1 >= step_end)) {
            const int32_t e = std::min(step_end, b0 + c0);
            err = guarded(b0, e, (int64_t)0, m.first, h->stream);
            b0 = e;
        } else {
            const int32_t e = std::min(step_end, b1 + c1);
            err = guarded(b1, e, m.first, h->N - m.first, h->split_stream);
            b1 = e;
        }
    }
    // the join is made whatever happened: the caller's stream never runs ahead of what was issued on the helper stream
    HIPCHK(hipEventRecord(h->split_join, h->split_stream));
    HIPCHK(hipStreamWaitEvent(h->stream, h->split_join, 0));
    HIPCHK(err);
    return RSCM_OK;
}

// ---- one builder per family: fill_<family> writes the arguments of a launch of [step_begin, step_end) into `a`, which the caller has
// zeroed (a local, or the op of a fused launch's table: lockstep.cpp compares ops bytewise, so nothing is assigned as a whole struct).
// The builders do not change the handle.  block_of (the families whose runs may be cut): the same arguments for steps [begin, end) of
// the `count` members from m0 on -- every per-member pointer moves with the block, the strides stay those of the ensemble.

// what every family's arguments begin with: members, axis, step range, parameter block, status bytes
template <class Args>
void fill_common(const rscm_ens* h, int32_t step_begin, int32_t step_end, Args& a)
{
    a.n_members = h->N;
    a.n_times = h->T;
    a.step_begin = step_begin;
    a.step_end = step_end;
    a.params = h->d_params;
    a.uniform_rows = h->uniform_rows;
    a.status = h->d_status;
}

// The year's uniform facts of a launch of [a.step_begin, a.step_end) with a's source and offset (TwoLayerArgs::year_facts): 0 for a fused
// launch (an empty range), and nothing about the forcing unless the launch reads the handle's plain table
// pair: the launch is handed the handle's current quotient constants (the stored run of step_launch that asked for them; every chunk alike)
uint32_t two_layer_year_facts(const rscm_ens* h, const rscm::TwoLayerArgs& a, bool pair = false)
{
    if (a.step_end <= a.step_begin) return 0;
    const int32_t nsub = h->schedule_dirty ? 0 : h->year_facts.nsub_uniform(a.step_begin, a.step_end);
    const bool plain = !a.link && a.n_comp == 0 && !a.noise_on && a.forcing == h->d_forcing && a.n_scen == h->n_scen;
    return rscm::year_facts_word(nsub, plain && h->year_facts.forcing_boxed(a.step_begin, a.step_end, a.src_off), plain && pair);
}
// Whether the stored run of [step_begin, step_end) is one the pair lane is for: EXACT, stand-alone, the plain table, ten sub-steps in
// every step, and long enough (or the hook says so)
bool pair_lane_wanted(const rscm_ens* h, int32_t step_begin, int32_t step_end, int32_t linked)
{
    if (t_tl_pair_lane == 0 || h->mode != RSCM_MODE_EXACT || linked || h->n_comp > 0 || h->noise_kind || !h->params_set) return false;
    if (t_tl_pair_lane < 0 && step_end - step_begin < kPairLaneMinSteps) return false;
    return !h->schedule_dirty && h->year_facts.nsub_uniform(step_begin, step_end) == 10;
}
// shared forcing and scenarios, sub-step table, guard hooks, series
void fill_two_layer(const rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::TwoLayerArgs& a,
                    bool pair = false)   // pair: the launch is handed the handle's current quotient constants (step_launch)
{
    fill_common(h, step_begin, step_end, a);
    a.row_stride = h->N;
    a.n_scen = linked ? 1 : h->n_scen;
    a.src_off = linked ? links.off[0] : (h->source == RSCM_SRC_UPSTREAM ? 1 : 0);
    a.n_comp = h->n_comp;
    a.lds_forcing = !linked && rscm::two_layer_fits_lds(h->n_scen, h->n_comp, step_end - step_begin) ? 1 : 0;
    a.forcing = h->d_forcing;
    a.link = linked ? links.row[0] : nullptr;
    a.scen = linked ? nullptr : h->d_scen;
    a.nsub = h->d_nsub_tl;
    a.h = h->h_tl;
    a.h_half = h->h_tl / 2.0;
    a.h_sixth = h->h_tl / 6.0;
    a.numerator_guard = t_tl_numerator_guard;
    a.count_guards = t_tl_count_guards;
    a.ts = h->series(RSCM_TL_VAR_TS);
    a.td = h->series(RSCM_TL_VAR_TD);
    if (h->noise_kind) {   // (rscm_ens_set_forcing_noise*; step_launch refuses a linked or fused launch of such a handle)
        a.noise_on = rscm::noise_code(h->noise_kind, false);
        a.noise_seed = h->noise_seed;
        a.noise_sigma = h->noise_sigma;
        a.noise_phi = h->noise_phi;
        a.noise_member0 = h->noise_offset;
        if (h->noise_red()) {   // e at the index before this launch's first comes from the cache if it stands there
            const int32_t t0 = step_begin + a.src_off;
            a.noise_state = h->d_noise_state;
            a.noise_on = rscm::noise_code(h->noise_kind, t0 > 0 && h->noise_state_index == t0 - 1);
        }
    }
    a.year_facts = two_layer_year_facts(h, a, pair);
}
rscm::TwoLayerArgs block_of(const rscm::TwoLayerArgs& a, int32_t begin, int32_t end, int64_t m0, int64_t count)
{
    rscm::TwoLayerArgs c = a;
    c.n_members = count;
    c.step_begin = begin;
    c.step_end = end;
    c.lds_forcing = rscm::two_layer_fits_lds(a.n_scen, a.n_comp, end - begin) ? 1 : 0;
    c.params = a.params + m0;   // every row moves with the block, a mix handle's coefficient rows and the noise rows included (stride N)
    if (a.scen) c.scen = a.scen + m0;
    c.ts = a.ts + m0;
    c.td = a.td + m0;
    c.status = a.status + m0;
    c.noise_member0 = a.noise_member0 + m0;   // the kernel counts members from the block's first: the noise is a function of the id in the ensemble
    // noise that keeps state: a block's first chunk carries the run's decision, every later one loads what the chunk before it stored
    // (run_member_split issues the chunks of one block on one stream, in order)
    if (rscm::noise_keeps_state(a.noise_on)) {
        c.noise_state = a.noise_state + m0;
        if (begin != a.step_begin) c.noise_on = rscm::noise_code(rscm::noise_kind(a.noise_on), true);
    }
    return c;
}

void fill_coupled(const rscm_ens* h, int32_t step_begin, int32_t step_end, rscm::CoupledArgs& a)
{
    fill_common(h, step_begin, step_end, a);
    a.row_stride = h->N;
    a.n_scen = h->n_scen;
    a.lds_forcing = (size_t)h->n_scen * (size_t)(step_end - step_begin) * sizeof(double) <= (size_t)rscm::kMaxLds - 1024 ? 1 : 0;
    a.emissions = h->d_forcing;
    a.scen = h->d_scen;
    a.nsub_tl = h->d_nsub_tl;
    a.nsub_cc = h->d_nsub_cc;
    a.h_tl = h->h_tl;
    a.h_cc = h->h_cc;
    a.ts = h->series(RSCM_CP_VAR_TS);
    a.td = h->series(RSCM_CP_VAR_TD);
    a.conc = h->series(RSCM_CP_VAR_CONC);
    a.cum_uptake = h->series(RSCM_CP_VAR_CUM_UPTAKE);
    a.cum_emis = h->series(RSCM_CP_VAR_CUM_EMIS);
    a.erf_co2 = h->series(RSCM_CP_VAR_ERF_CO2);
    a.erf_total = h->series(RSCM_CP_VAR_ERF);
}
rscm::CoupledArgs block_of(const rscm::CoupledArgs& a, int32_t begin, int32_t end, int64_t m0, int64_t count)
{
    rscm::CoupledArgs c = a;
    c.n_members = count;
    c.step_begin = begin;
    c.step_end = end;
    c.lds_forcing = (size_t)a.n_scen * (size_t)(end - begin) * sizeof(double) <= (size_t)rscm::kMaxLds - 1024 ? 1 : 0;
    c.params = a.params + m0;
    if (a.scen) c.scen = a.scen + m0;
    c.ts = a.ts + m0; c.td = a.td + m0; c.conc = a.conc + m0; c.cum_uptake = a.cum_uptake + m0; c.cum_emis = a.cum_emis + m0;
    c.erf_co2 = a.erf_co2 + m0; c.erf_total = a.erf_total + m0;
    c.status = a.status + m0;
    return c;
}

int fill_udeb(const rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::UdebArgs& a)
{
    if (!h->udeb_ready) return fail(RSCM_ERR_STATE, "ClimateUDEB parameters not configured");
    fill_common(h, step_begin, step_end, a);
    a.row_stride = h->N;
    a.n_total = h->N;
    a.n_scen = h->n_scen;
    a.n_layers = h->udeb_n_layers;
    a.steps_per_year = h->udeb_steps;
    a.land_hc = h->udeb_land_hc;
    a.efficacy_apply = h->udeb_efficacy;
    a.fast = h->mode == RSCM_MODE_FAST ? 1 : 0;
    a.derived = h->d_derived;
    a.derived_uniform = (h->uniform_rows & rscm::udeb_derive_sources()) == rscm::udeb_derive_sources() ? 1 : 0;
    a.erf = h->d_forcing;
    a.link = linked ? links.row[0] : nullptr;
    a.scen = linked ? nullptr : h->d_scen;
    a.bounds = h->d_bounds;
    a.win_kfull = h->d_win_kfull;
    a.win_partw = h->d_win_partw;
    if (h->udeb_tables.size() != (size_t)6 * h->udeb_n_layers) return fail(RSCM_ERR_STATE, "ClimateUDEB tables not built");
    if (rscm::udeb_layers_unrolled(h->udeb_n_layers))   // by value, in the kernel-argument segment (rows past n_layers stay zero)
        memcpy(a.tables, h->udeb_tables.data(), h->udeb_tables.size() * sizeof(double));
    if (!rscm::udeb_layers_fixed(h->udeb_n_layers)) {
        if (!h->d_udeb_tables || !h->d_udeb_work || h->udeb_work_layers() < h->udeb_n_layers)
            return fail(RSCM_ERR_STATE, "ClimateUDEB work arrays for %d layers not allocated", h->udeb_n_layers);
        a.tables_dev = h->d_udeb_tables;
        a.work = h->d_udeb_work;
    }
    a.ocean = h->d_ocean;
    a.scal = h->d_scal;
    a.hist = h->d_hist;
    a.st0 = h->series(RSCM_UD_VAR_ST_NH_OCEAN);
    a.st1 = h->series(RSCM_UD_VAR_ST_NH_LAND);
    a.st2 = h->series(RSCM_UD_VAR_ST_SH_OCEAN);
    a.st3 = h->series(RSCM_UD_VAR_ST_SH_LAND);
    a.heat_uptake = h->series(RSCM_UD_VAR_HEAT_UPTAKE);
    a.ohc = h->series(RSCM_UD_VAR_OHC);
    a.sst = h->series(RSCM_UD_VAR_SST);
    return RSCM_OK;
}
rscm::UdebArgs block_of(const rscm::UdebArgs& a, int32_t begin, int32_t end, int64_t m0, int64_t count)
{
    rscm::UdebArgs c = a;
    c.n_members = count;
    c.step_begin = begin;
    c.step_end = end;
    c.params = a.params + m0;
    c.derived = a.derived + m0;
    if (a.scen) c.scen = a.scen + m0;
    c.ocean = a.ocean + m0; c.scal = a.scal + m0; c.hist = a.hist + m0;
    if (a.work) c.work = a.work + m0;
    c.st0 = a.st0 + m0; c.st1 = a.st1 + m0; c.st2 = a.st2 + m0; c.st3 = a.st3 + m0;
    c.heat_uptake = a.heat_uptake + m0; c.ohc = a.ohc + m0; c.sst = a.sst + m0;
    c.status = a.status + m0;
    return c;
}

void fill_ghg(const rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::GhgArgs& a)
{
    fill_common(h, step_begin, step_end, a);
    a.rows = h->rows;
    a.method = h->ghg_method;
    a.derived = h->d_derived;
    a.derived_uniform = (h->uniform_rows & rscm::ghg_derive_sources(h->ghg_method)) == rscm::ghg_derive_sources(h->ghg_method) ? 1 : 0;
    a.tables = h->d_ghg_tables;
    a.scen = h->d_scen;
    a.conc = h->d_forcing;
    a.links = links;
    a.linked = linked;
    a.erf_co2 = h->series(RSCM_GH_VAR_ERF_CO2);
    a.erf_ch4 = h->series(RSCM_GH_VAR_ERF_CH4);
    a.erf_n2o = h->series(RSCM_GH_VAR_ERF_N2O);
}

void fill_pointwise(const rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::PointwiseArgs& a)
{
    fill_common(h, step_begin, step_end, a);
    a.rows = h->rows;
    a.kind = h->kind;
    a.inputs = h->d_forcing;
    a.scen = h->d_scen;
    a.links = links;
    a.linked = linked;
    a.n_inputs_used = h->ag_rows_set;
    for (int32_t k = 0; k < rscm::kMaxLinks && k < h->n_inputs; ++k)
        if (h->links[k].src) a.n_inputs_used = std::max(a.n_inputs_used, k + 1);
    a.out = h->series(1);
}

void fill_chem(const rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::ChemArgs& a)
{
    fill_common(h, step_begin, step_end, a);
    a.kind = h->kind;
    a.inputs = h->d_forcing;
    a.scen = h->d_scen;
    a.bounds = h->d_bounds;
    a.links = links;
    a.linked = linked;
    a.conc = h->series(RSCM_CHEM_VAR_CONC);
    a.lifetime = h->series(RSCM_CHEM_VAR_LIFETIME);
}

void fill_carbon(const rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::CarbonArgs& a)
{
    fill_common(h, step_begin, step_end, a);
    a.kind = h->kind;
    a.derived = h->d_derived;   // (TerrestrialCarbon only; nullptr for the other two kinds)
    a.derived_uniform = (h->uniform_rows & rscm::terrestrial_derive_sources()) == rscm::terrestrial_derive_sources() ? 1 : 0;
    a.inputs = h->d_forcing;
    a.scen = h->d_scen;
    a.links = links;
    a.linked = linked;
    a.bounds = h->d_bounds;
    a.nsub = h->d_nsub_cc;
    a.h = h->h_cc;
    a.h_half = h->h_cc / 2.0;
    a.h_sixth = h->h_cc / 6.0;
    a.rows = h->rows;
    a.series = h->series(1);
}

// (part -1 and rebuild 0: a launch that neither belongs to a split tile nor re-forms the running sums; ocean_advance decides)
void fill_ocean(const rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::OceanArgs& a)
{
    fill_common(h, step_begin, step_end, a);
    a.steps = h->ocean_steps;
    a.fused = h->mode == RSCM_MODE_FAST ? 1 : 0;
    a.max_hist = h->ocean_max_hist;
    a.inputs = h->d_forcing;
    a.scen = h->d_scen;
    a.bounds = h->d_bounds;
    a.links = links;
    a.linked = linked;
    a.irf = h->d_ocean_irf;
    a.hist = h->d_ocean_hist;
    a.hist_rows = (int32_t)h->ocean_hist_rows;
    a.partial = h->d_ocean_partial;
    a.part = -1;
    a.recur = (h->mode == RSCM_MODE_FAST && h->ocean_recur_ok) ? 1 : 0;
    if (a.recur) {
        a.near = h->ocean_near;
        a.modes = h->ocean_modes;
        a.mode_state = h->d_ocean_mode_state;
        a.mode_table = h->d_ocean_mode_table;
    }
    a.rows = h->rows;
    a.series = h->series(1);
}
// What the handle remembers from one OceanCarbon launch to the next, advanced for the launch `a` describes; its part and rebuild follow.
// The running mode sums (FAST with the fitted modes) stand at a time index: a launch that starts elsewhere re-forms them from the
// history.  One step at a time (linked graphs, Model::step): the steps are paired up so that the history is read once per two steps,
// as the two-year tiles of a whole run do -- the first parks its sums for the second in d_ocean_partial.
void ocean_advance(rscm_ens* h, rscm::OceanArgs& a)
{
    const int32_t tile_years = rscm::kOceanSplitYears, tile_base = h->ocean_tile_base;
    h->ocean_tile_base = -1;
    if (a.recur) {
        a.rebuild = h->ocean_modes_at == a.step_begin ? 0 : 1;
        h->ocean_modes_at = a.step_end;
        return;
    }
    h->ocean_modes_at = -1;  // this launch does not advance the running sums
    if (a.step_end - a.step_begin != 1 || !h->d_ocean_partial) return;
    const int32_t p = a.step_begin - tile_base;
    if (tile_base >= 0 && h->ocean_tile_years == tile_years && p > 0 && p < tile_years) {
        a.part = p;                                   // the next year of the tile in flight
        if (p < tile_years - 1) h->ocean_tile_base = tile_base;
    } else if (a.step_begin + tile_years <= h->T - 1) {  // all its steps exist: start a tile here
        a.part = 0;
        h->ocean_tile_base = a.step_begin;
        h->ocean_tile_years = tile_years;
    }
}

void fill_halo(const rscm_ens* h, int32_t step_begin, int32_t step_end, rscm::HaloArgs& a)
{
    fill_common(h, step_begin, step_end, a);
    a.emissions = h->d_forcing;
    a.scen = h->d_scen;
    a.bounds = h->d_bounds;
    a.rows = h->rows;
    a.series = h->series(1);
}

// `a` as one launch, or -- a whole-axis run of a large ensemble -- as two member blocks in chunks of steps (block_of beside each builder)
template <class Args, class Launch>
int launch_whole_or_split(rscm_ens* h, const Args& a, bool linked, bool halves, Launch launch)
{
    const MemberSplit ms = plan_member_split(h, a.step_begin, a.step_end, linked, halves);
    if (!ms.on) {
        HIPCHK(launch(a, h->stream));
        return RSCM_OK;
    }
    return run_member_split(h, ms, a.step_begin, a.step_end, [&](int32_t b, int32_t e, int64_t m0, int64_t cnt, hipStream_t st) {
        return launch(block_of(a, b, e, m0, cnt), st);
    });
}

}  // namespace

extern "C" {

void set_fail_chunk_launch(int32_t k) { t_fail_chunk = k; }

// What every launch of the two-layer kernels takes from the handle (step_launch here, the fused run + likelihood of loglik_host.cpp)
rscm::TwoLayerArgs two_layer_args(const rscm_ens* h, int32_t step_begin, int32_t step_end)
{
    rscm::TwoLayerArgs a{};
    fill_two_layer(h, step_begin, step_end, rscm::InputLinks{}, 0, a);
    return a;
}

// The launch -- or, with op_out, its arguments for the group kernel (csrc/group.hip): nothing is launched, the handle is not touched.
int step_launch(rscm_ens* h, int32_t step_begin, int32_t step_end, const rscm::InputLinks& links, int32_t linked, rscm::GroupOp* op_out)
{
    const rscm::Family family = h->info().family;
    if (h->n_comp > 0 && (linked || op_out))   // (rscm_ens_link_input and rscm_ens_run_lockstep refuse the handle before this)
        return fail(RSCM_ERR_INVALID, "a mix handle runs on its own: no linked input, no lock-step launch");
    if (h->noise_kind && (linked || op_out))   // (likewise refused before this)
        return fail(RSCM_ERR_INVALID, "a handle with forcing noise runs on its own: no linked input, no lock-step launch");
    if (op_out) {  // the step range is an argument of the fused launch, not part of the table
        if (!can_fuse(h)) return fail(RSCM_ERR_STATE, "this handle (kind %d) cannot be fused", h->kind);
        op_out->kind = h->kind;
        switch (family) {
            case rscm::Family::TwoLayer:
                fill_two_layer(h, 0, 0, links, linked, op_out->u.tl);
                op_out->u.tl.lds_forcing = 0;
                op_out->variant = h->mode;
                break;
            case rscm::Family::Ghg: fill_ghg(h, 0, 0, links, linked, op_out->u.ghg); op_out->variant = h->ghg_method; break;
            case rscm::Family::Chem: fill_chem(h, 0, 0, links, linked, op_out->u.chem); break;
            case rscm::Family::Carbon:
                fill_carbon(h, 0, 0, links, linked, op_out->u.carbon);
                op_out->variant = h->kind == RSCM_KIND_CARBON_CYCLE ? h->mode : 0;
                break;
            default: fill_pointwise(h, 0, 0, links, linked, op_out->u.pw); break;
        }
        return RSCM_OK;
    }
    h->last_blocks = h->last_chunks = 1;
    const int32_t mode = h->mode;
    switch (family) {
        case rscm::Family::TwoLayer: {
            // the pair lane's constants are formed here, for the run that uses them, and stated to every chunk alike
            const bool pair = step_end > step_begin && pair_lane_wanted(h, step_begin, step_end, linked);
            if (pair)
                if (int rc = ensure_pair_constants(h)) return rc;
            rscm::TwoLayerArgs a{};
            fill_two_layer(h, step_begin, step_end, links, linked, a, pair);
            // the noise cache is dropped while the run is issued and stands at the run's last index only if all of it was
            if (step_end > step_begin) h->noise_state_index = -1;
            // (a chunk of a cut run states the facts of its own steps: one step of another length costs one chunk the uniform year)
            if (int rc = launch_whole_or_split(h, a, linked != 0, false, [mode, h, pair](const rscm::TwoLayerArgs& c, hipStream_t st) {
                    rscm::TwoLayerArgs d = c;
                    d.year_facts = two_layer_year_facts(h, d, pair);
                    // (the constants move with the block like every per-member row: its first member is d.params - h->d_params)
                    return rscm::launch_two_layer(d, mode, st, pair ? h->d_derived.get() + (d.params - h->d_params.get()) : nullptr);
                }))
                return rc;
            if (rscm::noise_keeps_state(a.noise_on) && step_end > step_begin && h->noise_cache_kept()) h->noise_state_index = step_end - 1 + a.src_off;
            return RSCM_OK;
        }
        case rscm::Family::Coupled: {
            rscm::CoupledArgs a{};
            fill_coupled(h, step_begin, step_end, a);
            return launch_whole_or_split(h, a, false, false, [mode](const rscm::CoupledArgs& c, hipStream_t st) { return rscm::launch_coupled(c, mode, st); });
        }
        case rscm::Family::Udeb: {
            // (ClimateUDEB runs one wavefront per SIMD, so "rounds" of 65 536 members: halves even out best -- 1e5 members x 750 years
            // 106 -> 86 ms, 2e5 213 -> 168 ms, nothing to gain at 125 000 = 1.91 rounds; scripts/multi_stream_udeb.py)
            rscm::UdebArgs a{};
            if (int rc = fill_udeb(h, step_begin, step_end, links, linked, a)) return rc;
            return launch_whole_or_split(h, a, linked != 0, /*halves=*/true, [](const rscm::UdebArgs& c, hipStream_t st) { return rscm::launch_udeb(c, st); });
        }
        case rscm::Family::Ghg: { rscm::GhgArgs a{}; fill_ghg(h, step_begin, step_end, links, linked, a); HIPCHK(rscm::launch_ghg(a, h->stream)); break; }
        case rscm::Family::Pointwise: { rscm::PointwiseArgs a{}; fill_pointwise(h, step_begin, step_end, links, linked, a); HIPCHK(rscm::launch_pointwise(a, h->stream)); break; }
        case rscm::Family::Chem: { rscm::ChemArgs a{}; fill_chem(h, step_begin, step_end, links, linked, a); HIPCHK(rscm::launch_chem(a, h->stream)); break; }
        case rscm::Family::Carbon: { rscm::CarbonArgs a{}; fill_carbon(h, step_begin, step_end, links, linked, a); HIPCHK(rscm::launch_carbon(a, mode, h->stream)); break; }
        case rscm::Family::Ocean: {
            if (!h->ocean_ready) return fail(RSCM_ERR_STATE, "OceanCarbon parameters not configured");
            rscm::OceanArgs a{};
            fill_ocean(h, step_begin, step_end, links, linked, a);
            ocean_advance(h, a);
            HIPCHK(rscm::launch_ocean(a, h->stream));
            break;
        }
        case rscm::Family::Halo: { rscm::HaloArgs a{}; fill_halo(h, step_begin, step_end, a); HIPCHK(rscm::launch_halocarbon(a, h->stream)); break; }
    }
    return RSCM_OK;
}

// ---- (5) bookkeeping after the launch: time index, strided outputs, room for the next step ----
int step_finish(rscm_ens* h, int32_t step_begin, int32_t step_end)
{
    const int32_t keep = h->keep_rows();
    h->time_index = step_end;
    h->rows_written();
    if (h->windowed && step_end > step_begin) {
        if (h->n_out > 0)
            for (int32_t t = step_begin + 1; t <= step_end; ++t)
                if (int rc = window_store_row(h, t)) return rc;
        // make room for the next step now: consumers that run before this producer in the next step
        // resolve their links against the window as it will be when they read
        if (step_end + 1 >= h->win0 + h->rows && step_end < h->T - 1)
            if (int rc = window_slide(h, step_end - keep + 1)) return rc;
    }
    return RSCM_OK;
}

// One launch of the kind's kernel over [step_begin, step_end).  `timed` brackets it with the events
// rscm_ens_last_run_ms reads; the lock-step loop of rscm_ens_run_lockstep leaves them out.
int run_range(rscm_ens* h, int32_t step_begin, int32_t step_end, bool timed)
{
    NEED(h);
    if (int rc = step_check(h, step_begin, step_end, false)) return rc;
    if (int rc = step_window_pre(h, step_begin, step_end)) return rc;
    rscm::InputLinks links{};
    int32_t linked = 0;
    if (int rc = step_links(h, step_begin, step_end, links, linked)) return rc;
    if (timed) HIPCHK(hipEventRecord(h->ev0, h->stream));
    if (int rc = ensure_derived(h)) return rc;   // (after the first event: rscm_ens_last_run_ms includes the derive launch)
    if (int rc = step_launch(h, step_begin, step_end, links, linked, nullptr)) return rc;
    if (int rc = step_finish(h, step_begin, step_end)) return rc;
    if (timed) {
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        h->timed = true;
    }
    return RSCM_OK;
}

}  // extern "C"
