// A handle's state in time: initial values and state rows, the time index, the internal component state of a checkpoint, the branch
// (members of one handle copied into another at the source's time index), rewind and the clears.
#include "ens.hpp"

extern "C" {

int rscm_ens_set_initial(rscm_ens* h, int32_t var_id, const double* values, int64_t n_values)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (!values || (n_values != 1 && n_values != h->N))
        return fail(RSCM_ERR_INVALID, "initial values: need 1 or n_members values, got %lld", (long long)n_values);
    if (int rc = set_device(h)) return rc;
    if (h->windowed) {
        if (h->win0 != 0)
            if (int rc = window_reset(h, false)) return rc;
        h->row0_saved = false;  // saved again when step 0 starts
    }
    if (n_values == 1)
        HIPCHK(rscm::launch_fill(h->series(var_id), h->N, values[0], h->stream));
    else
        HIPCHK(hipMemcpyAsync(h->series(var_id), values, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->initial_set[var_id] = 1;
    h->initial_written();   // (not put_at(0): ens.hpp, at the rules)
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_state(rscm_ens* h, int32_t var_id, int32_t tidx, const double* values, int64_t n_values)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (h->windowed ? (tidx < h->win0 || tidx >= h->win0 + h->rows) : (tidx < 0 || tidx >= h->rows))
        return fail(RSCM_ERR_INVALID, h->windowed ? "time index %d is outside the stored window (move the stepper there first: rscm_ens_set_time_index)"
                                                   : "time index %d out of range", tidx);
    if (!values || (n_values != 1 && n_values != h->N))
        return fail(RSCM_ERR_INVALID, "state values: need 1 or n_members values, got %lld", (long long)n_values);
    if (int rc = set_device(h)) return rc;
    if (h->windowed && tidx == 0) h->row0_saved = false;
    double* row = h->series(var_id) + (size_t)tidx * h->N;
    if (n_values == 1)
        HIPCHK(rscm::launch_fill(row, h->N, values[0], h->stream));
    else
        HIPCHK(hipMemcpyAsync(row, values, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (tidx == 0) h->initial_set[var_id] = 1;
    h->rows_written();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_time_index(rscm_ens* h, int32_t tidx)
{
    GUARD_BEGIN
    NEED(h);
    if (tidx < 0 || tidx > (h->windowed ? h->T : h->rows) - 1) return fail(RSCM_ERR_INVALID, "time index %d out of range", tidx);
    // kinds whose components keep internal state in the reference (ComponentState: the UDEB ocean
    // columns, the OceanCarbon flux history) can only continue from where that state stands
    if (h->info().internal_state && tidx != 0 && tidx != h->time_index)
        return fail(RSCM_ERR_STATE, "this kind carries internal component state on the device: the time index can "
                                    "only be rewound to 0 or left at %d", h->time_index);
    if (tidx > 0) h->mark_states_set();   // a restored checkpoint carries its own state rows
    if (h->windowed && tidx != h->time_index) {
        if (int rc = set_device(h)) return rc;
        if (int rc = window_seek(h, tidx)) return rc;
    }
    h->put_at(tidx);
    return RSCM_OK;
    GUARD_END
}

// A checkpoint's internal component state: the runs of h->state_runs(k) (internal_state.hpp) one after the other, every row N doubles
int rscm_ens_internal_state_size(rscm_ens* h, int64_t* n_doubles)
{
    NEED(h);
    if (!n_doubles) return fail(RSCM_ERR_INVALID, "n_doubles is NULL");
    *n_doubles = h->state_runs(h->time_index).rows() * h->N;
    return RSCM_OK;
}

int rscm_ens_get_internal_state(rscm_ens* h, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    for (const rscm::StateRun& r : h->state_runs(h->time_index)) {
        HIPCHK(hipMemcpyAsync(out, h->state_buf(r.buf) + r.first * h->N, (size_t)(r.count * h->N) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        out += r.count * h->N;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_internal_state(rscm_ens* h, const double* in, int64_t n_doubles, int32_t time_index)
{
    GUARD_BEGIN
    NEED(h);
    if (time_index < 0 || time_index > (h->windowed ? h->T : h->rows) - 1) return fail(RSCM_ERR_INVALID, "time index %d out of range", time_index);
    if (!h->internal_ready()) return fail(RSCM_ERR_STATE, "set the parameters first: they size the internal state");
    const rscm::StateRuns runs = h->state_runs(time_index);
    const int64_t n = runs.rows() * h->N;
    if (n != n_doubles) return fail(RSCM_ERR_INVALID, "internal state at time index %d is %lld doubles, got %lld", time_index, (long long)n, (long long)n_doubles);
    if (n > 0 && !in) return fail(RSCM_ERR_INVALID, "in is NULL");
    if (int rc = set_device(h)) return rc;
    for (const rscm::StateRun& r : runs) {
        HIPCHK(hipMemcpyAsync(h->state_buf(r.buf) + r.first * h->N, in, (size_t)(r.count * h->N) * sizeof(double), hipMemcpyHostToDevice, h->stream));
        in += r.count * h->N;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (time_index > 0) h->mark_states_set();
    if (h->windowed && time_index != h->time_index)
        if (int rc = window_seek(h, time_index)) return rc;
    h->put_at(time_index);
    return RSCM_OK;
    GUARD_END
}

// ---- branching: members of one handle copied into another at the source's time index (ABI minor 10) ----
namespace {

struct GatherRow { const void* src; void* dst; int32_t elem_bytes; };

// Rows that follow each other at one pair of strides become one piece; the pieces go out kMaxGatherPieces per launch.
int gather_launch(const std::vector<GatherRow>& rows, int64_t src_N, int64_t dst_N, const int64_t* d_anc, int64_t count, hipStream_t stream)
{
    rscm::GatherBatch batch;
    memset((void*)&batch, 0, sizeof batch);
    int32_t n = 0;
    auto flush = [&]() -> hipError_t {
        const hipError_t e = n > 0 ? rscm::launch_gather_members(batch, n, d_anc, count, src_N, stream) : hipSuccess;
        n = 0;
        return e;
    };
    for (const GatherRow& r : rows) {
        if (n > 0) {
            rscm::GatherPiece& g = batch.pieces[n - 1];
            if (g.elem_bytes == r.elem_bytes) {
                const int64_t ds = ((const char*)r.src - (const char*)g.src) / r.elem_bytes, dd = ((char*)r.dst - (char*)g.dst) / r.elem_bytes;
                if (g.rows == 1 && ds > 0 && dd > 0) {
                    g.src_stride = ds; g.dst_stride = dd; g.rows = 2;
                    continue;
                }
                if (g.rows > 1 && ds == g.src_stride * g.rows && dd == g.dst_stride * g.rows && g.rows < (1 << 20)) {
                    ++g.rows;
                    continue;
                }
            }
        }
        if (n == rscm::kMaxGatherPieces) HIPCHK(flush());
        rscm::GatherPiece& g = batch.pieces[n++];
        g.src = r.src; g.dst = r.dst; g.src_stride = src_N; g.dst_stride = dst_N; g.rows = 1; g.elem_bytes = r.elem_bytes;
    }
    HIPCHK(flush());
    return RSCM_OK;
}

}  // namespace

int rscm_ens_gather_members(rscm_ens* dst, int64_t dst_offset, rscm_ens* src, const int64_t* anc, int32_t on_device, int64_t count)
{
    GUARD_BEGIN
    NEED(dst);
    NEED(src);
    if (dst == src) return fail(RSCM_ERR_INVALID, "source and destination are the same handle");
    if (count < 0 || dst_offset < 0 || dst_offset > dst->N || count > dst->N - dst_offset)
        return fail(RSCM_ERR_INVALID, "members [%lld, %lld + %lld) are outside the destination's %lld", (long long)dst_offset,
                    (long long)dst_offset, (long long)count, (long long)dst->N);
    if (count > 0 && !anc) return fail(RSCM_ERR_INVALID, "ancestors are NULL");
    if (dst->kind != src->kind) return fail(RSCM_ERR_INVALID, "kinds differ: destination %d, source %d", dst->kind, src->kind);
    if (dst->n_comp != src->n_comp)
        return fail(RSCM_ERR_INVALID, "the forcing component counts differ: destination %d, source %d", dst->n_comp, src->n_comp);
    if (dst->noise_rows != src->noise_rows)
        return fail(RSCM_ERR_INVALID, "one handle has the noise parameter rows (RSCM_FLAG_NOISE_PARAMS) and the other has not: destination %d, source %d",
                    (int)dst->noise_rows, (int)src->noise_rows);
    if (dst->device != src->device) return fail(RSCM_ERR_INVALID, "the handles live on devices %d and %d", dst->device, src->device);
    if (dst->T != src->T || memcmp(dst->bounds.data(), src->bounds.data(), src->bounds.size() * sizeof(double)) != 0)
        return fail(RSCM_ERR_INVALID, "the time axes differ");
    if (dst->mode != src->mode) return fail(RSCM_ERR_INVALID, "the arithmetic modes differ");
    if (memcmp(&dst->h_tl, &src->h_tl, sizeof(double)) != 0 || memcmp(&dst->h_cc, &src->h_cc, sizeof(double)) != 0)
        return fail(RSCM_ERR_INVALID, "the RK4 step sizes differ");
    if ((!dst->windowed && dst->rows != dst->T) || (!src->windowed && src->rows != src->T))
        return fail(RSCM_ERR_INVALID, "a handle without stored series (RSCM_FLAG_NO_SERIES) cannot be branched");
    if (dst->select || src->select) return fail(RSCM_ERR_STATE, "a select is in flight: rscm_ens_select_end it first");
    if (!src->params_set) return fail(RSCM_ERR_STATE, "the source has no parameters");
    if (!src->internal_ready()) return fail(RSCM_ERR_STATE, "the source is not configured");
    const int32_t k = src->time_index, P = src->P, V = src->V;
    const int32_t t0 = std::max(0, k - src->lookback);
    for (int32_t v = 1; v < V; ++v)
        for (int32_t t = t0; t <= k; ++t)
            if (!src->row_ptr(v, t))
                return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident in the source any more", t, v);
    const bool later = dst->gather_k >= 0 && dst->time_index == dst->gather_k && dst->params_set;   // another block of the same branch
    if (later && dst->gather_k != k)
        return fail(RSCM_ERR_STATE, "the destination was gathered at time index %d, this source stands at %d", dst->gather_k, k);
    if (int rc = set_device(src)) return rc;
    HIPCHK(hipStreamSynchronize(src->stream));
    HIPCHK(hipStreamSynchronize(dst->stream));

    // element 0 of every parameter row of the source: its structural rows are uniform, and they configure the destination
    std::vector<double> p0((size_t)P);
    HIPCHK(hipMemcpy2D(p0.data(), sizeof(double), src->d_params, (size_t)src->N * sizeof(double), sizeof(double), (size_t)P, hipMemcpyDeviceToHost));
    if (later) {
        for (int32_t j = 0; j < P; ++j)
            if (structural_row(src->kind, j) && memcmp(&p0[j], &dst->gather_p0[j], sizeof(double)) != 0)
                return fail(RSCM_ERR_INVALID, "parameter row %d (%s) of this source differs from the one the destination was configured from", j,
                            structural_row(src->kind, j));
        if (src->lookback != dst->lookback) return fail(RSCM_ERR_INVALID, "the look-back of this source differs from the destination's");
    }

    // the ancestors on the device, checked there before anything is written
    rscm::DevBuf<int64_t> d_tmp;
    rscm::DevBuf<int32_t> d_flag;
    const int64_t* d_anc = anc;
    if (count > 0) {
        if (!on_device) {
            HIPCHK(d_tmp.alloc((size_t)count));
            HIPCHK(hipMemcpyAsync(d_tmp.get(), anc, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, dst->stream));
            d_anc = d_tmp.get();
        }
        int32_t bad = 0;
        HIPCHK(d_flag.alloc(1));
        HIPCHK(hipMemsetAsync(d_flag.get(), 0, sizeof(int32_t), dst->stream));
        HIPCHK(rscm::launch_ancestors_check(d_anc, count, src->N, d_flag.get(), dst->stream));
        HIPCHK(hipMemcpyAsync(&bad, d_flag.get(), sizeof bad, hipMemcpyDeviceToHost, dst->stream));
        HIPCHK(hipStreamSynchronize(dst->stream));
        if (bad) return fail(RSCM_ERR_INVALID, "an ancestor is outside [0, %lld)", (long long)src->N);
    }

    if (!later) {
        // the destination takes the configuration the source derived from its structural rows, wherever its own state stands
        if (int rc = configure_kind(dst, {p0.data(), 1, 0, 1}, /*state_replaced=*/true)) return rc;
        dst->ghg_method = src->ghg_method;   // (the one the source runs with, should its caller have rewritten the row on the device)
        dst->lookback = src->lookback;
        if (dst->windowed) {
            if (dst->rows < 2 * dst->keep_rows())
                return fail(RSCM_ERR_INVALID, "the destination's window of %d rows is too short for a look-back of %d rows", dst->rows, dst->lookback);
            if (int rc2 = window_seek(dst, k)) return rc2;
            if (k == 0) dst->row0_saved = false;
        }
        dst->gather_p0 = p0;
    }
    if (dst->windowed && (t0 < dst->win0 || k >= dst->win0 + dst->rows))
        return fail(RSCM_ERR_STATE, "rows %d..%d do not lie in the destination's window [%d, %d)", t0, k, dst->win0, dst->win0 + dst->rows);

    std::vector<GatherRow> rows;
    for (int32_t j = 0; j < P; ++j)
        rows.push_back({src->d_params + (size_t)j * src->N, dst->d_params + (size_t)j * dst->N + dst_offset, 8});
    for (int32_t t = t0; t <= k; ++t)
        for (int32_t v = 1; v < V; ++v)
            rows.push_back({src->row_ptr(v, t), dst->series(v) + (size_t)t * dst->N + dst_offset, 8});
    if (src->kind == RSCM_KIND_OCEAN_CARBON && (dst->ocean_hist_rows != src->ocean_hist_rows || dst->ocean_steps != src->ocean_steps))
        return fail(RSCM_ERR_INVALID, "the flux-history rings differ: %lld and %lld rows", (long long)dst->ocean_hist_rows, (long long)src->ocean_hist_rows);
    // the internal state: the same rows of the same buffers on both sides (OceanCarbon: the pulses sit at the same ring positions)
    for (const rscm::StateRun& run : src->state_runs(k))
        for (int64_t r = run.first; r < run.first + run.count; ++r)
            rows.push_back({src->state_buf(run.buf) + (size_t)r * src->N, dst->state_buf(run.buf) + (size_t)r * dst->N + dst_offset, 8});
    rows.push_back({src->d_status, dst->d_status + dst_offset, 1});
    if (count > 0)
        if (int rc = gather_launch(rows, src->N, dst->N, d_anc, count, dst->stream)) return rc;
    HIPCHK(hipStreamSynchronize(dst->stream));

    // rows that hold one value for every member: only those that did in the source and, for a later block, hold the same bits as before
    uint64_t uni = src->uniform_rows;
    if (later) {
        uni &= dst->uniform_rows;
        for (int32_t j = 0; j < P && j < 64; ++j)
            if (memcmp(&p0[j], &dst->gather_p0[j], sizeof(double)) != 0) uni &= ~(1ull << j);
    } else if (dst_offset != 0)
        uni = 0;   // element 0, which the kernels read for such a row, is not among the members written
    dst->params_written(uni);
    dst->params_set = true;
    dst->mark_states_set();
    dst->put_at(k);
    dst->gather_k = k;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_rewind(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (h->windowed) {
        if (int rc = set_device(h)) return rc;
        if (int rc = window_reset(h, false)) return rc;
    }
    h->put_at(0);
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_clear_series(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = set_device(h)) return rc;
    if (h->windowed) {
        if (int rc = window_reset(h, true)) return rc;
        if (h->d_out)
            HIPCHK(rscm::launch_fill(h->d_out, (int64_t)h->n_out * h->out_rows * h->N, std::numeric_limits<double>::quiet_NaN(), h->stream));
    } else if (h->rows > 1)
        for (int32_t v = 1; v < h->V; ++v)
            HIPCHK(rscm::launch_fill(h->series(v) + h->N, (int64_t)(h->rows - 1) * h->N,
                                     std::numeric_limits<double>::quiet_NaN(), h->stream));
    h->put_at(0);
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_clear_rows_after(rscm_ens* h, int32_t tidx)
{
    GUARD_BEGIN
    NEED(h);
    if (tidx < 0 || tidx > h->T - 1) return fail(RSCM_ERR_INVALID, "time index %d out of range", tidx);
    if (int rc = set_device(h)) return rc;
    if (h->windowed) {
        const int32_t first = std::max(0, tidx + 1 - h->win0);
        HIPCHK(rscm::launch_fill_rows(h->d_series, h->N, h->rows, h->V - 1, first, std::numeric_limits<double>::quiet_NaN(), h->stream));
    } else if (h->rows == h->T && tidx < h->T - 1)
        for (int32_t v = 1; v < h->V; ++v)
            HIPCHK(rscm::launch_fill(h->series(v) + (size_t)(tidx + 1) * h->N, (int64_t)(h->T - 1 - tidx) * h->N,
                                     std::numeric_limits<double>::quiet_NaN(), h->stream));
    h->rows_written();
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
