// C-ABI layer of the MI355X ensemble runner: the error text, ABI and device queries, handle creation and teardown, the getters,
// streams, parameters, forcing, links, runs and the read-outs, with validation mirroring the reference's error behaviour.  The
// arithmetic of the hot path lives in the .hip kernels; the other concerns of the host layer have translation units of their own
// (ens.hpp lists them).
#include "ens.hpp"

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int alloc_or_fail(rscm::DevBuf<double>& buf, size_t n, bool grow, const char* what, ...)
{
    const hipError_t e = grow ? buf.reserve(n) : buf.alloc(n);
    if (e == hipSuccess) return RSCM_OK;
    char text[256];
    va_list ap;
    va_start(ap, what);
    vsnprintf(text, sizeof text, what, ap);
    va_end(ap);
    return fail(hip_code(e), "%s: %s", text, hipGetErrorString(e));
}

static_assert(rscm::kNoiseStreamTag == RSCM_NOISE_STREAM_TAG, "the noise stream's tag in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(RSCM_NOISE_STREAM_TAG != 0x57A7u && RSCM_NOISE_STREAM_TAG != 0xACCEu && RSCM_NOISE_STREAM_TAG != 0x5EEDu &&
                  RSCM_NOISE_STREAM_TAG != 0xA5A5u && RSCM_NOISE_STREAM_TAG != RSCM_RESAMPLE_STREAM_TAG,
              "every Philox stream of the library has a tag of its own");
static_assert(rscm::kPriorUniform == RSCM_PRIOR_UNIFORM && rscm::kPriorNormal == RSCM_PRIOR_NORMAL && rscm::kPriorLogNormal == RSCM_PRIOR_LOGNORMAL &&
                  rscm::kPriorReflect == RSCM_PRIOR_REFLECT, "the prior kinds in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(rscm::kMaxForcingComponents == RSCM_TL_MAX_COMPONENTS && rscm::kTwoLayerCoeff0 == RSCM_TL_P_COEFF0 && RSCM_TL_P_COEFF0 == RSCM_TL_NPARAMS,
              "the mix handle's constants in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(rscm::kKindOzoneForcing == RSCM_KIND_OZONE_FORCING && rscm::kKindAerosolDirect == RSCM_KIND_AEROSOL_DIRECT &&
                  rscm::kKindAerosolIndirect == RSCM_KIND_AEROSOL_INDIRECT && rscm::kKindCh4Chemistry == RSCM_KIND_CH4_CHEMISTRY &&
                  rscm::kKindN2oChemistry == RSCM_KIND_N2O_CHEMISTRY && rscm::kKindCo2Budget == RSCM_KIND_CO2_BUDGET &&
                  rscm::kKindTerrestrialCarbon == RSCM_KIND_TERRESTRIAL_CARBON && rscm::kKindFourBoxOhu == RSCM_KIND_FOURBOX_OHU &&
                  rscm::kKindOspp == RSCM_KIND_OSPP && rscm::kKindCarbonCycle == RSCM_KIND_CARBON_CYCLE &&
                  rscm::kKindCo2Erf == RSCM_KIND_CO2_ERF && rscm::kKindAggregate == RSCM_KIND_AGGREGATE,
              "rscm_device.hpp and include/rscm_gpu.h disagree on a kind value");

extern "C" {

int rscm_gpu_abi_version(void) { return RSCM_GPU_ABI_VERSION; }
int rscm_gpu_abi_minor(void) { return RSCM_GPU_ABI_MINOR; }

const char* rscm_gpu_last_error(void) { return g_last_error.c_str(); }

int rscm_gpu_device_count(int32_t* out)
{
    GUARD_BEGIN
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out = 0;
        return fail(RSCM_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out = n;
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_mem_info(int32_t device_id, uint64_t* free_bytes, uint64_t* total_bytes)
{
    GUARD_BEGIN
    if (!free_bytes || !total_bytes) return fail(RSCM_ERR_INVALID, "output pointer is NULL");
    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    size_t f = 0, t = 0;
    e = hipMemGetInfo(&f, &t);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "hipMemGetInfo: %s", hipGetErrorString(e));
    *free_bytes = (uint64_t)f;
    *total_bytes = (uint64_t)t;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_create(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                    int32_t device_id, rscm_ens** out)
{
    return rscm_ens_create_ex(kind, n_members, n_times, time_bounds, device_id, 0, out);
}

int rscm_ens_create_ex(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                       int32_t device_id, uint32_t flags, rscm_ens** out)
{
    return rscm_ens_create_windowed(kind, n_members, n_times, time_bounds, device_id, flags, 16, 0, -1, nullptr, out);
}

// n_components > 0: a two-layer mix handle (rscm_ens_create_mix, which has checked kind, flags and the count)
static int create_handle(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds, int32_t device_id, uint32_t flags,
                         int32_t window_rows, int32_t out_stride, int32_t n_out_vars, const int32_t* out_vars, int32_t n_components,
                         rscm_ens** out);

int rscm_ens_create_windowed(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds,
                             int32_t device_id, uint32_t flags, int32_t window_rows, int32_t out_stride,
                             int32_t n_out_vars, const int32_t* out_vars, rscm_ens** out)
{
    return create_handle(kind, n_members, n_times, time_bounds, device_id, flags, window_rows, out_stride, n_out_vars, out_vars, 0, out);
}

int rscm_ens_create_mix(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds, int32_t device_id, uint32_t flags,
                        int32_t n_components, rscm_ens** out)
{
    GUARD_BEGIN
    if (out) *out = nullptr;
    if (kind != RSCM_KIND_TWO_LAYER)
        return fail(RSCM_ERR_INVALID, "forcing components are available for the two-layer kind only (RSCM_KIND_TWO_LAYER), got kind %d", kind);
    if (flags & ~(uint32_t)(RSCM_FLAG_NO_SERIES | RSCM_FLAG_NOISE_PARAMS))
        return fail(RSCM_ERR_INVALID, "a mix handle takes flags 0, RSCM_FLAG_NO_SERIES or RSCM_FLAG_NOISE_PARAMS (no windowed storage), got 0x%x", flags);
    if (n_components < 1 || n_components > RSCM_TL_MAX_COMPONENTS)
        return fail(RSCM_ERR_INVALID, "n_components must be in [1, %d], got %d", RSCM_TL_MAX_COMPONENTS, n_components);
    return create_handle(kind, n_members, n_times, time_bounds, device_id, flags, 16, 0, -1, nullptr, n_components, out);
    GUARD_END
}

static int create_handle(int32_t kind, int64_t n_members, int32_t n_times, const double* time_bounds, int32_t device_id, uint32_t flags,
                         int32_t window_rows, int32_t out_stride, int32_t n_out_vars, const int32_t* out_vars, int32_t n_components,
                         rscm_ens** out)
{
    GUARD_BEGIN
    if (flags & ~(uint32_t)(RSCM_FLAG_NO_SERIES | RSCM_FLAG_WINDOWED | RSCM_FLAG_NOISE_PARAMS)) return fail(RSCM_ERR_INVALID, "unknown flags 0x%x", flags);
    if ((flags & RSCM_FLAG_NOISE_PARAMS) && kind != RSCM_KIND_TWO_LAYER)
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NOISE_PARAMS is only available for the two-layer kind");
    if ((flags & RSCM_FLAG_NOISE_PARAMS) && (flags & (RSCM_FLAG_NO_SERIES | RSCM_FLAG_WINDOWED)))
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NOISE_PARAMS needs a handle that stores its whole series (no RSCM_FLAG_NO_SERIES, no windowed storage): "
                    "the noise that reads the two rows is refused without");
    if ((flags & RSCM_FLAG_NO_SERIES) && kind != RSCM_KIND_TWO_LAYER)
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NO_SERIES is only available for the two-layer kind");
    if ((flags & RSCM_FLAG_NO_SERIES) && (flags & RSCM_FLAG_WINDOWED))
        return fail(RSCM_ERR_INVALID, "RSCM_FLAG_NO_SERIES and RSCM_FLAG_WINDOWED exclude each other");
    const bool windowed = (flags & RSCM_FLAG_WINDOWED) != 0;
    if (windowed && (window_rows < 4 || out_stride < 0 || (n_out_vars > 0 && !out_vars)))
        return fail(RSCM_ERR_INVALID, "a windowed ensemble needs window_rows >= 4, out_stride >= 0 and a variable list if n_out_vars > 0");
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (kind < RSCM_KIND_TWO_LAYER || kind > RSCM_KIND_AGGREGATE)
        return fail(RSCM_ERR_INVALID, "unknown kind %d", kind);
    if (n_members < 1) return fail(RSCM_ERR_INVALID, "n_members must be >= 1, got %lld", (long long)n_members);
    if (n_times < 2) return fail(RSCM_ERR_INVALID, "n_times must be >= 2 (TimeAxis::from_values asserts len >= 2)");
    if (!time_bounds) return fail(RSCM_ERR_INVALID, "time_bounds is NULL");
    for (int32_t i = 0; i < n_times; ++i)
        if (!(time_bounds[i + 1] > time_bounds[i]))  // timeseries.rs:47-52 assert!(is_monotonic)
            return fail(RSCM_ERR_INVALID, "time_bounds must be strictly increasing (index %d)", i);
    if ((uint64_t)n_members > (uint64_t)std::numeric_limits<int32_t>::max() * 256ull)
        return fail(RSCM_ERR_INVALID, "n_members too large for one launch grid");

    std::unique_ptr<rscm_ens> h(new rscm_ens());   // every return before the last goes through ~rscm_ens
    h->kind = kind;
    h->N = n_members;
    h->T = n_times;
    h->rows = (flags & RSCM_FLAG_NO_SERIES) ? 1 : n_times;
    if (windowed && window_rows < n_times) {  // a window as long as the axis is plain full storage
        h->windowed = true;
        h->rows = window_rows;
    }
    h->device = device_id;
    h->P = h->info().n_params;
    h->V = h->info().n_vars;
    h->n_inputs = h->info().n_inputs;
    if (n_components > 0) {   // the coefficients are parameter rows 6 .. 6 + K - 1, the components the K rows of the input block
        h->n_comp = n_components;
        h->P = RSCM_TL_P_COEFF0 + n_components;
        h->n_inputs = n_components;
    }
    if (flags & RSCM_FLAG_NOISE_PARAMS) {   // sigma_i and phi_i follow the six parameters and the coefficients
        h->noise_rows = true;
        h->P += 2;
    }
    h->bounds.assign(time_bounds, time_bounds + n_times + 1);
    h->initial_set.assign(h->V, 0);
    h->out_slot.assign(h->V, -1);
    h->lookback = h->info().lookback;   // (N2O: refreshed by set_params)
    if (h->windowed && out_stride > 0) {
        h->out_stride = out_stride;
        h->out_rows = (n_times - 1) / out_stride + 1;
        if (n_out_vars < 0)
            for (int32_t v = 1; v < h->V; ++v) h->out_vars.push_back(v);
        else
            for (int32_t k = 0; k < n_out_vars; ++k) {
                if (out_vars[k] < 1 || out_vars[k] >= h->V || h->out_slot[out_vars[k]] >= 0)
                    return fail(RSCM_ERR_INVALID, "output variable %d: not a stored variable of this kind, or listed twice", out_vars[k]);
                h->out_slot[out_vars[k]] = k;
                h->out_vars.push_back(out_vars[k]);
            }
        h->n_out = (int32_t)h->out_vars.size();
        for (int32_t k = 0; k < h->n_out; ++k) h->out_slot[h->out_vars[k]] = k;
    }

    hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(RSCM_ERR_DEVICE, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    const size_t series_elems = (size_t)(h->V - 1) * (size_t)h->rows * (size_t)h->N;
    HIPCHK(h->d_params.alloc((size_t)h->P * h->N));
    HIPCHK(h->d_series.alloc(series_elems));
    HIPCHK(h->d_status.alloc((size_t)h->N));
    if (h->windowed) {
        HIPCHK(h->d_row0.alloc((size_t)(h->V - 1) * h->N));
        if (h->n_out > 0) {
            const size_t out_elems = (size_t)h->n_out * h->out_rows * h->N;
            HIPCHK(h->d_out.alloc(out_elems));
            HIPCHK(h->d_out_vars.alloc((size_t)h->n_out));
            HIPCHK(hipMemcpy(h->d_out_vars, h->out_vars.data(), (size_t)h->n_out * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHK(rscm::launch_fill(h->d_out, (int64_t)out_elems, std::numeric_limits<double>::quiet_NaN(), h->stream));
        }
    }
    HIPCHK(h->d_nsub_tl.alloc((size_t)(h->T - 1)));
    HIPCHK(h->d_nsub_cc.alloc((size_t)(h->T - 1)));
    HIPCHK(h->d_partial.alloc(4 * 1024));
    HIPCHK(h->d_out4.alloc(4));
    if (kind == RSCM_KIND_UDEB) {
        HIPCHK(h->d_scal.alloc((size_t)rscm::kUdebScalars * h->N));
        HIPCHK(h->d_hist.alloc((size_t)h->T * h->N));
    }
    if (h->info().needs_bounds) {  // kinds that use the step length
        HIPCHK(h->d_bounds.alloc((size_t)(h->T + 1)));
        HIPCHK(hipMemcpyAsync(h->d_bounds, h->bounds.data(), (size_t)(h->T + 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (kind == RSCM_KIND_AGGREGATE) {  // contributors that are neither linked nor set stay NaN = skipped
        HIPCHK(h->d_forcing.alloc((size_t)h->n_inputs * h->T));
        HIPCHK(rscm::launch_fill(h->d_forcing, (int64_t)h->n_inputs * h->T, std::numeric_limits<double>::quiet_NaN(), h->stream));
        h->n_scen = 1;
        h->forcing_set = true;
    }
    HIPCHK(hipMemsetAsync(h->d_status, 0, (size_t)h->N, h->stream));
    // never-written entries are NaN (builder.rs:772-780)
    HIPCHK(rscm::launch_fill(h->d_series, (int64_t)series_elems, std::numeric_limits<double>::quiet_NaN(),
                         h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h.release();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_destroy(rscm_ens* h)
{
    if (!h) return RSCM_OK;
    if (h->link_refs > 0)
        return fail(RSCM_ERR_STATE, "%d linked input(s) of other ensembles still read this one's series: destroy or unlink them first", h->link_refs);
    (void)hipSetDevice(h->device);
    delete h;
    return RSCM_OK;
}

// What a handle holds that is not device memory; the buffers and then the stream follow (ens.hpp, at the struct).  The stream is
// synchronised here, not in rscm_ens_destroy, so that a handle whose construction failed half-way goes the same way.
rscm_ens::~rscm_ens()
{
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& l : links)
        if (l.src) --l.src->link_refs;
    select_release(this);
    delete plan;
}

int rscm_ens_n_params(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->P; return RSCM_OK; }
int rscm_ens_n_vars(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->V; return RSCM_OK; }
int rscm_ens_n_diagnostics(const rscm_ens* h, int32_t* out) { NEED(h); if (!out) return fail(RSCM_ERR_INVALID, "out is NULL"); *out = h->n_diag; return RSCM_OK; }
int rscm_ens_n_inputs(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->n_inputs; return RSCM_OK; }
int rscm_ens_n_forcing_components(const rscm_ens* h, int32_t* out) { NEED(h); if (!out) return fail(RSCM_ERR_INVALID, "out is NULL"); *out = h->n_comp; return RSCM_OK; }
int rscm_ens_n_members(const rscm_ens* h, int64_t* out) { NEED(h); *out = h->N; return RSCM_OK; }
int rscm_ens_n_times(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->T; return RSCM_OK; }
int rscm_ens_time_index(const rscm_ens* h, int32_t* out) { NEED(h); *out = h->time_index; return RSCM_OK; }

int rscm_ens_set_mode(rscm_ens* h, int32_t mode)
{
    NEED(h);
    if (mode != RSCM_MODE_EXACT && mode != RSCM_MODE_FAST) return fail(RSCM_ERR_INVALID, "unknown mode %d", mode);
    if (mode != h->mode) {  // sums parked / carried by the other arithmetic cannot be resumed
        h->ocean_forget_partial_sums();
    }
    h->mode = mode;
    h->rows_written();   // the next run writes other bits
    return RSCM_OK;
}

int rscm_ens_set_step_size(rscm_ens* h, int32_t component, double step)
{
    NEED(h);
    if (!(step > 0.0) || !std::isfinite(step)) return fail(RSCM_ERR_INVALID, "step must be positive and finite");
    if (component == RSCM_COMP_TWO_LAYER && h->kind != RSCM_KIND_CARBON_CYCLE)
        h->h_tl = step;
    else if (component == RSCM_COMP_CARBON_CYCLE && (h->kind == RSCM_KIND_COUPLED || h->kind == RSCM_KIND_CARBON_CYCLE))
        h->h_cc = step;
    else
        return fail(RSCM_ERR_INVALID, "component %d not part of this model kind", component);
    h->schedule_dirty = true;
    return RSCM_OK;
}

int rscm_gpu_stream_create(int32_t device_id, void** out_stream)
{
    GUARD_BEGIN
    if (!out_stream) return fail(RSCM_ERR_INVALID, "out_stream is NULL");
    HIPCHK(hipSetDevice(device_id));
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out_stream = (void*)s;
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_stream_destroy(int32_t device_id, void* hip_stream)
{
    GUARD_BEGIN
    if (!hip_stream) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    HIPCHK(hipStreamDestroy((hipStream_t)hip_stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_stream(rscm_ens* h, void* hip_stream)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->own_stream) {
        HIPCHK(hipStreamDestroy(h->stream));
        h->own_stream = false;
    }
    if (hip_stream) {
        h->stream = (hipStream_t)hip_stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_params(rscm_ens* h, const double* soa)
{
    GUARD_BEGIN
    NEED(h);
    if (!soa) return fail(RSCM_ERR_INVALID, "params is NULL");
    if (int rc = set_device(h)) return rc;
    if (int rc = configure_kind(h, {soa, h->N, 1, h->N})) return rc;
    if (h->kind == RSCM_KIND_N2O_CHEMISTRY) {  // the look-back of the largest delay among the members
        double d = 1.0;
        for (int64_t i = 0; i < h->N; ++i) d = std::max(d, soa[(size_t)rscm::kN2oDelayRow * h->N + i]);
        const int32_t lookback = n2o_lookback(d);
        // a window that has already slid kept only keep_rows() of the OLD look-back: the rows a longer delay
        // reads are gone (the body would read before the window's first row)
        if (h->windowed && h->win0 > 0 && std::max(0, h->time_index - lookback) < h->win0 && lookback > h->lookback)
            return fail(RSCM_ERR_STATE, "a stratospheric delay that looks %d rows back needs row %d, but the window already starts at row %d: "
                        "rewind (rscm_ens_rewind) or restore a checkpoint before raising the delay", lookback,
                        std::max(0, h->time_index - lookback), h->win0);
        h->lookback = lookback;
    }
    HIPCHK(hipMemcpyAsync(h->d_params, soa, (size_t)h->P * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    uint64_t uni = 0;   // rows that hold the same bits for every member
    for (int32_t j = 0; j < h->P && j < 64; ++j) {
        const double* row = soa + (size_t)j * h->N;
        bool same = true;
        for (int64_t i = 1; i < h->N && same; ++i) same = memcmp(&row[i], &row[0], sizeof(double)) == 0;
        if (same) uni |= 1ull << j;
    }
    h->params_written(uni);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->params_set = true;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_params_aos(rscm_ens* h, const double* aos)
{
    GUARD_BEGIN
    NEED(h);
    if (!aos) return fail(RSCM_ERR_INVALID, "params is NULL");
    std::vector<double> soa((size_t)h->P * h->N);
    for (int64_t i = 0; i < h->N; ++i)
        for (int32_t j = 0; j < h->P; ++j) soa[(size_t)j * h->N + i] = aos[(size_t)i * h->P + j];
    return rscm_ens_set_params(h, soa.data());
    GUARD_END
}

int rscm_ens_set_forcing(rscm_ens* h, int32_t var_id, int32_t n_scen, const double* series,
                         const int32_t* scenario_of_member, int32_t source)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id != 0) return fail(RSCM_ERR_INVALID, "variable %d is not the shared input of this kind", var_id);
    if (n_scen < 1 || !series) return fail(RSCM_ERR_INVALID, "need n_scen >= 1 and a series pointer");
    if (source != RSCM_SRC_EXOGENOUS && source != RSCM_SRC_UPSTREAM) return fail(RSCM_ERR_INVALID, "unknown source %d", source);
    if (h->kind == RSCM_KIND_COUPLED && source != RSCM_SRC_EXOGENOUS)
        return fail(RSCM_ERR_INVALID, "emissions of the coupled chain are exogenous (no component produces them)");
    if (h->kind == RSCM_KIND_UDEB && source != RSCM_SRC_EXOGENOUS)
        return fail(RSCM_ERR_INVALID, "ClimateUDEB reads its forcing as an exogenous series (at_start / at_end)");
    if (h->kind >= RSCM_KIND_GHG_FORCING && source != RSCM_SRC_EXOGENOUS)
        return fail(RSCM_ERR_INVALID, "the stateless forcing kinds read their inputs as exogenous series");
    if (scenario_of_member)
        for (int64_t i = 0; i < h->N; ++i)
            if (scenario_of_member[i] < 0 || scenario_of_member[i] >= n_scen)
                return fail(RSCM_ERR_INVALID, "scenario_of_member[%lld] = %d out of range [0, %d)", (long long)i,
                            scenario_of_member[i], n_scen);
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->year_facts.drop_forcing();   // from here on the table may change: the verdict on the new one is formed once it stands
    h->forcing_replaced();          // ... and so do the rows of the energy-budget diagnostics that read the forcing (ens.hpp)
    // Tables of the same scenario count are rewritten where they stand.  Tables of another count are built aside and moved in,
    // with n_scen, once they are written: a failure on the way leaves the handle with the tables and the count it had.
    const bool resize = n_scen != h->n_scen || !h->d_forcing;
    rscm::DevBuf<double> d_forcing_new, d_ghg_new;
    rscm::DevBuf<int32_t> d_scen_new;
    if (resize) {
        HIPCHK(d_forcing_new.alloc((size_t)n_scen * h->n_inputs * h->T));
        if (h->kind == RSCM_KIND_GHG_FORCING) HIPCHK(d_ghg_new.alloc((size_t)n_scen * rscm::kGhgRows * h->T));
    }
    double* const d_forcing = resize ? d_forcing_new : h->d_forcing;
    double* const d_ghg = resize ? d_ghg_new : h->d_ghg_tables;
    HIPCHK(hipMemcpyAsync(d_forcing, series, (size_t)n_scen * h->n_inputs * h->T * sizeof(double), hipMemcpyHostToDevice, h->stream));
    std::vector<double> ghg_tab;  // must outlive the copy below (synchronised before return)
    if (h->kind == RSCM_KIND_GHG_FORCING) {
        ghg_tab = ghg_tables(series, n_scen, h->T);
        HIPCHK(hipMemcpyAsync(d_ghg, ghg_tab.data(), ghg_tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (scenario_of_member) {   // (indices into the new tables: never written over the old ones' while those may stay)
        if (resize || !h->d_scen) HIPCHK(d_scen_new.alloc((size_t)h->N));
        HIPCHK(hipMemcpyAsync(d_scen_new ? d_scen_new : h->d_scen, scenario_of_member, (size_t)h->N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (resize) {
        h->d_forcing = std::move(d_forcing_new);
        if (h->kind == RSCM_KIND_GHG_FORCING) h->d_ghg_tables = std::move(d_ghg_new);
    }
    if (d_scen_new || !scenario_of_member) h->d_scen = std::move(d_scen_new);   // (omitted: the members' scenario table goes)
    h->n_scen = n_scen;
    h->source = source;
    h->forcing_set = true;
    if (h->kind == RSCM_KIND_TWO_LAYER && h->n_comp == 0) h->year_facts.set_forcing(series, n_scen, h->T);   // (a plain table: [S][T])
    if (h->kind == RSCM_KIND_AGGREGATE) {  // rows after the last non-NaN one of the block stay out of the sums anyway
        int32_t used = 0;
        for (int32_t sidx = 0; sidx < n_scen; ++sidx)
            for (int32_t k = 0; k < h->n_inputs; ++k)
                for (int32_t t = 0; t < h->T; ++t)
                    if (!std::isnan(series[((size_t)sidx * h->n_inputs + k) * h->T + t])) used = std::max(used, k + 1);
        h->ag_rows_set = used;
    }
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_link_input(rscm_ens* h, int32_t input_row, rscm_ens* src, int32_t src_var, int32_t source)
{
    GUARD_BEGIN
    NEED(h);
    if (!src) return fail(RSCM_ERR_INVALID, "source ensemble is NULL");
    if (src == h) return fail(RSCM_ERR_INVALID, "an ensemble cannot link to itself (its own states are read in the kernel)");
    if (h->kind == RSCM_KIND_COUPLED || h->kind == RSCM_KIND_HALOCARBON)
        return fail(RSCM_ERR_INVALID, "the inputs of this kind cannot be linked (they are exogenous emissions)");
    if (h->n_comp > 0)
        return fail(RSCM_ERR_INVALID, "the forcing components of a mix handle (rscm_ens_create_mix) cannot be linked: they are shared "
                                      "scenario rows scaled per member");
    if (h->noise_kind)
        return fail(RSCM_ERR_INVALID, "a handle with forcing noise (rscm_ens_set_forcing_noise) takes no linked input: the noise is added to "
                                      "its own shared forcing; clear the noise first");
    if (input_row < 0 || input_row >= h->n_inputs || input_row >= rscm::kMaxLinks)
        return fail(RSCM_ERR_INVALID, "input row %d out of range [0, %d)", input_row, h->n_inputs);
    if (src_var < 1 || src_var >= src->V) return fail(RSCM_ERR_INVALID, "variable %d of the source has no stored series", src_var);
    if (source != RSCM_SRC_EXOGENOUS && source != RSCM_SRC_UPSTREAM) return fail(RSCM_ERR_INVALID, "unknown source %d", source);
    if (src->N != h->N || src->T != h->T || src->device != h->device)
        return fail(RSCM_ERR_INVALID, "linked ensembles need the same members, time points and device (%lld x %d on %d vs %lld x %d on %d)",
                    (long long)src->N, src->T, src->device, (long long)h->N, h->T, h->device);
    if ((!src->windowed && src->rows != src->T) || (!h->windowed && h->rows != h->T))
        return fail(RSCM_ERR_INVALID, "linked ensembles must store their series (no RSCM_FLAG_NO_SERIES)");
    if (!h->link_order_check) src->read_ahead = true;
    auto& l = h->links[input_row];
    if (l.src) --l.src->link_refs;
    else ++h->n_linked;
    l.src = src;
    l.var = src_var;
    l.off = source == RSCM_SRC_UPSTREAM ? 1 : 0;
    ++src->link_refs;
    h->forcing_replaced();
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_link_order_check(rscm_ens* h, int32_t enabled)
{
    NEED(h);
    h->link_order_check = enabled != 0;
    if (!h->link_order_check)  // the producers' rows beyond what they have written must read as NaN
        for (auto& l : h->links)
            if (l.src) l.src->read_ahead = true;
    return RSCM_OK;
}

int rscm_ens_unlink_input(rscm_ens* h, int32_t input_row)
{
    NEED(h);
    if (input_row < 0 || input_row >= h->n_inputs || input_row >= rscm::kMaxLinks)
        return fail(RSCM_ERR_INVALID, "input row %d out of range [0, %d)", input_row, h->n_inputs);
    auto& l = h->links[input_row];
    if (l.src) {
        --l.src->link_refs;
        --h->n_linked;
        l = rscm_ens::Link{};
        h->forcing_replaced();
    }
    return RSCM_OK;
}

int rscm_ens_run_async(rscm_ens* h, int32_t step_begin, int32_t step_end)
{
    GUARD_BEGIN
    return run_range(h, step_begin, step_end, true);
    GUARD_END
}

int rscm_ens_sync(rscm_ens* h)
{
    GUARD_BEGIN
    NEED(h);
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_run(rscm_ens* h, int32_t step_begin, int32_t step_end)
{
    if (int rc = rscm_ens_run_async(h, step_begin, step_end)) return rc;
    return rscm_ens_sync(h);
}

int rscm_ens_last_run_plan(rscm_ens* h, int32_t* member_blocks, int32_t* step_chunks)
{
    NEED(h);
    if (member_blocks) *member_blocks = h->last_blocks;
    if (step_chunks) *step_chunks = h->last_chunks;
    return RSCM_OK;
}

int rscm_ens_last_run_ms(rscm_ens* h, float* out_ms)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_ms) return fail(RSCM_ERR_INVALID, "out_ms is NULL");
    if (!h->timed) return fail(RSCM_ERR_STATE, "no run has been launched yet");
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(out_ms, h->ev0, h->ev1));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_get_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride,
                        int64_t m_begin, int64_t m_end, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!h->has_rows(var_id)) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (t_begin < 0 || t_end > h->T || t_begin > t_end || t_stride < 1)
        return fail(RSCM_ERR_INVALID, "bad time range [%d, %d) stride %d", t_begin, t_end, t_stride);
    if (!h->windowed && h->rows != h->T && t_end > 1)
        return fail(RSCM_ERR_STATE, "this handle stores only the initial row (RSCM_FLAG_NO_SERIES)");
    if (m_begin < 0 || m_end > h->N || m_begin > m_end || !out)
        return fail(RSCM_ERR_INVALID, "bad member range [%lld, %lld)", (long long)m_begin, (long long)m_end);
    const bool diagnostic = h->is_diagnostic(var_id);
    if (int rc = check_diagnostic_current(h, var_id)) return rc;
    const int64_t width = m_end - m_begin;
    if (width == 0 || t_begin == t_end) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    if (h->windowed || diagnostic) {  // row by row from wherever each row is resident: the output store or the window; a diagnostic's store
        int64_t r = 0;
        for (int32_t t = t_begin; t < t_end; t += t_stride, ++r) {
            double* dst = out + r * width;
            if (t > h->time_index) {
                for (int64_t m = 0; m < width; ++m) dst[m] = std::numeric_limits<double>::quiet_NaN();
                continue;
            }
            const double* src = h->row_ptr(var_id, t);
            if (!src && diagnostic) {
                (void)hipStreamSynchronize(h->stream);   // the copies enqueued so far read the caller's buffer no longer
                return fail(RSCM_ERR_STATE, "row %d of diagnostic %d is not held: rscm_ens_compute_diagnostic over a range with it first", t, var_id);
            }
            if (!src)
                return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident: the window holds [%d, %d) and the output store every %d-th row%s",
                            t, var_id, h->win0, h->win0 + h->rows, h->out_stride, h->out_slot[var_id] < 0 ? " of other variables" : "");
            HIPCHK(hipMemcpyAsync(dst, src + m_begin, (size_t)width * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        return RSCM_OK;
    }
    // rows beyond the current time index were never computed by this model instance: NaN
    int64_t n_rows = 0, n_valid = 0;
    for (int32_t t = t_begin; t < t_end; t += t_stride) {
        ++n_rows;
        if (t <= h->time_index) ++n_valid;
    }
    if (n_valid > 0)
        HIPCHK(hipMemcpy2DAsync(out, (size_t)width * sizeof(double),
                                h->series(var_id) + (size_t)t_begin * h->N + m_begin,
                                (size_t)h->N * sizeof(double) * (size_t)t_stride, (size_t)width * sizeof(double),
                                (size_t)n_valid, hipMemcpyDeviceToHost, h->stream));
    for (int64_t r = n_valid; r < n_rows; ++r)
        for (int64_t m = 0; m < width; ++m) out[r * width + m] = std::numeric_limits<double>::quiet_NaN();
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_series_devptr(rscm_ens* h, int32_t var_id, void** out)
{
    NEED(h);
    if (!out || var_id < 1 || var_id >= h->V) return fail(RSCM_ERR_INVALID, "variable %d has no stored series", var_id);
    if (h->windowed) return fail(RSCM_ERR_STATE, "a windowed ensemble has no contiguous [T][N] series: read rows with rscm_ens_get_series");
    *out = h->series(var_id);
    return RSCM_OK;
}

int rscm_ens_params_devptr(rscm_ens* h, void** out)
{
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = h->d_params;
    // Whatever the caller writes there, now or later through a pointer it kept: from here on no row of this
    // handle is ever treated as uniform again (rscm_ens_set_params keeps the flag clear as well).
    h->expose_params();   // (and noise_cache_kept() is false from here on; the diagnostics' epoch does not move: rscm_gpu.h)
    h->params_set = true;  // the caller fills it on the device
    return RSCM_OK;
}

int rscm_ens_status(rscm_ens* h, uint8_t* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipMemcpyAsync(out, h->d_status, (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_status_devptr(rscm_ens* h, void** out)
{
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = h->d_status;
    return RSCM_OK;
}

// Everything rscm_ens_run_loglik needs of the handle besides the observations.
int check_loglik_ready(rscm_ens* h)
{
    if (h->time_index != 0) return fail(RSCM_ERR_STATE, "run_loglik starts from time index 0 (call rscm_ens_rewind)");
    if (!h->params_set) return fail(RSCM_ERR_STATE, "parameters not set");
    if (h->n_linked) return fail(RSCM_ERR_STATE, "the fused run+likelihood launch takes no linked inputs: use rscm_ens_run and rscm_ens_loglik");
    if (!h->forcing_set) return fail(RSCM_ERR_STATE, "shared input series not set");
    for (int32_t v = 1; v < h->V; ++v)
        if (h->is_state(v) && !h->initial_set[v])
            return fail(RSCM_ERR_STATE, "state variable %d has no initial value (MissingInitialValue)", v);
    if (int rc = set_device(h)) return rc;
    return refresh_schedule(h);
}

int rscm_gpu_copy_to_device(int32_t device_id, void* device_ptr, const void* host, int64_t n_bytes)
{
    GUARD_BEGIN
    if (n_bytes < 0 || (n_bytes > 0 && (!host || !device_ptr))) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n_bytes == 0) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipMemcpy(device_ptr, host, (size_t)n_bytes, hipMemcpyHostToDevice));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_summary_series(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (var_id < 1 || var_id >= h->V || t_begin < 0 || t_end > h->T || t_begin > t_end || !out)
        return fail(RSCM_ERR_INVALID, "bad variable / time range");
    if (h->windowed || h->rows != h->T) return fail(RSCM_ERR_STATE, "this handle does not store whole series (RSCM_FLAG_NO_SERIES / RSCM_FLAG_WINDOWED): use rscm_ens_summary row by row");
    const int32_t n_rows = t_end - t_begin;
    // rows beyond the current time index have not been computed: empty summaries, as rscm_ens_summary
    const int32_t computed = std::max(0, std::min(t_end, h->time_index + 1) - t_begin);
    for (int32_t r = computed; r < n_rows; ++r) {
        out[4 * r + 0] = 0.0; out[4 * r + 1] = 0.0;
        out[4 * r + 2] = std::numeric_limits<double>::infinity();
        out[4 * r + 3] = -std::numeric_limits<double>::infinity();
    }
    if (computed == 0) return RSCM_OK;
    if (int rc = set_device(h)) return rc;
    const int32_t nb = rscm::summary_blocks(h->N);
    rscm::DevBuf<double> d_partial, d_out;
    HIPCHK(d_partial.alloc((size_t)computed * nb * 4));
    HIPCHK(d_out.alloc((size_t)computed * 4));
    HIPCHK(rscm::launch_summary_rows(h->series(var_id) + (size_t)t_begin * h->N, h->N, computed, d_partial.get(), nb, d_out.get(), h->stream));
    HIPCHK(hipMemcpyAsync(out, d_out.get(), (size_t)computed * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_summary(rscm_ens* h, int32_t var_id, int32_t tidx, double out[4])
{
    GUARD_BEGIN
    NEED(h);
    if (!h->has_rows(var_id) || tidx < 0 || tidx >= h->T || !out)
        return fail(RSCM_ERR_INVALID, "bad variable/time index");
    if (int rc = check_diagnostic_current(h, var_id)) return rc;
    if (tidx > h->time_index) {
        out[0] = 0.0; out[1] = 0.0;
        out[2] = std::numeric_limits<double>::infinity();
        out[3] = -std::numeric_limits<double>::infinity();
        return RSCM_OK;
    }
    if (int rc = set_device(h)) return rc;
    const int32_t nb = rscm::summary_blocks(h->N);
    const double* row = h->row_ptr(var_id, tidx);
    if (!row) return fail(RSCM_ERR_STATE, "row %d of variable %d is not resident on this handle", tidx, var_id);
    HIPCHK(rscm::launch_summary_rows(row, h->N, 1, h->d_partial, nb, h->d_out4, h->stream));
    HIPCHK(hipMemcpyAsync(out, h->d_out4, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_sample_lhs(rscm_ens* h, uint64_t seed, const double* low, const double* high,
                        int64_t member_offset, int64_t n_total)
{
    GUARD_BEGIN
    NEED(h);
    if (!low || !high) return fail(RSCM_ERR_INVALID, "low/high is NULL");
    if (member_offset < 0 || n_total < 1 || member_offset + h->N > n_total)
        return fail(RSCM_ERR_INVALID, "member block [%lld, %lld) outside the global ensemble of %lld",
                    (long long)member_offset, (long long)(member_offset + h->N), (long long)n_total);
    if (int rc = set_device(h)) return rc;
    for (const rscm::StructuralRow& s : rscm::kStructuralRows)   // (N2O's delay is not `uniform`: the look-back is sized for the largest)
        if (s.kind == h->kind && s.uniform && low[s.row] != high[s.row])
            return fail(RSCM_ERR_INVALID, "parameter row %d (%s) is structural: low must equal high", s.row, s.name);
    if (int rc = configure_kind(h, {low, 1, 0, 1})) return rc;   // (low == high in every structural row)
    if (h->kind == RSCM_KIND_N2O_CHEMISTRY) h->lookback = n2o_lookback(high[rscm::kN2oDelayRow]);   // no member draws a larger delay
    rscm::DevBuf<double> d_lh;   // [P] low, then [P] high
    HIPCHK(d_lh.alloc(2 * (size_t)h->P));
    HIPCHK(hipMemcpyAsync(d_lh.get(), low, (size_t)h->P * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_lh.get() + h->P, high, (size_t)h->P * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(rscm::launch_lhs(h->d_params, h->P, h->N, seed, d_lh.get(), d_lh.get() + h->P, member_offset, n_total, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->params_written(0);   // conservatively: low + u (high - low) need not reproduce low's bits for every u
    h->params_set = true;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_sample_lhs_priors(rscm_ens* h, uint64_t seed, const int32_t* kind, const double* a, const double* b, const double* p0,
                               const double* p1, const double* lo, const double* hi, int64_t member_offset, int64_t n_total)
{
    GUARD_BEGIN
    NEED(h);
    if (!kind || !a || !b || !p0 || !p1 || !lo || !hi) return fail(RSCM_ERR_INVALID, "a prior array is NULL");
    if (member_offset < 0 || n_total < 1 || member_offset + h->N > n_total)
        return fail(RSCM_ERR_INVALID, "member block [%lld, %lld) outside the global ensemble of %lld",
                    (long long)member_offset, (long long)(member_offset + h->N), (long long)n_total);
    std::vector<rscm::LhsPriorRow> rows((size_t)h->P);
    bool any_quantile = false;
    for (int32_t j = 0; j < h->P; ++j) {
        const int32_t family = kind[j] & ~RSCM_PRIOR_REFLECT;
        if (family != RSCM_PRIOR_UNIFORM && family != RSCM_PRIOR_NORMAL && family != RSCM_PRIOR_LOGNORMAL)
            return fail(RSCM_ERR_INVALID, "parameter row %d: unknown prior kind %d", j, kind[j]);
        if (family == RSCM_PRIOR_UNIFORM) {
            if (kind[j] != RSCM_PRIOR_UNIFORM) return fail(RSCM_ERR_INVALID, "parameter row %d: RSCM_PRIOR_REFLECT on a uniform row", j);
        } else {
            if (!(b[j] > 0.0) || !std::isfinite(b[j])) return fail(RSCM_ERR_INVALID, "parameter row %d: the scale b must be positive and finite", j);
            if (!(0.0 <= p0[j] && p0[j] < p1[j] && p1[j] <= 1.0)) return fail(RSCM_ERR_INVALID, "parameter row %d: needs 0 <= p0 < p1 <= 1", j);
            if (!(lo[j] <= hi[j])) return fail(RSCM_ERR_INVALID, "parameter row %d: needs lo <= hi", j);
        }
        rows[(size_t)j] = {a[j], b[j], p0[j], p1[j], lo[j], hi[j], kind[j], 0};
        any_quantile |= family != RSCM_PRIOR_UNIFORM;
    }
    if (int rc = set_device(h)) return rc;
    for (const rscm::StructuralRow& s : rscm::kStructuralRows) {   // (N2O's delay is not `uniform`: the look-back is sized for the largest)
        if (s.kind != h->kind) continue;
        if (kind[s.row] != RSCM_PRIOR_UNIFORM)
            return fail(RSCM_ERR_INVALID, "parameter row %d (%s) is structural: its prior must be RSCM_PRIOR_UNIFORM", s.row, s.name);
        if (s.uniform && a[s.row] != b[s.row])
            return fail(RSCM_ERR_INVALID, "parameter row %d (%s) is structural: a must equal b", s.row, s.name);
    }
    if (int rc = configure_kind(h, {a, 1, 0, 1})) return rc;   // (a == b in every structural row)
    if (h->kind == RSCM_KIND_N2O_CHEMISTRY) h->lookback = n2o_lookback(b[rscm::kN2oDelayRow]);   // no member draws a larger delay
    rscm::DevBuf<rscm::LhsPriorRow> d_rows;
    HIPCHK(d_rows.alloc(rows.size()));
    HIPCHK(hipMemcpyAsync(d_rows.get(), rows.data(), rows.size() * sizeof(rscm::LhsPriorRow), hipMemcpyHostToDevice, h->stream));
    HIPCHK(rscm::launch_lhs_priors(h->d_params, h->P, h->N, seed, d_rows.get(), any_quantile, member_offset, n_total, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->params_written(0);   // as rscm_ens_sample_lhs
    h->params_set = true;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_get_params(rscm_ens* h, double* out_soa)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_soa) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipMemcpyAsync(out_soa, h->d_params, (size_t)h->P * h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_copy_to_host(int32_t device_id, void* host, const void* device_ptr, int64_t n_bytes)
{
    GUARD_BEGIN
    if (n_bytes < 0 || (n_bytes > 0 && (!host || !device_ptr))) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n_bytes == 0) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipMemcpy(host, device_ptr, (size_t)n_bytes, hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_host_alloc(int64_t n_bytes, void** out)
{
    GUARD_BEGIN
    if (!out || n_bytes <= 0) return fail(RSCM_ERR_INVALID, "bad arguments");
    *out = nullptr;
    HIPCHK(hipHostMalloc(out, (size_t)n_bytes, hipHostMallocDefault));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_host_free(void* p)
{
    GUARD_BEGIN
    if (p) HIPCHK(hipHostFree(p));
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
