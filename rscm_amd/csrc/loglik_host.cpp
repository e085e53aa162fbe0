// The Gaussian likelihood's host side: the stored path (rscm_ens_loglik*, and the tables the samplers of sampler_host.cpp score with:
// one validator, one table builder, one kernel -- loglik_kernel, ensemble_ops.hip) and the fused two-layer run + likelihood
// (rscm_ens_run_loglik*; kernels: two_layer.hip).  Reference periods: DESIGN.md section 7.
#include "ens.hpp"

extern "C" {

int check_reference(int32_t T, int32_t n_ref, const int32_t* ref_owner, const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end,
                    const int32_t* ref_stride)
{
    if (n_ref < 0 || (n_ref > 0 && (!ref_var || !ref_begin || !ref_end || !ref_stride))) return fail(RSCM_ERR_INVALID, "bad reference-period arrays");
    for (int32_t e = 0; e < n_ref; ++e) {
        if (ref_begin[e] < 0 || ref_end[e] > T || ref_begin[e] >= ref_end[e] || ref_stride[e] < 1)
            return fail(RSCM_ERR_INVALID, "reference period %d: bad time range [%d, %d) stride %d (at least one row)", e, ref_begin[e], ref_end[e],
                        ref_stride[e]);
        for (int32_t k = 0; k < e; ++k)
            if (ref_var[k] == ref_var[e] && (!ref_owner || ref_owner[k] == ref_owner[e])) return fail(RSCM_ERR_INVALID, "reference period %d: variable %d has a period already", e, ref_var[e]);
    }
    return RSCM_OK;
}

int resolve_loglik_rows(rscm_ens* const* handles, int32_t n_handles, bool whole_series, const ObsList& o, const RefList& r, LoglikRows* out)
{
    if (o.n < 0 || (o.n > 0 && (!o.var || !o.tidx || !o.value || !o.sigma))) return fail(RSCM_ERR_INVALID, "bad observation arrays");
    if (int rc = check_reference(handles[0]->T, r.n, r.owner, r.var, r.begin, r.end, r.stride)) return rc;
    auto obs_owner = [&](int32_t j) { return o.owner ? o.owner[j] : 0; };
    auto ref_owner = [&](int32_t e) { return r.owner ? r.owner[e] : 0; };
    *out = LoglikRows();
    out->grp.resize((size_t)o.n);
    out->obs_ref.assign((size_t)o.n, -1);
    out->ref_off.assign((size_t)r.n + 1, 0);
    for (int32_t j = 0; j < o.n; ++j) {
        if (o.owner && (o.owner[j] < 0 || o.owner[j] >= n_handles)) return fail(RSCM_ERR_INVALID, "observation %d: owner %d out of range", j, o.owner[j]);
        const rscm_ens* h = handles[obs_owner(j)];
        // (a handle's own likelihood reads a diagnostic's rows like any others; the samplers' evaluators are run afresh for every score)
        if (!(whole_series ? o.var[j] >= 1 && o.var[j] < h->V : h->has_rows(o.var[j])))
            return fail(RSCM_ERR_INVALID, "observation %d: variable %d has no stored series", j, o.var[j]);
        if (!whole_series)
            if (int rc = check_diagnostic_current(h, o.var[j])) return rc;
        if (o.tidx[j] < 0 || o.tidx[j] >= h->T) return fail(RSCM_ERR_INVALID, "observation %d: time index %d out of range", j, o.tidx[j]);
        if (!whole_series && o.tidx[j] > h->time_index) out->uncomputed = true;  // NaN there -> skipped by extract_outputs -> missing time -> Err
        out->last_row = std::max(out->last_row, o.tidx[j]);
        // one contiguous run per (owner, variable), as the host likelihood requires: the kernel closes a partial sum at every change of
        // group, so an interleaved order would change the association of the sum (likelihood.rs:206-248)
        const bool same = j > 0 && obs_owner(j) == obs_owner(j - 1) && o.var[j] == o.var[j - 1];
        if (j > 0 && !same)
            for (int32_t k = 0; k < j; ++k)
                if (obs_owner(k) == obs_owner(j) && o.var[k] == o.var[j])
                    return o.owner ? fail(RSCM_ERR_INVALID, "observation %d: the observations of (handle %d, variable %d) must be contiguous", j,
                                          o.owner[j], o.var[j])
                                   : fail(RSCM_ERR_INVALID, "observations must be grouped by variable");
        // the group id: the index of the run's first observation (unique per (owner, variable) whatever the variable count)
        out->grp[(size_t)j] = same ? out->grp[(size_t)j - 1] : j;
    }
    for (int32_t e = 0; e < r.n; ++e) {
        if (r.owner && (r.owner[e] < 0 || r.owner[e] >= n_handles)) return fail(RSCM_ERR_INVALID, "reference period %d: owner %d out of range", e, r.owner[e]);
        const rscm_ens* h = handles[ref_owner(e)];
        if (whole_series) {  // (a handle's own likelihood reports such a variable as one without observation)
            if (r.var[e] < 1 || r.var[e] >= h->V) return fail(RSCM_ERR_INVALID, "reference period %d: variable %d has no stored series", e, r.var[e]);
            if (r.end[e] > h->T) return fail(RSCM_ERR_INVALID, "reference period %d: rows beyond the owner's axis", e);
        }
        bool observed = false;
        for (int32_t j = 0; j < o.n; ++j)
            if (obs_owner(j) == ref_owner(e) && o.var[j] == r.var[e]) {
                out->obs_ref[(size_t)j] = e;
                observed = true;
            }
        if (!observed) return fail(RSCM_ERR_INVALID, "reference period %d: variable %d has no observation", e, r.var[e]);
        for (int32_t t = r.begin[e]; t < r.end[e]; t += r.stride[e]) {
            if (!whole_series && t > h->time_index) out->uncomputed = true;  // a reference row not yet computed: as an observation there
            out->last_row = std::max(out->last_row, t);
        }
    }
    if (out->uncomputed) return RSCM_OK;  // every member scores -inf: no row is read
    auto row = [&](const rscm_ens* h, int32_t var, int32_t t) -> const double* {
        return whole_series ? h->series(var) + (size_t)t * h->N : h->row_ptr(var, t);
    };
    for (int32_t j = 0; j < o.n; ++j) {
        const double* p = row(handles[obs_owner(j)], o.var[j], o.tidx[j]);
        if (!p)
            return fail(RSCM_ERR_STATE, "observation %d: row %d of variable %d is not resident (NO_SERIES handle, or outside the window and the output stride)",
                        j, o.tidx[j], o.var[j]);
        out->obs_rows.push_back(p);
    }
    for (int32_t e = 0; e < r.n; ++e) {
        for (int32_t t = r.begin[e]; t < r.end[e]; t += r.stride[e]) {
            const double* p = row(handles[ref_owner(e)], r.var[e], t);
            if (!p)
                return fail(RSCM_ERR_STATE, "reference period %d: row %d of variable %d is not resident (NO_SERIES handle, or outside the window and the output stride)",
                            e, t, r.var[e]);
            out->ref_rows.push_back(p);
        }
        out->ref_off[(size_t)e + 1] = (int32_t)out->ref_rows.size();
    }
    return RSCM_OK;
}

int upload_loglik(LoglikRows& rows, const ObsList& o, int64_t n_members, double* out, hipStream_t stream, rscm::DevBuf<unsigned char>& d_blob,
                  rscm::LoglikArgs* args)
{
    const size_t sz_ptr = (size_t)o.n * sizeof(double*), sz_rptr = rows.ref_rows.size() * sizeof(double*), sz_d = (size_t)o.n * sizeof(double),
                 sz_i = (size_t)o.n * sizeof(int32_t), sz_off = rows.ref_off.size() * sizeof(int32_t);
    const size_t off_rptr = sz_ptr, off_val = off_rptr + sz_rptr, off_sig = off_val + sz_d, off_grp = off_sig + sz_d, off_ref = off_grp + sz_i,
                 off_off = off_ref + sz_i;
    std::vector<unsigned char>& blob = rows.staging;
    blob.assign(off_off + sz_off + 8, 0);
    if (o.n > 0) {
        memcpy(blob.data(), rows.obs_rows.data(), sz_ptr);
        memcpy(blob.data() + off_val, o.value, sz_d);
        memcpy(blob.data() + off_sig, o.sigma, sz_d);
        memcpy(blob.data() + off_grp, rows.grp.data(), sz_i);
        memcpy(blob.data() + off_ref, rows.obs_ref.data(), sz_i);
    }
    if (sz_rptr > 0) memcpy(blob.data() + off_rptr, rows.ref_rows.data(), sz_rptr);
    memcpy(blob.data() + off_off, rows.ref_off.data(), sz_off);
    HIPCHK(d_blob.alloc(blob.size()));
    // enqueued, not waited for: the launch follows on the same stream and the caller synchronises once (rows.staging lives until then)
    HIPCHK(hipMemcpyAsync(d_blob.get(), blob.data(), blob.size(), hipMemcpyHostToDevice, stream));
    const char* d = (const char*)d_blob.get();
    args->n_members = n_members;
    args->n_obs = o.n;
    args->normalize = o.normalize ? 1 : 0;
    args->obs_series = (const double* const*)d;
    args->ref_rows = (const double* const*)(d + off_rptr);
    args->obs_value = (const double*)(d + off_val);
    args->obs_sigma = (const double*)(d + off_sig);
    args->obs_group = (const int32_t*)(d + off_grp);
    args->obs_ref = rows.ref_rows.empty() ? nullptr : (const int32_t*)(d + off_ref);   // null: no period, the period-free instantiation
    args->ref_off = (const int32_t*)(d + off_off);
    args->out = out;
    return RSCM_OK;
}

// Gaussian log-likelihood of every member from the rows the handle holds, into h->d_loglik (device), synchronised before return.
static int loglik_on_device(rscm_ens* h, const ObsList& o, const RefList& r)
{
    LoglikRows rows;
    if (int rc = resolve_loglik_rows(&h, 1, false, o, r, &rows)) return rc;
    if (int rc = set_device(h)) return rc;
    HIPCHK(h->d_loglik.reserve((size_t)h->N));
    if (rows.uncomputed) {
        HIPCHK(rscm::launch_fill(h->d_loglik, h->N, -std::numeric_limits<double>::infinity(), h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return RSCM_OK;
    }
    rscm::DevBuf<unsigned char> d_blob;
    rscm::LoglikArgs a{};
    if (int rc = upload_loglik(rows, o, h->N, h->d_loglik, h->stream, d_blob, &a)) return rc;
    HIPCHK(rscm::launch_loglik(a, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
}

// the four entry points of the stored path: the result to the host (out) or left on the device (out_dev)
static int stored_loglik(rscm_ens* h, const ObsList& o, const RefList& r, double* out, void** out_dev)
{
    if (int rc = loglik_on_device(h, o, r)) return rc;
    if (out) HIPCHK(hipMemcpy(out, h->d_loglik, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost));
    else *out_dev = h->d_loglik;
    return RSCM_OK;
}

int rscm_ens_loglik(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                    const double* obs_value, const double* obs_sigma, int32_t normalize, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    return stored_loglik(h, {n_obs, nullptr, obs_var, obs_tidx, obs_value, obs_sigma, normalize}, {}, out, nullptr);
    GUARD_END
}

int rscm_ens_loglik_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                           const double* obs_value, const double* obs_sigma, int32_t normalize, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    return stored_loglik(h, {n_obs, nullptr, obs_var, obs_tidx, obs_value, obs_sigma, normalize}, {}, nullptr, out_dev);
    GUARD_END
}

int rscm_ens_loglik_ref(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx, const double* obs_value,
                        const double* obs_sigma, int32_t normalize, int32_t n_ref, const int32_t* ref_var, const int32_t* ref_begin,
                        const int32_t* ref_end, const int32_t* ref_stride, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    return stored_loglik(h, {n_obs, nullptr, obs_var, obs_tidx, obs_value, obs_sigma, normalize},
                         {n_ref, nullptr, ref_var, ref_begin, ref_end, ref_stride}, out, nullptr);
    GUARD_END
}

int rscm_ens_loglik_ref_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx, const double* obs_value,
                               const double* obs_sigma, int32_t normalize, int32_t n_ref, const int32_t* ref_var, const int32_t* ref_begin,
                               const int32_t* ref_end, const int32_t* ref_stride, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    return stored_loglik(h, {n_obs, nullptr, obs_var, obs_tidx, obs_value, obs_sigma, normalize},
                         {n_ref, nullptr, ref_var, ref_begin, ref_end, ref_stride}, nullptr, out_dev);
    GUARD_END
}

// ---------------------------------------------------------------------------------------------
// Fused two-layer run + likelihood
// ---------------------------------------------------------------------------------------------
// Validate a set of observations for the fused run+likelihood kernel and keep it on the device
// (h->d_obs): groups of one variable each, ascending time indices inside a group.
int prepare_obs(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                const double* obs_value, const double* obs_sigma, int32_t normalize)
{
    if (h->kind != RSCM_KIND_TWO_LAYER) return fail(RSCM_ERR_INVALID, "run_loglik supports the two-layer kind");
    if (h->windowed) return fail(RSCM_ERR_INVALID, "run_loglik writes no series: use a plain or RSCM_FLAG_NO_SERIES handle, not a windowed one");
    if (n_obs < 0 || (n_obs > 0 && (!obs_var || !obs_tidx || !obs_value || !obs_sigma)))
        return fail(RSCM_ERR_INVALID, "bad observation arrays");
    const int32_t first_var = n_obs > 0 ? obs_var[0] : RSCM_TL_VAR_TS;
    for (int32_t j = 0; j < n_obs; ++j) {
        if (obs_var[j] != RSCM_TL_VAR_TS && obs_var[j] != RSCM_TL_VAR_TD)
            return fail(RSCM_ERR_INVALID, "observation %d: variable %d has no stored series", j, obs_var[j]);
        if (obs_tidx[j] < 0 || obs_tidx[j] >= h->T) return fail(RSCM_ERR_INVALID, "observation %d: time index %d out of range", j, obs_tidx[j]);
        if (j > 0 && obs_var[j] != obs_var[j - 1] && obs_var[j] == first_var)
            return fail(RSCM_ERR_INVALID, "observations must be grouped by variable");
        if (j > 0 && obs_var[j] == obs_var[j - 1] && obs_tidx[j] < obs_tidx[j - 1])
            return fail(RSCM_ERR_INVALID, "run_loglik needs ascending time indices inside a variable group "
                                          "(use rscm_ens_run + rscm_ens_loglik for arbitrary order)");
    }
    if (int rc = set_device(h)) return rc;
    // merge the (at most two) groups by time index; ties keep the first group's variable first
    std::vector<int32_t> order(n_obs);
    for (int32_t j = 0; j < n_obs; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return obs_tidx[x] < obs_tidx[y]; });
    const size_t sz_i = (size_t)n_obs * sizeof(int32_t), sz_d = (size_t)n_obs * sizeof(double);
    std::vector<unsigned char> blob(2 * sz_d + 2 * sz_i + 16);
    double* bv = (double*)blob.data();
    double* bs = bv + n_obs;
    int32_t* bt = (int32_t*)(bs + n_obs);
    int32_t* bd = bt + n_obs;
    for (int32_t k = 0; k < n_obs; ++k) {
        const int32_t j = order[k];
        bv[k] = obs_value[j];
        bs[k] = obs_sigma[j];
        bt[k] = obs_tidx[j];
        bd[k] = obs_var[j] == RSCM_TL_VAR_TD ? 1 : 0;
    }
    HIPCHK(hipStreamSynchronize(h->stream));  // a launch may still be reading the previous plan
    HIPCHK(h->d_loglik.reserve((size_t)h->N));
    // rewritten where it stands while it is large enough; a larger table is built aside and moved in once it is written, so a
    // failure leaves the previous observations prepared, whole
    rscm::DevBuf<unsigned char> d_grown;
    if (h->d_obs.size() < blob.size()) HIPCHK(d_grown.alloc(blob.size()));
    HIPCHK(hipMemcpy(d_grown ? d_grown : h->d_obs, blob.data(), blob.size(), hipMemcpyHostToDevice));
    if (d_grown) h->d_obs = std::move(d_grown);
    h->obs_merged_tidx.assign(bt, bt + n_obs);
    h->obs_merged_deep.assign(bd, bd + n_obs);
    h->ref_active = false;
    h->ref_last_row = 0;
    h->obs_n = n_obs;
    h->obs_last_tidx = 0;
    for (int32_t j = 0; j < n_obs; ++j) h->obs_last_tidx = std::max(h->obs_last_tidx, obs_tidx[j]);
    h->obs_normalize = normalize ? 1 : 0;
    h->obs_first_is_deep = first_var == RSCM_TL_VAR_TD ? 1 : 0;
    return RSCM_OK;
}

int prepare_ref(rscm_ens* h, int32_t n_ref, const int32_t* ref_var, const int32_t* ref_begin, const int32_t* ref_end, const int32_t* ref_stride)
{
    h->ref_active = false;
    h->ref_last_row = 0;
    if (int rc = check_reference(h->T, n_ref, nullptr, ref_var, ref_begin, ref_end, ref_stride)) return rc;
    if (n_ref == 0) return RSCM_OK;
    rscm::TwoLayerRefArgs r{};
    for (int32_t e = 0; e < n_ref; ++e) {
        if (ref_var[e] != RSCM_TL_VAR_TS && ref_var[e] != RSCM_TL_VAR_TD)
            return fail(RSCM_ERR_INVALID, "reference period %d: variable %d has no stored series", e, ref_var[e]);
        const int32_t v = ref_var[e] == RSCM_TL_VAR_TD ? 1 : 0;
        if (std::find(h->obs_merged_deep.begin(), h->obs_merged_deep.end(), v) == h->obs_merged_deep.end())
            return fail(RSCM_ERR_INVALID, "reference period %d: variable %d has no observation", e, ref_var[e]);
        r.on[v] = 1;
        r.begin[v] = ref_begin[e];
        r.stride[v] = ref_stride[e];
        r.count[v] = (ref_end[e] - ref_begin[e] + ref_stride[e] - 1) / ref_stride[e];
        r.last[v] = ref_begin[e] + (r.count[v] - 1) * ref_stride[e];
        h->ref_last_row = std::max(h->ref_last_row, r.last[v]);
    }
    // an observation of a variable with a period, at a row up to the period's last, waits in the scratch for its variable's b
    std::vector<int32_t> slot((size_t)h->obs_n, -1);
    int32_t n_defer = 0;
    for (int32_t k = 0; k < h->obs_n; ++k) {
        const int32_t v = h->obs_merged_deep[(size_t)k];
        if (r.on[v] && h->obs_merged_tidx[(size_t)k] <= r.last[v]) slot[(size_t)k] = n_defer++;
    }
    if (int rc = set_device(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));  // a launch may still be using the previous layout
    // (ref_active is off from the first line on: a failure below leaves a handle that scores without reference periods and
    // launches on neither buffer.)  The slot table grows as the observation table does; the scratch, [n_defer][N], in place
    rscm::DevBuf<int32_t> d_grown;
    if (h->d_ref_slot.size() < slot.size()) HIPCHK(d_grown.alloc(slot.size()));
    HIPCHK(hipMemcpy(d_grown ? d_grown : h->d_ref_slot, slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (d_grown) h->d_ref_slot = std::move(d_grown);
    HIPCHK(h->d_defer.reserve((size_t)n_defer * (size_t)h->N));
    r.obs_slot = h->d_ref_slot;
    r.defer = h->d_defer;
    h->ref = r;
    h->ref_active = true;
    return RSCM_OK;
}

// Asynchronous fused run+likelihood launch with the prepared observations; fills h->d_loglik.
hipError_t launch_loglik(rscm_ens* h)
{
    // Steps after the last observed index cannot change ln L (GaussianLikelihood reads the model at the
    // observation times only, likelihood.rs:206-226): a caller that uses nothing but ln L -- the device
    // sampler -- lets the launch end there (1850-2020 observations on a 1750-2500 axis: 270 of 750 steps).
    // With reference periods (prepare_ref) "observed" includes the reference rows.
    const int32_t last_read = h->ref_active ? std::max(h->obs_last_tidx, h->ref_last_row) : h->obs_last_tidx;
    const int32_t len = h->loglik_stop_at_last_obs ? std::max(1, std::min(h->T - 1, last_read)) : h->T - 1;
    rscm::TwoLayerArgs a = two_layer_args(h, 0, len);
    a.n_obs = h->obs_n;
    a.normalize = h->obs_normalize;
    a.first_is_deep = h->obs_first_is_deep;
    a.obs_value = (const double*)h->d_obs.get();
    a.obs_sigma = a.obs_value + h->obs_n;
    a.obs_tidx = (const int32_t*)(a.obs_sigma + h->obs_n);
    a.obs_is_deep = a.obs_tidx + h->obs_n;
    a.loglik = h->d_loglik;
    h->rows_written();   // the fused run rewrites the stored rows (and a sampler's proposals the parameter block before it)
    if (h->ref_active) return rscm::launch_two_layer_loglik_ref(a, h->ref, h->mode, h->stream);
    return rscm::launch_two_layer_loglik(a, h->mode, h->stream);
}

static int run_loglik_impl(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                           const double* obs_value, const double* obs_sigma, int32_t normalize, double* out_host, int32_t n_ref = 0,
                           const int32_t* ref_var = nullptr, const int32_t* ref_begin = nullptr, const int32_t* ref_end = nullptr,
                           const int32_t* ref_stride = nullptr)
{
    if (h->noise_kind)
        return fail(RSCM_ERR_INVALID, "the fused run + likelihood is not available on a handle with forcing noise (rscm_ens_set_forcing_noise): "
                                      "run it and score the stored series with rscm_ens_loglik*");
    if (int rc = prepare_obs(h, n_obs, obs_var, obs_tidx, obs_value, obs_sigma, normalize)) return rc;
    if (n_ref != 0)
        if (int rc = prepare_ref(h, n_ref, ref_var, ref_begin, ref_end, ref_stride)) return rc;
    if (int rc = check_loglik_ready(h)) return rc;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    HIPCHK(launch_loglik(h));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    if (out_host) HIPCHK(hipMemcpyAsync(out_host, h->d_loglik, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timed = true;
    return RSCM_OK;
}

int rscm_ens_run_loglik(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                        const double* obs_value, const double* obs_sigma, int32_t normalize, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    return run_loglik_impl(h, n_obs, obs_var, obs_tidx, obs_value, obs_sigma, normalize, out);
    GUARD_END
}

int rscm_ens_run_loglik_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                               const double* obs_value, const double* obs_sigma, int32_t normalize, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (int rc = run_loglik_impl(h, n_obs, obs_var, obs_tidx, obs_value, obs_sigma, normalize, nullptr)) return rc;
    *out_dev = h->d_loglik;
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_run_loglik_ref(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx, const double* obs_value,
                            const double* obs_sigma, int32_t normalize, int32_t n_ref, const int32_t* ref_var, const int32_t* ref_begin,
                            const int32_t* ref_end, const int32_t* ref_stride, double* out)
{
    GUARD_BEGIN
    NEED(h);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    return run_loglik_impl(h, n_obs, obs_var, obs_tidx, obs_value, obs_sigma, normalize, out, n_ref, ref_var, ref_begin, ref_end, ref_stride);
    GUARD_END
}

int rscm_ens_run_loglik_ref_device(rscm_ens* h, int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx, const double* obs_value,
                                   const double* obs_sigma, int32_t normalize, int32_t n_ref, const int32_t* ref_var,
                                   const int32_t* ref_begin, const int32_t* ref_end, const int32_t* ref_stride, void** out_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
    *out_dev = nullptr;
    if (int rc = run_loglik_impl(h, n_obs, obs_var, obs_tidx, obs_value, obs_sigma, normalize, nullptr, n_ref, ref_var, ref_begin, ref_end,
                                 ref_stride))
        return rc;
    *out_dev = h->d_loglik;
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
