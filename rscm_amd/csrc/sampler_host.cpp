// The device stretch-move sampler behind rscm_sampler_* (kernels: csrc/sampler.hip): what the reference does on the host per
// iteration in EnsembleSampler::run / update_group (crates/rscm-calibrate/src/sampler/ensemble.rs:496-547) driven as launches on
// the evaluator's stream -- one evaluating ensemble (the fused two-layer run+likelihood, or any kind scored from its stored
// series) or a graph of linked ensembles (rscm_sampler_create_graph).
#include "ens.hpp"

extern "C" {

// ---------------------------------------------------------------------------------------------
// Device stretch-move sampler (csrc/sampler.hip)
// ---------------------------------------------------------------------------------------------
struct rscm_sampler {
    rscm_ens* ev = nullptr;  // evaluates one half-ensemble per launch; not owned
    int32_t W = 0, D = 0, groups = 1;
    bool sharded = false;            // driven half-step by half-step with an exchange in between
    int32_t rank = 0, n_ranks = 1;   // sharded: this rank owns half-walkers [rank * n_local, (rank + 1) * n_local) of both halves
    int32_t n_local = 0;             // = members of the evaluator
    rscm::DevBuf<double> d_send;        // [D + 1][n_local]
    rscm::DevBuf<double> d_recv;        // [n_ranks][D + 1][n_local]
    double stretch_a = 2.0;
    uint64_t seed = 0;
    int32_t iteration = 0;
    bool positions_set = false;
    rscm::DevBuf<int32_t> d_rows;
    rscm::DevBuf<int32_t> d_kind;
    rscm::DevBuf<double> d_base;
    rscm::DevBuf<double> d_pa;
    rscm::DevBuf<double> d_pb;
    rscm::DevBuf<double> d_plo;
    rscm::DevBuf<double> d_phi;
    rscm::DevBuf<double> d_pos;
    rscm::DevBuf<double> d_logp;
    rscm::DevBuf<double> d_prop;
    rscm::DevBuf<double> d_z;
    rscm::DevBuf<double> d_lp;
    rscm::DevBuf<int64_t> d_nacc;
    rscm::DevBuf<int64_t> d_nprop;
    // fused: the two-layer run+likelihood kernel scores a half; otherwise the half is run through
    // rscm_ens_run_async (any kind, stored series) and scored by the likelihood kernel
    bool fused = true;
    rscm::DevBuf<unsigned char> d_sobs; // stored path: the tables lik points into (upload_loglik)
    rscm::LoglikArgs lik{};
    // the observations as given at creation (rscm_sampler_set_reference lays the stored path's tables out again)
    std::vector<int32_t> obs_owner, obs_var, obs_tidx;
    std::vector<double> obs_value, obs_sigma;
    int32_t normalize = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // graph evaluator (rscm_sampler_create_graph): every half-step rewinds these handles, runs them in lock-step up
    // to the last observed index and scores the stored series; ev is the first of them
    std::vector<rscm_ens*> graph;
    std::vector<uint64_t> graph_sampled_rows;  // per handle: bit j = parameter row j is written by the proposal kernel
    bool graph_clear = false;                  // NaN the stored rows before every run (graphs in which a consumer runs ahead of its producer)
    int32_t graph_last_step = 0;
    rscm::DevBuf<double*> d_param_ptr;         // [D] device addresses of the sampled rows
    ~rscm_sampler()   // the buffers follow, once nothing on the evaluator's stream reads them any more
    {
        if (ev) (void)hipStreamSynchronize(ev->stream);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    ObsList observations() const
    {
        return {(int32_t)obs_var.size(), graph.empty() ? nullptr : obs_owner.data(), obs_var.data(), obs_tidx.data(), obs_value.data(),
                obs_sigma.data(), normalize};
    }
};

namespace {

rscm::SamplerArgs sampler_args(const rscm_sampler* s, int32_t half, int32_t identity)
{
    rscm::SamplerArgs a{};
    a.n_walkers = s->W;
    a.n_dims = s->D;
    a.n_params = s->ev->P;
    a.n_groups = s->groups;
    a.half = half;
    a.k_offset = s->rank * s->n_local;
    a.n_local = s->n_local;
    a.n_ranks = s->n_ranks;
    a.exchange = nullptr;
    a.iteration = s->iteration;
    a.identity = identity;
    a.seed = s->seed;
    a.stretch_a = s->stretch_a;
    a.param_rows = s->d_rows;
    a.base_params = s->d_base;
    a.prior_kind = s->d_kind;
    a.prior_a = s->d_pa;
    a.prior_b = s->d_pb;
    a.prior_lo = s->d_plo;
    a.prior_hi = s->d_phi;
    a.pos = s->d_pos;
    a.logp = s->d_logp;
    a.proposal = s->d_prop;
    a.z = s->d_z;
    a.lp = s->d_lp;
    a.loglik = s->ev->d_loglik;
    a.eval_params = s->ev->d_params;
    a.param_ptr = s->d_param_ptr;
    a.n_accepted = s->d_nacc;
    a.n_proposed = s->d_nprop;
    return a;
}

// propose (or re-score) one half, evaluate it, accept: all on the evaluator's stream
int sampler_half_step(rscm_sampler* s, int32_t half, int32_t identity)
{
    const rscm::SamplerArgs a = sampler_args(s, half, identity);
    if (!s->graph.empty()) {
        // Model::run of the whole graph for this half's proposals: a fresh collection, the proposal kernel writes each
        // sampled parameter into its owner's block, the graph steps to the last observed index (later steps cannot
        // change ln L), the likelihood kernel reads the observation rows where the owners store them
        for (size_t k = 0; k < s->graph.size(); ++k) {
            rscm_ens* g = s->graph[k];
            g->params_kernel_writes(s->graph_sampled_rows[k]);   // the proposal kernel is about to write its parameter block
            if (int rc = s->graph_clear ? rscm_ens_clear_series(g) : rscm_ens_rewind(g)) return rc;
        }
        HIPCHK(rscm::launch_sampler_propose(a, s->ev->stream));
        if (s->graph_last_step > 0)
            if (int rc = rscm_ens_run_lockstep(s->graph.data(), (int32_t)s->graph.size(), 0, s->graph_last_step)) return rc;
        HIPCHK(rscm::launch_loglik(s->lik, s->ev->stream));
        HIPCHK(rscm::launch_sampler_accept(a, s->ev->stream));
        if (s->sharded) {
            rscm::SamplerArgs p = a;
            p.exchange = s->d_send;
            HIPCHK(rscm::launch_sampler_pack(p, s->ev->stream));
        }
        return RSCM_OK;
    }
    s->ev->params_kernel_writes(~0ull);  // the proposal kernel writes the evaluator's parameter block
    HIPCHK(rscm::launch_sampler_propose(a, s->ev->stream));
    if (s->fused) {
        HIPCHK(launch_loglik(s->ev));
    } else {
        s->ev->put_at(0);  // every evaluation is a fresh Model::run of the half
        if (int rc = rscm_ens_run_async(s->ev, 0, s->ev->T - 1)) return rc;
        s->ev->put_at(0);
        HIPCHK(rscm::launch_loglik(s->lik, s->ev->stream));
    }
    HIPCHK(rscm::launch_sampler_accept(a, s->ev->stream));
    if (s->sharded) {  // this rank's block of the updated half, ready for the all-gather
        rscm::SamplerArgs p = a;
        p.exchange = s->d_send;
        HIPCHK(rscm::launch_sampler_pack(p, s->ev->stream));
    }
    return RSCM_OK;
}

// what both creators ask of the walkers, the ranks and the stretch scale
int check_walkers(int32_t n_walkers, int32_t rank, int32_t n_ranks, double stretch_a)
{
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(RSCM_ERR_INVALID, "bad rank %d of %d", rank, n_ranks);
    if (n_walkers < 2) return fail(RSCM_ERR_INVALID, "Must have at least 2 walkers");          // ensemble.rs:120-127
    if (n_walkers % 2) return fail(RSCM_ERR_INVALID, "Number of walkers must be even");
    if ((n_walkers / 2) % n_ranks)
        return fail(RSCM_ERR_INVALID, "half the walkers (%d) must split evenly over %d ranks", n_walkers / 2, n_ranks);
    if (!(stretch_a > 1.0)) return fail(RSCM_ERR_INVALID, "Stretch move scale parameter must be > 1.0, got %g", stretch_a);  // moves.rs:40-48
    return RSCM_OK;
}

// ... and of the prior of dimension d
int check_prior(int32_t d, const int32_t* prior_kind, const double* prior_a, const double* prior_b, const double* prior_low, const double* prior_high)
{
    if (prior_kind[d] < 0 || prior_kind[d] > 2) return fail(RSCM_ERR_INVALID, "dimension %d: unknown prior kind %d", d, prior_kind[d]);
    if (prior_kind[d] == 0 && !(prior_b[d] > prior_a[d])) return fail(RSCM_ERR_INVALID, "dimension %d: Uniform needs high > low", d);
    if (prior_kind[d] != 0 && !(prior_b[d] > 0.0)) return fail(RSCM_ERR_INVALID, "dimension %d: the scale parameter must be > 0", d);
    if ((prior_low && prior_high) && !(prior_low[d] < prior_high[d])) return fail(RSCM_ERR_INVALID, "dimension %d: Bound needs low < high", d);
    return RSCM_OK;
}

// What both creators set, allocate and upload: the walkers' state, the priors, the exchange buffers, counters and events; the
// observations are kept for rscm_sampler_set_reference.
int sampler_init(rscm_sampler* s, rscm_ens* ev, int32_t n_walkers, int32_t n_dims, const int32_t* prior_kind, const double* prior_a,
                 const double* prior_b, const double* prior_low, const double* prior_high, const ObsList& o, double stretch_a, uint64_t seed,
                 int32_t rank, int32_t n_ranks)
{
    s->ev = ev;
    s->W = n_walkers;
    s->D = n_dims;
    s->rank = rank;
    s->n_ranks = n_ranks;
    s->sharded = n_ranks > 1;
    s->n_local = (int32_t)ev->N;
    s->stretch_a = stretch_a;
    s->seed = seed;
    if (o.n > 0) {
        if (o.owner) s->obs_owner.assign(o.owner, o.owner + o.n);
        s->obs_var.assign(o.var, o.var + o.n);
        s->obs_tidx.assign(o.tidx, o.tidx + o.n);
        s->obs_value.assign(o.value, o.value + o.n);
        s->obs_sigma.assign(o.sigma, o.sigma + o.n);
    }
    s->normalize = o.normalize ? 1 : 0;
    const size_t W = (size_t)n_walkers, H = (size_t)ev->N, D = (size_t)n_dims;  // H: this rank's block of a half
    HIPCHK(s->d_kind.alloc(D));
    HIPCHK(s->d_pa.alloc(D));
    HIPCHK(s->d_pb.alloc(D));
    HIPCHK(s->d_plo.alloc(D));
    HIPCHK(s->d_phi.alloc(D));
    HIPCHK(s->d_pos.alloc(D * W));
    HIPCHK(s->d_logp.alloc(W));
    HIPCHK(s->d_prop.alloc(D * H));
    HIPCHK(s->d_z.alloc(H));
    HIPCHK(s->d_lp.alloc(H));
    HIPCHK(s->d_send.alloc((D + 1) * H));   // 2 x (D + 1) x H doubles: also for one rank (the exchange of
    HIPCHK(s->d_recv.alloc((size_t)n_ranks * (D + 1) * H));   // a one-rank group is a copy)
    HIPCHK(s->d_nacc.alloc(W));
    HIPCHK(s->d_nprop.alloc(W));
    HIPCHK(hipMemcpy(s->d_kind, prior_kind, D * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->d_pa, prior_a, D * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->d_pb, prior_b, D * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> lo(D, -std::numeric_limits<double>::infinity()), hi(D, std::numeric_limits<double>::infinity());
    if (prior_low && prior_high)
        for (size_t d = 0; d < D; ++d) { lo[d] = prior_low[d]; hi[d] = prior_high[d]; }
    HIPCHK(hipMemcpy(s->d_plo, lo.data(), D * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->d_phi, hi.data(), D * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s->d_nacc, 0, W * sizeof(int64_t)));
    HIPCHK(hipMemset(s->d_nprop, 0, W * sizeof(int64_t)));
    HIPCHK(hipEventCreate(&s->ev0));
    HIPCHK(hipEventCreate(&s->ev1));
    return RSCM_OK;
}

// Puts the stored path's table for these resolved rows (of the observations kept in s) in place of the one s holds; the graph steps to
// the last row the likelihood reads.  On failure s keeps its table.
int sampler_install_table(rscm_sampler* s, LoglikRows& rows)
{
    rscm_ens* h = s->ev;
    if (int rc = set_device(h)) return rc;
    rscm::DevBuf<unsigned char> d_new;
    rscm::LoglikArgs a{};
    if (int rc = upload_loglik(rows, s->observations(), h->N, h->d_loglik, h->stream, d_new, &a)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));   // the copy is in, and no launch reads the previous table any more
    s->d_sobs = std::move(d_new);
    s->lik = a;
    s->graph_last_step = rows.last_row;
    return RSCM_OK;
}

}  // namespace

int rscm_sampler_create(rscm_ens* evaluator, int32_t n_walkers, int32_t n_dims, const int32_t* param_rows,
                        const double* base_params, const int32_t* prior_kind, const double* prior_a,
                        const double* prior_b, const double* prior_low, const double* prior_high,
                        int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                        const double* obs_value, const double* obs_sigma, int32_t normalize, double stretch_a,
                        uint64_t seed, rscm_sampler** out)
{
    return rscm_sampler_create_sharded(evaluator, n_walkers, n_dims, param_rows, base_params, prior_kind, prior_a, prior_b,
                                       prior_low, prior_high, n_obs, obs_var, obs_tidx, obs_value, obs_sigma, normalize,
                                       stretch_a, seed, 0, 1, out);
}

int rscm_sampler_create_sharded(rscm_ens* evaluator, int32_t n_walkers, int32_t n_dims, const int32_t* param_rows,
                        const double* base_params, const int32_t* prior_kind, const double* prior_a,
                        const double* prior_b, const double* prior_low, const double* prior_high,
                        int32_t n_obs, const int32_t* obs_var, const int32_t* obs_tidx,
                        const double* obs_value, const double* obs_sigma, int32_t normalize, double stretch_a,
                        uint64_t seed, int32_t rank, int32_t n_ranks, rscm_sampler** out)
{
    GUARD_BEGIN
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    rscm_ens* h = evaluator;
    NEED(h);
    if (h->windowed) return fail(RSCM_ERR_INVALID, "the sampler's evaluator must not be a windowed ensemble");
    if (h->noise_kind)
        return fail(RSCM_ERR_INVALID, "the evaluating ensemble has forcing noise (rscm_ens_set_forcing_noise): the likelihood of one noise "
                                      "realisation per walker index is not a target the stretch move samples; clear the noise first");
    if (int rc = check_walkers(n_walkers, rank, n_ranks, stretch_a)) return rc;
    if (h->N != n_walkers / 2 / n_ranks)
        return fail(RSCM_ERR_INVALID, "the evaluating ensemble must have n_walkers / 2 / n_ranks = %d members, it has %lld",
                    n_walkers / 2 / n_ranks, (long long)h->N);
    if (n_dims < 1 || n_dims > h->P || !param_rows || !base_params || !prior_kind || !prior_a || !prior_b)
        return fail(RSCM_ERR_INVALID, "bad parameter description");
    for (int32_t d = 0; d < n_dims; ++d) {
        if (param_rows[d] < 0 || param_rows[d] >= h->P) return fail(RSCM_ERR_INVALID, "dimension %d: parameter row %d out of range", d, param_rows[d]);
        if (const char* name = structural_row(h->kind, param_rows[d]))
            return fail(RSCM_ERR_INVALID, "dimension %d: parameter row %d (%s) is structural -- the host derives tables from it when the "
                        "parameters are set -- and cannot be sampled on the device", d, param_rows[d], name);
        for (int32_t e2 = 0; e2 < d; ++e2)
            if (param_rows[e2] == param_rows[d]) return fail(RSCM_ERR_INVALID, "parameter row %d sampled twice", param_rows[d]);
        if (int rc = check_prior(d, prior_kind, prior_a, prior_b, prior_low, prior_high)) return rc;
    }
    // the fused kernel takes two-layer observations with ascending time indices inside a group
    bool fused = h->kind == RSCM_KIND_TWO_LAYER;
    for (int32_t j = 0; j < n_obs && fused; ++j) {
        if (!obs_var || !obs_tidx) return fail(RSCM_ERR_INVALID, "bad observation arrays");
        if (j > 0 && obs_var[j] == obs_var[j - 1] && obs_tidx[j] < obs_tidx[j - 1]) fused = false;
    }
    const ObsList o = {n_obs, nullptr, obs_var, obs_tidx, obs_value, obs_sigma, normalize};
    LoglikRows rows;   // stored path: resolved before anything is allocated, uploaded once the sampler exists
    if (fused) {
        if (int rc = prepare_obs(h, n_obs, obs_var, obs_tidx, obs_value, obs_sigma, normalize)) return rc;
    } else {
        if (h->rows != h->T)
            return fail(RSCM_ERR_INVALID, "this evaluator stores no series: only the fused two-layer likelihood "
                                          "(ascending observation times) is available for it");
        if (int rc = resolve_loglik_rows(&h, 1, true, o, {}, &rows)) return rc;
        if (int rc = set_device(h)) return rc;
        HIPCHK(h->d_loglik.reserve((size_t)h->N));
    }
    std::unique_ptr<rscm_sampler> s(new rscm_sampler());
    s->fused = fused;
    if (int rc = sampler_init(s.get(), h, n_walkers, n_dims, prior_kind, prior_a, prior_b, prior_low, prior_high, o, stretch_a, seed, rank, n_ranks))
        return rc;
    HIPCHK(s->d_rows.alloc((size_t)n_dims));
    HIPCHK(s->d_base.alloc((size_t)h->P));
    HIPCHK(hipMemcpy(s->d_rows, param_rows, (size_t)n_dims * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->d_base, base_params, (size_t)h->P * sizeof(double), hipMemcpyHostToDevice));
    if (!fused)   // the observation rows of the stored series, once
        if (int rc = sampler_install_table(s.get(), rows)) return rc;
    if (fused) h->loglik_stop_at_last_obs = true;   // only now that the sampler stands; cleared again by rscm_sampler_destroy
    *out = s.release();
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_create_graph(rscm_ens* const* handles, int32_t n_handles, int32_t clear_between_runs, int32_t n_walkers, int32_t n_dims,
                              const int32_t* param_owner, const int32_t* param_rows, const int32_t* prior_kind, const double* prior_a,
                              const double* prior_b, const double* prior_low, const double* prior_high, int32_t n_obs,
                              const int32_t* obs_owner, const int32_t* obs_var, const int32_t* obs_tidx, const double* obs_value,
                              const double* obs_sigma, int32_t normalize, double stretch_a, uint64_t seed, int32_t rank, int32_t n_ranks,
                              rscm_sampler** out)
{
    GUARD_BEGIN
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!handles || n_handles < 1) return fail(RSCM_ERR_INVALID, "need at least one handle");
    if (int rc = check_walkers(n_walkers, rank, n_ranks, stretch_a)) return rc;
    if (n_dims < 1 || !param_owner || !param_rows || !prior_kind || !prior_a || !prior_b) return fail(RSCM_ERR_INVALID, "bad parameter description");
    rscm_ens* lead = handles[0];
    for (int32_t k = 0; k < n_handles; ++k) {
        rscm_ens* h = handles[k];
        NEED(h);
        if (h->n_comp > 0)
            return fail(RSCM_ERR_INVALID, "handle %d is a mix handle (rscm_ens_create_mix): it cannot be part of a graph sampler; "
                                          "rscm_sampler_create takes it as its one evaluator", k);
        if (h->noise_kind)
            return fail(RSCM_ERR_INVALID, "handle %d has forcing noise (rscm_ens_set_forcing_noise): it cannot be part of a graph sampler", k);
        if (h->N != n_walkers / 2 / n_ranks)
            return fail(RSCM_ERR_INVALID, "handle %d: every ensemble of the graph must have n_walkers / 2 / n_ranks = %d members, it has %lld", k,
                        n_walkers / 2 / n_ranks, (long long)h->N);
        if (h->windowed || h->rows != h->T) return fail(RSCM_ERR_INVALID, "handle %d: the sampler's evaluators store their whole series (no window, no RSCM_FLAG_NO_SERIES)", k);
        if (h->stream != lead->stream || h->device != lead->device) return fail(RSCM_ERR_STATE, "handle %d runs on another stream or device than handle 0", k);
        if (!h->params_set) return fail(RSCM_ERR_STATE, "handle %d: set the parameters once (rscm_ens_set_params) before sampling", k);
    }
    std::vector<uint64_t> sampled((size_t)n_handles, 0);
    for (int32_t d = 0; d < n_dims; ++d) {
        if (param_owner[d] < 0 || param_owner[d] >= n_handles) return fail(RSCM_ERR_INVALID, "dimension %d: owner %d out of range", d, param_owner[d]);
        const rscm_ens* h = handles[param_owner[d]];
        if (param_rows[d] < 0 || param_rows[d] >= h->P) return fail(RSCM_ERR_INVALID, "dimension %d: parameter row %d out of range", d, param_rows[d]);
        if (const char* name = structural_row(h->kind, param_rows[d]))
            return fail(RSCM_ERR_INVALID, "dimension %d: parameter row %d (%s) of handle %d is structural -- the host derives tables from it "
                        "when the parameters are set -- and cannot be sampled on the device", d, param_rows[d], name, param_owner[d]);
        for (int32_t e2 = 0; e2 < d; ++e2)
            if (param_owner[e2] == param_owner[d] && param_rows[e2] == param_rows[d])
                return fail(RSCM_ERR_INVALID, "parameter row %d of handle %d sampled twice", param_rows[d], param_owner[d]);
        if (int rc = check_prior(d, prior_kind, prior_a, prior_b, prior_low, prior_high)) return rc;
        if (param_rows[d] < 64) sampled[(size_t)param_owner[d]] |= 1ull << param_rows[d];
    }
    if (n_obs > 0 && !obs_owner) return fail(RSCM_ERR_INVALID, "bad observation arrays");
    const ObsList o = {n_obs, obs_owner, obs_var, obs_tidx, obs_value, obs_sigma, normalize};
    LoglikRows rows;
    if (int rc = resolve_loglik_rows(handles, n_handles, true, o, {}, &rows)) return rc;
    if (int rc = set_device(lead)) return rc;
    HIPCHK(lead->d_loglik.reserve((size_t)lead->N));
    std::unique_ptr<rscm_sampler> s(new rscm_sampler());
    s->fused = false;
    s->graph.assign(handles, handles + n_handles);
    s->graph_sampled_rows = sampled;
    s->graph_clear = clear_between_runs != 0;
    if (int rc = sampler_init(s.get(), lead, n_walkers, n_dims, prior_kind, prior_a, prior_b, prior_low, prior_high, o, stretch_a, seed, rank, n_ranks))
        return rc;
    std::vector<double*> ptrs((size_t)n_dims);
    for (int32_t d = 0; d < n_dims; ++d) ptrs[(size_t)d] = handles[param_owner[d]]->d_params + (size_t)param_rows[d] * (size_t)lead->N;
    HIPCHK(s->d_param_ptr.alloc(ptrs.size()));
    HIPCHK(hipMemcpy(s->d_param_ptr, ptrs.data(), ptrs.size() * sizeof(double*), hipMemcpyHostToDevice));
    // the observation rows where their owners store them; one partial sum per (owner, variable) in the caller's order
    if (int rc = sampler_install_table(s.get(), rows)) return rc;
    *out = s.release();
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_destroy(rscm_sampler* s)
{
    if (!s) return RSCM_OK;
    if (s->ev) {
        s->ev->loglik_stop_at_last_obs = false;
        s->ev->ref_active = false;
    }
    delete s;   // synchronises the evaluator's stream, then frees (~rscm_sampler)
    return RSCM_OK;
}

// what must hold before a half-step is enqueued
static int sampler_ready(rscm_sampler* s)
{
    rscm_ens* h = s->ev;
    if (!s->graph.empty()) return set_device(h);   // rscm_ens_run_lockstep checks every handle of the graph when it runs
    h->put_at(0);
    return check_loglik_ready(h);
}

int rscm_sampler_set_reference(rscm_sampler* s, int32_t n_ref, const int32_t* ref_owner, const int32_t* ref_var, const int32_t* ref_begin,
                               const int32_t* ref_end, const int32_t* ref_stride)
{
    GUARD_BEGIN
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    if (s->positions_set) return fail(RSCM_ERR_STATE, "reference periods are set before the walker positions (rscm_sampler_set_positions scores with them)");
    rscm_ens* h = s->ev;
    const bool graph = !s->graph.empty();
    if (n_ref > 0 && graph != (ref_owner != nullptr))
        return fail(RSCM_ERR_INVALID, graph ? "a graph sampler needs ref_owner" : "ref_owner is for graph samplers: pass NULL");
    if (s->fused) return prepare_ref(h, n_ref, ref_var, ref_begin, ref_end, ref_stride);
    LoglikRows rows;
    if (int rc = resolve_loglik_rows(graph ? s->graph.data() : &h, graph ? (int32_t)s->graph.size() : 1, true, s->observations(),
                                     {n_ref, graph ? ref_owner : nullptr, ref_var, ref_begin, ref_end, ref_stride}, &rows))
        return rc;
    return sampler_install_table(s, rows);
    GUARD_END
}

int rscm_sampler_set_groups(rscm_sampler* s, int32_t n_groups)
{
    GUARD_BEGIN
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    if (n_groups < 1 || s->W % n_groups != 0 || (s->W / n_groups) % 2 != 0 || s->W / n_groups < 2)
        return fail(RSCM_ERR_INVALID, "%d walkers do not split into %d groups of an even number (>= 2) of walkers", s->W, n_groups);
    if ((s->n_ranks > 1 || s->sharded) && n_groups != 1) return fail(RSCM_ERR_INVALID, "a sharded sampler runs one ensemble (n_groups = 1)");
    s->groups = n_groups;
    s->positions_set = false;  // positions are scored per group layout: set them again
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_set_positions(rscm_sampler* s, const double* positions)
{
    GUARD_BEGIN
    if (!s || !positions) return fail(RSCM_ERR_INVALID, "sampler or positions is NULL");
    rscm_ens* h = s->ev;
    if (!h->params_set)  // kinds with structural rows (ClimateUDEB) are configured by rscm_ens_set_params
        return fail(RSCM_ERR_STATE, "set the evaluator's parameters once (rscm_ens_set_params) before sampling");
    if (int rc = sampler_ready(s)) return rc;
    const size_t W = (size_t)s->W, D = (size_t)s->D;
    std::vector<double> soa(D * W);  // [W][D] row-major in, [D][W] on the device
    for (size_t w = 0; w < W; ++w)
        for (size_t d = 0; d < D; ++d) soa[d * W + w] = positions[w * D + d];
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(s->d_pos, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s->d_nacc, 0, W * sizeof(int64_t)));
    HIPCHK(hipMemset(s->d_nprop, 0, W * sizeof(int64_t)));
    s->iteration = 0;
    s->positions_set = true;
    if (s->sharded) {  // scored half by half through rscm_sampler_half_step(identity = 1) + the exchange
        HIPCHK(rscm::launch_fill(s->d_logp, (int64_t)W, -std::numeric_limits<double>::infinity(), h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return RSCM_OK;
    }
    for (int32_t half = 0; half < 2; ++half)
        if (int rc = sampler_half_step(s, half, 1)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_iterate(rscm_sampler* s, int32_t n_iterations)
{
    GUARD_BEGIN
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    if (!s->positions_set) return fail(RSCM_ERR_STATE, "walker positions not set");
    if (n_iterations < 0) return fail(RSCM_ERR_INVALID, "n_iterations must be >= 0");
    if (s->sharded)
        return fail(RSCM_ERR_STATE, "a sharded sampler is driven half-step by half-step (rscm_sampler_half_step, all-gather, "
                                    "rscm_sampler_apply_exchange)");
    rscm_ens* h = s->ev;
    if (int rc = sampler_ready(s)) return rc;
    HIPCHK(hipEventRecord(s->ev0, h->stream));
    for (int32_t it = 0; it < n_iterations; ++it) {
        s->iteration += 1;
        // first half against the second, then the second against the updated first (ensemble.rs:509-515)
        if (int rc = sampler_half_step(s, 0, 0)) return rc;
        if (int rc = sampler_half_step(s, 1, 0)) return rc;
    }
    HIPCHK(hipEventRecord(s->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_begin_iteration(rscm_sampler* s)
{
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    if (!s->positions_set) return fail(RSCM_ERR_STATE, "walker positions not set");
    s->iteration += 1;
    return RSCM_OK;
}

int rscm_sampler_half_step(rscm_sampler* s, int32_t half, int32_t identity)
{
    GUARD_BEGIN
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    if (!s->positions_set) return fail(RSCM_ERR_STATE, "walker positions not set");
    if (half != 0 && half != 1) return fail(RSCM_ERR_INVALID, "half must be 0 or 1");
    if (int rc = sampler_ready(s)) return rc;
    return sampler_half_step(s, half, identity ? 1 : 0);
    GUARD_END
}

int rscm_sampler_exchange_buffers(rscm_sampler* s, void** send, void** recv, int64_t* doubles_per_rank)
{
    if (!s || !send || !recv || !doubles_per_rank) return fail(RSCM_ERR_INVALID, "NULL argument");
    s->sharded = true;   // from here on the caller drives the half-steps and the exchange
    *send = s->d_send;
    *recv = s->d_recv;
    *doubles_per_rank = (int64_t)(s->D + 1) * s->n_local;
    return RSCM_OK;
}

int rscm_sampler_apply_exchange(rscm_sampler* s, int32_t half)
{
    GUARD_BEGIN
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    if (!s->sharded) return fail(RSCM_ERR_STATE, "this sampler is not sharded (rscm_sampler_exchange_buffers first)");
    if (half != 0 && half != 1) return fail(RSCM_ERR_INVALID, "half must be 0 or 1");
    rscm::SamplerArgs a = sampler_args(s, half, 0);
    a.exchange = s->d_recv;
    HIPCHK(rscm::launch_sampler_unpack(a, s->ev->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_sync(rscm_sampler* s)
{
    GUARD_BEGIN
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    HIPCHK(hipStreamSynchronize(s->ev->stream));
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_last_ms(const rscm_sampler* s, float* out)
{
    GUARD_BEGIN
    if (!s || !out) return fail(RSCM_ERR_INVALID, "sampler or out is NULL");
    HIPCHK(hipEventElapsedTime(out, s->ev0, s->ev1));
    return RSCM_OK;
    GUARD_END
}

int rscm_sampler_get(rscm_sampler* s, double* positions, double* log_prob, int64_t* n_accepted, int64_t* n_proposed)
{
    GUARD_BEGIN
    if (!s) return fail(RSCM_ERR_INVALID, "sampler is NULL");
    if (!s->positions_set) return fail(RSCM_ERR_STATE, "walker positions not set");
    const size_t W = (size_t)s->W, D = (size_t)s->D;
    HIPCHK(hipStreamSynchronize(s->ev->stream));
    if (positions) {
        std::vector<double> soa(D * W);
        HIPCHK(hipMemcpy(soa.data(), s->d_pos, soa.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t w = 0; w < W; ++w)
            for (size_t d = 0; d < D; ++d) positions[w * D + d] = soa[d * W + w];
    }
    if (log_prob) HIPCHK(hipMemcpy(log_prob, s->d_logp, W * sizeof(double), hipMemcpyDeviceToHost));
    if (n_accepted) HIPCHK(hipMemcpy(n_accepted, s->d_nacc, W * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (n_proposed) HIPCHK(hipMemcpy(n_proposed, s->d_nprop, W * sizeof(int64_t), hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
