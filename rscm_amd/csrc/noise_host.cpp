// The forcing-noise setting of a two-layer handle (ens.hpp): its one writer and the entry points in front of it.
#include "ens.hpp"

extern "C" {

// The one writer of a handle's forcing-noise setting (ens.hpp).  sigma: white and red; phi: red; 0 where the kind does not read them
static int set_noise(rscm_ens* h, int32_t kind, uint64_t seed, double sigma, double phi, int64_t member_offset)
{
    GUARD_BEGIN
    if (kind != rscm::kNoiseKindNone) {
        if (h->kind != RSCM_KIND_TWO_LAYER)
            return fail(RSCM_ERR_INVALID, "forcing noise is available for the two-layer kind only (RSCM_KIND_TWO_LAYER), this handle has kind %d", h->kind);
        if (!(sigma >= 0.0) || !std::isfinite(sigma)) return fail(RSCM_ERR_INVALID, "sigma must be finite and not negative, got %g", sigma);
        if (!std::isfinite(phi) || !(std::fabs(phi) < 1.0)) return fail(RSCM_ERR_INVALID, "phi must be finite with |phi| < 1, got %g", phi);
        if (member_offset < 0) return fail(RSCM_ERR_INVALID, "member_offset must not be negative, got %lld", (long long)member_offset);
        if (h->windowed || h->rows != h->T)
            return fail(RSCM_ERR_INVALID, "forcing noise needs a handle that stores its whole series (no windowed storage, no RSCM_FLAG_NO_SERIES)");
        if (h->n_linked > 0) return fail(RSCM_ERR_INVALID, "this handle has a linked input: the noise is added to a handle's own shared forcing");
    }
    if (rscm::noise_kind_keeps_state(kind) && !h->d_noise_state) {
        if (int rc = set_device(h)) return rc;
        HIPCHK(h->d_noise_state.alloc((size_t)h->N));
    }
    h->noise_kind = kind;
    h->noise_seed = seed;
    h->noise_sigma = sigma;
    h->noise_phi = phi;
    h->noise_offset = member_offset;
    h->noise_state_index = -1;   // the cache belonged to the setting before
    h->rows_written();           // and so did every row a run has written
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_set_forcing_noise_ar1(rscm_ens* h, uint64_t seed, double sigma, double phi, int64_t member_offset)
{
    NEED(h);
    if (phi == 0.0) return set_noise(h, rscm::kNoiseKindWhite, seed, sigma, 0.0, member_offset);   // (-0.0 is white too: the white kernels, no buffer)
    return set_noise(h, rscm::kNoiseKindRed, seed, sigma, phi, member_offset);
}

int rscm_ens_set_forcing_noise(rscm_ens* h, uint64_t seed, double sigma, int64_t member_offset)
{
    NEED(h);
    return set_noise(h, rscm::kNoiseKindWhite, seed, sigma, 0.0, member_offset);
}

int rscm_ens_set_forcing_noise_members(rscm_ens* h, uint64_t seed, int64_t member_offset)
{
    NEED(h);
    if (!h->noise_rows)
        return fail(RSCM_ERR_INVALID, "this handle has no noise parameter rows: create it with RSCM_FLAG_NOISE_PARAMS");
    return set_noise(h, rscm::kNoiseKindMembers, seed, 0.0, 0.0, member_offset);   // sigma and phi are the rows'
}

int rscm_ens_clear_forcing_noise(rscm_ens* h)
{
    NEED(h);
    return set_noise(h, rscm::kNoiseKindNone, 0, 0.0, 0.0, 0);
}

int rscm_ens_forcing_noise(const rscm_ens* h, int32_t* on, uint64_t* seed, double* sigma, int64_t* member_offset)
{
    NEED(h);
    if (on) *on = h->noise_kind != rscm::kNoiseKindNone ? 1 : 0;
    if (seed) *seed = h->noise_seed;
    if (sigma) *sigma = h->noise_sigma;
    if (member_offset) *member_offset = h->noise_offset;
    return RSCM_OK;
}

int rscm_ens_forcing_noise_ar1(const rscm_ens* h, double* phi, int32_t* cached_index)
{
    NEED(h);
    if (phi) *phi = h->noise_phi;
    if (cached_index) *cached_index = h->noise_red() ? h->noise_state_index : -1;
    return RSCM_OK;
}

int rscm_ens_forcing_noise_members(const rscm_ens* h, int32_t* per_member, int32_t* sigma_row, int32_t* phi_row)
{
    NEED(h);
    if (per_member) *per_member = h->noise_kind == rscm::kNoiseKindMembers ? 1 : 0;
    if (sigma_row) *sigma_row = h->noise_sigma_row();
    if (phi_row) *phi_row = h->noise_phi_row();
    return RSCM_OK;
}

int rscm_ens_forcing_noise_rows(rscm_ens* h, int32_t t_begin, int32_t t_end, double* out, int32_t on_device)
{
    GUARD_BEGIN
    NEED(h);
    if (!h->noise_kind) return fail(RSCM_ERR_STATE, "this handle has no forcing noise (rscm_ens_set_forcing_noise)");
    if (t_begin < 0 || t_end < t_begin || t_end > h->T)
        return fail(RSCM_ERR_INVALID, "rows [%d, %d) are not within the forcing axis [0, %d)", t_begin, t_end, h->T);
    if (t_end == t_begin) return RSCM_OK;
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if (int rc = set_device(h)) return rc;
    const size_t elems = (size_t)(t_end - t_begin) * (size_t)h->N;
    rscm::DevBuf<double> tmp;   // host output: the rows are formed here
    if (!on_device) HIPCHK(tmp.alloc(elems));
    double* d = on_device ? out : tmp.get();
    HIPCHK(rscm::launch_forcing_noise_rows(h->noise_kind, h->noise_seed, h->noise_sigma, h->noise_phi, h->d_params, h->uniform_rows,
                                           h->noise_sigma_row(), h->noise_phi_row(), h->noise_offset, h->N, t_begin, t_end, d, h->stream));
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(out, d, elems * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
