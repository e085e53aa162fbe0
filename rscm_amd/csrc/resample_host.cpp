// Host side of the posterior resampling (kernels: resample.hip): exact weight statistics, the systematic draw of one handle's
// share of a global draw, and the offset every rank derives for itself from the seed.  The gather of the drawn members,
// rscm_ens_gather_members, lives in state_host.cpp with the rest of a handle's state in time.
#include "ens.hpp"

namespace {

// Philox4x32-10 on the host, the rounds of philox.hpp (the device copy) word for word
void philox4x32_10_host(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// t_k = floor((s + k W) / M) = k q + floor((s + k r) / M) in 64 bits (resample.hip, ancestors_kernel)
inline uint64_t point(uint64_t k, uint64_t q, uint64_t r, uint64_t s, uint64_t M) { return k * q + (s + k * r) / M; }

// the smallest k in [0, M] with t_k >= x (M if there is none); t_k is non-decreasing in k
int64_t first_draw_at(uint64_t x, uint64_t q, uint64_t r, uint64_t s, uint64_t M)
{
    uint64_t lo = 0, hi = M;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (point(mid, q, r, s, M) >= x) hi = mid;
        else lo = mid + 1;
    }
    return (int64_t)lo;
}

}  // namespace

extern "C" {

int rscm_ens_weights_stats(rscm_ens* h, int64_t* total, int64_t* n_nonzero, int64_t* w_max, uint64_t sum_sq[2])
{
    GUARD_BEGIN
    NEED(h);
    if (!total || !n_nonzero || !w_max || !sum_sq) return fail(RSCM_ERR_INVALID, "an output pointer is NULL");
    if (!h->d_weights) return fail(RSCM_ERR_STATE, "no member weights set");
    if (int rc = set_device(h)) return rc;
    const int32_t n_partial = rscm::weights_stats_partials(h->N);
    rscm::DevBuf<unsigned long long> d_buf;   // [5 * n_partial] partials, then the five results
    HIPCHK(d_buf.alloc((size_t)5 * (n_partial + 1)));
    unsigned long long* d_res = d_buf.get() + (size_t)5 * n_partial;
    unsigned long long out[5] = {};
    HIPCHK(rscm::launch_weights_stats(h->d_weights, h->N, d_buf.get(), d_res, h->stream));
    HIPCHK(hipMemcpyAsync(out, d_res, sizeof out, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *total = (int64_t)out[0];
    *n_nonzero = (int64_t)out[1];
    *w_max = (int64_t)out[2];
    sum_sq[0] = out[4];   // (hi, lo)
    sum_sq[1] = out[3];
    return RSCM_OK;
    GUARD_END
}

int rscm_ens_resample(rscm_ens* h, int64_t M, int64_t s, int64_t w_before, int64_t w_total, int64_t* k_first, int64_t* count, void** anc_dev)
{
    GUARD_BEGIN
    NEED(h);
    if (!k_first || !count || !anc_dev) return fail(RSCM_ERR_INVALID, "an output pointer is NULL");
    if (!h->d_weights) return fail(RSCM_ERR_STATE, "no member weights set");
    if (h->select) return fail(RSCM_ERR_STATE, "a select is in flight on this handle: rscm_ens_select_end it first");
    if (M < 1 || M > ((int64_t)1 << 31)) return fail(RSCM_ERR_INVALID, "the number of draws must be in [1, 2^31], got %lld", (long long)M);
    if (w_total <= 0) return fail(RSCM_ERR_INVALID, "the total weight must be positive, got %lld", (long long)w_total);
    if (s < 0 || s >= w_total) return fail(RSCM_ERR_INVALID, "the offset must be in [0, w_total), got %lld", (long long)s);
    if (w_before < 0 || w_before > w_total) return fail(RSCM_ERR_INVALID, "w_before = %lld is outside [0, w_total]", (long long)w_before);
    if (int rc = set_device(h)) return rc;
    HIPCHK(h->d_cumw.reserve((size_t)(h->N + rscm::scan_scratch_elems(h->N))));
    HIPCHK(rscm::launch_inclusive_scan(h->d_weights, h->d_cumw, h->N, h->d_cumw + h->N, h->stream));
    int64_t w_local = 0;
    HIPCHK(hipMemcpyAsync(&w_local, h->d_cumw + (h->N - 1), sizeof w_local, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (w_local > w_total - w_before)
        return fail(RSCM_ERR_INVALID, "this handle's weights [%lld, %lld + %lld) reach past the total %lld", (long long)w_before,
                    (long long)w_before, (long long)w_local, (long long)w_total);
    const uint64_t Mu = (uint64_t)M, q = (uint64_t)w_total / Mu, r = (uint64_t)w_total % Mu;
    const int64_t k0 = first_draw_at((uint64_t)w_before, q, r, (uint64_t)s, Mu);
    const int64_t k1 = first_draw_at((uint64_t)w_before + (uint64_t)w_local, q, r, (uint64_t)s, Mu);
    const int64_t n = k1 - k0;
    HIPCHK(h->d_anc.reserve((size_t)std::max<int64_t>(n, 1)));   // (the last draw's ancestors go: the caller was handed the address)
    HIPCHK(rscm::launch_ancestors(h->d_cumw, h->N, k0, n, Mu, q, r, (uint64_t)s, (uint64_t)w_before, h->d_anc, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *k_first = k0;
    *count = n;
    *anc_dev = h->d_anc;
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_resample_offset(uint64_t seed, int64_t w_total, int64_t* s)
{
    if (!s) return fail(RSCM_ERR_INVALID, "s is NULL");
    if (w_total <= 0) return fail(RSCM_ERR_INVALID, "the total weight must be positive, got %lld", (long long)w_total);
    uint32_t c[4] = {0u, 0u, 0u, RSCM_RESAMPLE_STREAM_TAG};
    philox4x32_10_host(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t R = ((uint64_t)c[1] << 32) | c[0];
    *s = (int64_t)(uint64_t)(((unsigned __int128)R * (unsigned __int128)(uint64_t)w_total) >> 64);
    return RSCM_OK;
}

}  // extern "C"
