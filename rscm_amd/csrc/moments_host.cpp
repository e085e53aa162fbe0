// Host side of the exact moments across members (rscm_ens_moment_sums, rscm_gpu_moment_finish, rscm_ens_moments; the definition is
// stated in include/rscm_gpu.h, the kernels are in moments.hip, the finishing step in moments_finish.hpp).
//
// A call uploads the vector addresses and, for order 2, the centre; the mask kernel marks the counted members and forms n and W
// per group, the sum kernel the blocks.  Everything lands in one int64 array [G][2 + blocks * 69], the caller's if it is on the
// device, else a temporary that is copied out.  Every temporary is a DevBuf.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "ens.hpp"
#include "moments_finish.hpp"

static_assert(RSCM_MOMENT_BLOCK == rscm::kMomentBlock, "the header states the block the finishing step reads");
static_assert(RSCM_MOMENT_MAX_VECTORS == rscm::kMaxMomentVectors, "the header states the kernel's vector limit");

int check_device_out(const rscm_ens* h, const int64_t* p, size_t n)
{
    if ((uintptr_t)p & 7) return fail(RSCM_ERR_INVALID, "out is not 8-byte aligned");
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != h->device) {
        (void)hipGetLastError();
        return fail(RSCM_ERR_INVALID, "out is not device memory on device %d", h->device);
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess ||
        (const char*)p + n * sizeof(int64_t) > (const char*)base + size) {
        (void)hipGetLastError();
        return fail(RSCM_ERR_INVALID, "out does not hold %zu int64", n);
    }
    return RSCM_OK;
}

namespace {

int32_t moment_blocks(int32_t n_vec, int32_t order) { return order == 1 ? n_vec : n_vec * (n_vec + 1) / 2; }

int moment_sums(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t flags, int32_t order, const double* center, int64_t* out,
                int32_t on_device)
{
    if (flags & RSCM_SELECT_ANOMALY) return fail(RSCM_ERR_INVALID, "RSCM_SELECT_ANOMALY applies to stored rows, not to moments of vectors");
    if (flags & ~(RSCM_SELECT_WEIGHTED | RSCM_SELECT_GROUPED)) return fail(RSCM_ERR_INVALID, "unknown moment flags 0x%x", flags);
    if (order != 1 && order != 2) return fail(RSCM_ERR_INVALID, "order %d: must be 1 or 2", order);
    if (order == 2 && !center) return fail(RSCM_ERR_INVALID, "order 2 needs a centre");
    if (!vec_dev || n_vec < 1 || n_vec > RSCM_MOMENT_MAX_VECTORS)
        return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors)", RSCM_MOMENT_MAX_VECTORS);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    const bool weighted = (flags & RSCM_SELECT_WEIGHTED) != 0, grouped = (flags & RSCM_SELECT_GROUPED) != 0;
    if (weighted && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if (grouped && !h->d_groups) return fail(RSCM_ERR_STATE, "no member groups: rscm_ens_set_member_groups first");
    if ((int64_t)h->N >= rscm::kMomentMaxTerms) return fail(RSCM_ERR_INVALID, "moments take fewer than 2^31 members per handle");
    if (int rc = set_device(h)) return rc;
    for (int32_t k = 0; k < n_vec; ++k) {
        char what[24];
        std::snprintf(what, sizeof what, "vector %d", k);
        if (int rc = check_member_vector(h, vec_dev[k], what)) return rc;
    }
    const int32_t G = grouped ? h->n_groups : 1;
    const size_t stride = 2 + (size_t)moment_blocks(n_vec, order) * rscm::kMomentBlock, total = (size_t)G * stride;
    if (on_device)
        if (int rc = check_device_out(h, out, total)) return rc;

    rscm::DevBuf<const double*> d_vec;
    rscm::DevBuf<double> d_centre;
    rscm::DevBuf<unsigned long long> d_mask, d_tmp;
    std::vector<double> c;
    HIPCHK(d_vec.alloc((size_t)n_vec));
    HIPCHK(hipMemcpyAsync(d_vec.get(), vec_dev, (size_t)n_vec * sizeof(double*), hipMemcpyHostToDevice, h->stream));
    if (order == 2) {
        // a group with a non-finite centre: every term of every block is counted as non-finite (NaN centres do that in the kernel)
        c.assign(center, center + (size_t)G * n_vec);
        for (int32_t g = 0; g < G; ++g) {
            bool finite = true;
            for (int32_t k = 0; k < n_vec; ++k) finite = finite && std::isfinite(c[(size_t)g * n_vec + k]);
            if (!finite)
                for (int32_t k = 0; k < n_vec; ++k) c[(size_t)g * n_vec + k] = std::nan("");
        }
        HIPCHK(d_centre.alloc(c.size()));
        HIPCHK(hipMemcpyAsync(d_centre.get(), c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(d_mask.alloc((size_t)((h->N + 63) / 64) + 1));
    unsigned long long* d_out = reinterpret_cast<unsigned long long*>(out);
    if (!on_device) {
        HIPCHK(d_tmp.alloc(total));
        d_out = d_tmp.get();
    }
    HIPCHK(hipMemsetAsync(d_out, 0, total * sizeof(int64_t), h->stream));
    HIPCHK(rscm::launch_moment_sums(d_vec.get(), n_vec, weighted ? h->d_weights.get() : nullptr, grouped ? h->d_groups.get() : nullptr, G,
                                    order, d_centre.get(), h->N, d_mask.get(), d_out, h->stream));
    if (!on_device) HIPCHK(hipMemcpyAsync(out, d_out, total * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the temporaries and the host copies above go out of scope
    return RSCM_OK;
}

int finish(const int64_t* blocks, int32_t n_blocks, const int64_t* divisor, int64_t n_terms, double* out)
{
    if (rscm::moment_finish(blocks, n_blocks, divisor, n_terms, out))
        return fail(RSCM_ERR_INVALID, "moment finish: a NULL argument, a negative divisor or block count, or n_terms = %lld outside [0, 2^31)",
                    (long long)n_terms);
    return RSCM_OK;
}

}  // namespace

extern "C" {

int rscm_ens_moment_sums(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t flags, int32_t order, const double* center,
                         int64_t* out, int32_t on_device)
{
    GUARD_BEGIN
    NEED(h);
    return moment_sums(h, n_vec, vec_dev, flags, order, center, out, on_device);
    GUARD_END
}

int rscm_gpu_moment_finish(const int64_t* blocks, int32_t n_blocks, const int64_t* divisor, int64_t n_terms, double* out)
{
    GUARD_BEGIN
    return finish(blocks, n_blocks, divisor, n_terms, out);
    GUARD_END
}

int rscm_ens_moments(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t flags, double* mean, double* cov, int64_t* n,
                     int64_t* weight)
{
    GUARD_BEGIN
    NEED(h);
    if (!mean || !cov) return fail(RSCM_ERR_INVALID, "mean or cov is NULL");
    if (n_vec < 1 || n_vec > RSCM_MOMENT_MAX_VECTORS) return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors)", RSCM_MOMENT_MAX_VECTORS);
    const int32_t K = n_vec, B2 = moment_blocks(K, 2);
    const size_t G = (flags & RSCM_SELECT_GROUPED) && h->d_groups ? (size_t)h->n_groups : 1;
    const size_t s1 = 2 + (size_t)K * rscm::kMomentBlock, s2 = 2 + (size_t)B2 * rscm::kMomentBlock;
    std::vector<int64_t> sums1(G * s1), sums2(G * s2), div((size_t)B2);
    std::vector<double> tri((size_t)B2);
    if (int rc = moment_sums(h, K, vec_dev, flags, 1, nullptr, sums1.data(), 0)) return rc;
    for (size_t g = 0; g < G; ++g) {
        const int64_t* row = &sums1[g * s1];
        std::fill(div.begin(), div.end(), row[1]);
        if (int rc = finish(row + 2, K, div.data(), row[0], mean + g * K)) return rc;
        if (n) n[g] = row[0];
        if (weight) weight[g] = row[1];
    }
    if (int rc = moment_sums(h, K, vec_dev, flags, 2, mean, sums2.data(), 0)) return rc;
    for (size_t g = 0; g < G; ++g) {
        const int64_t* row = &sums2[g * s2];
        std::fill(div.begin(), div.end(), row[1]);
        if (int rc = finish(row + 2, B2, div.data(), row[0], tri.data())) return rc;
        double* c = cov + g * K * K;
        for (int32_t a = 0, k = 0; a < K; ++a)
            for (int32_t b = a; b < K; ++b, ++k) c[a * K + b] = c[b * K + a] = tri[(size_t)k];
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
