// Host side of the exact moments across members (rscm_ens_moment_sums, rscm_gpu_moment_finish, rscm_ens_moments; the definition is
// stated in include/rscm_gpu.h, the kernels are in moments.hip, the finishing step in moments_finish.hpp).
//
// A call uploads the vector addresses and, for order 2, the centre; the mask kernel marks the counted members and forms n and W
// per group, the sum kernel the blocks.  Everything lands in one int64 array [G][2 + blocks * 69], the caller's if it is on the
// device, else a temporary that is copied out.  Every temporary is a DevBuf.
// What the moments of stored rows (moment_rows_host.cpp) need as well is declared in ens.hpp and defined below moment_sums.
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

int finish(const int64_t* blocks, int32_t n_blocks, const int64_t* divisor, int64_t n_terms, double* out)
{
    if (rscm::moment_finish(blocks, n_blocks, divisor, n_terms, out))
        return fail(RSCM_ERR_INVALID, "moment finish: a NULL argument, a negative divisor or block count, or n_terms = %lld outside [0, 2^31)",
                    (long long)n_terms);
    return RSCM_OK;
}

int32_t moment_blocks(int32_t n_vec, int32_t order) { return order == 1 ? n_vec : n_vec * (n_vec + 1) / 2; }

int moment_sums(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t flags, int32_t order, const double* center, int64_t* out,
                int32_t on_device)
{
    if (flags & RSCM_SELECT_ANOMALY) return fail(RSCM_ERR_INVALID, "RSCM_SELECT_ANOMALY applies to stored rows, not to moments of vectors");
    if (int rc = check_moment_call(h, flags, RSCM_SELECT_WEIGHTED | RSCM_SELECT_GROUPED, order, center, n_vec, vec_dev, 1,
                                   RSCM_MOMENT_MAX_VECTORS, out))
        return rc;
    const bool weighted = (flags & RSCM_SELECT_WEIGHTED) != 0, grouped = (flags & RSCM_SELECT_GROUPED) != 0;
    if (int rc = check_member_vectors(h, n_vec, vec_dev)) return rc;
    const int32_t G = grouped ? h->n_groups : 1;
    const size_t total = (size_t)G * (2 + (size_t)moment_blocks(n_vec, order) * rscm::kMomentBlock);
    if (on_device)
        if (int rc = check_device_out(h, out, total)) return rc;

    rscm::DevBuf<const double*> d_vec;
    rscm::DevBuf<double> d_centre;
    rscm::DevBuf<unsigned long long> d_mask, d_tmp;
    std::vector<double> c;
    unsigned long long* d_out = nullptr;
    HIPCHK(d_vec.alloc((size_t)n_vec));
    HIPCHK(hipMemcpyAsync(d_vec.get(), vec_dev, (size_t)n_vec * sizeof(double*), hipMemcpyHostToDevice, h->stream));
    if (int rc = upload_moment_centre(h, order == 2 ? center : nullptr, (size_t)G, (size_t)n_vec, c, d_centre)) return rc;
    HIPCHK(d_mask.alloc((size_t)((h->N + 63) / 64) + 1));
    if (int rc = begin_moment_out(h, out, total, on_device, d_tmp, &d_out)) return rc;
    HIPCHK(rscm::launch_moment_sums(d_vec.get(), n_vec, weighted ? h->d_weights.get() : nullptr, grouped ? h->d_groups.get() : nullptr, G,
                                    order, d_centre.get(), h->N, d_mask.get(), d_out, h->stream));
    return end_moment_out(h, out, d_out, total, on_device);
}

}  // namespace

int check_moment_call(const rscm_ens* h, int32_t flags, int32_t allowed, int32_t order, const double* center, int32_t n_vec,
                      const double* const* vec_dev, int32_t min_vec, int32_t max_vec, const int64_t* out)
{
    if (flags & ~allowed) return fail(RSCM_ERR_INVALID, "unknown moment flags 0x%x", flags);
    if (order != 1 && order != 2) return fail(RSCM_ERR_INVALID, "order %d: must be 1 or 2", order);
    if (order == 2 && !center) return fail(RSCM_ERR_INVALID, "order 2 needs a centre");
    if (n_vec < min_vec || n_vec > max_vec || (n_vec > 0 && !vec_dev))
        return fail(RSCM_ERR_INVALID, "bad vector list (%d to %d vectors)", min_vec, max_vec);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    if ((flags & RSCM_SELECT_WEIGHTED) && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if ((flags & RSCM_SELECT_GROUPED) && !h->d_groups) return fail(RSCM_ERR_STATE, "no member groups: rscm_ens_set_member_groups first");
    if ((flags & RSCM_SELECT_ANOMALY) && !h->d_base)
        return fail(RSCM_ERR_STATE, "no baseline: rscm_ens_set_baseline or rscm_ens_set_baseline_values first");
    if ((int64_t)h->N >= rscm::kMomentMaxTerms) return fail(RSCM_ERR_INVALID, "moments take fewer than 2^31 members per handle");
    return RSCM_OK;
}

int check_member_vectors(const rscm_ens* h, int32_t n_vec, const double* const* vec_dev)
{
    if (int rc = set_device(h)) return rc;
    for (int32_t k = 0; k < n_vec; ++k) {
        char what[24];
        std::snprintf(what, sizeof what, "vector %d", k);
        if (int rc = check_member_vector(h, vec_dev[k], what)) return rc;
    }
    return RSCM_OK;
}

int upload_moment_centre(rscm_ens* h, const double* center, size_t n, size_t width, std::vector<double>& c, rscm::DevBuf<double>& d_centre)
{
    if (!center) return RSCM_OK;
    c.assign(center, center + n * width);
    for (size_t r = 0; r < n; ++r) {
        const auto rec = c.begin() + r * width;
        if (!std::all_of(rec, rec + width, [](double x) { return std::isfinite(x); })) std::fill(rec, rec + width, std::nan(""));
    }
    HIPCHK(d_centre.alloc(c.size()));
    HIPCHK(hipMemcpyAsync(d_centre.get(), c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return RSCM_OK;
}

int begin_moment_out(rscm_ens* h, int64_t* out, size_t total, int32_t on_device, rscm::DevBuf<unsigned long long>& d_tmp,
                     unsigned long long** d_out)
{
    *d_out = reinterpret_cast<unsigned long long*>(out);
    if (!on_device) {
        HIPCHK(d_tmp.alloc(total));
        *d_out = d_tmp.get();
    }
    HIPCHK(hipMemsetAsync(*d_out, 0, total * sizeof(int64_t), h->stream));
    return RSCM_OK;
}

int end_moment_out(rscm_ens* h, int64_t* out, const unsigned long long* d_out, size_t total, int32_t on_device)
{
    if (!on_device) HIPCHK(hipMemcpyAsync(out, d_out, total * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the caller's temporaries and host copies go out of scope after this
    return RSCM_OK;
}

int finish_moment_sums(const int64_t* sums, size_t RG, int32_t B, double* out, int64_t* n, int64_t* weight)
{
    const size_t stride = 2 + (size_t)B * rscm::kMomentBlock;
    std::vector<int64_t> div((size_t)B);
    for (size_t rg = 0; rg < RG; ++rg) {
        const int64_t* rec = sums + rg * stride;
        std::fill(div.begin(), div.end(), rec[1]);
        if (int rc = finish(rec + 2, B, div.data(), rec[0], out + rg * B)) return rc;
        if (n) n[rg] = rec[0];
        if (weight) weight[rg] = rec[1];
    }
    return RSCM_OK;
}

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
    std::vector<int64_t> sums(G * (2 + (size_t)B2 * rscm::kMomentBlock));   // B2 >= K: room for either order
    std::vector<double> tri(G * (size_t)B2);
    if (int rc = moment_sums(h, K, vec_dev, flags, 1, nullptr, sums.data(), 0)) return rc;
    if (int rc = finish_moment_sums(sums.data(), G, K, mean, n, weight)) return rc;
    if (int rc = moment_sums(h, K, vec_dev, flags, 2, mean, sums.data(), 0)) return rc;
    if (int rc = finish_moment_sums(sums.data(), G, B2, tri.data(), nullptr, nullptr)) return rc;
    for (size_t g = 0; g < G; ++g) {
        double* c = cov + g * K * K;
        for (int32_t a = 0, k = 0; a < K; ++a)
            for (int32_t b = a; b < K; ++b, ++k) c[a * K + b] = c[b * K + a] = tri[g * B2 + (size_t)k];
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
