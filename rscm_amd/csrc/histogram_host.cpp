// Host side of the histograms of stored rows, of member vectors and of two vectors jointly (rscm_ens_histogram_rows,
// rscm_ens_histogram_vectors, rscm_ens_histogram2d; the definition is stated in include/rscm_gpu.h, the kernels are in histogram.hip).
//
// A call checks the edges, resolves the rows where they are resident (resolve_rows: full storage, the window, the output store) or
// takes the caller's vectors as rows, uploads their addresses and the edges, and launches once for all rows.  The sums land in one
// zeroed int64 array [rows][G][B + 2] (counts, below, above; two dimensions: [G][Bx By + 1]) on the device, which is copied out and
// dealt to the caller's arrays with total = below + sum(counts) + above; rows beyond the time index stay zero.  Every temporary is a
// DevBuf, everything runs on the handle's stream, and one synchronise ends the call.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ens.hpp"

static_assert(RSCM_HISTOGRAM_MAX_EDGES == rscm::kHistogramMaxEdges, "the header states the kernel's edge limit");
static_assert(RSCM_HISTOGRAM_MAX_SLOTS == rscm::kHistogramMaxSlots, "the header states the slots a block keeps in LDS");
static_assert(RSCM_HISTOGRAM_MAX_VECTORS == 8, "the header states the vector limit");

namespace {

// n_tables tables of E finite, strictly ascending edges, 2 <= E <= RSCM_HISTOGRAM_MAX_EDGES
int check_edges(int32_t E, const double* edges, size_t n_tables, const char* what)
{
    if (E < 2 || E > RSCM_HISTOGRAM_MAX_EDGES || !edges)
        return fail(RSCM_ERR_INVALID, "bad %s (2 to %d finite, strictly ascending values)", what, RSCM_HISTOGRAM_MAX_EDGES);
    for (size_t t = 0; t < n_tables; ++t) {
        const double* e = edges + t * (size_t)E;
        for (int32_t j = 0; j < E; ++j)
            if (!std::isfinite(e[j]) || (j > 0 && !(e[j - 1] < e[j])))
                return fail(RSCM_ERR_INVALID, "bad %s: entry %d of table %zu is not finite or not above the one before it", what, j, t);
    }
    return RSCM_OK;
}

// the member weights, groups and baseline that the flags ask for are set
int check_flag_data(const rscm_ens* h, int32_t flags)
{
    if ((flags & RSCM_SELECT_WEIGHTED) && !h->d_weights)
        return fail(RSCM_ERR_STATE, "no member weights: rscm_ens_set_member_weights or rscm_ens_set_weights_from_loglik first");
    if ((flags & RSCM_SELECT_GROUPED) && !h->d_groups) return fail(RSCM_ERR_STATE, "no member groups: rscm_ens_set_member_groups first");
    if ((flags & RSCM_SELECT_ANOMALY) && !h->d_base)
        return fail(RSCM_ERR_STATE, "no baseline: rscm_ens_set_baseline or rscm_ens_set_baseline_values first");
    return RSCM_OK;
}

int check_slots(int64_t G, int64_t per_group, const char* product)
{
    if (G * per_group > RSCM_HISTOGRAM_MAX_SLOTS)
        return fail(RSCM_ERR_INVALID, "%lld groups x %lld slots (%s) = %lld slots: a call takes at most %d", (long long)G, (long long)per_group,
                    product, (long long)(G * per_group), RSCM_HISTOGRAM_MAX_SLOTS);
    return RSCM_OK;
}

// the histogram of the device rows `rows` among n_tables = 1 or rows.size() edge tables, dealt to counts[rows][G][B] and
// below, above, total [rows][G]; every check has been made
int histogram_of_rows(rscm_ens* h, const std::vector<const double*>& rows, int32_t E, const double* edges, bool per_row, int32_t flags,
                      int64_t* counts, int64_t* below, int64_t* above, int64_t* total)
{
    const int32_t G = (flags & RSCM_SELECT_GROUPED) ? h->n_groups : 1, B = E - 1;
    const size_t S = (size_t)E + 1, n_acc = rows.size() * G * S, n_edge = (per_row ? rows.size() : 1) * (size_t)E;
    rscm::DevBuf<const double*> d_rows;
    rscm::DevBuf<double> d_edges;
    rscm::DevBuf<unsigned long long> d_acc;
    std::vector<unsigned long long> acc(n_acc);
    if (int rc = upload_rows(h, rows, d_rows)) return rc;
    HIPCHK(d_edges.alloc(n_edge));
    HIPCHK(hipMemcpyAsync(d_edges.get(), edges, n_edge * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(d_acc.alloc(n_acc));
    HIPCHK(hipMemsetAsync(d_acc.get(), 0, n_acc * sizeof(unsigned long long), h->stream));
    rscm::HistogramArgs a{};
    a.rows = d_rows.get();
    a.edges = d_edges.get();
    a.w = (flags & RSCM_SELECT_WEIGHTED) ? h->d_weights.get() : nullptr;
    a.group = (flags & RSCM_SELECT_GROUPED) ? h->d_groups.get() : nullptr;
    a.base = (flags & RSCM_SELECT_ANOMALY) ? h->d_base.get() : nullptr;
    a.acc = d_acc.get();
    a.N = h->N;
    a.n_rows = (int32_t)rows.size();
    a.n_groups = G;
    a.n_edges = E;
    a.edge_stride = per_row ? E : 0;
    HIPCHK(rscm::launch_histogram(a, h->stream));
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc.get(), n_acc * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the temporaries and host copies go out of scope after this
    for (size_t rg = 0; rg < rows.size() * G; ++rg) {
        const unsigned long long* rec = acc.data() + rg * S;
        int64_t sum = 0;
        for (int32_t k = 0; k < B; ++k) sum += counts[rg * B + k] = (int64_t)rec[k];
        below[rg] = (int64_t)rec[B];
        above[rg] = (int64_t)rec[B + 1];
        total[rg] = below[rg] + sum + above[rg];
    }
    return RSCM_OK;
}

}  // namespace

extern "C" {

int rscm_ens_histogram_rows(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t n_edges, const double* edges,
                            int32_t flags, int64_t* counts, int64_t* below, int64_t* above, int64_t* total)
{
    GUARD_BEGIN
    NEED(h);
    if (flags & ~(RSCM_SELECT_WEIGHTED | RSCM_SELECT_ANOMALY | RSCM_SELECT_GROUPED)) return fail(RSCM_ERR_INVALID, "unknown histogram flags 0x%x", flags);
    if (int rc = check_edges(n_edges, edges, 1, "edge list")) return rc;
    if (!counts || !below || !above || !total) return fail(RSCM_ERR_INVALID, "counts, below, above or total is NULL");
    if (int rc = check_flag_data(h, flags)) return rc;
    const int32_t G = (flags & RSCM_SELECT_GROUPED) ? h->n_groups : 1, B = n_edges - 1;
    if (int rc = check_slots(G, (int64_t)B + 2, "bins + 2")) return rc;
    if (int rc = no_select(h)) return rc;
    if (int rc = check_row_range(h, var_id, t_begin, t_end, t_stride, false)) return rc;
    if (int rc = check_series_stored(h, t_end)) return rc;
    if (int rc = set_device(h)) return rc;
    const size_t n_range = t_begin < t_end ? (size_t)(((int64_t)t_end - t_begin + t_stride - 1) / t_stride) : 0;
    std::vector<const double*> rows;
    int32_t n_rows = 0;
    if (int rc = resolve_rows(h, var_id, t_begin, t_end, t_stride, rows, &n_rows)) return rc;
    std::fill(counts, counts + n_range * G * B, (int64_t)0);
    std::fill(below, below + n_range * G, (int64_t)0);
    std::fill(above, above + n_range * G, (int64_t)0);
    std::fill(total, total + n_range * G, (int64_t)0);
    if (rows.empty()) return RSCM_OK;   // the computed rows come first: resolve_rows leaves out the rows beyond the time index
    return histogram_of_rows(h, rows, n_edges, edges, false, flags, counts, below, above, total);
    GUARD_END
}

int rscm_ens_histogram_vectors(rscm_ens* h, int32_t n_vec, const double* const* vec_dev, int32_t n_edges, const double* edges,
                               int32_t edges_per_vector, int32_t flags, int64_t* counts, int64_t* below, int64_t* above, int64_t* total)
{
    GUARD_BEGIN
    NEED(h);
    if (flags & RSCM_SELECT_ANOMALY) return fail(RSCM_ERR_INVALID, "RSCM_SELECT_ANOMALY applies to stored rows, not to histograms of vectors");
    if (flags & ~(RSCM_SELECT_WEIGHTED | RSCM_SELECT_GROUPED)) return fail(RSCM_ERR_INVALID, "unknown histogram flags 0x%x", flags);
    if (n_vec < 1 || n_vec > RSCM_HISTOGRAM_MAX_VECTORS || !vec_dev)
        return fail(RSCM_ERR_INVALID, "bad vector list (1 to %d vectors)", RSCM_HISTOGRAM_MAX_VECTORS);
    if (int rc = check_edges(n_edges, edges, edges_per_vector ? (size_t)n_vec : 1, "edge list")) return rc;
    if (!counts || !below || !above || !total) return fail(RSCM_ERR_INVALID, "counts, below, above or total is NULL");
    if (int rc = check_flag_data(h, flags)) return rc;
    const int32_t G = (flags & RSCM_SELECT_GROUPED) ? h->n_groups : 1;
    if (int rc = check_slots(G, (int64_t)n_edges + 1, "bins + 2")) return rc;
    if (int rc = no_select(h)) return rc;
    if (int rc = check_member_vectors(h, n_vec, vec_dev)) return rc;
    const std::vector<const double*> rows(vec_dev, vec_dev + n_vec);
    return histogram_of_rows(h, rows, n_edges, edges, edges_per_vector != 0, flags, counts, below, above, total);
    GUARD_END
}

int rscm_ens_histogram2d(rscm_ens* h, const double* x_dev, const double* y_dev, int32_t n_edges_x, const double* edges_x, int32_t n_edges_y,
                         const double* edges_y, int32_t flags, int64_t* counts, int64_t* outside, int64_t* total)
{
    GUARD_BEGIN
    NEED(h);
    if (flags & RSCM_SELECT_ANOMALY) return fail(RSCM_ERR_INVALID, "RSCM_SELECT_ANOMALY applies to stored rows, not to histograms of vectors");
    if (flags & ~(RSCM_SELECT_WEIGHTED | RSCM_SELECT_GROUPED)) return fail(RSCM_ERR_INVALID, "unknown histogram flags 0x%x", flags);
    if (int rc = check_edges(n_edges_x, edges_x, 1, "edge list of x")) return rc;
    if (int rc = check_edges(n_edges_y, edges_y, 1, "edge list of y")) return rc;
    if (!counts || !outside || !total) return fail(RSCM_ERR_INVALID, "counts, outside or total is NULL");
    if (int rc = check_flag_data(h, flags)) return rc;
    const int32_t G = (flags & RSCM_SELECT_GROUPED) ? h->n_groups : 1;
    const size_t cells = (size_t)(n_edges_x - 1) * (size_t)(n_edges_y - 1), S = cells + 1, n_acc = (size_t)G * S;
    if (int rc = check_slots(G, (int64_t)S, "bins of x x bins of y + 1")) return rc;
    if (int rc = no_select(h)) return rc;
    const double* const vec[2] = {x_dev, y_dev};
    if (int rc = check_member_vectors(h, 2, vec)) return rc;

    std::vector<double> e(edges_x, edges_x + n_edges_x);
    e.insert(e.end(), edges_y, edges_y + n_edges_y);
    rscm::DevBuf<double> d_edges;
    rscm::DevBuf<unsigned long long> d_acc;
    std::vector<unsigned long long> acc(n_acc);
    HIPCHK(d_edges.alloc(e.size()));
    HIPCHK(hipMemcpyAsync(d_edges.get(), e.data(), e.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(d_acc.alloc(n_acc));
    HIPCHK(hipMemsetAsync(d_acc.get(), 0, n_acc * sizeof(unsigned long long), h->stream));
    rscm::Histogram2dArgs a{};
    a.x = x_dev;
    a.y = y_dev;
    a.edges = d_edges.get();
    a.w = (flags & RSCM_SELECT_WEIGHTED) ? h->d_weights.get() : nullptr;
    a.group = (flags & RSCM_SELECT_GROUPED) ? h->d_groups.get() : nullptr;
    a.acc = d_acc.get();
    a.N = h->N;
    a.n_groups = G;
    a.n_edges_x = n_edges_x;
    a.n_edges_y = n_edges_y;
    HIPCHK(rscm::launch_histogram2d(a, h->stream));
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc.get(), n_acc * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the temporaries and host copies go out of scope after this
    for (int32_t g = 0; g < G; ++g) {
        const unsigned long long* rec = acc.data() + (size_t)g * S;
        int64_t sum = 0;
        for (size_t k = 0; k < cells; ++k) sum += counts[(size_t)g * cells + k] = (int64_t)rec[k];
        outside[g] = (int64_t)rec[cells];
        total[g] = sum + outside[g];
    }
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
