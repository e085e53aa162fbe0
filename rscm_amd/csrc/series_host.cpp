// Host side of the per-member series statistics of one variable or a pair -- rscm_ens_member_variability, _spectrum,
// _covariability and _cross_spectrum -- and of the spectral tables (rscm_gpu_spectrum_coefficients, rscm_gpu_spectrum_sines); kernels
// in variability.hip, spectrum.hip, covariability.hip and cross_spectrum.hip over series_walk.hpp.  What the four entry points
// share is stated once: the call's frame (SeriesCall), the spectral table (SpectralTable) and the folding of an angle into the first
// octant.  The statistics share the rows and the slots of the indicators (indicators_host.cpp).
#include <cmath>
#include <cstring>

#include "ens.hpp"

namespace {

static_assert(rscm::kVarMean == RSCM_VAR_MEAN && rscm::kVarLinear == RSCM_VAR_LINEAR && rscm::kVarDifference == RSCM_VAR_DIFFERENCE,
              "the detrending modes in rscm_device.hpp and rscm_gpu.h must agree");
static_assert(5 <= 3 + rscm::kMaxThresholds, "the variability statistics share the indicator slots");
static_assert(rscm::kCovMaxLags == RSCM_COV_MAX_LAGS && 5 + 2 * RSCM_COV_MAX_LAGS <= 3 + rscm::kMaxThresholds,
              "the covariability statistics at every lag share the indicator slots");
static_assert(rscm::kMaxCrossSpectrumBands == RSCM_XSPEC_MAX_BANDS && 2 + 3 * RSCM_XSPEC_MAX_BANDS <= 3 + rscm::kMaxThresholds,
              "the cross-spectrum statistics of every band share the indicator slots");

constexpr int32_t kSpectrumMaxTerms = 4096;   // the cap on the working series' length that bounds the recurrence's error

int check_detrending(int32_t mode)
{
    if (mode != RSCM_VAR_MEAN && mode != RSCM_VAR_LINEAR && mode != RSCM_VAR_DIFFERENCE)
        return fail(RSCM_ERR_INVALID, "unknown detrending mode %d (RSCM_VAR_MEAN, RSCM_VAR_LINEAR, RSCM_VAR_DIFFERENCE)", mode);
    return RSCM_OK;
}

// The working series of n_rows rows under a detrending mode: its length n, 3 to max_terms (0: no upper bound), and stt = n (n^2 - 1) / 12
struct WorkingSeries {
    int64_t n = 0;
    double stt = 0.0;
};
int working_series(size_t n_rows, int32_t mode, int32_t max_terms, WorkingSeries* w)
{
    const int64_t n = (int64_t)n_rows - (mode == RSCM_VAR_DIFFERENCE ? 1 : 0);
    if (n < 3 && !max_terms) return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: at least 3 are needed", (int)n_rows, (long long)n);
    if (max_terms && (n < 3 || n > max_terms))
        return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: 3 to %d are needed", (int)n_rows, (long long)n, max_terms);
    w->n = n;
    w->stt = (double)(n * (n * n - 1)) / 12.0;
    return RSCM_OK;
}

// The frame of one call on K = 1 or 2 variables; an entry point is its own checks and one launch between these steps, in this order
struct SeriesCall {
    rscm_ens* h;
    int32_t slot;
    void** out_dev;
    int K;
    int32_t var[2], mode[2];
    std::vector<const double*> rows[2];
    rscm::DevBuf<const double*> d_rows[2];
    WorkingSeries w;

    int32_t n_rows() const { return (int32_t)rows[0].size(); }
    double* out() const { return h->d_ind[slot]; }

    // what is refused before the entry point's own arguments are looked at
    int check_args()
    {
        NEED(h);
        if (!out_dev) return fail(RSCM_ERR_INVALID, "out_dev is NULL");
        *out_dev = nullptr;
        if (int rc = check_slot(slot)) return rc;
        for (int v = 0; v < K; ++v)
            if (int rc = check_detrending(mode[v])) return rc;
        return RSCM_OK;
    }
    // The rows of each variable and the common working series, of at most max_terms terms (0: no cap) and at least 3 + n_lags: every
    // series of the call has the length of the differenced one as soon as any variable is differenced (the others are taken at the
    // midpoints)
    int resolve(int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t max_terms, int32_t n_lags)
    {
        if (int rc = no_select(h)) return rc;
        bool differenced = false;
        for (int v = 0; v < K; ++v) {
            std::vector<double> times;
            if (int rc = period_rows(h, var[v], t_begin, t_end, t_stride, rows[v], times)) return rc;
            differenced = differenced || mode[v] == RSCM_VAR_DIFFERENCE;
        }
        if (int rc = working_series(rows[0].size(), differenced ? RSCM_VAR_DIFFERENCE : RSCM_VAR_MEAN, max_terms, &w)) return rc;
        if (w.n < 3 + n_lags)
            return fail(RSCM_ERR_INVALID, "the working series of %d rows has %lld terms: at least %d are needed at %d lags", n_rows(), (long long)w.n,
                        3 + n_lags, n_lags);
        return RSCM_OK;
    }
    // the handle's device, the slot's buffer and the row pointers on their way to the device
    int to_device()
    {
        if (int rc = set_device(h)) return rc;
        if (int rc = slot_buffer(h, slot)) return rc;
        for (int v = 0; v < K; ++v)
            if (int rc = upload_rows(h, rows[v], d_rows[v])) return rc;
        return RSCM_OK;
    }
    // after the launch: wait for it and hand the slot out
    int finish()
    {
        HIPCHK(hipStreamSynchronize(h->stream));
        *out_dev = out();
        return RSCM_OK;
    }
};

// out[j - 1], j = 1 .. (n - 1) / 2: the double nearest sin(2 pi j / n) (sine; every entry > 0), else 2 C_j with C_j the double nearest
// cos(2 pi j / n).  The angle is pi p / q with p = 2 j, q = n, 0 < p / q < 1; in integers it is folded first into the first quadrant
// (p -> q - p: the cosine changes its sign, the sine keeps it) and then into the first octant, where the function of the complement
// is the other function of what is left: both are evaluated in long double below pi / 4 only, so no argument loses bits to
// cancellation near pi / 2, and 2 p == q is +0.0 or 1.0 exactly.
void circle_table(int32_t n, bool sine, double* out)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    const int64_t q = n;
    for (int64_t j = 1; j <= (n - 1) / 2; ++j) {
        int64_t p = 2 * j;
        const bool neg = 2 * p > q;
        if (neg) p = q - p;
        const bool octant = 4 * p <= q;
        const long double x = octant ? pi * (long double)p / (long double)q : pi * (long double)(q - 2 * p) / (long double)(2 * q);
        const long double v = 2 * p == q ? (sine ? 1.0L : 0.0L) : sine == octant ? sinl(x) : cosl(x);
        const double r = (double)v;
        out[j - 1] = sine ? r : 2.0 * (neg ? -r : r);
    }
}

// rscm_gpu_spectrum_coefficients and rscm_gpu_spectrum_sines
int table_accessor(int32_t n, bool sine, double* out)
{
    if (n < 3 || n > kSpectrumMaxTerms) return fail(RSCM_ERR_INVALID, "n = %d: the working series has 3 to %d terms", n, kSpectrumMaxTerms);
    if (!out) return fail(RSCM_ERR_INVALID, "out is NULL");
    circle_table(n, sine, out);
    return RSCM_OK;
}

// The band list of the spectral entry points: its shape against the entry's maximum, and its edges against a working series of n terms
int check_band_list(int32_t n_bands, int32_t max_bands, const int32_t* edges)
{
    if (n_bands < 1 || n_bands > max_bands || !edges) return fail(RSCM_ERR_INVALID, "bad band list (1 to %d bands, n_bands + 1 edges)", max_bands);
    return RSCM_OK;
}
int check_band_edges(int64_t n, int32_t n_bands, const int32_t* edges)
{
    const int32_t J = (int32_t)((n - 1) / 2);
    if (edges[0] < 1 || edges[n_bands] > J + 1) return fail(RSCM_ERR_INVALID, "the band edges must lie in [1, %d] (J + 1 of %lld terms)", J + 1, (long long)n);
    for (int32_t b = 0; b < n_bands; ++b)
        if (edges[b] >= edges[b + 1]) return fail(RSCM_ERR_INVALID, "the band edges must be strictly ascending (edge %d)", b + 1);
    return RSCM_OK;
}

// The one table a spectral kernel is given, for the J = (n - 1) / 2 frequencies of n terms: c2[J], with sines g[J] after it, each
// followed by kSpectrumTablePad zeros the last tile may read, then the int32 edges (8-byte aligned: the table counts in doubles)
struct SpectralTable {
    std::vector<double> host;   // the source of the asynchronous copy: lives until the call has synchronised the stream
    rscm::DevBuf<double> dev;
    size_t n_tab = 0, n_sets = 1;

    int build(int64_t n, bool sines, int32_t n_bands, const int32_t* edges)
    {
        if (int rc = check_band_edges(n, n_bands, edges)) return rc;
        n_tab = (size_t)((n - 1) / 2) + rscm::kSpectrumTablePad;
        n_sets = sines ? 2 : 1;
        host.assign(n_sets * n_tab + (size_t)(n_bands + 2) / 2, 0.0);
        circle_table((int32_t)n, false, host.data());
        if (sines) circle_table((int32_t)n, true, host.data() + n_tab);
        std::memcpy(host.data() + n_sets * n_tab, edges, (size_t)(n_bands + 1) * sizeof(int32_t));
        return RSCM_OK;
    }
    int upload(hipStream_t stream)
    {
        HIPCHK(dev.alloc(host.size()));
        HIPCHK(hipMemcpyAsync(dev.get(), host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        return RSCM_OK;
    }
    const double* c2() const { return dev.get(); }
    const double* g() const { return dev.get() + n_tab; }
    const int32_t* edges() const { return reinterpret_cast<const int32_t*>(dev.get() + n_sets * n_tab); }
};

}  // namespace

extern "C" {

int rscm_ens_member_variability(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode, int32_t slot,
                                void** out_dev)
{
    GUARD_BEGIN
    SeriesCall c{h, slot, out_dev, 1, {var_id}, {mode}};
    if (int rc = c.check_args()) return rc;
    if (int rc = c.resolve(t_begin, t_end, t_stride, 0, 0)) return rc;
    if (int rc = c.to_device()) return rc;
    HIPCHK(rscm::launch_variability(c.d_rows[0].get(), c.n_rows(), mode, c.w.stt, h->N, c.out(), h->stream));
    return c.finish();
    GUARD_END
}

int rscm_ens_member_covariability(rscm_ens* h, int32_t var_x, int32_t var_y, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode_x,
                                  int32_t mode_y, int32_t n_lags, int32_t slot, void** out_dev)
{
    GUARD_BEGIN
    SeriesCall c{h, slot, out_dev, 2, {var_x, var_y}, {mode_x, mode_y}};
    if (int rc = c.check_args()) return rc;
    if (n_lags < 0 || n_lags > RSCM_COV_MAX_LAGS) return fail(RSCM_ERR_INVALID, "n_lags = %d: must be in [0, %d]", n_lags, RSCM_COV_MAX_LAGS);
    if (int rc = c.resolve(t_begin, t_end, t_stride, 0, n_lags)) return rc;
    if (int rc = c.to_device()) return rc;
    HIPCHK(rscm::launch_covariability(c.d_rows[0].get(), c.d_rows[1].get(), c.n_rows(), mode_x, mode_y, n_lags, c.w.stt, h->N, c.out(), h->stream));
    return c.finish();
    GUARD_END
}

int rscm_gpu_spectrum_coefficients(int32_t n, double* out)
{
    GUARD_BEGIN
    return table_accessor(n, false, out);
    GUARD_END
}

int rscm_gpu_spectrum_sines(int32_t n, double* out)
{
    GUARD_BEGIN
    return table_accessor(n, true, out);
    GUARD_END
}

int rscm_ens_member_spectrum(rscm_ens* h, int32_t var_id, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode, int32_t n_bands,
                             const int32_t* edges, int32_t slot, void** out_dev)
{
    GUARD_BEGIN
    SeriesCall c{h, slot, out_dev, 1, {var_id}, {mode}};
    SpectralTable t;
    if (int rc = c.check_args()) return rc;
    if (int rc = check_band_list(n_bands, rscm::kMaxSpectrumBands, edges)) return rc;
    if (int rc = c.resolve(t_begin, t_end, t_stride, kSpectrumMaxTerms, 0)) return rc;
    if (int rc = t.build(c.w.n, false, n_bands, edges)) return rc;
    if (int rc = c.to_device()) return rc;
    if (int rc = t.upload(h->stream)) return rc;
    HIPCHK(rscm::launch_spectrum(c.d_rows[0].get(), c.n_rows(), mode, c.w.stt, t.c2(), t.edges(), n_bands, h->N, c.out(), h->stream));
    return c.finish();
    GUARD_END
}

int rscm_ens_member_cross_spectrum(rscm_ens* h, int32_t var_x, int32_t var_y, int32_t t_begin, int32_t t_end, int32_t t_stride, int32_t mode_x,
                                   int32_t mode_y, int32_t n_bands, const int32_t* edges, int32_t slot, void** out_dev)
{
    GUARD_BEGIN
    SeriesCall c{h, slot, out_dev, 2, {var_x, var_y}, {mode_x, mode_y}};
    SpectralTable t;
    if (int rc = c.check_args()) return rc;
    if (int rc = check_band_list(n_bands, RSCM_XSPEC_MAX_BANDS, edges)) return rc;
    if (int rc = c.resolve(t_begin, t_end, t_stride, kSpectrumMaxTerms, 0)) return rc;
    if (int rc = t.build(c.w.n, true, n_bands, edges)) return rc;
    if (int rc = c.to_device()) return rc;
    if (int rc = t.upload(h->stream)) return rc;
    HIPCHK(rscm::launch_cross_spectrum(c.d_rows[0].get(), c.d_rows[1].get(), c.n_rows(), mode_x, mode_y, c.w.stt, t.c2(), t.g(), t.edges(), n_bands,
                                       h->N, c.out(), h->stream));
    return c.finish();
    GUARD_END
}

}  // extern "C"
