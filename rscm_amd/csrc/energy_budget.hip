// Energy-budget diagnostics of a two-layer handle for gfx950 (MI355X): the member's forcing, its radiative response, its deep-ocean heat
// uptake and its top-of-atmosphere imbalance as rows, pointwise functions of the stored rows, the parameters and the forcing the
// stepping kernel applies.  The definition is the one include/rscm_gpu.h states under "energy-budget diagnostics"; every line of
// budget_of below is one f64 operation rounded on its own (-ffp-contract=off: no FMA), the same in either arithmetic mode.
//
// The forcing statements are those documented at the head of two_layer_body.hpp (MIX, NOISE), restated here from the same helpers
// (forcing_noise.hpp, param_at, the noise-kind constants) so that the stepping kernels' translation unit is not touched:
//   plain   F = table[scen][f]
//   mix     F = S_0[f] * c_0;  F = F + S_k[f] * c_k  for k = 1 .. K - 1 in order
//   white   F = F + sigma * z(seed, member0 + i, f)
//   red     F = F + e_f,  e_0 = sigma z_0,  e_f = (phi e_{f-1}) + ((sigma sqrt(1 - phi phi)) z_f); per-member: sigma_i, phi_i from their rows
//
// budget_tile_kernel<FORCED, MIX, WHITE>: one thread per member (x, 256 threads) and one tile of kDiagTile rows per block (y), the shape
// of diagnostic.hip; the two loads of kDiagBatch rows are issued before the first is used.  Traffic 24 B per element (Ts, Td, the
// result); the six parameters and the mix coefficients are read once per thread and tile, the scenario table through L2.
// budget_walk_kernel<MIX, MEMBERS>: red and per-member noise.  e is a recurrence from forcing index 0, so one thread per member walks
// the indices in ascending order up to the last one a requested row reads and writes each requested row as it passes it, as
// forcing_noise_rows_kernel does; no [R][N] noise rows are materialised.  No LDS, no scratch in either.
#include <hip/hip_runtime.h>

#include "diagnostic.hpp"
#include "energy_budget.hpp"
#include "forcing_noise.hpp"
#include "rscm_device.hpp"

namespace rscm {

namespace {

constexpr int kBudgetThreads = 256;

struct BudgetMember {
    double p0, p1, p3, ee;   // lambda0, a, eta, efficacy * eta
};

__device__ __forceinline__ BudgetMember budget_member(const EnergyBudgetArgs& a, int64_t i)
{
    BudgetMember m;
    m.p0 = param_at(a.d_params, a.uniform_rows, 0, a.N, i);
    m.p1 = param_at(a.d_params, a.uniform_rows, 1, a.N, i);
    const double p2 = param_at(a.d_params, a.uniform_rows, 2, a.N, i);
    m.p3 = param_at(a.d_params, a.uniform_rows, 3, a.N, i);
    m.ee = p2 * m.p3;
    return m;
}

// scale * the quantity; F is read only by the two quantities that have it
__device__ __forceinline__ double budget_of(int32_t quantity, double scale, const BudgetMember& m, double ts, double td, double F)
{
    const double d = ts - td;
    const double u = m.p1 * ts;
    const double lam = m.p0 - u;
    const double R = lam * ts;
    const double X = m.ee * d;
    const double H = m.p3 * d;
    double g = F - R;
    g = g - X;
    const double N = g + H;
    const double q = quantity == kBudgetForcing ? F : quantity == kBudgetResponse ? R : quantity == kBudgetDeepUptake ? H : N;
    return scale * q;
}

// The member's shared forcing before the noise: its scenario's table value, or the mix sum
template <bool MIX>
struct BudgetForcing {
    const double* row0;   // the member's scenario: [T], a mix handle's [K][T]
    int32_t n_times, n_comp;
    double coeff[MIX ? kMaxForcingComponents : 1];

    __device__ __forceinline__ void init(const EnergyBudgetArgs& a, int64_t i)
    {
        const int32_t scen = a.d_scen ? a.d_scen[i] : 0;
        n_times = a.n_times;
        n_comp = MIX ? a.n_comp : 1;   // wave-uniform (kernarg)
        row0 = a.d_forcing + (int64_t)scen * n_comp * n_times;
        if constexpr (MIX) {
#pragma unroll
            for (int k = 0; k < kMaxForcingComponents; ++k)
                coeff[k] = k < n_comp ? param_at(a.d_params, a.uniform_rows, kTwoLayerCoeff0 + k, a.N, i) : 0.0;
        }
    }
    __device__ __forceinline__ double at(int32_t f) const
    {
        if constexpr (MIX) {
            double F = row0[f] * coeff[0];
#pragma unroll
            for (int k = 1; k < kMaxForcingComponents; ++k)
                if (k < n_comp) F = F + row0[(int64_t)k * n_times + f] * coeff[k];
            return F;
        } else {
            return row0[f];
        }
    }
};

template <bool FORCED, bool MIX, bool WHITE>
__global__ __launch_bounds__(kBudgetThreads) void budget_tile_kernel(EnergyBudgetArgs a)
{
    static_assert(FORCED || (!MIX && !WHITE), "a quantity without forcing has one instance");
    const int64_t i = (int64_t)blockIdx.x * kBudgetThreads + threadIdx.x;
    if (i >= a.N) return;
    const int32_t r_end = min((int32_t)(blockIdx.y + 1) * kDiagTile, a.n_rows);
    int32_t r = (int32_t)blockIdx.y * kDiagTile;

    const BudgetMember m = budget_member(a, i);
    [[maybe_unused]] BudgetForcing<MIX> table;
    if constexpr (FORCED) table.init(a, i);
    [[maybe_unused]] const uint64_t g = (uint64_t)(a.noise_member0 + i);
    auto forcing_of = [&](int32_t row) -> double {
        if constexpr (FORCED) {
            const int32_t f = a.f0 + row * a.f_stride;
            const double F = table.at(f);
            if constexpr (WHITE) return F + a.noise_sigma * noise::draw(a.noise_seed, g, (uint32_t)f);
            else return F;
        } else {
            return 0.0;
        }
    };

    const double* const* __restrict__ rows = a.d_rows;
    double* __restrict__ out = a.d_out;
    for (; r + kDiagBatch <= r_end; r += kDiagBatch) {
        double ts[kDiagBatch], td[kDiagBatch];
#pragma unroll
        for (int j = 0; j < kDiagBatch; ++j) {
            ts[j] = rows[r + j][i];
            td[j] = rows[(int64_t)a.n_rows + r + j][i];
        }
#pragma unroll
        for (int j = 0; j < kDiagBatch; ++j) out[(int64_t)(r + j) * a.N + i] = budget_of(a.quantity, a.scale, m, ts[j], td[j], forcing_of(r + j));
    }
    for (; r < r_end; ++r) {
        const double ts = rows[r][i], td = rows[(int64_t)a.n_rows + r][i];
        out[(int64_t)r * a.N + i] = budget_of(a.quantity, a.scale, m, ts, td, forcing_of(r));
    }
}

template <bool MIX, bool MEMBERS>
__global__ __launch_bounds__(kBudgetThreads) void budget_walk_kernel(EnergyBudgetArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kBudgetThreads + threadIdx.x;
    if (i >= a.N) return;
    const BudgetMember m = budget_member(a, i);
    BudgetForcing<MIX> table;
    table.init(a, i);
    const uint64_t g = (uint64_t)(a.noise_member0 + i);
    double sigma = a.noise_sigma, phi = a.noise_phi;
    if constexpr (MEMBERS) {
        sigma = param_at(a.d_params, a.uniform_rows, a.noise_sigma_row, a.N, i);
        phi = param_at(a.d_params, a.uniform_rows, a.noise_phi_row, a.N, i);
    }
    const double se = sigma * __builtin_sqrt(1.0 - phi * phi);
    const double* const* __restrict__ rows = a.d_rows;
    double* __restrict__ out = a.d_out;
    double e = 0.0;
    int32_t r = 0, next = a.f0;   // row r reads index `next`; f_stride >= 1, so the rows are met in order
    const int32_t f_end = a.f0 + (a.n_rows - 1) * a.f_stride + 1;
    for (int32_t f = 0; f < f_end; ++f) {
        const double z = noise::draw(a.noise_seed, g, (uint32_t)f);
        e = f == 0 ? sigma * z : (phi * e) + (se * z);
        if (f == next) {   // wave-uniform
            const double ts = rows[r][i], td = rows[(int64_t)a.n_rows + r][i];
            out[(int64_t)r * a.N + i] = budget_of(a.quantity, a.scale, m, ts, td, table.at(f) + e);
            ++r;
            next += a.f_stride;
        }
    }
}

}  // namespace

hipError_t launch_energy_budget(const EnergyBudgetArgs& a, int32_t noise_kind, hipStream_t s)
{
    if (a.N <= 0 || a.n_rows <= 0) return hipSuccess;
    if (a.quantity < kBudgetForcing || a.quantity > kBudgetImbalance || !a.d_rows || !a.d_params || !a.d_out) return hipErrorInvalidValue;
    const bool forced = budget_reads_forcing(a.quantity);
    const bool mix = a.n_comp > 0;
    const dim3 block(kBudgetThreads);
    const unsigned gx = (unsigned)((a.N + kBudgetThreads - 1) / kBudgetThreads);
    void (*kern)(EnergyBudgetArgs) = budget_tile_kernel<false, false, false>;
    bool walk = false;
    if (forced) {
        if (!a.d_forcing || a.n_comp < 0 || a.n_comp > kMaxForcingComponents || a.f0 < 0 || a.f_stride < 1 ||
            (int64_t)a.f0 + (int64_t)(a.n_rows - 1) * a.f_stride >= a.n_times)
            return hipErrorInvalidValue;
        switch (noise_kind) {
            case kNoiseKindNone: kern = mix ? budget_tile_kernel<true, true, false> : budget_tile_kernel<true, false, false>; break;
            case kNoiseKindWhite: kern = mix ? budget_tile_kernel<true, true, true> : budget_tile_kernel<true, false, true>; break;
            case kNoiseKindRed:
                kern = mix ? budget_walk_kernel<true, false> : budget_walk_kernel<false, false>;
                walk = true;
                break;
            case kNoiseKindMembers:
                if (a.noise_sigma_row < 0 || a.noise_phi_row < 0) return hipErrorInvalidValue;
                kern = mix ? budget_walk_kernel<true, true> : budget_walk_kernel<false, true>;
                walk = true;
                break;
            default: return hipErrorInvalidValue;
        }
    }
    const dim3 grid(gx, walk ? 1u : (unsigned)((a.n_rows + kDiagTile - 1) / kDiagTile));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace rscm
