// Baseline terms marginalised under correlated noise: scan_rows_kernel<ONE, OuColsFilter<K>> (trxg_chi2_grid_ou_baseline,
// include/trx_gls.h).  Included by trx_kernels.hip only, after trx_noise.hpp.
//
// With y = flux - model[r], the Kalman tables alpha, beta, omega of the dataset's noise (datasets.ou_system) and the
// innovations z[x]_n = x_n - g_n, g_0 = 0, g_n = alpha_n g_(n-1) + beta_n x_(n-1), the row's term is
//     S2 = sum_n omega_n z[y]_n^2,   b~_k = sum_n c_k[n] z[y]_n,   h[r] = 0.5 max(S2 - b~^T M b~, 0),
// c_k[n] = omega_n z[B_k]_n / sqrt(D_k) the whitened, scaled columns from the host (datasets.ou_baseline_system: they do
// not depend on the row) and M the inverse of the scaled system matrix, packed upper triangle by rows, by value in the
// kernel arguments.  coef_out[r][i] = sum_j M_ij b~_j.
//
// What OuColsFilter<K> adds to OuFilter (trx_noise.hpp): a trip's tables hold the lane's pair of every column next to
// OuTrip, and next to acc = sum omega z^2 -- the same ou_innovations, the same two fma, so M = 0 gives trxn_chi2_grid_ou's
// bits -- a lane keeps the K sums fma(c_k[n], z_n, acc_k) over the same z0, z1.  wave_sum for S2 and one gls_wave_total --
// the same total in the scan's DPP moves -- per column sum; the store is Chi2Baseline<K>'s (clamp at 0, a NaN stays a NaN,
// secdepth / sec_limit / accumulate as chi2w_store).
#pragma once
#include "trx_noise.hpp"

namespace {

// K from which the kernel needs more than 128 VGPRs, so that two waves a SIMD are resident instead of four
// (trxg_chi2_grid_ou_baseline's blocks a CU; tests/test_build_resources_gls.py holds this against the code object's
// register counts).  The build reports 66 - 82 VGPRs at K <= 2 and 86 - 114 at K = 3, 4: no K is wide.
constexpr int kGlsWideFrom = 5;

// the lane's pair of every whitened column in a trip: 0 past the row's end
// (indexed by unrolled loops over the template argument only, so it lives in registers)
template <int K>
struct GlsCols {
    double c0[K], c1[K];
};

template <int K>
__device__ __forceinline__ GlsCols<K> gls_cols(const double* __restrict__ columns, int n_time, int base, int lane)
{
    const int n0 = base + 2 * lane, n1 = n0 + 1;
    GlsCols<K> c;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double* ck = columns + (size_t)k * n_time;
        c.c0[k] = n0 < n_time ? ck[n0] : 0.0;
        c.c1[k] = n1 < n_time ? ck[n1] : 0.0;
    }
    return c;
}

// The total of a lane value over the wave in the scan's DPP moves (ou_scan_source with the addend 0 outside a step's reach:
// after the six steps lane 63 holds the sum of all 64), read back to every lane.  The K column sums take this in place of
// wave_sum's butterfly: that is twelve ds_bpermute a sum and row through the LDS crossbar the CU's four SIMDs share, and
// at one trip a row (n_time <= 128) K of them outweigh the row's scan (measured at 100 stamps, K = 4: 2.20 x the OU filter
// with wave_sum, 1.57 x with this; profiles/gls/results.txt).  S2 keeps wave_sum: its bits are the OU filter's.
template <int S>
__device__ __forceinline__ void gls_fold(double& v)
{
    v += ou_scan_source<S>(v, 0.0);
    if constexpr (S < 5) gls_fold<S + 1>(v);
}

__device__ __forceinline__ double gls_wave_total(double v)
{
    gls_fold<0>(v);
    return wave_read_lane<63>(v);
}

template <int K>
struct OuColsFilter {
    static_assert(K >= 1 && K <= kChi2bMaxTerms, "one to four columns");
    struct Trip {
        OuTrip t;
        GlsCols<K> c;
    };
    struct Row {
        double carry = 0.0;
        Chi2Sums<K> s;
    };
    const double *alpha, *beta, *omega, *columns;
    Chi2Baseline<K> terms;            // (wbasis unused: the columns come through the trip's tables)
    __device__ __forceinline__ Trip trip(const double* __restrict__ flux, int n_time, int base, int lane) const
    {
        return {ou_trip(flux, alpha, beta, omega, n_time, base, lane), gls_cols<K>(columns, n_time, base, lane)};
    }
    static __device__ __forceinline__ void row_trip(const Trip& t, double m0, double m1, Row& row, int lane)
    {
        double z0, z1;
        const double uinc = ou_innovations(t.t, m0, m1, row.carry, lane, z0, z1);
        row.s.s2 = fma(t.t.w0 * z0, z0, row.s.s2);
        row.s.s2 = fma(t.t.w1 * z1, z1, row.s.s2);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            row.s.x[k] = fma(t.c.c0[k], z0, row.s.x[k]);
            row.s.x[k] = fma(t.c.c1[k], z1, row.s.x[k]);
        }
        row.carry = wave_read_lane<63>(uinc);
    }
    static __device__ __forceinline__ void wave_sums(Row& row)
    {
        row.s.s2 = wave_sum(row.s.s2);
#pragma unroll
        for (int k = 0; k < K; ++k) row.s.x[k] = gls_wave_total(row.s.x[k]);
    }
    __device__ __forceinline__ void store(const Row& row, long r, const double* __restrict__ secdepth, double sec_limit,
                                          int accumulate, double* __restrict__ out) const
    {
        terms.store(row.s, r, secdepth, sec_limit, accumulate, out);
    }
};

}  // namespace
