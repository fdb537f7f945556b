// Baseline terms marginalised under correlated noise with a two-dimensional state: scan_rows_kernel<ONE, Ss2ColsFilter<K>>
// (trxk_chi2_grid_ss2_baseline, include/trx_ss.h).  Included by trx_kernels.hip only, after
// trx_ss2.hpp and trx_gls.hpp.
//
// With y = flux - model[r], the Kalman tables A, g, omega of the dataset's noise (datasets.ss2_system) and the innovations
// z[x]_n = x_n - u_(n-1)[0], u_(-1) = 0, u_n = A_n u_(n-1) + g_n x_n, the row's term is
//     S2 = sum_n omega_n z[y]_n^2,   b~_k = sum_n c_k[n] z[y]_n,   h[r] = 0.5 max(S2 - b~^T M b~, 0),
// c_k[n] = omega_n z[B_k]_n / sqrt(D_k) the whitened, scaled columns from the host (datasets.ss2_baseline_system: they do
// not depend on the row) and M the inverse of the scaled system matrix, packed upper triangle by rows, by value in the
// kernel arguments.  coef_out[r][i] = sum_j M_ij b~_j.
//
// Ss2ColsFilter<K> is to Ss2Filter (trx_ss2.hpp) what OuColsFilter<K> (trx_gls.hpp) is to OuFilter: a trip's tables hold
// the lane's pair of every column next to Ss2Trip, and next to s2 = sum omega z^2 -- the same ss2_innovations, the same two
// fma, so M = 0 gives trxs_chi2_grid_ss2's bits -- a lane keeps the K sums fma(c_k[n], z_n, x_k) over the same z0, z1.
// wave_sum for S2 and one gls_wave_total per column sum; the store is Chi2Baseline<K>'s.  No LDS, no workspace: a row's
// bits depend on n_time, the tables and its values alone.
#pragma once
#include "trx_ss2.hpp"
#include "trx_gls.hpp"

namespace {

// Blocks of 256 threads a CU that trxk_chi2_grid_ss2_baseline caps its grid at, per instantiation: [ONE][K - 1].  The
// kernel has no LDS, so its registers decide what is resident: 4 waves a SIMD at up to 128 VGPRs, 3 at up to 168, 2
// beyond (512 registers a lane and SIMD, allotted in eights).  Ss2Trip alone is 39 doubles; a column adds two to the
// trip and one per row in flight.  The build reports 130 / 138 / 146 / 155 VGPRs at K = 1 .. 4 and 116 / 130 / 124 / 162
// with ONE (the scheduler's outcome, not monotonic in K); tests/test_build_resources_ss2_cols.py holds every entry against
// the code object's register count.  Measured at 100 stamps, the fourth wave is worth 10 - 13 % (K = 1, 3 capped at 3
// blocks a CU against 4: profiles/ss2_gls/results.txt), so an entry says 4 wherever the count allows it.
constexpr int kSs2ColsBlocksPerCu[2][kChi2bMaxTerms] = {
    {3, 3, 3, 3},                     // a trip's tables formed per trip (n_time > kOuTrip), K = 1 .. 4
    {4, 3, 4, 3},                     // ONE: formed once per wave
};

constexpr int ss2_cols_blocks_per_cu(bool one, int k) { return kSs2ColsBlocksPerCu[one ? 1 : 0][k - 1]; }

template <int K>
struct Ss2ColsFilter {
    static_assert(K >= 1 && K <= kChi2bMaxTerms, "one to four columns");
    struct Trip {
        Ss2Trip t;
        GlsCols<K> c;
    };
    struct Row {
        Ss2Vec carry = {0.0, 0.0};    // u before the trip's first stamp
        Chi2Sums<K> s;
    };
    const double *A, *g, *omega, *columns;
    Chi2Baseline<K> terms;            // (wbasis unused: the columns come through the trip's tables)
    __device__ __forceinline__ Trip trip(const double* __restrict__ flux, int n_time, int base, int lane) const
    {
        return {ss2_trip(flux, A, g, omega, n_time, base, lane), gls_cols<K>(columns, n_time, base, lane)};
    }
    static __device__ __forceinline__ void row_trip(const Trip& t, double m0, double m1, Row& row, int lane)
    {
        double z0, z1;
        const Ss2Vec uinc = ss2_innovations(t.t, m0, m1, row.carry, lane, z0, z1);
        row.s.s2 = fma(t.t.w0 * z0, z0, row.s.s2);
        row.s.s2 = fma(t.t.w1 * z1, z1, row.s.s2);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            row.s.x[k] = fma(t.c.c0[k], z0, row.s.x[k]);
            row.s.x[k] = fma(t.c.c1[k], z1, row.s.x[k]);
        }
        row.carry.x = wave_read_lane<63>(uinc.x);                      // the last lane's u, to every lane
        row.carry.y = wave_read_lane<63>(uinc.y);
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
