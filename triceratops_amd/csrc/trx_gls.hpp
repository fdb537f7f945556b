// Baseline terms marginalised under correlated noise: gls_ou_kernel<ONE, K> (trxg_chi2_grid_ou_baseline,
// include/trx_gls.h).  Included by trx_kernels.hip only, after trx_noise.hpp.
//
// With y = flux - model[r], the Kalman tables alpha, beta, omega of the dataset's noise (datasets.ou_system) and the
// innovations z[x]_n = x_n - g_n, g_0 = 0, g_n = alpha_n g_(n-1) + beta_n x_(n-1), the row's term is
//     S2 = sum_n omega_n z[y]_n^2,   b~_k = sum_n c_k[n] z[y]_n,   h[r] = 0.5 max(S2 - b~^T M b~, 0),
// c_k[n] = omega_n z[B_k]_n / sqrt(D_k) the whitened, scaled columns from the host (datasets.ou_baseline_system: they do
// not depend on the row) and M the inverse of the scaled system matrix, packed upper triangle by rows, by value in the
// kernel arguments.  coef_out[r][i] = sum_j M_ij b~_j.
//
// The layout is chi2_ou_kernel's: one wavefront per row, two rows in flight, trips of kOuTrip stamps, lane l the pair
// (2 l, 2 l + 1), the scan of trx_noise.hpp (ou_trip, ou_scan_b, ou_shift_up1), every grid value read once
// (non-temporal), no LDS, no workspace.  gls_row_trip forms z0, z1 and S2 term for term as ou_row_trip does -- M = 0
// gives trxn_chi2_grid_ou's bits -- and next to acc = sum omega z^2 a lane keeps the K sums fma(c_k[n], z_n, acc_k) over
// the same z0, z1.  The lane's pair of every column is loaded per trip (ONE: once per wave); wave_sum for S2 and one
// gls_wave_total -- the same total in the scan's DPP moves -- per column sum; the store is Chi2Baseline<K>'s (clamp at 0, a NaN stays a NaN, secdepth / sec_limit / accumulate as chi2w_store).
//
// The order of a row's arithmetic is fixed by n_time alone, as in chi2_ou_kernel: neither the launch geometry, the row's
// position, its alignment nor the other rows enter.
#pragma once
#include "trx_noise.hpp"

namespace {

// K from which the kernel needs more than 128 VGPRs, so that two waves a SIMD are resident instead of four (gls_ou_launch;
// tests/test_build_resources_gls.py holds this against the code object's register counts).  The build reports 66 - 82
// VGPRs at K <= 2 and 86 - 114 at K = 3, 4: no K is wide.
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

// ou_row_trip with the K further sums: the same operations in the same order up to acc, then fma(c_k, z, x_k)
template <int K>
__device__ __forceinline__ void gls_row_trip(const OuTrip& t, const GlsCols<K>& c, double m0, double m1, double& carry,
                                             Chi2Sums<K>& s, int lane)
{
    const double y0 = t.f0 - m0, y1 = t.f1 - m1;
    const double by0 = t.B0 * y0;
    double b = fma(t.A1, by0, t.B1 * y1);
    ou_scan_b<0>(t.m, b);
    const double uinc = fma(t.ainc, carry, b);                 // u after the lane's second stamp
    const double uin = ou_shift_up1(uinc, carry, lane);       // ... and before its first
    const double z0 = y0 - uin;
    const double z1 = y1 - fma(t.A0, uin, by0);
    s.s2 = fma(t.w0 * z0, z0, s.s2);
    s.s2 = fma(t.w1 * z1, z1, s.s2);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s.x[k] = fma(c.c0[k], z0, s.x[k]);
        s.x[k] = fma(c.c1[k], z1, s.x[k]);
    }
    const long long ub = __double_as_longlong(uinc);          // the last lane's u, to every lane
    carry = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(ub >> 32), 63) << 32) |
                                 (long long)(unsigned)__builtin_amdgcn_readlane((int)ub, 63));
}

// The total of a lane value over the wave in the scan's DPP moves (ou_scan_source with the addend 0 outside a step's reach:
// after the six steps lane 63 holds the sum of all 64), read back to every lane.  The K column sums take this in place of
// wave_sum's butterfly: that is twelve ds_bpermute a sum and row through the LDS crossbar the CU's four SIMDs share, and
// at one trip a row (n_time <= 128) K of them outweigh the row's scan (measured at 100 stamps, K = 4: 2.20 x chi2_ou_kernel
// with wave_sum, 1.57 x with this; profiles/gls/results.txt).  S2 keeps wave_sum: its bits are chi2_ou_kernel's.
template <int S>
__device__ __forceinline__ void gls_fold(double& v)
{
    v += ou_scan_source<S>(v, 0.0);
    if constexpr (S < 5) gls_fold<S + 1>(v);
}

__device__ __forceinline__ double gls_wave_total(double v)
{
    gls_fold<0>(v);
    const long long b = __double_as_longlong(v);
    return __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(b >> 32), 63) << 32) |
                                (long long)(unsigned)__builtin_amdgcn_readlane((int)b, 63));
}

template <int K>
__device__ __forceinline__ void gls_wave_sums(Chi2Sums<K>& s)
{
    s.s2 = wave_sum(s.s2);
#pragma unroll
    for (int k = 0; k < K; ++k) s.x[k] = gls_wave_total(s.x[k]);
}

template <bool ONE, int K>
__global__ __launch_bounds__(256) void gls_ou_kernel(const double* __restrict__ flux, const double* __restrict__ grid,
                                                     int n_time, long n, const double* __restrict__ secdepth,
                                                     double sec_limit, int accumulate, double* __restrict__ out,
                                                     const double* __restrict__ alpha, const double* __restrict__ beta,
                                                     const double* __restrict__ omega,
                                                     const double* __restrict__ columns, Chi2bM M,
                                                     double* __restrict__ coef_out)
{
    static_assert(K >= 1 && K <= kChi2bMaxTerms, "one to four columns");
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long nwaves = (long)gridDim.x * 4;
    const Chi2Baseline<K> terms{nullptr, M, coef_out};
    OuTrip t;
    GlsCols<K> c;
    if (ONE) {
        t = ou_trip(flux, alpha, beta, omega, n_time, 0, lane);
        c = gls_cols<K>(columns, n_time, 0, lane);
    }
    for (long r = wave0; r < n; r += 2 * nwaves) {
        // two rows per pass, their loads in flight together; each row's arithmetic is its own
        const long r2 = r + nwaves;
        const bool two = r2 < n;
        const double* row0 = grid + (size_t)r * n_time;
        const double* row1 = grid + (size_t)(two ? r2 : r) * n_time;
        const bool vec0 = ((uintptr_t)row0 & 15) == 0, vec1 = ((uintptr_t)row1 & 15) == 0;      // (per row: wave-uniform)
        double carry0 = 0.0, carry1 = 0.0;
        Chi2Sums<K> s0, s1;
        for (int base = 0; base < n_time; base += kOuTrip) {
            double a0, a1, b0 = 0.0, b1 = 0.0;
            ou_load_pair(row0, n_time, base, lane, vec0, a0, a1);
            if (two) ou_load_pair(row1, n_time, base, lane, vec1, b0, b1);
            if (!ONE) {
                t = ou_trip(flux, alpha, beta, omega, n_time, base, lane);
                c = gls_cols<K>(columns, n_time, base, lane);
            }
            gls_row_trip<K>(t, c, a0, a1, carry0, s0, lane);
            if (two) gls_row_trip<K>(t, c, b0, b1, carry1, s1, lane);
            if (ONE) break;                                   // (n_time <= kOuTrip)
        }
        gls_wave_sums(s0);
        gls_wave_sums(s1);
        if (lane == 0) {
            terms.store(s0, r, secdepth, sec_limit, accumulate, out);
            if (two) terms.store(s1, r2, secdepth, sec_limit, accumulate, out);
        }
    }
}

}  // namespace
