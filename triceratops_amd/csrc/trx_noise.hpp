// Correlated noise of a dataset: scan_rows_kernel<ONE, OuFilter> (trxn_chi2_grid_ou, include/trx_noise.h; DESIGN.md
// section 14), the row reduction of a materialised grid under white noise plus one exponential (Ornstein-Uhlenbeck) term,
// in its Kalman form.  Included by trx_kernels.hip only.
//
// With y_t = flux_t - model[r][t] and the row-independent alpha, beta, omega of datasets.ou_system:
//     g_0 = 0,  g_n = alpha_n g_(n-1) + beta_n y_(n-1),    h[r] = 0.5 sum_n omega_n (y_n - g_n)^2.
// The kernel carries u_n = g_(n+1) -- the prediction for the stamp after n, u_n = A_n u_(n-1) + B_n y_n with
// A_n = alpha_(n+1), B_n = beta_(n+1), u_(-1) = 0 -- so that the lane that holds y_n owns both terms of its step.
//
// The layout is scan_rows_kernel's (trx_scan.hpp), OuFilter its filter.  A lane folds its pair into one affine map
// u -> a u + b, a = A_0 A_1 (the same for every row), b = A_1 (B_0 y_0) + B_1 y_1; a step of the scan is one fma and one
// cross-lane move of b, the multipliers m[s] -- the a-products of the spans, and ainc, the product from the trip's start
// -- formed by the same scan on a alone.  The last lane's u is carried into the next trip; A = B = omega = 0 past n_time.
// 8 table values per lane and trip.  The wave reduction is wave_sum's butterfly, the store chi2w_store.
#pragma once
#include "trx_scan.hpp"

namespace {

// what a trip needs besides the rows' values: the same for every row
// (m[]: indexed by unrolled loops only, so it lives in registers)
struct OuTrip {
    double f0, f1, w0, w1;            // flux and omega of the lane's two stamps
    double A0, A1, B0, B1;            // alpha and beta of the stamps after them (0 past the end)
    double m[kOuScanSteps];           // multiplier of scan step s: the a-product of the lanes folded into this one so far
    double ainc;                      // the a-product from the trip's first stamp to this lane's second
};

// the scan's step S on a lane's map (a: its multiplier before the step)
template <int S>
__device__ __forceinline__ void ou_scan_a(double (&m)[6], double& a)
{
    m[S] = a;
    a *= ou_scan_source<S>(a, 1.0);
    if constexpr (S < 5) ou_scan_a<S + 1>(m, a);
}

template <int S>
__device__ __forceinline__ void ou_scan_b(const double (&m)[6], double& b)
{
    b = fma(m[S], ou_scan_source<S>(b, 0.0), b);
    if constexpr (S < 5) ou_scan_b<S + 1>(m, b);
}

__device__ __forceinline__ OuTrip ou_trip(const double* __restrict__ flux, const double* __restrict__ alpha,
                                          const double* __restrict__ beta, const double* __restrict__ omega, int n_time,
                                          int base, int lane)
{
    const int n0 = base + 2 * lane, n1 = n0 + 1, n2 = n0 + 2;
    OuTrip t;
    t.f0 = n0 < n_time ? flux[n0] : 0.0;
    t.w0 = n0 < n_time ? omega[n0] : 0.0;
    t.f1 = n1 < n_time ? flux[n1] : 0.0;
    t.w1 = n1 < n_time ? omega[n1] : 0.0;
    t.A0 = n1 < n_time ? alpha[n1] : 0.0;
    t.B0 = n1 < n_time ? beta[n1] : 0.0;
    t.A1 = n2 < n_time ? alpha[n2] : 0.0;
    t.B1 = n2 < n_time ? beta[n2] : 0.0;
    double a = t.A0 * t.A1;
    ou_scan_a<0>(t.m, a);            // (a lane that a step leaves out meets the factor 1 here and b = 0 in a row's scan)
    t.ainc = a;
    return t;
}

// One trip of one row up to its innovations z0, z1 (carry: u before the trip's first stamp).  Returns the lane's u after
// its second stamp: the last lane's is the next trip's carry.
__device__ __forceinline__ double ou_innovations(const OuTrip& t, double m0, double m1, double carry, int lane, double& z0,
                                                 double& z1)
{
    const double y0 = t.f0 - m0, y1 = t.f1 - m1;
    const double by0 = t.B0 * y0;
    double b = fma(t.A1, by0, t.B1 * y1);
    ou_scan_b<0>(t.m, b);
    const double uinc = fma(t.ainc, carry, b);                 // u after the lane's second stamp
    const double uin = ou_shift_up1(uinc, carry, lane);       // ... and before its first
    z0 = y0 - uin;
    z1 = y1 - fma(t.A0, uin, by0);
    return uinc;
}

// one trip of one row: carry = u before the trip's first stamp, acc the lane's share of sum omega z^2
__device__ __forceinline__ void ou_row_trip(const OuTrip& t, double m0, double m1, double& carry, double& acc, int lane)
{
    double z0, z1;
    const double uinc = ou_innovations(t, m0, m1, carry, lane, z0, z1);
    acc = fma(t.w0 * z0, z0, acc);
    acc = fma(t.w1 * z1, z1, acc);
    carry = wave_read_lane<63>(uinc);
}

struct OuRow {
    double carry = 0.0, acc = 0.0;
};

struct OuFilter {
    using Trip = OuTrip;
    using Row = OuRow;
    const double *alpha, *beta, *omega;
    __device__ __forceinline__ OuTrip trip(const double* __restrict__ flux, int n_time, int base, int lane) const
    {
        return ou_trip(flux, alpha, beta, omega, n_time, base, lane);
    }
    static __device__ __forceinline__ void row_trip(const OuTrip& t, double m0, double m1, OuRow& s, int lane)
    {
        ou_row_trip(t, m0, m1, s.carry, s.acc, lane);
    }
    static __device__ __forceinline__ void wave_sums(OuRow& s) { s.acc = wave_sum(s.acc); }
    __device__ __forceinline__ void store(const OuRow& s, long r, const double* __restrict__ secdepth, double sec_limit,
                                          int accumulate, double* __restrict__ out) const
    {
        chi2w_store(s.acc, r, secdepth, sec_limit, accumulate, out);
    }
};

}  // namespace

