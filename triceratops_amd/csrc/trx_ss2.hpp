// Correlated noise with a state of dimension two: scan_rows_kernel<ONE, Ss2Filter> (trxs_chi2_grid_ss2, include/trx_ss.h;
// DESIGN.md section 14), the row reduction of a materialised grid under white noise plus a process whose Kalman filter
// carries two states -- a Matern-3/2 term, two exponential terms, any other celerite-style term of that size.  Included
// by trx_kernels.hip only.
//
// With y_t = flux_t - model[r][t] and the row-independent A [T][2][2], g [T][2], omega [T] of datasets.ss2_system:
//     u_(-1) = 0,   z_n = y_n - u_(n-1)[0],   u_n = A_n u_(n-1) + g_n y_n,    h[r] = 0.5 sum_n omega_n z_n^2.
//
// The layout is scan_rows_kernel's (trx_scan.hpp), Ss2Filter its filter.  A lane folds its pair into one affine map
// u -> M u + v, M = A_1 A_0 (the same for every row), v = (A_1 g_0) y_0 + g_1 y_1.  The multipliers m[s] -- the M-products
// of the spans, 2 x 2 each -- and minc, the product from the trip's start, are formed by the scan on M alone; a row's scan
// moves only v: two doubles and four fma a step.  The last lane's u is carried into the next trip; A = 0, g = 0,
// omega = 0 past n_time.  16 table values per lane and trip.  The wave reduction is wave_sum's butterfly, the store
// chi2w_store.
#pragma once
#include "trx_scan.hpp"

namespace {

// a 2 x 2 matrix by rows and a 2-vector, in registers
struct Ss2Mat {
    double a, b, c, d;                // [[a, b], [c, d]]
};

struct Ss2Vec {
    double x, y;
};

// what a trip needs besides the rows' values: the same for every row
// (m[]: indexed by unrolled loops only, so it lives in registers)
struct Ss2Trip {
    double f0, f1, w0, w1;            // flux and omega of the lane's two stamps
    double a00, a01, g00;             // the first row of A and of g of the lane's first stamp: the prediction for its second
    Ss2Vec h, g1;                     // v = h y_0 + g1 y_1: h = A_1 g_0, g1 = g of the second stamp
    Ss2Mat m[kOuScanSteps];           // multiplier of scan step s: the M-product of the lanes folded into this one so far
    Ss2Mat minc;                      // the M-product from the trip's first stamp to this lane's second
};

// p q: q acts first
__device__ __forceinline__ Ss2Mat ss2_mul(const Ss2Mat& p, const Ss2Mat& q)
{
    Ss2Mat r;
    r.a = fma(p.a, q.a, p.b * q.c);
    r.b = fma(p.a, q.b, p.b * q.d);
    r.c = fma(p.c, q.a, p.d * q.c);
    r.d = fma(p.c, q.b, p.d * q.d);
    return r;
}

// v + p s
__device__ __forceinline__ Ss2Vec ss2_apply(const Ss2Mat& p, const Ss2Vec& s, const Ss2Vec& v)
{
    Ss2Vec r;
    r.x = fma(p.a, s.x, fma(p.b, s.y, v.x));
    r.y = fma(p.c, s.x, fma(p.d, s.y, v.y));
    return r;
}

__device__ __forceinline__ Ss2Mat ss2_load_mat(const double* __restrict__ A, int n, int n_time)
{
    Ss2Mat r = {0.0, 0.0, 0.0, 0.0};
    if (n < n_time) {
        const double* p = A + 4 * (size_t)n;
        r.a = p[0]; r.b = p[1]; r.c = p[2]; r.d = p[3];
    }
    return r;
}

__device__ __forceinline__ Ss2Vec ss2_load_vec(const double* __restrict__ g, int n, int n_time)
{
    Ss2Vec r = {0.0, 0.0};
    if (n < n_time) {
        r.x = g[2 * (size_t)n];
        r.y = g[2 * (size_t)n + 1];
    }
    return r;
}

// the scan's step S on a lane's matrix (M: its multiplier before the step; a lane that the step leaves out meets the
// identity here and v = 0 in a row's scan)
template <int S>
__device__ __forceinline__ void ss2_scan_m(Ss2Mat (&m)[kOuScanSteps], Ss2Mat& M)
{
    m[S] = M;
    Ss2Mat s;
    s.a = ou_scan_source<S>(M.a, 1.0);
    s.b = ou_scan_source<S>(M.b, 0.0);
    s.c = ou_scan_source<S>(M.c, 0.0);
    s.d = ou_scan_source<S>(M.d, 1.0);
    M = ss2_mul(M, s);
    if constexpr (S < kOuScanSteps - 1) ss2_scan_m<S + 1>(m, M);
}

template <int S>
__device__ __forceinline__ void ss2_scan_v(const Ss2Mat (&m)[kOuScanSteps], Ss2Vec& v)
{
    Ss2Vec s;
    s.x = ou_scan_source<S>(v.x, 0.0);
    s.y = ou_scan_source<S>(v.y, 0.0);
    v = ss2_apply(m[S], s, v);
    if constexpr (S < kOuScanSteps - 1) ss2_scan_v<S + 1>(m, v);
}

__device__ __forceinline__ Ss2Trip ss2_trip(const double* __restrict__ flux, const double* __restrict__ A,
                                            const double* __restrict__ g, const double* __restrict__ omega, int n_time,
                                            int base, int lane)
{
    const int n0 = base + 2 * lane, n1 = n0 + 1;
    Ss2Trip t;
    t.f0 = n0 < n_time ? flux[n0] : 0.0;
    t.w0 = n0 < n_time ? omega[n0] : 0.0;
    t.f1 = n1 < n_time ? flux[n1] : 0.0;
    t.w1 = n1 < n_time ? omega[n1] : 0.0;
    const Ss2Mat A0 = ss2_load_mat(A, n0, n_time), A1 = ss2_load_mat(A, n1, n_time);
    const Ss2Vec g0 = ss2_load_vec(g, n0, n_time);
    t.g1 = ss2_load_vec(g, n1, n_time);
    t.a00 = A0.a;
    t.a01 = A0.b;
    t.g00 = g0.x;
    t.h.x = fma(A1.a, g0.x, A1.b * g0.y);
    t.h.y = fma(A1.c, g0.x, A1.d * g0.y);
    Ss2Mat M = ss2_mul(A1, A0);
    ss2_scan_m<0>(t.m, M);
    t.minc = M;
    return t;
}


// One trip of one row up to its innovations z0, z1 (carry: u before the trip's first stamp).  Returns the lane's u after
// its second stamp: the last lane's is the next trip's carry.  Ss2Filter and Ss2ColsFilter<K> (trx_ss2_cols.hpp) both go
// through here, so their z0, z1 are the same bits.
__device__ __forceinline__ Ss2Vec ss2_innovations(const Ss2Trip& t, double m0, double m1, const Ss2Vec& carry, int lane,
                                                  double& z0, double& z1)
{
    const double y0 = t.f0 - m0, y1 = t.f1 - m1;
    Ss2Vec v;
    v.x = fma(t.h.x, y0, t.g1.x * y1);
    v.y = fma(t.h.y, y0, t.g1.y * y1);
    ss2_scan_v<0>(t.m, v);
    const Ss2Vec uinc = ss2_apply(t.minc, carry, v);               // u after the lane's second stamp
    const double uin0 = ou_shift_up1(uinc.x, carry.x, lane);       // ... and before its first
    const double uin1 = ou_shift_up1(uinc.y, carry.y, lane);
    z0 = y0 - uin0;
    z1 = y1 - fma(t.a00, uin0, fma(t.a01, uin1, t.g00 * y0));
    return uinc;
}

struct Ss2Row {
    Ss2Vec carry = {0.0, 0.0};        // u before the trip's first stamp
    double acc = 0.0;                 // the lane's share of sum omega z^2
};

struct Ss2Filter {
    using Trip = Ss2Trip;
    using Row = Ss2Row;
    const double *A, *g, *omega;
    __device__ __forceinline__ Ss2Trip trip(const double* __restrict__ flux, int n_time, int base, int lane) const
    {
        return ss2_trip(flux, A, g, omega, n_time, base, lane);
    }
    static __device__ __forceinline__ void row_trip(const Ss2Trip& t, double m0, double m1, Ss2Row& s, int lane)
    {
        double z0, z1;
        const Ss2Vec uinc = ss2_innovations(t, m0, m1, s.carry, lane, z0, z1);
        s.acc = fma(t.w0 * z0, z0, s.acc);
        s.acc = fma(t.w1 * z1, z1, s.acc);
        s.carry.x = wave_read_lane<63>(uinc.x);                        // the last lane's u, to every lane
        s.carry.y = wave_read_lane<63>(uinc.y);
    }
    static __device__ __forceinline__ void wave_sums(Ss2Row& s) { s.acc = wave_sum(s.acc); }
    __device__ __forceinline__ void store(const Ss2Row& s, long r, const double* __restrict__ secdepth, double sec_limit,
                                          int accumulate, double* __restrict__ out) const
    {
        chi2w_store(s.acc, r, secdepth, sec_limit, accumulate, out);
    }
};

}  // namespace
