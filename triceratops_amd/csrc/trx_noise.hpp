// Correlated noise of a dataset: chi2_ou_kernel<ONE> (trxn_chi2_grid_ou, include/trx_noise.h), the
// row reduction of a materialised grid under white noise plus one exponential (Ornstein-Uhlenbeck) term, in its Kalman
// form.  Included by trx_kernels.hip only.
//
// With y_t = flux_t - model[r][t] and the row-independent alpha, beta, omega of datasets.ou_system:
//     g_0 = 0,  g_n = alpha_n g_(n-1) + beta_n y_(n-1),    h[r] = 0.5 sum_n omega_n (y_n - g_n)^2.
// The kernel carries u_n = g_(n+1) -- the prediction for the stamp after n, u_n = A_n u_(n-1) + B_n y_n with
// A_n = alpha_(n+1), B_n = beta_(n+1), u_(-1) = 0 -- so that the lane that holds y_n owns both terms of its step.
//
// One wavefront per row, two rows in flight per wave.  A trip is kOuTrip = 128 consecutive stamps, lane l the pair
// (2 l, 2 l + 1) of it: one 16-byte load where the row's address allows it, two 8-byte loads of the same values
// elsewhere, every grid value read once (non-temporal).  A lane folds its pair into one affine map u -> a u + b,
// a = A_0 A_1 (the same for every row), b = A_1 (B_0 y_0) + B_1 y_1; a log-step scan over the lanes composes the maps:
// six steps of one fma and one cross-lane move of b each -- DPP moves (ou_scan_source): four within the rows of 16 lanes,
// two broadcasts across them --, the multipliers m[s] -- the a-products of the spans, and ainc, the product from the
// trip's start -- formed by the same scan on a alone, once per trip for both rows (ONE: n_time <= kOuTrip, once per wave
// before its first row, in registers for all its rows).  The last lane's u is carried into the next trip.  Stamps past n_time enter as y = 0, A = B = omega = 0.  No LDS, no workspace: flux and the three tables are
// read through the caches, 8 values per lane and trip.
//
// The order of a row's arithmetic is fixed by n_time alone: the trips, the lane of every stamp, the scan's steps and
// wave_sum's butterfly.  Neither the launch geometry, the row's position, its alignment nor the other rows enter.
#pragma once
#include "trx_reduce.hpp"

namespace {

constexpr int kOuTrip = 128;          // stamps of one trip: two per lane
constexpr int kOuScanSteps = 6;       // log2(64)

// what a trip needs besides the rows' values: the same for every row
// (m[]: indexed by unrolled loops only, so it lives in registers)
struct OuTrip {
    double f0, f1, w0, w1;            // flux and omega of the lane's two stamps
    double A0, A1, B0, B1;            // alpha and beta of the stamps after them (0 past the end)
    double m[kOuScanSteps];           // multiplier of scan step s: the a-product of the lanes folded into this one so far
    double ainc;                      // the a-product from the trip's first stamp to this lane's second
};

// lane l receives lane l - 1's value, lane 0 `fill`
__device__ __forceinline__ double ou_shift_up1(double v, double fill, int lane)
{
    const double s = __shfl_up(v, 1, 64);
    return lane >= 1 ? s : fill;
}

// one DPP move of a double (two 32-bit moves): the lanes the control and the row mask leave out receive `fill`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double ou_dpp(double v, double fill)
{
    const long long vb = __double_as_longlong(v), fb = __double_as_longlong(fill);
    const int lo = __builtin_amdgcn_update_dpp((int)fb, (int)vb, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(fb >> 32), (int)(vb >> 32), CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// The source of scan step S over the 64 lanes, in DPP moves alone (no LDS crossbar): S = 0 .. 3 the lane 1, 2, 4, 8
// below within the lane's row of 16 (row_shr; the row's first lanes: `fill`), S = 4 the last lane of the row before for
// the odd rows (row_bcast:15), S = 5 lane 31 for the upper half (row_bcast:31).  After step S a lane holds the fold of
// min(2^(S+1), l % 16 + 1) lanes of its row, then of its half, then of the wave up to itself.
template <int S>
__device__ __forceinline__ double ou_scan_source(double v, double fill)
{
    static_assert(S >= 0 && S < 6, "six steps: 64 lanes");
    if constexpr (S == 0) return ou_dpp<0x111, 0xf>(v, fill);
    else if constexpr (S == 1) return ou_dpp<0x112, 0xf>(v, fill);
    else if constexpr (S == 2) return ou_dpp<0x114, 0xf>(v, fill);
    else if constexpr (S == 3) return ou_dpp<0x118, 0xf>(v, fill);
    else if constexpr (S == 4) return ou_dpp<0x142, 0xa>(v, fill);
    else return ou_dpp<0x143, 0xc>(v, fill);
}

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

// the lane's two values of a row's trip: 0 past the row's end, which is never read
__device__ __forceinline__ void ou_load_pair(const double* __restrict__ row, int n_time, int base, int lane, bool vec,
                                             double& m0, double& m1)
{
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    const int n0 = base + 2 * lane;
    m0 = 0.0;
    m1 = 0.0;
    if (n0 + 1 < n_time) {
        if (vec) {
            const dvec2 m = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(row + n0));
            m0 = m.x; m1 = m.y;
        } else {
            m0 = __builtin_nontemporal_load(row + n0);
            m1 = __builtin_nontemporal_load(row + n0 + 1);
        }
    } else if (n0 < n_time) {
        m0 = __builtin_nontemporal_load(row + n0);
    }
}

// one trip of one row: carry = u before the trip's first stamp, acc the lane's share of sum omega z^2
__device__ __forceinline__ void ou_row_trip(const OuTrip& t, double m0, double m1, double& carry, double& acc, int lane)
{
    const double y0 = t.f0 - m0, y1 = t.f1 - m1;
    const double by0 = t.B0 * y0;
    double b = fma(t.A1, by0, t.B1 * y1);
    ou_scan_b<0>(t.m, b);
    const double uinc = fma(t.ainc, carry, b);                 // u after the lane's second stamp
    const double uin = ou_shift_up1(uinc, carry, lane);       // ... and before its first
    const double z0 = y0 - uin;
    const double z1 = y1 - fma(t.A0, uin, by0);
    acc = fma(t.w0 * z0, z0, acc);
    acc = fma(t.w1 * z1, z1, acc);
    const long long ub = __double_as_longlong(uinc);          // the last lane's u, to every lane
    carry = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(ub >> 32), 63) << 32) |
                                 (long long)(unsigned)__builtin_amdgcn_readlane((int)ub, 63));
}

template <bool ONE>
__global__ __launch_bounds__(256) void chi2_ou_kernel(const double* __restrict__ flux, const double* __restrict__ grid,
                                                      int n_time, long n, const double* __restrict__ secdepth,
                                                      double sec_limit, int accumulate, double* __restrict__ out,
                                                      const double* __restrict__ alpha, const double* __restrict__ beta,
                                                      const double* __restrict__ omega)
{
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long nwaves = (long)gridDim.x * 4;
    OuTrip t;
    if (ONE) t = ou_trip(flux, alpha, beta, omega, n_time, 0, lane);
    for (long r = wave0; r < n; r += 2 * nwaves) {
        // two rows per pass, their loads in flight together; each row's arithmetic is its own
        const long r2 = r + nwaves;
        const bool two = r2 < n;
        const double* row0 = grid + (size_t)r * n_time;
        const double* row1 = grid + (size_t)(two ? r2 : r) * n_time;
        const bool vec0 = ((uintptr_t)row0 & 15) == 0, vec1 = ((uintptr_t)row1 & 15) == 0;      // (per row: wave-uniform)
        double carry0 = 0.0, carry1 = 0.0, acc0 = 0.0, acc1 = 0.0;
        for (int base = 0; base < n_time; base += kOuTrip) {
            double a0, a1, b0 = 0.0, b1 = 0.0;
            ou_load_pair(row0, n_time, base, lane, vec0, a0, a1);
            if (two) ou_load_pair(row1, n_time, base, lane, vec1, b0, b1);
            if (!ONE) t = ou_trip(flux, alpha, beta, omega, n_time, base, lane);
            ou_row_trip(t, a0, a1, carry0, acc0, lane);
            if (two) ou_row_trip(t, b0, b1, carry1, acc1, lane);
            if (ONE) break;                                   // (n_time <= kOuTrip)
        }
        const double tot0 = wave_sum(acc0), tot1 = wave_sum(acc1);
        if (lane == 0) {
            chi2w_store(tot0, r, secdepth, sec_limit, accumulate, out);
            if (two) chi2w_store(tot1, r2, secdepth, sec_limit, accumulate, out);
        }
    }
}

}  // namespace
