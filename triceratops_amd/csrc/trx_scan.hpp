// The row reductions of a materialised grid under correlated noise: scan_rows_kernel<ONE, Filter>,
// the layout they share, and its pieces -- the trip's loads, the DPP moves of the scan over the lanes, the read of one
// lane, the soft minimum's tail.  Included by trx_kernels.hip only.
//
// One wavefront per row, two rows in flight per wave.  A trip is kOuTrip = 128 consecutive stamps, lane l the pair
// (2 l, 2 l + 1) of it: one 16-byte load where the row's address allows it, two 8-byte loads of the same values
// elsewhere, every grid value read once (non-temporal).  A Kalman filter's step is an affine map of its state; a lane
// folds its pair into one map, and a log-step scan over the lanes composes the maps: six steps, their cross-lane moves
// DPP moves (ou_scan_source): four within the rows of 16 lanes, two broadcasts across them.  What does not depend on the
// row -- the light curve's values and the noise tables of the lane's pair, the multipliers of the scan's steps -- is a
// filter's Trip, formed once per trip for both rows (ONE: n_time <= kOuTrip, once per wave before its first row, in
// registers for all its rows).  The last lane's state is carried into the next trip.  Stamps past n_time enter as y = 0
// with tables of 0.  No LDS, no workspace: flux and the tables are read through the caches.
//
// The order of a row's arithmetic is fixed by n_time alone: the trips, the lane of every stamp, the scan's steps and the
// wave reduction.  Neither the launch geometry, the row's position, its alignment nor the other rows enter.
//
// A Filter, by value in the kernel arguments as Terms is in chi2_rows_kernel's, supplies what differs:
//   Trip                               the row-independent tables of a trip, and trip(flux, n_time, base, lane) to form them
//   Row                                a row's running state, its carry and sums: value-initialised at the row's start
//   row_trip(t, m0, m1, row, lane)     one trip of one row from the lane's two grid values
//   wave_sums(row), store(row, r, ..)  the wave reduction, and what lane 0 makes of it
// OuFilter (trx_noise.hpp), OuColsFilter<K> (trx_gls.hpp), Ss2Filter (trx_ss2.hpp), Ss2ColsFilter<K> (trx_ss2_cols.hpp).
// ou_mix_kernel (trx_noise_mix.hpp) is a kernel of its own over the same pieces.
#pragma once
#include "trx_reduce.hpp"

namespace {

constexpr int kOuTrip = 128;          // stamps of one trip: two per lane
constexpr int kOuScanSteps = 6;       // log2(64)

// lane l receives lane l - 1's value, lane 0 `fill`
__device__ __forceinline__ double ou_shift_up1(double v, double fill, int lane)
{
    const double s = __shfl_up(v, 1, 64);
    return lane >= 1 ? s : fill;
}

// lane SRC's value, to every lane
template <int SRC>
__device__ __forceinline__ double wave_read_lane(double v)
{
    const long long b = __double_as_longlong(v);
    return __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(b >> 32), SRC) << 32) |
                                (long long)(unsigned)__builtin_amdgcn_readlane((int)b, SRC));
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

// The two rows of a wave's pass, r and r + nwaves (`two`: the second exists), their loads in flight together; each row's
// arithmetic is its own.
struct ScanPair {
    long r2;
    bool two, vec0, vec1;             // (the alignment is per row: wave-uniform)
    const double *row0, *row1;
    __device__ __forceinline__ ScanPair(const double* __restrict__ grid, int n_time, long n, long r, long nwaves)
        : r2(r + nwaves), two(r2 < n), row0(grid + (size_t)r * n_time), row1(grid + (size_t)(two ? r2 : r) * n_time)
    {
        vec0 = ((uintptr_t)row0 & 15) == 0;
        vec1 = ((uintptr_t)row1 & 15) == 0;
    }
    __device__ __forceinline__ void load(int n_time, int base, int lane, double& a0, double& a1, double& b0,
                                         double& b1) const
    {
        b0 = b1 = 0.0;
        ou_load_pair(row0, n_time, base, lane, vec0, a0, a1);
        if (two) ou_load_pair(row1, n_time, base, lane, vec1, b0, b1);
    }
};

template <bool ONE, class Filter>
__global__ __launch_bounds__(256) void scan_rows_kernel(const double* __restrict__ flux, const double* __restrict__ grid,
                                                        int n_time, long n, const double* __restrict__ secdepth,
                                                        double sec_limit, int accumulate, double* __restrict__ out,
                                                        const Filter filter)
{
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long nwaves = (long)gridDim.x * 4;
    typename Filter::Trip t;
    if (ONE) t = filter.trip(flux, n_time, 0, lane);
    for (long r = wave0; r < n; r += 2 * nwaves) {
        const ScanPair p(grid, n_time, n, r, nwaves);
        typename Filter::Row s0{}, s1{};
        for (int base = 0; base < n_time; base += kOuTrip) {
            double a0, a1, b0, b1;
            p.load(n_time, base, lane, a0, a1, b0, b1);
            if (!ONE) t = filter.trip(flux, n_time, base, lane);
            Filter::row_trip(t, a0, a1, s0, lane);
            if (p.two) Filter::row_trip(t, b0, b1, s1, lane);
            if (ONE) break;                                   // (n_time <= kOuTrip)
        }
        Filter::wave_sums(s0);
        Filter::wave_sums(s1);
        if (lane == 0) {
            filter.store(s0, r, secdepth, sec_limit, accumulate, out);
            if (p.two) filter.store(s1, p.r2, secdepth, sec_limit, accumulate, out);
        }
    }
}

// The soft minimum's tail: T = m - ln s for m = min_j a_j and s = sum_j exp(m - a_j), clamped at 0.
__device__ __forceinline__ double softmin_tail(double m, double s)
{
    double t = m - log(s);
    t = m < INFINITY ? t : m;                            // (every candidate +inf, or a NaN row: no inf - inf)
    return t < 0.0 ? 0.0 : t;                            // (a NaN stays a NaN)
}

// the log-weights of up to eight candidates, by value in the kernel arguments
struct Lnc8 {
    double v[8];
};

}  // namespace
