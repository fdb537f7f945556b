// The outlier-tolerant row reduction of a materialised grid: chi2_robust_kernel<STAGE> (trxr_chi2_grid_robust,
// include/trx_robust.h).  Included by trx_kernels.hip only.
//
// Every point is a two-component mixture: with probability 1 - eps it has its stated error, with probability eps it comes
// from a Gaussian kappa times wider; the membership is integrated out per point.  With d_t = flux_t - model[r][t],
// w = inv_var and the row-independent constants c0 = -log1p(-eps), c1 = ln kappa - ln eps, k2 = 1 / kappa^2 (from the host:
// datasets.robust_constants) a value's term is, in this order and with every operation rounded on its own (no
// contraction):
//     d  = f - m
//     a  = 0.5 * (w * d) * d              ((0.5 * (w * d)) * d: the halving is exact)
//     A  = a + c0
//     B  = fma(a, k2, c1)
//     lo = fmin(A, B)
//     e  = exp(-fabs(A - B))
//     acc += lo - log1p(e)
// -- the statement of _numerics.robust_halfchi2 --, h[r] = sum_t of them, a total that rounding drives below 0 stored as
// 0 (every term is >= 0 in exact arithmetic), a NaN stays a NaN.  h[r] is written or added to out[r]; +inf where
// secdepth[r] >= sec_limit.  The total is not halved: the terms are log-weights already.
//
// The layout is chi2_rows_kernel's (trx_reduce.hpp): one wavefront per row, two rows in flight per wave -- a trip loads
// the pair of both rows, then works through the four terms --, every grid value read once (non-temporal); flux and
// inv_var from LDS (STAGE: staged once per block) while n_time <= kChi2wStageMax, from the caches past that.  Lane l takes
// the stamp pairs (2 j, 2 j + 1), j = l, l + 64, ... in ascending order, an odd n_time's last stamp after them on lane
// (n_time / 2) % 64, then one wave_sum's butterfly per row.  A row whose address is a multiple of 16 reads each pair with
// one 16-byte load, any other row with two 8-byte loads of the same values into the same arithmetic.  The three constants
// arrive by value; no workspace.  A row's bits depend on n_time, the constants and the row's values alone: neither the
// launch geometry, the row's position, its alignment nor the other rows enter.
//
// Unlike its siblings this kernel is bound by the fp64 VALU port, not by HBM: exp and log1p are OCML's software sequences
// (gfx950 has no fp64 exp instruction).  A scheduling region ends after every term: four inlined exp and four log1p in one
// region are what crashed the register allocator in softmin_rows_kernel (trx_softmin.hpp), and a trip's loads are all
// issued before its first term, so nothing that hides latency is lost.
#pragma once
#include "trx_reduce.hpp"

namespace {

struct RobustC {
    double c0, c1, k2;
};

__device__ __forceinline__ double robust_term(double f, double m, double w, const RobustC& c)
{
#pragma clang fp contract(off)
    const double d = f - m;
    const double a = (0.5 * (w * d)) * d;
    const double A = a + c.c0;
    const double B = fma(a, c.k2, c.c1);
    const double lo = fmin(A, B);
    const double e = exp(-fabs(A - B));
    return lo - log1p(e);
}

__device__ __forceinline__ void robust_load_pair(const double* __restrict__ row, int j, bool vec, double& m0, double& m1)
{
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    if (vec) {
        const dvec2 m = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(row) + j);
        m0 = m.x; m1 = m.y;
    } else {
        m0 = __builtin_nontemporal_load(row + 2 * j);
        m1 = __builtin_nontemporal_load(row + 2 * j + 1);
    }
}

__device__ __forceinline__ void robust_store(double tot, long r, const double* __restrict__ secdepth, double sec_limit,
                                             int accumulate, double* __restrict__ out)
{
    double h = tot < 0.0 ? 0.0 : tot;                               // (a NaN stays a NaN)
    if (secdepth && secdepth[r] >= sec_limit) h = INFINITY;        // (false for a NaN depth, as in numpy)
    out[r] = accumulate ? out[r] + h : h;                           // (+inf stays +inf: h is never -inf)
}

template <bool STAGE>
__global__ __launch_bounds__(256) void chi2_robust_kernel(const double* __restrict__ flux,
                                                          const double* __restrict__ inv_var,
                                                          const double* __restrict__ grid, int n_time, long n,
                                                          const double* __restrict__ secdepth, double sec_limit,
                                                          int accumulate, double* __restrict__ out, const RobustC c)
{
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    // STAGE: [2][n_time rounded up to even]
    extern __shared__ __attribute__((aligned(16))) double robust_lds[];
    const double* f = flux;
    const double* w = inv_var;
    if (STAGE) {
        const int n_pad = (n_time + 1) & ~1;
        for (int t = threadIdx.x; t < n_time; t += 256) {
            robust_lds[t] = flux[t];
            robust_lds[n_pad + t] = inv_var[t];
        }
        __syncthreads();
        f = robust_lds;
        w = robust_lds + n_pad;
    }
    const int lane = threadIdx.x & 63;
    const int nv = n_time >> 1;
    const long wave0 = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long nwaves = (long)gridDim.x * 4;
    for (long r = wave0; r < n; r += 2 * nwaves) {
        // two rows per pass, their loads in flight together; each row's arithmetic is its own
        const long r2 = r + nwaves;
        const bool two = r2 < n;
        const double* row0 = grid + (size_t)r * n_time;
        const double* row1 = grid + (size_t)(two ? r2 : r) * n_time;
        const bool vec0 = ((uintptr_t)row0 & 15) == 0, vec1 = ((uintptr_t)row1 & 15) == 0;      // (per row: wave-uniform)
        double acc0 = 0.0, acc1 = 0.0;
        for (int j = lane; j < nv; j += 64) {
            double a0, a1, b0 = 0.0, b1 = 0.0, f0, f1, w0, w1;
            robust_load_pair(row0, j, vec0, a0, a1);
            if (two) robust_load_pair(row1, j, vec1, b0, b1);
            if (STAGE) {
                // (the staged copies are 16-byte aligned whatever the caller's pointers are)
                const dvec2 fv = reinterpret_cast<const dvec2*>(f)[j], wv = reinterpret_cast<const dvec2*>(w)[j];
                f0 = fv.x; f1 = fv.y; w0 = wv.x; w1 = wv.y;
            } else {
                f0 = f[2 * j]; f1 = f[2 * j + 1]; w0 = w[2 * j]; w1 = w[2 * j + 1];
            }
            __builtin_amdgcn_sched_barrier(0);
            acc0 += robust_term(f0, a0, w0, c);
            __builtin_amdgcn_sched_barrier(0);
            acc0 += robust_term(f1, a1, w1, c);
            __builtin_amdgcn_sched_barrier(0);
            if (two) {
                acc1 += robust_term(f0, b0, w0, c);
                __builtin_amdgcn_sched_barrier(0);
                acc1 += robust_term(f1, b1, w1, c);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if ((n_time & 1) && lane == (nv & 63)) {
            const int t = n_time - 1;
            const double ft = f[t], wt = w[t];
            const double m0 = __builtin_nontemporal_load(row0 + t);
            const double m1 = two ? __builtin_nontemporal_load(row1 + t) : 0.0;
            __builtin_amdgcn_sched_barrier(0);
            acc0 += robust_term(ft, m0, wt, c);
            __builtin_amdgcn_sched_barrier(0);
            if (two) acc1 += robust_term(ft, m1, wt, c);
            __builtin_amdgcn_sched_barrier(0);
        }
        const double tot0 = wave_sum(acc0), tot1 = wave_sum(acc1);
        if (lane == 0) {
            robust_store(tot0, r, secdepth, sec_limit, accumulate, out);
            if (two) robust_store(tot1, r2, secdepth, sec_limit, accumulate, out);
        }
    }
}

}  // namespace
