// The soft minimum of J candidate values per row: softmin_rows_kernel<J> (trxt_softmin_rows, include/trx_shift.h; DESIGN.md
// section 14).  Included by trx_kernels.hip only.
//
// A dataset with a t0_grid has its term of the log-weight evaluated on J shifted copies of its stamps; candidate j's values
// lie in row j of cand ([J] rows of `stride` doubles, n of them used).  Per row r
//     a_j = cand[j][r] - lnc_j,  m = min_j a_j,  T[r] = m - ln sum_j exp(m - a_j)  =  -ln sum_j exp(lnc_j - cand[j][r]),
// clamped at 0, written or added to out[r] -- the statement of _numerics.t0_mix_halfchi2, the fmin chain and the sum in
// ascending j.
//
// One lane per row: the J loads of a wave are 512 contiguous bytes each (non-temporal: every value is read once), then J exp
// and one log in registers.  No LDS, no scratch, no cross-lane traffic: a row's bits depend on its J values and lnc alone.
#pragma once
#include "trx_scan.hpp"

namespace {

constexpr int kSoftminMax = 8;          // candidates (datasets.MAX_T0_NODES)
static_assert(kSoftminMax * sizeof(double) <= sizeof(Lnc8), "a log-weight per candidate");

template <int J>
__global__ __launch_bounds__(256) void softmin_rows_kernel(const double* __restrict__ cand, long stride, long n,
                                                           Lnc8 lnc, int accumulate, double* __restrict__ out)
{
    static_assert(J >= 1 && J <= kSoftminMax, "1 .. 8 candidates");
    const long step = (long)gridDim.x * 256;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < n; r += step) {
        double a[J];
#pragma unroll
        for (int j = 0; j < J; ++j) a[j] = __builtin_nontemporal_load(cand + (size_t)j * (size_t)stride + r) - lnc.v[j];
        double m = a[0];
#pragma unroll
        for (int j = 1; j < J; ++j) m = fmin(m, a[j]);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            s += exp(m - a[j]);
            // (a scheduling region of eight inlined exp and the log crashes the register allocator of ROCm 7.2's clang
            // under -amdgpu-sched-strategy=iterative-ilp; a region ends here after every fourth term.  The loads are all
            // issued above, so nothing that hides latency is lost.)
            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        const double t = softmin_tail(m, s);
        out[r] = accumulate ? out[r] + t : t;                // (+inf stays +inf: t is never -inf)
    }
}

}  // namespace
