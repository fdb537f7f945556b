// White noise whose size is marginalised over a small grid of candidate variance models: chi2_white_mix_kernel<STAGE, J>
// (trxv_chi2_grid_white_mix, include/trx_mix.h).  Included by trx_kernels.hip only, after
// trx_noise_mix.hpp.
//
// Candidate j = 0 .. J - 1 has a weight vector w_j[t] = 1 / (k_j^2 sigma_t^2 + s_j^2) ([J][n_time],
// datasets.white_mix_system) and a log-weight lnc_j (ln prior + 0.5 sum_t ln w_j[t], normalised on the host).  With
// d_t = flux_t - model[r][t] and h_j[r] = 0.5 sum_t w_j[t] d_t^2 -- the bits of chi2_rows_kernel<STAGE, Chi2Plain> on
// inv_var = w_j --
//     a_j = h_j - lnc_j,  m = min_j a_j,  T[r] = m - ln sum_j exp(m - a_j)  =  -ln sum_j exp(lnc_j - h_j[r]),
// clamped at 0, then the secondary rule and the accumulate (T is not halved again); cand_out[r][j] = h_j[r].
//
// A kernel of its own, as chi2_robust_kernel is: chi2_rows_kernel's instantiations stay what they are.  The layout is
// theirs (trx_reduce.hpp): 256 threads, one wavefront per row, two rows in flight per wave -- a trip loads the pair of both
// rows, forms the four residuals once and feeds them to all J candidates --, every grid value read once (non-temporal);
// flux and the J weight vectors from LDS (STAGE: [1 + J][n_time rounded up to even] doubles, staged once per block) while
// they fit the 32 KB of kChi2wStageMax -- white_stage_max(J) stamps: 2048, 1364, 1024, 818, 682, 584, 512, 454 --, from
// the caches past that.  Lane l takes the stamp pairs (2 i, 2 i + 1), i = l, l + 64, ... in ascending order, an odd
// n_time's last stamp after them on lane (n_time / 2) % 64; a term is fma(w_j * d, d, acc_j) with the product rounded on
// its own, then one wave_sum's butterfly per candidate and row and the factor 0.5: chi2_row_partial's arithmetic in its
// order.  A row whose address is a multiple of 16 reads each pair with one 16-byte load, any other row with two 8-byte
// loads of the same values.  The finish is ou_mix_kernel's (ou_mix_finish: one exp and one log a pass, softmin_tail, the
// candidates in ascending j); one candidate needs neither (white_store_one: the same bits).  A row's bits depend on n_time, J, its values and the tables alone: neither the launch
// geometry, the row's position nor its alignment enters.
//
// Resources (gfx950, as built; tests/test_build_resources_white_mix.py): no scratch; VGPRs
//   J          1    2    3    4    5    6    7    8
//   STAGE      34   48   60   72   84   97  109  121
//   !STAGE     32   46   58   70   83   95  107  117
#pragma once
#include "trx_noise_mix.hpp"
#include "trx_robust.hpp"

namespace {

constexpr int kWhiteMixMax = 8;         // candidates (datasets.MAX_WHITE_CANDIDATES)
static_assert(kWhiteMixMax * sizeof(double) <= sizeof(Lnc8), "a log-weight per candidate");

// stamps up to which flux and the j weight vectors are staged in LDS
constexpr int white_stage_max(int j) { return ((2 * kChi2wStageMax) / (1 + j)) & ~1; }
static_assert(white_stage_max(1) == kChi2wStageMax, "one candidate: chi2_rows_kernel's two staged vectors");
static_assert(white_stage_max(2) == 1364 && white_stage_max(8) == 454, "the limits the tests straddle");

// what the kernel takes behind chi2_rows_kernel's arguments: the candidates' weights [J][n_time], their log-weights and
// the optional [n][J] output of the h_j
struct WhiteMix {
    const double* weights;
    Lnc8 lnc;
    double* cand_out;
};

// One candidate: T = h - lnc without the exp and the log -- the bits of ou_mix_finish<1>, whose sum is exp(0) = 1 and whose
// tail is m - log(1) = m (a row of 100 stamps is one trip: the two would be a tenth of its time).
__device__ __forceinline__ void white_store_one(double h, long r, const WhiteMix& mix, const double* __restrict__ secdepth,
                                                double sec_limit, int accumulate, double* __restrict__ out)
{
    double t = h - mix.lnc.v[0];
    t = t < 0.0 ? 0.0 : t;                                          // (a NaN stays a NaN, lnc = -inf gives +inf)
    if (secdepth && secdepth[r] >= sec_limit) t = INFINITY;        // (false for a NaN depth, as in numpy)
    out[r] = accumulate ? out[r] + t : t;                           // (+inf stays +inf: t is never -inf)
    if (mix.cand_out) mix.cand_out[r] = h;
}

template <bool STAGE, int J>
__global__ __launch_bounds__(256) void chi2_white_mix_kernel(const double* __restrict__ flux,
                                                             const double* __restrict__ grid, int n_time, long n,
                                                             const double* __restrict__ secdepth, double sec_limit,
                                                             int accumulate, double* __restrict__ out, const WhiteMix mix)
{
    static_assert(J >= 1 && J <= kWhiteMixMax, "1 .. 8 candidates");
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    // STAGE: [1 + J][n_time rounded up to even]
    extern __shared__ __attribute__((aligned(16))) double white_lds[];
    const double* f = flux;
    const double* w = mix.weights;
    int w_stride = n_time;
    if (STAGE) {
        const int n_pad = (n_time + 1) & ~1;
        for (int t = threadIdx.x; t < n_time; t += 256) {
            white_lds[t] = flux[t];
#pragma unroll
            for (int j = 0; j < J; ++j) white_lds[(1 + j) * n_pad + t] = mix.weights[(size_t)j * n_time + t];
        }
        __syncthreads();
        f = white_lds;
        w = white_lds + n_pad;
        w_stride = n_pad;
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
        double acc0[J], acc1[J];
#pragma unroll
        for (int j = 0; j < J; ++j) acc0[j] = acc1[j] = 0.0;
        for (int i = lane; i < nv; i += 64) {
            double a0, a1, b0 = 0.0, b1 = 0.0, f0, f1;
            robust_load_pair(row0, i, vec0, a0, a1);
            if (two) robust_load_pair(row1, i, vec1, b0, b1);
            if (STAGE) {
                // (the staged copies are 16-byte aligned whatever the caller's pointers are)
                const dvec2 fv = reinterpret_cast<const dvec2*>(f)[i];
                f0 = fv.x; f1 = fv.y;
            } else {
                f0 = f[2 * i]; f1 = f[2 * i + 1];
            }
            const double d00 = f0 - a0, d01 = f1 - a1, d10 = f0 - b0, d11 = f1 - b1;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double* wj = w + (size_t)j * w_stride;
                double w0, w1;
                if (STAGE) {
                    const dvec2 wv = reinterpret_cast<const dvec2*>(wj)[i];
                    w0 = wv.x; w1 = wv.y;
                } else {
                    w0 = wj[2 * i]; w1 = wj[2 * i + 1];
                }
                acc0[j] = fma(w0 * d00, d00, acc0[j]);
                acc0[j] = fma(w1 * d01, d01, acc0[j]);
                if (two) {
                    acc1[j] = fma(w0 * d10, d10, acc1[j]);
                    acc1[j] = fma(w1 * d11, d11, acc1[j]);
                }
            }
        }
        if ((n_time & 1) && lane == (nv & 63)) {
            const int t = n_time - 1;
            const double ft = f[t];
            const double d0 = ft - __builtin_nontemporal_load(row0 + t);
            const double d1 = ft - __builtin_nontemporal_load(row1 + t);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double wt = w[(size_t)j * w_stride + t];
                acc0[j] = fma(wt * d0, d0, acc0[j]);
                if (two) acc1[j] = fma(wt * d1, d1, acc1[j]);
            }
        }
        double h0[J], h1[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            h0[j] = 0.5 * wave_sum(acc0[j]);
            h1[j] = 0.5 * wave_sum(acc1[j]);
        }
        if constexpr (J == 1) {
            if (lane == 0) {
                white_store_one(h0[0], r, mix, secdepth, sec_limit, accumulate, out);
                if (two) white_store_one(h1[0], r2, mix, secdepth, sec_limit, accumulate, out);
            }
        } else {
            ou_mix_finish<J>(h0, h1, r, r2, two, mix.lnc, secdepth, sec_limit, accumulate, out, mix.cand_out, lane);
        }
    }
}

}  // namespace
