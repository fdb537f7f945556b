// Correlated noise with its amplitude and time scale marginalised over a small grid of candidates: ou_mix_kernel<ONE, J>
// (trxm_chi2_grid_ou_mix, include/trx_mix.h).  Included by trx_kernels.hip only, after trx_noise.hpp.
//
// Candidate j = 0 .. J - 1 has tables alpha_j, beta_j, omega_j ([J][n_time], datasets.ou_mix_system) and a log-weight lnc_j
// (ln prior + 0.5 sum ln omega_j, normalised on the host).  With h_j[r] what the OU filter computes from candidate j's
// tables -- ou_row_trip on ou_trip's tables, so the same bits --
//     a_j = h_j - lnc_j,  m = min_j a_j,  T[r] = m - ln sum_j exp(m - a_j)  =  -ln sum_j exp(lnc_j - h_j[r]),
// clamped at 0, then the secondary rule and the accumulate of chi2w_store (T is not halved again).
//
// A kernel of its own, not a filter of scan_rows_kernel (trx_scan.hpp), over the same pieces -- ScanPair, ou_trip,
// ou_row_trip, wave_read_lane, softmin_tail: a row's values are loaded once (non-temporal) and their residuals serve
// all J candidates inside a trip, the tables may be staged once per block behind a barrier, and the finish takes both rows
// of a pass together.  What differs between the instantiations is where a candidate's trip tables (OuTrip without the
// flux: kOuMixFields doubles a lane) live:
//   ONE, J <= kOuMixRegCands   in registers, formed once per wave (J * 26 VGPRs)
//   ONE, J >  kOuMixRegCands   in LDS, formed once per block ([J][kOuMixFields][64] doubles, 52 KB at J = 8: lane-contiguous,
//                              no bank conflicts), read once per candidate for both rows of a pass
//   !ONE                       formed per trip and candidate from the cached tables, as the OU filter does
// and the per-candidate carry / acc of both rows are registers (4 J doubles).  No scratch, at most 256 VGPRs
// (__launch_bounds__(256, 2): two waves a SIMD).
//
// The soft minimum costs one exp and one log a pass, not 2 J + 2: h_j is wave-uniform after wave_sum, lane 8 i + j forms
// exp(m - a_j) of the pass' row i, and lanes 0 and 8 sum their row's J terms in ascending j (read from the lanes that formed
// them), take the log and store.  The order of a row's arithmetic is fixed by n_time and J alone.
#pragma once
#include "trx_noise.hpp"

namespace {

constexpr int kOuMixMax = 8;            // candidates (datasets.MAX_RED_CANDIDATES)
static_assert(kOuMixMax * sizeof(double) <= sizeof(Lnc8), "a log-weight per candidate");
constexpr int kOuMixRegCands = 4;       // ONE: up to here the candidates' tables stay in registers
constexpr int kOuMixFields = 13;        // OuTrip without f0, f1

// what the kernel takes behind scan_rows_kernel's arguments: the candidates' tables [J][n_time], their log-weights and
// the optional [n][J] output of the h_j
struct OuMix {
    const double *alpha, *beta, *omega;
    Lnc8 lnc;
    double* cand_out;
};

__device__ __forceinline__ void ou_mix_put(double* __restrict__ s, const OuTrip& t, int lane)
{
    s[0 * 64 + lane] = t.w0;
    s[1 * 64 + lane] = t.w1;
    s[2 * 64 + lane] = t.A0;
    s[3 * 64 + lane] = t.A1;
    s[4 * 64 + lane] = t.B0;
    s[5 * 64 + lane] = t.B1;
#pragma unroll
    for (int k = 0; k < kOuScanSteps; ++k) s[(6 + k) * 64 + lane] = t.m[k];
    s[12 * 64 + lane] = t.ainc;
}

__device__ __forceinline__ OuTrip ou_mix_get(const double* __restrict__ s, double f0, double f1, int lane)
{
    OuTrip t;
    t.f0 = f0;
    t.f1 = f1;
    t.w0 = s[0 * 64 + lane];
    t.w1 = s[1 * 64 + lane];
    t.A0 = s[2 * 64 + lane];
    t.A1 = s[3 * 64 + lane];
    t.B0 = s[4 * 64 + lane];
    t.B1 = s[5 * 64 + lane];
#pragma unroll
    for (int k = 0; k < kOuScanSteps; ++k) t.m[k] = s[(6 + k) * 64 + lane];
    t.ainc = s[12 * 64 + lane];
    return t;
}

// e of the lanes 8 ROW + 0 .. K, summed in ascending order: ((e_0 + e_1) + e_2) + ...
template <int ROW, int K>
__device__ __forceinline__ double ou_mix_sum(double e)
{
    if constexpr (K == 0) return wave_read_lane<8 * ROW>(e);
    else return ou_mix_sum<ROW, K - 1>(e) + wave_read_lane<8 * ROW + K>(e);
}

// The pass' two rows from their candidates' h (wave-uniform): T, the clamp, the secondary rule, the accumulate; cand_out.
template <int J>
__device__ __forceinline__ void ou_mix_finish(const double (&h0)[J], const double (&h1)[J], long r, long r2, bool two,
                                              const Lnc8& lnc, const double* __restrict__ secdepth, double sec_limit,
                                              int accumulate, double* __restrict__ out, double* __restrict__ cand_out,
                                              int lane)
{
    const int jj = lane & 7;
    const bool second = (lane & 8) != 0;
    double m0 = h0[0] - lnc.v[0], m1 = h1[0] - lnc.v[0];
    double mine = second ? m1 : m0;
#pragma unroll
    for (int j = 1; j < J; ++j) {
        const double a0 = h0[j] - lnc.v[j], a1 = h1[j] - lnc.v[j];
        m0 = fmin(m0, a0);
        m1 = fmin(m1, a1);
        if (jj == j) mine = second ? a1 : a0;
    }
    const double m = second ? m1 : m0;
    const double e = exp(m - mine);                     // (lane 8 i + j: the term of candidate j of row i)
    const double s0 = ou_mix_sum<0, J - 1>(e), s1 = ou_mix_sum<1, J - 1>(e);
    double t = softmin_tail(m, second ? s1 : s0);
    if (lane == 0 || (lane == 8 && two)) {
        const long row = second ? r2 : r;
        if (secdepth && secdepth[row] >= sec_limit) t = INFINITY;          // (false for a NaN depth, as in numpy)
        out[row] = accumulate ? out[row] + t : t;                           // (+inf stays +inf: t is never -inf)
        if (cand_out) {
#pragma unroll
            for (int j = 0; j < J; ++j) cand_out[row * J + j] = second ? h1[j] : h0[j];
        }
    }
}

template <bool ONE, int J>
__global__ __launch_bounds__(256, 2) void ou_mix_kernel(const double* __restrict__ flux, const double* __restrict__ grid,
                                                        int n_time, long n, const double* __restrict__ secdepth,
                                                        double sec_limit, int accumulate, double* __restrict__ out,
                                                        const OuMix mix)
{
    static_assert(J >= 1 && J <= kOuMixMax, "1 .. 8 candidates");
    constexpr bool REGS = ONE && J <= kOuMixRegCands, LDS = ONE && !REGS;
    __shared__ double tab[LDS ? J * kOuMixFields * 64 : 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long wave0 = (long)blockIdx.x * 4 + wave;
    const long nwaves = (long)gridDim.x * 4;
    // candidate j's tables of the trip from `base`
    const auto trip = [&](int j, int base) {
        return ou_trip(flux, mix.alpha + (size_t)j * n_time, mix.beta + (size_t)j * n_time,
                       mix.omega + (size_t)j * n_time, n_time, base, lane);
    };
    OuTrip tr[REGS ? J : 1];
    double f0 = 0.0, f1 = 0.0;
    if constexpr (REGS) {
#pragma unroll
        for (int j = 0; j < J; ++j) tr[j] = trip(j, 0);
    }
    if constexpr (LDS) {
        // (wave w forms the candidates w, w + 4: every wave reaches the barrier)
        for (int j = wave; j < J; j += 4) ou_mix_put(tab + j * kOuMixFields * 64, trip(j, 0), lane);
        f0 = 2 * lane < n_time ? flux[2 * lane] : 0.0;
        f1 = 2 * lane + 1 < n_time ? flux[2 * lane + 1] : 0.0;
        __syncthreads();
    }
    for (long r = wave0; r < n; r += 2 * nwaves) {
        const ScanPair p(grid, n_time, n, r, nwaves);
        double carry0[J], carry1[J], acc0[J], acc1[J];
#pragma unroll
        for (int j = 0; j < J; ++j) carry0[j] = carry1[j] = acc0[j] = acc1[j] = 0.0;
        for (int base = 0; base < n_time; base += kOuTrip) {
            double a0, a1, b0, b1;
            p.load(n_time, base, lane, a0, a1, b0, b1);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                OuTrip t;
                if constexpr (REGS) t = tr[j];
                else if constexpr (LDS) t = ou_mix_get(tab + j * kOuMixFields * 64, f0, f1, lane);
                else t = trip(j, base);
                ou_row_trip(t, a0, a1, carry0[j], acc0[j], lane);
                if (p.two) ou_row_trip(t, b0, b1, carry1[j], acc1[j], lane);
            }
            if (ONE) break;                                   // (n_time <= kOuTrip)
        }
        double h0[J], h1[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            h0[j] = 0.5 * wave_sum(acc0[j]);
            h1[j] = 0.5 * wave_sum(acc1[j]);
        }
        ou_mix_finish<J>(h0, h1, r, p.r2, p.two, mix.lnc, secdepth, sec_limit, accumulate, out, mix.cand_out, lane);
    }
}

}  // namespace
