// Baseline terms marginalised next to white noise of unknown size: chi2_white_lin_kernel<STAGE, J, K>
// (trxb_chi2_grid_white_baseline, include/trx_gls.h).  Included by trx_kernels.hip only, after
// trx_white_mix.hpp.
//
// Candidate j = 0 .. J - 1 has a weight vector w_j[t] = 1 / (k_j^2 sigma_t^2 + s_j^2) ([J][n_time]), the K baseline columns
// B_k[t] ([K][n_time]) are the same for all of them, and the host forms per candidate the inverse of the system matrix
// A_j = B^T W_j B + diag(1 / s_k^2) -- packed upper triangle by rows, in the units of the raw sums, by value in the kernel
// arguments -- and the log-weight lnc_j (ln prior + 0.5 sum_t ln w_j[t] - 0.5 ln det A_j, normalised;
// datasets.white_baseline_system).  With d_t = flux_t - model[r][t]:
//     S2_j = sum_t w_j[t] d_t^2,   b_jk = sum_t w_j[t] B_k[t] d_t,   c_j = A_j^-1 b_j,
//     h_j = 0.5 max(S2_j - b_j . c_j, 0),   T[r] = -ln sum_j exp(lnc_j - h_j)   (ou_mix_finish; white_store_one for J = 1),
// then the secondary rule and the accumulate; cand_out[r][j] = h_j, coef_out[r][j][k] = c_jk.  minv = 0 gives 0.5 S2_j.
//
// A kernel of its own, in chi2_white_mix_kernel's layout: 256 threads, one wavefront per row, every grid value read once
// (non-temporal, robust_load_pair for both alignments); flux, the J weight vectors and the K columns from LDS (STAGE:
// [1 + J + K][n_time rounded up to even] doubles, staged once per block) while they fit the 32 KB of kChi2wStageMax --
// wlin_stage_max(J, K) stamps --, from the caches past that.  Lane l takes the stamp pairs l, l + 64, ... in ascending
// order, an odd n_time's last stamp after them on lane (n_time / 2) % 64.  Per value and candidate: u = w_j d rounded on
// its own, S2_j = fma(u, d, S2_j), b_jk = fma(B_k, u, b_jk).  A wave keeps two rows in flight while the J (1 + K) sums of
// both fit the registers (J (1 + K) <= kWlinTwoRowSums), one row past that.
//
// The J (1 + K) cross-lane sums of a row, up to 40, are folded together (wlin_fold).  In each of the first three steps a
// lane keeps the sums of one half of the candidates it holds and adds to them what its partner -- the mirror lane of its
// row of 16, of its half row, of its quad: one DPP move each -- held of the same candidates, so that the sums a lane holds
// halve with every step (8, 4, 2, 1 candidates); the fourth step (the neighbour) and two butterfly steps across the four
// rows of 16 add up the 1 + K sums of the one candidate left.  A candidate's totals then sit together on the lanes that
// kept it (wlin_lane_of_cand), and those lanes form its quadratic form with its A^-1 -- read once per wave from
// the copy in LDS that the block makes of the kernel arguments' --, so the forms of all candidates cost one candidate's instructions and no total is read across lanes;
// only the J values h_j are (wlin_gather) for the finish.  About J (1 + K) + 5 (1 + K) move-and-add steps in place of
// 6 J (1 + K).  The order of a row's arithmetic is fixed by n_time, J and K alone: neither the launch geometry, the row's
// position nor its alignment enters.
//
// Resources (gfx950, as built; tests/test_build_resources_white_lin.py): no scratch, no static LDS; VGPRs (STAGE / !STAGE)
//   J        1      2      3       4        5        6        7        8
//   K = 1  42/38  60/56   76/73   93/89  111/107   79/81    87/89    95/97
//   K = 2  52/50  78/72   95/93   82/83   87/91    95/99  105/109  119/119
//   K = 3  66/64  94/90   84/88   98/99  105/109  117/121  129/133  145/145
//   K = 4  82/80 116/111 100/104 118/117 127/131  141/145  155/159  175/173
// Two rows in flight with 12 sums took 128 - 131 VGPRs (J = 6, K = 1; J = 4, K = 2; J = 3, K = 3), with 16 up to 156: hence
// kWlinTwoRowSums = 10.  The launcher's cap of blocks a CU assumes wlin_vgpr_bound(J, K): 128 up to 24 sums (four waves a
// SIMD), 168 up to 35 (three), 256 at 40 (two).
//
// Measured on one MI355X: profiles/white_baseline/results.txt.
#pragma once
#include "trx_white_mix.hpp"

namespace {

constexpr int kWlinMaxCands = 8;        // candidates (datasets.MAX_WHITE_CANDIDATES)
constexpr int kWlinMaxTerms = kChi2bMaxTerms;
constexpr int kWlinPacked = kWlinMaxTerms * (kWlinMaxTerms + 1) / 2;
constexpr int kWlinTwoRowSums = 10;     // J (1 + K) up to which a wave keeps two rows in flight: with 12 they need 128 - 131 VGPRs
constexpr int kWlinFourWaveSums = 24;   // J (1 + K) up to which an instantiation stays within 128 VGPRs
constexpr int kWlinThreeWaveSums = 35;  // ... within 168
// stamps up to which flux, the j weight vectors and the k columns are staged in LDS
constexpr int wlin_stage_max(int j, int k) { return ((2 * kChi2wStageMax) / (1 + j + k)) & ~1; }
static_assert(wlin_stage_max(1, 1) == 1364 && wlin_stage_max(8, 4) == 314, "the limits the tests straddle");

// doubles of LDS in front of the staged vectors: the candidates' packed A^-1, rounded up to keep the vectors 16-byte aligned
constexpr int wlin_minv_doubles(int j, int k) { return (j * (k * (k + 1) / 2) + 1) & ~1; }

// the VGPRs an instantiation may take (tests/test_build_resources_white_lin.py holds the code object against it): what
// the launcher's cap of resident blocks counts on
constexpr int wlin_vgpr_bound(int j, int k)
{
    return j * (1 + k) <= kWlinFourWaveSums ? 128 : j * (1 + k) <= kWlinThreeWaveSums ? 168 : 256;
}

// what the kernel takes behind chi2_rows_kernel's arguments
struct WhiteLin {
    const double* weights;              // [J][n_time]
    const double* basis;                // [K][n_time]
    Lnc8 lnc;
    double minv[kWlinMaxCands][kWlinPacked];    // candidate j's A_j^-1, i <= l at chi2b_at<K>(i, l)
    double* cand_out;                   // [n][J] or null
    double* coef_out;                   // [n][J][K] or null
};

// the partner's value in halving step S: the mirror lane of the row of 16, of the half row, of the quad, the neighbour
template <int S>
__device__ __forceinline__ double wlin_partner(double v)
{
    static_assert(S >= 0 && S < 4, "four steps inside a row of 16 lanes");
    if constexpr (S == 0) return ou_dpp<0x140, 0xf>(v, 0.0);          // row_mirror
    else if constexpr (S == 1) return ou_dpp<0x141, 0xf>(v, 0.0);     // row_half_mirror
    else if constexpr (S == 2) return ou_dpp<0x01b, 0xf>(v, 0.0);     // quad_perm [3, 2, 1, 0]
    else return ou_dpp<0x0b1, 0xf>(v, 0.0);                           // quad_perm [1, 0, 3, 2]
}

// Where candidate j of J ends up after the halving steps: the lane of the first row of 16 whose bits 8, 4, 2 say which
// half was kept in steps 0, 1, 2 (a step splits ceil(count / 2) candidates from the rest; an odd count pads the upper half).
constexpr int wlin_lane_of_cand(int j, int J)
{
    int lane = 0;
    for (int s = 0, cnt = J; s < 3 && cnt > 1; ++s) {
        const int half = (cnt + 1) / 2;
        if (j >= half) {
            j -= half;
            lane |= 8 >> s;
        }
        cnt = half;
    }
    return lane;
}

// the candidate whose totals a lane holds after the fold, or -1 (a padded place of an odd split)
template <int J>
__device__ __forceinline__ int wlin_cand_of_lane(int lane)
{
    int j = 0, live = J, cnt = J;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (cnt > 1) {
            const int half = (cnt + 1) / 2;
            if (lane & (8 >> s)) {
                j += half;
                live -= half;
            } else {
                live = live < half ? live : half;
            }
            cnt = half;
        }
    }
    return live > 0 ? j : -1;
}

// Step S of the fold on the CNT candidates' sums v[0 .. CNT (1 + K)) a lane still holds.  While it holds more than one
// candidate (steps 0 .. 2), the lanes whose bit (8 >> S) is clear keep the first ceil(CNT / 2) candidates, the others the
// rest (an odd CNT: zeros in the last place), and each adds its partner's share of what it keeps; with one candidate left
// a step adds the partner's sums of that candidate; after the four steps, a butterfly across the four rows of 16.
template <int K, int CNT, int S, int NV>
__device__ __forceinline__ void wlin_halve(double (&v)[NV], int lane)
{
    constexpr int W = 1 + K;
    if constexpr (S < 3 && CNT > 1) {
        constexpr int half = (CNT + 1) / 2;
        const bool up = (lane & (8 >> S)) != 0;
#pragma unroll
        for (int i = 0; i < half * W; ++i) {
            const double lo = v[i];
            const double hi = half * W + i < CNT * W ? v[half * W + i] : 0.0;
            const double keep = up ? hi : lo, send = up ? lo : hi;
            v[i] = keep + wlin_partner<S>(send);
        }
        wlin_halve<K, half, S + 1>(v, lane);
    } else if constexpr (S < 4) {
        static_assert(CNT == 1, "eight candidates at most: three halving steps leave one");
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] += wlin_partner<S>(v[i]);
        wlin_halve<K, 1, S + 1>(v, lane);
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            v[i] += __shfl_xor(v[i], 16, 64);
            v[i] += __shfl_xor(v[i], 32, 64);
        }
    }
}

// The totals over the wave of the J (1 + K) sums a lane holds: afterwards acc[0 .. 1 + K) are the totals of the lane's own
// candidate (wlin_cand_of_lane; anything on a lane without one).
template <int J, int K>
__device__ __forceinline__ void wlin_fold(double (&acc)[J * (1 + K)], int lane)
{
    wlin_halve<K, J, 0>(acc, lane);
}

// one stamp's terms of every candidate's sums: acc[j (1 + K)] = S2_j, acc[j (1 + K) + 1 + k] = b_jk
template <int J, int K>
__device__ __forceinline__ void wlin_terms(double (&acc)[J * (1 + K)], const double (&w)[J], const double (&b)[K], double d)
{
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double u = w[j] * d;
        acc[j * (1 + K)] = fma(u, d, acc[j * (1 + K)]);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[j * (1 + K) + 1 + k] = fma(b[k], u, acc[j * (1 + K) + 1 + k]);
    }
}

// The lane's own candidate from its totals tot[0 .. 1 + K) and its packed A^-1: h, and the coefficients where asked for
template <int J, int K>
__device__ __forceinline__ double wlin_form(const double (&tot)[J * (1 + K)], const double (&mv)[K * (K + 1) / 2], long r,
                                            int cand, bool write, double* __restrict__ coef_out)
{
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double c = 0.0;
#pragma unroll
        for (int l = 0; l < K; ++l) c = fma(mv[chi2b_at<K>(i, l)], tot[1 + l], c);
        q = fma(tot[1 + i], c, q);
        if (write) coef_out[(r * J + cand) * K + i] = c;
    }
    const double t = tot[0] - q;
    return 0.5 * (t < 0.0 ? 0.0 : t);                                  // (a NaN stays a NaN)
}

// candidate j's h from the lane that formed it, to every lane
template <int J, int I>
__device__ __forceinline__ void wlin_gather(double hl, double (&h)[J])
{
    h[I] = wave_read_lane<wlin_lane_of_cand(I, J)>(hl);
    if constexpr (I + 1 < J) wlin_gather<J, I + 1>(hl, h);
}

template <bool STAGE, int J, int K>
__global__ __launch_bounds__(256) void chi2_white_lin_kernel(const double* __restrict__ flux,
                                                             const double* __restrict__ grid, int n_time, long n,
                                                             const double* __restrict__ secdepth, double sec_limit,
                                                             int accumulate, double* __restrict__ out, const WhiteLin lin)
{
    static_assert(J >= 1 && J <= kWlinMaxCands && K >= 1 && K <= kWlinMaxTerms, "1 .. 8 candidates, 1 .. 4 columns");
    constexpr int N = J * (1 + K);
    constexpr bool TWO = N <= kWlinTwoRowSums;
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    constexpr int P = K * (K + 1) / 2;
    // [J][P] the candidates' packed A^-1 (rounded up to an even count), then STAGE: [1 + J + K][n_time rounded up to even]
    extern __shared__ __attribute__((aligned(16))) double wlin_all[];
    double* wlin_lds = wlin_all + wlin_minv_doubles(J, K);
    // (thread j P + p copies one entry from the kernel arguments: a lane picks its candidate's by index below, which the
    // scalar registers that hold the arguments do not allow; one candidate's scalar loads at a time)
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (threadIdx.x == j * P + p) wlin_all[j * P + p] = lin.minv[j][p];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const double* f = flux;
    const double* w = lin.weights;
    const double* g = lin.basis;
    int stride = n_time;
    if (STAGE) {
        const int n_pad = (n_time + 1) & ~1;
        for (int t = threadIdx.x; t < n_time; t += 256) {
            wlin_lds[t] = flux[t];
#pragma unroll
            for (int j = 0; j < J; ++j) wlin_lds[(1 + j) * n_pad + t] = lin.weights[(size_t)j * n_time + t];
#pragma unroll
            for (int k = 0; k < K; ++k) wlin_lds[(1 + J + k) * n_pad + t] = lin.basis[(size_t)k * n_time + t];
        }
        f = wlin_lds;
        w = wlin_lds + n_pad;
        g = wlin_lds + (1 + J) * n_pad;
        stride = n_pad;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int nv = n_time >> 1;
    const long wave0 = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long nwaves = (long)gridDim.x * 4;
    // the candidate whose totals the fold leaves on this lane, its A^-1, and whether the lane writes its coefficients
    const int cand = wlin_cand_of_lane<J>(lane);
    double mv[P];
#pragma unroll
    for (int p = 0; p < P; ++p) mv[p] = cand >= 0 ? wlin_all[cand * P + p] : 0.0;
    const bool writer = lin.coef_out && cand >= 0 && (lane & ~14) == 0;
    for (long r = wave0; r < n; r += (TWO ? 2 : 1) * nwaves) {
        // TWO: two rows per pass, their loads in flight together; each row's arithmetic is its own
        const long r2 = r + nwaves;
        const bool two = TWO && r2 < n;
        const double* row0 = grid + (size_t)r * n_time;
        const double* row1 = grid + (size_t)(two ? r2 : r) * n_time;
        const bool vec0 = ((uintptr_t)row0 & 15) == 0, vec1 = ((uintptr_t)row1 & 15) == 0;      // (per row: wave-uniform)
        double acc0[N], acc1[TWO ? N : 1];
#pragma unroll
        for (int i = 0; i < N; ++i) acc0[i] = 0.0;
        if constexpr (TWO) {
#pragma unroll
            for (int i = 0; i < N; ++i) acc1[i] = 0.0;
        }
        for (int i = lane; i < nv; i += 64) {
            double a0, a1, b0 = 0.0, b1 = 0.0, f0, f1, w0[J], w1[J], g0[K], g1[K];
            robust_load_pair(row0, i, vec0, a0, a1);
            if (two) robust_load_pair(row1, i, vec1, b0, b1);
            if (STAGE) {
                // (the staged copies are 16-byte aligned whatever the caller's pointers are)
                const dvec2 fv = reinterpret_cast<const dvec2*>(f)[i];
                f0 = fv.x; f1 = fv.y;
            } else {
                f0 = f[2 * i]; f1 = f[2 * i + 1];
            }
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double* wj = w + (size_t)j * stride;
                if (STAGE) {
                    const dvec2 wv = reinterpret_cast<const dvec2*>(wj)[i];
                    w0[j] = wv.x; w1[j] = wv.y;
                } else {
                    w0[j] = wj[2 * i]; w1[j] = wj[2 * i + 1];
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double* gk = g + (size_t)k * stride;
                if (STAGE) {
                    const dvec2 gv = reinterpret_cast<const dvec2*>(gk)[i];
                    g0[k] = gv.x; g1[k] = gv.y;
                } else {
                    g0[k] = gk[2 * i]; g1[k] = gk[2 * i + 1];
                }
            }
            wlin_terms<J, K>(acc0, w0, g0, f0 - a0);
            wlin_terms<J, K>(acc0, w1, g1, f1 - a1);
            if constexpr (TWO) {
                if (two) {
                    wlin_terms<J, K>(acc1, w0, g0, f0 - b0);
                    wlin_terms<J, K>(acc1, w1, g1, f1 - b1);
                }
            }
        }
        if ((n_time & 1) && lane == (nv & 63)) {
            const int t = n_time - 1;
            const double ft = f[t];
            double wt[J], gt[K];
#pragma unroll
            for (int j = 0; j < J; ++j) wt[j] = w[(size_t)j * stride + t];
#pragma unroll
            for (int k = 0; k < K; ++k) gt[k] = g[(size_t)k * stride + t];
            wlin_terms<J, K>(acc0, wt, gt, ft - __builtin_nontemporal_load(row0 + t));
            if constexpr (TWO) {
                if (two) wlin_terms<J, K>(acc1, wt, gt, ft - __builtin_nontemporal_load(row1 + t));
            }
        }
        double h0[J], h1[J];
        wlin_fold<J, K>(acc0, lane);
        wlin_gather<J, 0>(wlin_form<J, K>(acc0, mv, r, cand, writer, lin.coef_out), h0);
        if constexpr (TWO) {
            wlin_fold<J, K>(acc1, lane);
            wlin_gather<J, 0>(wlin_form<J, K>(acc1, mv, r2, cand, writer && two, lin.coef_out), h1);
        } else {
#pragma unroll
            for (int j = 0; j < J; ++j) h1[j] = h0[j];
        }
        if constexpr (J == 1) {
            if (lane == 0) {
                const WhiteMix mix{lin.weights, lin.lnc, lin.cand_out};
                white_store_one(h0[0], r, mix, secdepth, sec_limit, accumulate, out);
                if (two) white_store_one(h1[0], r2, mix, secdepth, sec_limit, accumulate, out);
            }
        } else {
            ou_mix_finish<J>(h0, h1, r, r2, two, lin.lnc, secdepth, sec_limit, accumulate, out, lin.cand_out, lane);
        }
    }
}

}  // namespace
