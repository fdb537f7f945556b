// The HBM-bound reductions: chi2_grid_kernel and chi2_rows_kernel<STAGE, Terms> (row reductions over a materialised
// grid; Terms = Chi2Plain, Chi2Offset, Chi2Baseline<K>) and the log-mean-exp kernels
// (lme_partial_kernel / lme_partial_kernel_star with the scenario's final stage, lme_final_kernel).  Included by
// trx_kernels.hip only.
#pragma once
#include "trx_cells.hpp"

namespace {

// ---------------------------------------------------------------------------------------
// 0.5 * sum_t (flux_t - model[r][t])^2 / sigma^2, one wavefront per row, 16 B/lane loads.
__global__ __launch_bounds__(256) void chi2_grid_kernel(const double* __restrict__ flux,
                                                        const double* __restrict__ grid,
                                                        int n_time, long n, double sigma,
                                                        double* __restrict__ out, int vec_ok)
{
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long nwaves = (long)gridDim.x * 4;
    const double s2 = sigma * sigma;
    for (long r = wave0; r < n; r += nwaves) {
        const double* row = grid + (size_t)r * n_time;
        double acc = 0.0;
        if (vec_ok) {
            typedef double dvec2 __attribute__((ext_vector_type(2)));
            const dvec2* row2 = reinterpret_cast<const dvec2*>(row);
            const dvec2* fl2 = reinterpret_cast<const dvec2*>(flux);
            const int nv = n_time >> 1;
            for (int j = lane; j < nv; j += 64) {
                const dvec2 m = __builtin_nontemporal_load(&row2[j]);
                const dvec2 f = fl2[j];
                const double d0 = f.x - m.x, d1 = f.y - m.y;
                acc += (d0 * d0) / s2;
                acc += (d1 * d1) / s2;
            }
        } else {
            for (int j = lane; j < n_time; j += 64) {
                const double d = flux[j] - row[j];
                acc += (d * d) / s2;
            }
        }
        const double tot = wave_sum(acc);
        if (lane == 0) out[r] = 0.5 * tot;
    }
}

// ---------------------------------------------------------------------------------------
// The weighted row reductions over a materialised grid (trx_chi2_grid_weighted, trx_chi2_grid_offset,
// trx_chi2_grid_baseline): chi2_rows_kernel<STAGE, Terms>.  With d_t = flux_t - model[r][t] every
// form needs S2 = sum_t w_t d_t^2, w = inv_var; the Terms policy says which further sums over the same residuals ride
// along with it and what the store makes of them:
//   Chi2Plain         none                              h[r] = 0.5 * S2
//   Chi2Offset        S1 = sum_t w_t d_t                h[r] = 0.5 * (S2 - S1^2 / (sum_w + prior_prec)),
//                                                       offset_out[r] = S1 / (sum_w + prior_prec)
//   Chi2Baseline<K>   b_k = sum_t g_k[t] d_t, K = 1..4  h[r] = 0.5 * max(S2 - sum_ij M_ij b_i b_j, 0),
//                                                       coef_out[r][i] = sum_j M_ij b_j
// h[r] is written or added to out[r]; +inf where secdepth[r] >= sec_limit.  Chi2Offset marginalises a per-dataset
// baseline offset c ~ N(0, s^2): sum_w = sum_t w_t and prior_prec = 1 / s^2 from the host (0: a flat prior; +inf: no
// offset, Chi2Plain's bits).  Chi2Baseline<K> marginalises a linear baseline model sum_k c_k B_k[t], c_k ~ N(0, s_k^2):
// g_k[t] = w_t B_k[t] / sqrt(D_k) from the host, M the inverse of the unit-diagonal system matrix, packed upper triangle
// by rows, by value in the kernel arguments (it does not depend on the row); M = 0 gives Chi2Plain's bits.  A difference
// that rounding drives below 0 is stored as 0; a NaN stays a NaN.  The offset keeps a form of its own: a column of ones
// through the baseline's store rounds differently.
//
// One wavefront per row, two rows in flight per wave; every grid value is read once (non-temporal); flux, inv_var and
// the K columns come from LDS (STAGE: staged once per block) while they fit the 32 KB of kChi2wStageMax -- 2048 stamps
// without columns, chi2b_stage_max(K) with K -- and from the caches past that.
//
// The order of summation of a row is fixed by n_time alone: lane l takes the stamp pairs (2 j, 2 j + 1), j = l, l + 64,
// ... in ascending order -- an odd n_time's last stamp after them, on lane (n_time / 2) % 64 --, every term of S2 is
// fma(w * d, d, acc) with the product rounded on its own, every term of a further sum fma(column, d, acc_k) in the same
// trip, then one wave_sum's butterfly per sum.  A row whose address is a multiple of 16 reads each pair with one 16-byte
// load, any other row (odd n_time: every second one; a grid view offset by one double) with two 8-byte loads: the same
// values into the same arithmetic, so the same bits.  Neither the launch geometry nor a row's position in the grid
// enters its result.
constexpr int kChi2wStageMax = 2048;                // stamps whose flux and inv_var are staged in LDS: 32 KB a block
constexpr int kChi2bMaxTerms = 4;

constexpr int chi2b_stage_max(int k) { return ((2 * kChi2wStageMax) / (2 + k)) & ~1; }     // 1364, 1024, 818, 682
static_assert(chi2b_stage_max(0) == kChi2wStageMax, "no columns: the two staged vectors alone");

struct Chi2bM {
    double m[kChi2bMaxTerms * (kChi2bMaxTerms + 1) / 2];       // M_ij, i <= j, at chi2b_at<K>(i, j)
};

template <int K>
__device__ __forceinline__ constexpr int chi2b_at(int i, int j)
{
    return i <= j ? i * K - i * (i - 1) / 2 + (j - i) : j * K - j * (j - 1) / 2 + (i - j);
}

// S2 and the N further sums of one row
// (x[]: indexed by unrolled loops over the template argument only, so it lives in registers)
template <int N>
struct Chi2Sums {
    double s2 = 0.0;
    double x[N] = {};
};
template <>
struct Chi2Sums<0> {
    double s2 = 0.0;
};

__device__ __forceinline__ void chi2w_store(double tot, long r, const double* __restrict__ secdepth, double sec_limit,
                                            int accumulate, double* __restrict__ out)
{
    double h = 0.5 * tot;
    if (secdepth && secdepth[r] >= sec_limit) h = INFINITY;        // (false for a NaN depth, as in numpy)
    out[r] = accumulate ? out[r] + h : h;                           // (+inf stays +inf: h is never -inf)
}

// The policies.  kSums: the further sums; kCols: the columns of their own that they run over, staged behind flux and
// inv_var (none: the one sum runs over the weights, which the row's trip already holds).
struct Chi2Plain {
    static constexpr int kSums = 0, kCols = 0;
    __device__ const double* columns() const { return nullptr; }
    __device__ __forceinline__ void store(const Chi2Sums<0>& s, long r, const double* __restrict__ secdepth,
                                          double sec_limit, int accumulate, double* __restrict__ out) const
    {
        chi2w_store(s.s2, r, secdepth, sec_limit, accumulate, out);
    }
};

struct Chi2Offset {
    static constexpr int kSums = 1, kCols = 0;
    double sum_w, prior_prec;
    double* offset_out;
    __device__ const double* columns() const { return nullptr; }
    __device__ __forceinline__ void store(const Chi2Sums<1>& s, long r, const double* __restrict__ secdepth,
                                          double sec_limit, int accumulate, double* __restrict__ out) const
    {
        const double den = sum_w + prior_prec;          // (the same for every row: one addition a thread)
        const double s1 = s.x[0];
        const double tot = s.s2 - s1 * s1 / den;
        chi2w_store(tot < 0.0 ? 0.0 : tot, r, secdepth, sec_limit, accumulate, out);      // (0.5 * tot: the clamp commutes)
        if (offset_out) offset_out[r] = s1 / den;
    }
};

template <int K>
struct Chi2Baseline {
    static constexpr int kSums = K, kCols = K;
    const double* wbasis;
    Chi2bM M;
    double* coef_out;
    __device__ const double* columns() const { return wbasis; }
    __device__ __forceinline__ void store(const Chi2Sums<K>& s, long r, const double* __restrict__ secdepth,
                                          double sec_limit, int accumulate, double* __restrict__ out) const
    {
        // c_i = sum_j M_ij b_j, then q = sum_i b_i c_i: the quadratic form and the coefficients from the same products
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double c = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) c = fma(M.m[chi2b_at<K>(i, j)], s.x[j], c);
            q = fma(s.x[i], c, q);
            if (coef_out) coef_out[r * K + i] = c;
        }
        const double tot = s.s2 - q;
        chi2w_store(tot < 0.0 ? 0.0 : tot, r, secdepth, sec_limit, accumulate, out);      // (a NaN stays a NaN)
    }
};

// one lane's share of a row's sums; g: the policy's columns, g_stride apart (unused without)
template <bool STAGE, class Terms>
__device__ __forceinline__ Chi2Sums<Terms::kSums> chi2_row_partial(const double* __restrict__ row, const double* f,
                                                                   const double* w, const double* g, int g_stride,
                                                                   int n_time, int lane)
{
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    const int nv = n_time >> 1;
    const bool vec = ((uintptr_t)row & 15) == 0;      // (per row: wave-uniform)
    Chi2Sums<Terms::kSums> s;
    for (int j = lane; j < nv; j += 64) {
        double m0, m1, f0, f1, w0, w1;
        if (vec) {
            const dvec2 m = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(row) + j);
            m0 = m.x; m1 = m.y;
        } else {
            m0 = __builtin_nontemporal_load(row + 2 * j);
            m1 = __builtin_nontemporal_load(row + 2 * j + 1);
        }
        if (STAGE) {
            // (the staged copies are 16-byte aligned whatever the caller's pointers are)
            const dvec2 fv = reinterpret_cast<const dvec2*>(f)[j], wv = reinterpret_cast<const dvec2*>(w)[j];
            f0 = fv.x; f1 = fv.y; w0 = wv.x; w1 = wv.y;
        } else {
            f0 = f[2 * j]; f1 = f[2 * j + 1]; w0 = w[2 * j]; w1 = w[2 * j + 1];
        }
        const double d0 = f0 - m0, d1 = f1 - m1;
        s.s2 = fma(w0 * d0, d0, s.s2);
        s.s2 = fma(w1 * d1, d1, s.s2);
        if constexpr (Terms::kSums > 0) {
#pragma unroll
            for (int k = 0; k < Terms::kSums; ++k) {
                double g0 = w0, g1 = w1;
                if constexpr (Terms::kCols > 0) {
                    const double* gk = g + (size_t)k * g_stride;
                    if (STAGE) {
                        const dvec2 gv = reinterpret_cast<const dvec2*>(gk)[j];
                        g0 = gv.x; g1 = gv.y;
                    } else {
                        g0 = gk[2 * j]; g1 = gk[2 * j + 1];
                    }
                }
                s.x[k] = fma(g0, d0, s.x[k]);
                s.x[k] = fma(g1, d1, s.x[k]);
            }
        }
    }
    if ((n_time & 1) && lane == (nv & 63)) {
        const int t = n_time - 1;
        const double d = f[t] - __builtin_nontemporal_load(row + t);
        const double wt = w[t];
        s.s2 = fma(wt * d, d, s.s2);
        if constexpr (Terms::kSums > 0) {
#pragma unroll
            for (int k = 0; k < Terms::kSums; ++k) {
                double gt = wt;
                if constexpr (Terms::kCols > 0) gt = g[(size_t)k * g_stride + t];
                s.x[k] = fma(gt, d, s.x[k]);
            }
        }
    }
    return s;
}

template <int N>
__device__ __forceinline__ void chi2_wave_sums(Chi2Sums<N>& s)
{
    s.s2 = wave_sum(s.s2);
    if constexpr (N > 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s.x[k] = wave_sum(s.x[k]);
    }
}

template <bool STAGE, class Terms>
__global__ __launch_bounds__(256) void chi2_rows_kernel(const double* __restrict__ flux,
                                                        const double* __restrict__ inv_var,
                                                        const double* __restrict__ grid, int n_time, long n,
                                                        const double* __restrict__ secdepth, double sec_limit,
                                                        int accumulate, double* __restrict__ out, const Terms terms)
{
    // STAGE: [2 + Terms::kCols][n_time rounded up to even]
    extern __shared__ __attribute__((aligned(16))) double chi2_lds[];
    const double* f = flux;
    const double* w = inv_var;
    const double* g = terms.columns();
    int g_stride = n_time;
    if (STAGE) {
        const int n_pad = (n_time + 1) & ~1;
        for (int t = threadIdx.x; t < n_time; t += 256) {
            chi2_lds[t] = flux[t];
            chi2_lds[n_pad + t] = inv_var[t];
            if constexpr (Terms::kCols > 0) {
#pragma unroll
                for (int k = 0; k < Terms::kCols; ++k) chi2_lds[(2 + k) * n_pad + t] = g[(size_t)k * n_time + t];
            }
        }
        __syncthreads();
        f = chi2_lds;
        w = chi2_lds + n_pad;
        g = chi2_lds + 2 * n_pad;
        g_stride = n_pad;
    }
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long nwaves = (long)gridDim.x * 4;
    for (long r = wave0; r < n; r += 2 * nwaves) {
        // two rows per trip, their loads in flight together; each row's arithmetic is its own
        const long r2 = r + nwaves;
        const bool two = r2 < n;
        Chi2Sums<Terms::kSums> s0 = chi2_row_partial<STAGE, Terms>(grid + (size_t)r * n_time, f, w, g, g_stride, n_time, lane);
        Chi2Sums<Terms::kSums> s1;
        if (two) s1 = chi2_row_partial<STAGE, Terms>(grid + (size_t)r2 * n_time, f, w, g, g_stride, n_time, lane);
        chi2_wave_sums(s0);
        chi2_wave_sums(s1);
        if (lane == 0) {
            terms.store(s0, r, secdepth, sec_limit, accumulate, out);
            if (two) terms.store(s1, r2, secdepth, sec_limit, accumulate, out);
        }
    }
}

// ---------------------------------------------------------------------------------------
// log-mean-exp.  Partial state per thread: running max m (finite or -inf), s = sum exp(x - m),
// pinf = saw +inf.  NaN and -inf carry zero weight (_numerics.py:48).
// (struct Lme, lme_merge: trx_device.hpp)

// x_i = c0 - h_i + lnprior_i (fused lnZ tail) when h != null, else x_i = logw_i
__device__ __forceinline__ double lme_value(const double* logw, const double* h,
                                            const double* lnprior, double c0, long i)
{
    if (!h) return logw[i];  // plain log-weights
    double x = c0 - h[i];
    if (lnprior) x += lnprior[i];
    return x;
}

// fold four values into the running (max, sum) state: one rescale, exps only for terms that can
// reach the sum: s >= 1 always (the max contributes exp(0)), so a term with d = x - max < -80
// is < 1.8e-35 and even 2^60 of them stay below fp64 resolution of s (also covers -inf).
// s2 takes the squares of the same terms (e * e of the exp already computed; the rescale squared)
__device__ __forceinline__ void lme_fold4(Lme& st, double x0, double x1, double x2, double x3)
{
    double x[4] = {x0, x1, x2, x3};
    double cm = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        double v = x[u];
        if (v == INFINITY) { st.pinf = 1; v = -INFINITY; }
        if (!(v == v)) v = -INFINITY;
        x[u] = v;
        cm = fmax(cm, v);
    }
    if (cm == -INFINITY) return;
    if (cm > st.m) {
        const double d = st.m - cm;
        const double e = exp(d);
        st.s = (d > -80.0) ? st.s * e : 0.0;
        st.s2 = (d > -80.0) ? st.s2 * (e * e) : 0.0;
        st.m = cm;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const double d = x[u] - st.m;
        if (d > -80.0) {
            const double e = exp(d);
            st.s += e;
            st.s2 = fma(e, e, st.s2);
        }
    }
}

// Loads per lane per trip (16 B each) and whether the next trip's loads are issued before the
// current trip is folded (profiles/r02/lme_variants.txt)
#ifndef TRX_LME_LOADS
#define TRX_LME_LOADS 2
#endif
#ifndef TRX_LME_PREFETCH
#define TRX_LME_PREFETCH 0
#endif
// slots of the per-thread queue of terms that can still count
#ifndef TRX_LME_QUEUE
#define TRX_LME_QUEUE 8
#endif


// SCEN (trx_scenario_evidence): the element count comes from the device (n_dev; the grid was sized for
// its upper bound and the blocks beyond lme_blocks(n) leave at once), lnprior is indexed by the draw
// (src_idx: the masked draws are not gathered), and the pass also finds the first minimum of h
// (argmin partials in buffers of their own next to the kLmePart * 2048 partials of the sums).
constexpr int kLmeMaxBlocks = 2048;
// same value for the search of the smallest chi^2 (NaN equals NaN there: torch.argmin's order)
__device__ __forceinline__ bool argmin_same(double a, double b) { return a == b || (a != a && b != b); }

// merge of two (value, first position, number of rows holding that value) states of the search
__device__ __forceinline__ void argmin_merge(double& v, long& i, long& c, double ov, long oi, long oc)
{
    if (oi < 0) return;
    if (i < 0) { v = ov; i = oi; c = oc; return; }
    if (argmin_same(v, ov)) { c += oc; i = oi < i ? oi : i; return; }
    if (argmin_before(ov, oi, v, i)) { v = ov; i = oi; c = oc; }
}

template <bool SCEN>
__device__ __forceinline__ void lme_partial_body(const double* __restrict__ logw,
                                                 const double* __restrict__ h,
                                                 const double* __restrict__ lnprior,
                                                 double c0, long n, int vec_ok,
                                                 double* __restrict__ ws,
                                                 const long* __restrict__ n_dev,
                                                 const int* __restrict__ src_idx,
                                                 double* __restrict__ amin_pv, long* __restrict__ amin_pi,
                                                 const double* __restrict__ bounds_base, const ScenFinal& fin)
{
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    Lme st{-INFINITY, 0.0, 0, 0.0};
    unsigned nblocks = gridDim.x;
    // SCEN after a bounded evaluation (cells_kernel<PRUNE>): the launch header holds the largest log-weight M
    // of the call, and every term below M - 90 is taken as -inf.  Such a term carries no weight either way;
    // but WHICH rows were abandoned (and report a bound instead of their value) depends on timing, and a term
    // that is large against a thread's running maximum steers the fold below (queues, the census): filtered,
    // the fold sees the same numbers every run -- the rows within 90 of M are never abandoned.
    double floor_x = -INFINITY;
    if (SCEN) {
        n = *n_dev;
        nblocks = (unsigned)lme_blocks(n);
        if (blockIdx.x >= nblocks) return;
        if (bounds_base) floor_x = bounds_base[n * kRowDoubles + kHdrXmax] - 90.0;
    }
    double amin_v = INFINITY;          // SCEN: this thread's first minimum of h ...
    long amin_i = -1, amin_c = 0;      // ... and the number of its rows that hold that value
    bool unwritten = false;            // SCEN: a row still carries rowc_kernel's "never written" mark
    long stride = (long)nblocks * blockDim.x;
    long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec_ok) {
        // 16 B per lane per load, TRX_LME_LOADS independent loads per trip (issuing the next
        // trip's loads before the fold, TRX_LME_PREFETCH, measured slower: profiles/r02/lme_variants.txt).
        // The fold itself leans on IEEE max: fmax ignores a NaN operand, so NaN never reaches the
        // running maximum, `x - max > -80` is false for NaN and for -inf, and a +inf drives the
        // maximum to +inf (detected once, after the loop) -- no per-value inf / NaN tests.
        // Terms within 80 of the running maximum are rare once the maximum has settled (a few
        // per cent of a broad log-likelihood distribution) but with 64 lanes x 4-8 values per trip
        // some lane nearly always holds one, and the whole wave would run exp several times per
        // trip.  So a term that can still count is parked in a per-thread queue in LDS and the
        // exps run over the queues only when one of them fills.  The parked values are raw, so a
        // later, larger maximum needs no bookkeeping.
        constexpr int kL = TRX_LME_LOADS, kV = 2 * kL;
        // Every block streams ONE contiguous segment of the vector (a multiple of 4 KB), its waves 1 KB
        // apart: 6.35 TB/s on the 3.2 GB stress vector against 5.75 with the usual grid-stride loop,
        // where a block's consecutive loads are gridDim x 4 KB apart (profiles/r02/lme_variants.txt).
        const long nv_all = n >> 1;
        const long seg = ((nv_all + nblocks - 1) / nblocks + 255) & ~255L;
        const long seg0 = (long)blockIdx.x * seg;
        const long nv = (seg0 + seg < nv_all) ? (seg0 + seg) : nv_all;
        stride = blockDim.x;
        tid = seg0 + threadIdx.x;
        const dvec2* src = reinterpret_cast<const dvec2*>(h ? h : logw);
        const dvec2* pri = reinterpret_cast<const dvec2*>(lnprior);
        constexpr int kQ = (kV > 4 && TRX_LME_QUEUE < 12) ? 12 : TRX_LME_QUEUE;
        __shared__ double qbuf[kQ][256];
        int qc = 0;
        auto flush = [&]() {
            for (int i = 0; i < kQ; ++i) {
                if (i < qc) {
                    const double d = qbuf[i][threadIdx.x] - st.m;
                    if (d > -80.0) {
                        const double e = exp(d);
                        st.s += e;
                        st.s2 = fma(e, e, st.s2);
                    }
                }
            }
            qc = 0;
        };
        // unconditional loads at clamped indices (a predicated load forces vmcnt(0) at the join);
        // slots past the end are masked to -inf when the trip is folded
        auto fetch = [&](long v0, dvec2* a, dvec2* p) {
#pragma unroll
            for (int u = 0; u < kL; ++u) {
                long j = v0 + u * stride;
                j = (j < nv) ? j : (nv - 1);
                a[u] = __builtin_nontemporal_load(&src[j]);
                if (SCEN) {
                    if (lnprior) {
                        // the prior of rows 2 j, 2 j + 1: dense (one 16-byte read; the twin branch's run is stored from
                        // the top down), or by draw index through the list
                        if (fin.dense) {
                            if (fin.branch) { p[u].x = lnprior[fin.N - 1 - 2 * j]; p[u].y = lnprior[fin.N - 2 - 2 * j]; }
                            else { p[u].x = lnprior[2 * j]; p[u].y = lnprior[2 * j + 1]; }
                        } else {
                            p[u].x = lnprior[src_idx[2 * j]];
                            p[u].y = lnprior[src_idx[2 * j + 1]];
                        }
                    }
                } else if (pri) p[u] = __builtin_nontemporal_load(&pri[j]);
            }
        };
        dvec2 cur[kL], curp[kL], nxt[kL], nxtp[kL];
        if (tid < nv) fetch(tid, cur, curp);
        for (long v = tid; v < nv; v += kL * stride) {
            const long vn = v + kL * stride;
            if (TRX_LME_PREFETCH && vn < nv) fetch(vn, nxt, nxtp);
            double x[kV];
#pragma unroll
            for (int u = 0; u < kL; ++u) {
                dvec2 a = cur[u];
                const bool ok = v + u * stride < nv;
                if (SCEN && ok) {
                    // (a thread meets its elements in ascending order: a later one wins only when strictly before)
                    const long e = 2 * (v + u * stride);
                    if (amin_i < 0 || argmin_before(a.x, e, amin_v, amin_i)) { amin_v = a.x; amin_i = e; amin_c = 1; }
                    else if (argmin_same(a.x, amin_v)) ++amin_c;
                    if (argmin_before(a.y, e + 1, amin_v, amin_i)) { amin_v = a.y; amin_i = e + 1; amin_c = 1; }
                    else if (argmin_same(a.y, amin_v)) ++amin_c;
                    unwritten = unwritten || (unsigned long long)__double_as_longlong(a.x) == kUnwrittenBits ||
                                (unsigned long long)__double_as_longlong(a.y) == kUnwrittenBits;
                }
                if (h) {
                    a = c0 - a;
                    if (pri) a += curp[u];
                }
                if (SCEN) {
                    a.x = (a.x < floor_x) ? -INFINITY : a.x;
                    a.y = (a.y < floor_x) ? -INFINITY : a.y;
                }
                x[2 * u] = ok ? a.x : -INFINITY;
                x[2 * u + 1] = ok ? a.y : -INFINITY;
            }
            double cm = x[0];
#pragma unroll
            for (int u = 1; u < kV; ++u) cm = fmax(cm, x[u]);
            if (cm > st.m) {
                const double d = st.m - cm;
                const double e = exp(d);
                st.s = (d > -80.0) ? st.s * e : 0.0;
                st.s2 = (d > -80.0) ? st.s2 * (e * e) : 0.0;
                st.m = cm;
            }
            bool live[kV];
            int crowd = 0;
#pragma unroll
            for (int u = 0; u < kV; ++u) {
                live[u] = x[u] - st.m > -80.0;
#ifndef TRX_LME_NOCROWD
                crowd += __popcll(__ballot(live[u]));
#endif
            }
            if (crowd > 24 * kV) {
                // a narrow distribution: most terms count, nothing to gain from parking them
#pragma unroll
                for (int u = 0; u < kV; ++u)
                    if (live[u]) {
                        const double e = exp(x[u] - st.m);
                        st.s += e;
                        st.s2 = fma(e, e, st.s2);
                    }
            } else {
                if (__any(qc > kQ - kV)) flush();
#pragma unroll
                for (int u = 0; u < kV; ++u) {
                    if (live[u]) {
                        qbuf[qc][threadIdx.x] = x[u];
                        ++qc;
                    }
                }
            }
            if (TRX_LME_PREFETCH) {
#pragma unroll
                for (int u = 0; u < kL; ++u) { cur[u] = nxt[u]; curp[u] = nxtp[u]; }
            } else if (vn < nv) {
                fetch(vn, cur, curp);
            }
        }
        flush();
        if (st.m == INFINITY) { st.pinf = 1; st.m = -INFINITY; st.s = 0.0; st.s2 = 0.0; }
        if ((n & 1) && tid == 0) {
            if (SCEN) {
                const double hv = h[n - 1];
                argmin_merge(amin_v, amin_i, amin_c, hv, n - 1, 1);
                unwritten = unwritten || (unsigned long long)__double_as_longlong(hv) == kUnwrittenBits;
                double x = c0 - hv;
                if (lnprior) x += lnprior[fin.dense ? (fin.branch ? fin.N - n : n - 1) : (long)src_idx[n - 1]];
                if (x < floor_x) x = -INFINITY;
                lme_fold4(st, x, -INFINITY, -INFINITY, -INFINITY);
            } else {
                lme_fold4(st, lme_value(logw, h, lnprior, c0, n - 1), -INFINITY, -INFINITY, -INFINITY);
            }
        }
    } else {
        for (long i0 = tid * 4; i0 < n; i0 += stride * 4) {
            double x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                x[u] = (i0 + u < n) ? lme_value(logw, h, lnprior, c0, i0 + u) : -INFINITY;
            lme_fold4(st, x[0], x[1], x[2], x[3]);
        }
    }
    if (SCEN && unwritten) st.pinf |= 2;           // (bit 1 of the flag word travels with the partials: lme_merge ORs it)
    // wave combine (fixed butterfly order => deterministic)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lme_merge(st, lme_shfl_xor(st, o));
    __shared__ double sm[4], ss[4], ss2[4];
    __shared__ int sp[4];
    __shared__ double av[4];
    __shared__ long ai[4], ac[4];
    const int wave = threadIdx.x >> 6;
    if (SCEN) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(amin_v, o, 64);
            const long oi = __shfl_xor(amin_i, o, 64);
            const long oc = __shfl_xor(amin_c, o, 64);
            argmin_merge(amin_v, amin_i, amin_c, ov, oi, oc);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        sm[wave] = st.m; ss[wave] = st.s; sp[wave] = st.pinf; ss2[wave] = st.s2;
        if (SCEN) { av[wave] = amin_v; ai[wave] = amin_i; ac[wave] = amin_c; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Lme t{sm[0], ss[0], sp[0], ss2[0]};
        for (int w = 1; w < 4; ++w) { Lme o{sm[w], ss[w], sp[w], ss2[w]}; lme_merge(t, o); }
        ws[kLmePart * blockIdx.x + 0] = t.m;
        ws[kLmePart * blockIdx.x + 1] = t.s;
        ws[kLmePart * blockIdx.x + 2] = (double)t.pinf;
        ws[kLmePart * blockIdx.x + 3] = t.s2;
        if (SCEN) {
            double bv = av[0];
            long bi = ai[0], bc = ac[0];
            for (int w = 1; w < 4; ++w) argmin_merge(bv, bi, bc, av[w], ai[w], ac[w]);
            amin_pv[blockIdx.x] = bv;
            amin_pi[blockIdx.x] = bi;
            amin_pi[kLmeMaxBlocks + blockIdx.x] = bc;        // (the counts ride behind the positions)
        }
    }
    if (SCEN && fin.state) {
        // the block that finishes last turns the partials into the branch's record (scenario_final): what was a
        // launch of its own (final_kernel) until round 3
        __shared__ int is_last;
        if (threadIdx.x == 0) {
            __threadfence();                                   // this block's partials before its ticket
            const unsigned ticket = atomicAdd(&fin.state[0], 1u);
            is_last = ticket == nblocks - 1;
        }
        __syncthreads();
        if (is_last && threadIdx.x < 64) {
            __threadfence();                                   // the other blocks' partials after their tickets
            scenario_final(fin, ws, amin_pv, amin_pi, amin_pi + kLmeMaxBlocks, n, (int)threadIdx.x);
        }
    }
}

template <bool SCEN>
__global__ __launch_bounds__(256) void lme_partial_kernel(const double* __restrict__ logw,
                                                          const double* __restrict__ h,
                                                          const double* __restrict__ lnprior,
                                                          double c0, long n, int vec_ok,
                                                          double* __restrict__ ws,
                                                          const long* __restrict__ n_dev,
                                                          const int* __restrict__ src_idx,
                                                          double* __restrict__ amin_pv, long* __restrict__ amin_pi,
                                                          const double* __restrict__ bounds_base, const ScenFinal fin)
{
    lme_partial_body<SCEN>(logw, h, lnprior, c0, n, vec_ok, ws, n_dev, src_idx, amin_pv, amin_pi, bounds_base, fin);
}

// chain: the reductions of all branches in one launch, branch = blockIdx.y
struct LmeBranch {
    const double* h;
    const double* lnprior;
    double c0;
    double* ws;
    const long* n_dev;
    double* amin_pv;
    long* amin_pi;
    const double* bounds_base;
    ScenFinal fin;             // (fin.idx is the branch's src_idx)
};
struct LmeTab {
    LmeBranch b[kChainMaxBranches];
};
static_assert(sizeof(LmeTab) + 16 <= 4096, "kernel argument buffer");

__global__ __launch_bounds__(256) void lme_partial_kernel_star(LmeTab tab, long n_upper)
{
    const LmeBranch& b = tab.b[blockIdx.y];
    lme_partial_body<true>(nullptr, b.h, b.lnprior, b.c0, n_upper, 1, b.ws, b.n_dev, b.fin.idx, b.amin_pv, b.amin_pi,
                           b.bounds_base, b.fin);
}

// moments != 0: out[1] = lnM2, out[2] = lnWmax as well (trx_lnz_moments_from_halfchi2)
__global__ __launch_bounds__(64) void lme_final_kernel(const double* __restrict__ ws, int nparts,
                                                       long n_total, double* __restrict__ out, int moments)
{
    // lane l folds partials l, l+64, ... in order, then a fixed butterfly: deterministic
    Lme t{-INFINITY, 0.0, 0, 0.0};
    for (int i = threadIdx.x; i < nparts; i += 64) {
        Lme o{ws[kLmePart * i], ws[kLmePart * i + 1], ws[kLmePart * i + 2] != 0.0, ws[kLmePart * i + 3]};
        lme_merge(t, o);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lme_merge(t, lme_shfl_xor(t, o));
    if (threadIdx.x != 0) return;
    double r;
    if (t.pinf) r = INFINITY;                                   // _numerics.py:46-47
    else if (t.m == -INFINITY) r = -INFINITY;                   // :49-50
    else r = log(t.s) + t.m - log((double)n_total);             // :51
    out[0] = r;
    if (moments) lme_moments(t, n_total, out[1], out[2]);
}

}  // namespace
