// Column quantiles of a row-major grid of model curves (trx_grid_quantiles: include/trx.h): the
// pointwise credible band of the light curves of a scenario's posterior samples.  Included by trx_kernels.hip only.
//
// Input: g[n_grid_rows][n_cols] as trx_flux_grid writes it (one curve per row), an optional gather list rows[n_rows]
// (repeats allowed) and an optional per-gathered-row scale: the value of row r at column c is
//     v = g[rows[r]][c]                          (scale == NULL)
//     v = 1 - scale[r] * (1 - g[rows[r]][c])     (the inverse of funcs.renorm_flux; two roundings, never contracted)
// Output: out[n_q][n_cols], out[.][c] = np.quantile(v[:, c], q) under numpy's default "linear" method:
//     h = (n_rows - 1) q,  lo = floor(h),  hi = min(lo + 1, n_rows - 1),  t = h - lo,  a = v_(lo), b = v_(hi)
//     result = a + (b - a) t   for t < 0.5,    b - (b - a) (1 - t)   for t >= 0.5,    exactly a where a == b
// (numpy's _lerp, every operation rounded on its own), and NaN for every q of a column that holds a NaN.
//
//   band_quantile_kernel   one workgroup of 256 threads per C adjacent columns.  The gathered rows of those columns are
//                          staged in LDS as SORT KEYS (the double's bits, sign-folded so that unsigned integer order is
//                          numeric order; every NaN becomes the one largest key), column-major [C][P] with P = n_rows
//                          rounded up to a power of two and the tail padded with +inf.  C = min(8, 8192 / P): the
//                          image is at most 64 KiB (2 columns at 4096 rows, 8 at 1000 and below), and a row's read is
//                          one run of 8 C bytes.  All C columns are sorted side by side by ONE bitonic network over
//                          the C P keys -- a compare-exchange never crosses a column, its direction follows from the
//                          index inside the column -- one barrier per stage, every loop bound uniform over the
//                          workgroup, no wave shuffles.  Then C n_q threads read the two order statistics of their
//                          (column, q) and interpolate.  A column holds a NaN exactly when its last key is the NaN key.
// Order statistics do not depend on how they were found and every thread's arithmetic is a function of its (column, q)
// alone: the result does not depend on the launch geometry and repeats bit for bit.  No scratch, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/trx.h"

namespace trx {
namespace {

constexpr int kBandThreads = 256;
constexpr int kBandMaxKeys = 8192;      // 64 KiB of LDS
constexpr int kBandMaxCols = 8;         // columns per workgroup: a 64-byte run of every gathered row
constexpr int kBandMaxQ = 16;

struct BandArgs {
    const double* g;
    long n_grid_rows;
    int n_cols;
    const long* rows;         // [n_rows] or null: rows 0 .. n_rows - 1
    const double* scale;      // [n_rows] or null
    int n_rows;
    int pad_log2;             // P = 1 << pad_log2 >= n_rows
    int cols_log2;            // C = 1 << cols_log2
    int n_q;
    double* out;              // [n_q][n_cols]
    double q[kBandMaxQ];
};

// columns per workgroup and padded rows of a call
inline void band_geometry(long n_rows, int& pad_log2, int& cols_log2)
{
    pad_log2 = 0;
    while ((1L << pad_log2) < n_rows) ++pad_log2;
    int c = kBandMaxKeys >> pad_log2;
    if (c > kBandMaxCols) c = kBandMaxCols;
    cols_log2 = 0;
    while ((2 << cols_log2) <= c) ++cols_log2;
}

typedef unsigned long long band_key_t;
constexpr band_key_t kBandNaN = ~0ull;
constexpr band_key_t kBandInf = 0xfff0000000000000ull;      // band_key(+inf)

__device__ __forceinline__ band_key_t band_key(double v)
{
    if (v != v) return kBandNaN;
    const band_key_t b = (band_key_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

__device__ __forceinline__ double band_value(band_key_t k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// numpy's _lerp of the order statistics a <= b
__device__ __forceinline__ double band_lerp(double a, double b, double t)
{
#pragma clang fp contract(off)
    const double d = b - a;
    const double up = d * t, down = d * (1.0 - t);
    const double r = (t >= 0.5) ? b - down : a + up;
    return a == b ? a : r;
}

__device__ __forceinline__ double band_rescale(double v, double s)
{
#pragma clang fp contract(off)
    const double depth = 1.0 - v;
    const double scaled = s * depth;
    return 1.0 - scaled;
}

__global__ __launch_bounds__(kBandThreads) void band_quantile_kernel(BandArgs a)
{
    extern __shared__ __attribute__((aligned(16))) band_key_t band_keys[];
    const int tid = (int)threadIdx.x;
    const int P = 1 << a.pad_log2, C = 1 << a.cols_log2, E = C << a.pad_log2;
    const int c0 = (int)blockIdx.x << a.cols_log2;

    // stage: consecutive threads take the C adjacent columns of one gathered row (a column beyond the grid, a padding
    // row and a list entry outside the grid's rows never touch memory)
    for (int i = tid; i < E; i += kBandThreads) {
        const int r = i >> a.cols_log2, cc = i & (C - 1), col = c0 + cc;
        band_key_t k = kBandInf;
        if (r < a.n_rows && col < a.n_cols) {
            const long src = a.rows ? a.rows[r] : (long)r;
            double v = NAN;
            if (src >= 0 && src < a.n_grid_rows) {
                v = a.g[src * (long)a.n_cols + col];
                if (a.scale) v = band_rescale(v, a.scale[r]);
            }
            k = band_key(v);
        }
        band_keys[(cc << a.pad_log2) + r] = k;
    }

    // bitonic network over every column at once: pair p of a stage is (i, i | j) with bit j of i clear; ascending where
    // bit k of the index INSIDE the column is clear (the last merge, k == P, ascends everywhere)
    const int half = E >> 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int p = tid; p < half; p += kBandThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool ascending = ((i & (P - 1)) & k) == 0;
                const band_key_t x = band_keys[i], y = band_keys[l];
                if ((x > y) == ascending) {
                    band_keys[i] = y;
                    band_keys[l] = x;
                }
            }
        }
    }
    __syncthreads();

    if (tid < (a.n_q << a.cols_log2)) {
        const int cc = tid / a.n_q, iq = tid - cc * a.n_q, col = c0 + cc;
        if (col < a.n_cols) {
            const band_key_t* s = band_keys + (cc << a.pad_log2);
            double res = NAN;
            if (s[P - 1] != kBandNaN) {
                double h, t;
                {
#pragma clang fp contract(off)
                    h = (double)(a.n_rows - 1) * a.q[iq];
                    const double f = floor(h);
                    t = h - f;
                    h = f;
                }
                int lo = (int)h;
                if (lo > a.n_rows - 1) lo = a.n_rows - 1;
                const int hi = lo + 1 < a.n_rows ? lo + 1 : a.n_rows - 1;
                res = band_lerp(band_value(s[lo]), band_value(s[hi]), t);
            }
            a.out[(long)iq * a.n_cols + col] = res;
        }
    }
}

hipError_t band_launch(BandArgs& a, hipStream_t st)
{
    band_geometry(a.n_rows, a.pad_log2, a.cols_log2);
    const int C = 1 << a.cols_log2;
    const unsigned blocks = (unsigned)((a.n_cols + C - 1) / C);
    const size_t lds = sizeof(band_key_t) * ((size_t)C << a.pad_log2);
    hipLaunchKernelGGL(band_quantile_kernel, dim3(blocks), dim3(kBandThreads), lds, st, a);
    return hipGetLastError();
}

}  // namespace
}  // namespace trx
