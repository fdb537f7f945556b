// Posterior samples of one scenario branch: systematic resampling of its weighted draws on the device
// (trx_scenario_args.post_rows, trx_posterior_from_halfchi2: include/trx.h).  Included by
// trx_scenario.hip only.
//
// The n masked draws of a branch, in list order, carry the evidence's own log-weights
//     x_i = -ln(sigma) - 0.5 ln(2 pi) - h_i (+ lnprior_i),      w_i = exp(x_i - X) where x_i - X > -80, else 0
// (X = the largest x_i; NaN and -inf: 0 -- the rule of lme_fold4, trx_reduce.hpp).  M samples: one uniform u,
// targets t_j = (u + j) / M * S with S = sum w_i, sample j = the first list position r with C_r = w_0 + ... + w_r > t_j.
//
// A floating-point running sum is neither associative nor -- scanned in parallel -- monotonic to the last bit, and a
// selection by binary search needs both: the per-tile sums of one pass must equal the totals of the in-tile scans of
// the next, or a target falls between two tiles, and a prefix that steps back by one ulp can hand a target to a row of
// weight zero.  So the sums are taken in FIXED POINT: q_i = w_i * 2^96 truncated to an unsigned 128-bit integer (at least
// 1 where w_i > 0, so that every row that carries weight can be drawn).  w_i <= 1 and n < 2^31 keep every sum below
// 2^127; a weight keeps its full 53-bit mantissa down to 2^-43 and is cut at an ABSOLUTE 2^-96 below that: the sum is off
// by less than n 2^-96 S, far inside the n 2^-53 S of any fp64 summation.  Integer sums are exact, so every partition,
// scan order and tree gives the same bits, the cumulative sums are monotonic by construction and the results repeat bit
// for bit -- no floating-point atomics, no order to fix.
//
//   post_sum_kernel     one workgroup per tile (chunks of 2048 rows; the chunks per tile follow from the launch bound): sum of q and the number
//                       of rows with w > 0.  X comes from the call's scratch: the evidence's final stage left it there
//                       (scenario_final, ScenFinal.post_x) -- or, for trx_posterior_from_halfchi2, post_max_kernel /
//                       post_x_kernel found it (there is no evidence pass to take it from)
//   post_select_kernel  one workgroup per tile: the exclusive prefix of the tile sums and their total (at most 2048
//                       values), the targets that fall into this tile, then per chunk of 2048 rows the inclusive scan
//                       (8 consecutive rows per thread, wave scan by shuffles, cross-wave fix-up through LDS) kept in LDS
//                       in a [8][256] layout -- consecutive lanes touch consecutive 8-byte words, no bank conflicts --,
//                       a binary search over the 256 thread totals and a step through that thread's 8 rows for every
//                       target, and the gather of the chosen draw's columns from the dense column block into the
//                       caller's block.  Tile 0 writes the header (and the NaN rows of a branch without weight).
//   post_sum_chain_kernel, post_select_chain_kernel
//                       the same two for every branch of a launch chain that wants samples (trx_star_enqueue,
//                       enqueue_chain): the branch is the grid's second dimension and picks its PostArgs from a table in
//                       the chain's arena.  The bodies are the single-call kernels' (post_sum_body, post_select_body), so
//                       a block from a chain is the block of the call on its own, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/trx.h"
#include "trx_device.hpp"

namespace trx {
namespace {

typedef unsigned __int128 u128;
typedef unsigned long long u64;

constexpr int kPostChunk = 2048;        // rows scanned at a time: 256 threads x 8 consecutive rows
constexpr int kPostMaxTiles = 2048;     // tiles of a branch (a tile is as many chunks as that takes)
constexpr int kPostFrac = 96;           // fixed point: q = w * 2^96
constexpr unsigned kPostSlot = 0x504f5354u;      // Philox counter word 2 of the resampler's uniform: no draw slot (0 .. 18)
// scratch of one branch: [tiles] u128 sums | [tiles] doubles (tile maxima, then the counts of rows with w > 0) | X
constexpr size_t kPostWsSums = sizeof(u128) * kPostMaxTiles, kPostWsCounts = sizeof(double) * kPostMaxTiles;
constexpr size_t kPostWsBytes = kPostWsSums + kPostWsCounts + 256;

struct PostArgs {
    const double* h;          // chi^2/2 of the masked draws, list order
    const double* lnprior;    // null, or per row: position r (twin: N - 1 - r)
    const long* n_dev;        // the number of rows on the device, or null: n
    long n;                   // (n_dev: its upper bound, which sized the grid)
    long N;                   // stride of `cols`, and the twin branch's mirror
    int twin;
    double c0;                // -0.5 ln(2 pi) - ln(sigma)
    int M;
    int branch;
    u64 seed;
    double* xmax;             // [1] X
    u128* tile_q;
    long* tile_cnt;
    double* tile_max;         // (aliases tile_cnt: read by post_x_kernel before post_sum_kernel writes the counts)
    const double* cols;       // [ncol][N] dense column block, or null
    int ncol;
    double* block;            // TRX_POST_BRANCH(M) doubles, or null
    long* out_pos;            // [M] or null
    double* out_hdr;          // [4] or null
};

// Tiles of a vector of n rows, and chunks per tile.  The chunks per tile follow from the bound the launch was sized for
// (n_upper: the number of draws; the number of masked draws is known on the device only), the tiles in use from n itself.
// (The integer sums make the result independent of the partition; it only has to cover the rows.)
__host__ __device__ inline void post_geometry(long n, long n_upper, int& tiles, int& per_tile)
{
    long chunks_upper = (n_upper + kPostChunk - 1) / kPostChunk, chunks = (n + kPostChunk - 1) / kPostChunk;
    if (chunks_upper < 1) chunks_upper = 1;
    if (chunks < 1) chunks = 1;
    per_tile = (int)((chunks_upper + kPostMaxTiles - 1) / kPostMaxTiles);
    tiles = (int)((chunks + per_tile - 1) / per_tile);
}

__device__ __forceinline__ double post_x(const PostArgs& a, long r)
{
    double x = a.c0 - a.h[r];                                // (lme_partial_body's expression: the same bits)
    if (a.lnprior) x += a.lnprior[a.twin ? a.N - 1 - r : r];
    return x;
}

// d = m 2^(e - 52) >= 0 -> floor(d 2^shift) as an integer (d 2^shift < 2^128)
__device__ __forceinline__ u128 post_fixed(double d, int shift)
{
    const u64 b = (u64)__double_as_longlong(d);
    const int be = (int)(b >> 52) & 0x7ff;
    if (be == 0) return 0;                                   // zero (and denormals: below every weight and target)
    const u64 m = (b & ((1ull << 52) - 1)) | (1ull << 52);
    const int sh = be - 1023 - 52 + shift;
    if (sh >= 0) return (u128)m << sh;
    return sh > -64 ? (u128)(m >> -sh) : (u128)0;
}

// one place for the weight of a row, so that every pass forms the same bits
__device__ __noinline__ u128 post_weight(double x, double X)
{
    const double d = x - X;
    if (!(d > -80.0)) return 0;                              // the evidence's cut; NaN, -inf
    const double w = fmin(exp(d), 1.0);
    const u128 q = post_fixed(w, kPostFrac);
    return q ? q : (u128)1;
}

__device__ __forceinline__ double post_to_double(u128 q)
{
    return (double)(u64)(q >> 64) * 18446744073709551616.0 + (double)(u64)q;
}

__device__ __forceinline__ u128 post_shfl_xor(u128 v, int o)
{
    const u64 lo = __shfl_xor((u64)v, o, 64), hi = __shfl_xor((u64)(v >> 64), o, 64);
    return ((u128)hi << 64) | lo;
}

__device__ __forceinline__ u128 post_shfl_up(u128 v, int o)
{
    const u64 lo = __shfl_up((u64)v, o, 64), hi = __shfl_up((u64)(v >> 64), o, 64);
    return ((u128)hi << 64) | lo;
}

// sum over the 256 threads of a workgroup, on every thread (slot: one of the LDS staging rows)
__device__ __forceinline__ u128 post_block_sum(u128 v, u64 (*stage)[2])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += post_shfl_xor(v, o);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                         // (the staging rows may still be read from the last use)
    if ((threadIdx.x & 63) == 0) { stage[wave][0] = (u64)v; stage[wave][1] = (u64)(v >> 64); }
    __syncthreads();
    u128 t = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) t += ((u128)stage[w][1] << 64) | stage[w][0];
    return t;
}

// the masked count is the same on every lane: kept in scalar registers (the compiler cannot know that the earlier
// kernels' store is done, so it loads per lane, and the tile geometry that follows from it would sit in VGPRs)
__device__ __forceinline__ long post_rows_of(const PostArgs& a)
{
    const long n = a.n_dev ? *a.n_dev : a.n;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)n);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)n >> 32));
    return (long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ bool post_live(double X) { return X == X && X != INFINITY && X != -INFINITY; }

// target j of M on a total of Q (Qd = Q as a double): floor((u + j) / M * Q), below Q; non-decreasing in j
__device__ __forceinline__ u128 post_target(double u, int j, int M, double Qd, u128 Q)
{
    const u128 t = post_fixed(((u + (double)j) / (double)M) * Qd, 0);
    return t < Q ? t : Q - 1;
}

// Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011), as the draw kernel's: key = seed, counter = (branch, 0, slot, 0);
// 53 bits from the first two words (numpy's construction)
__device__ __forceinline__ double post_uniform(u64 seed, int branch)
{
    unsigned c0 = (unsigned)branch, c1 = 0u, c2 = kPostSlot, c3 = 0u, k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * (1.0 / 9007199254740992.0);
}

// trx_posterior_from_halfchi2 only: the largest log-weight of every tile (NaN ignored; +inf stays)
__global__ __launch_bounds__(256) void post_max_kernel(PostArgs a)
{
    int tiles, per_tile;
    post_geometry(a.n, a.n, tiles, per_tile);
    if ((int)blockIdx.x >= tiles) return;
    const long lo = (long)blockIdx.x * per_tile * kPostChunk;
    long hi = lo + (long)per_tile * kPostChunk;
    if (hi > a.n) hi = a.n;
    double m = -INFINITY;
    for (long r = lo + threadIdx.x; r < hi; r += 256) m = fmax(m, post_x(a, r));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    __shared__ double sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) a.tile_max[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

// ... and of the vector: X, or NaN where a +inf term makes the evidence +inf (no posterior then)
__global__ __launch_bounds__(256) void post_x_kernel(PostArgs a)
{
    int tiles, per_tile;
    post_geometry(a.n, a.n, tiles, per_tile);
    double m = -INFINITY;
    for (int i = threadIdx.x; i < tiles; i += 256) m = fmax(m, a.tile_max[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    __shared__ double sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
        a.xmax[0] = (m == INFINITY) ? NAN : m;
    }
}

__device__ __forceinline__ void post_sum_body(const PostArgs& a, const int tile, u64 (*stage)[2])
{
    const long n = post_rows_of(a);
    int tiles, per_tile;
    post_geometry(n < a.n ? n : a.n, a.n, tiles, per_tile);
    if (tile >= tiles) return;
    const double X = a.xmax[0];
    u128 q = 0, cnt = 0;
    if (post_live(X)) {
        const long lo = (long)tile * per_tile * kPostChunk;
        long hi = lo + (long)per_tile * kPostChunk;
        if (hi > n) hi = n;
        for (long r = lo + threadIdx.x; r < hi; r += 256) {
            const u128 qi = post_weight(post_x(a, r), X);
            q += qi;
            cnt += qi ? 1 : 0;
        }
    }
    q = post_block_sum(q, stage);
    cnt = post_block_sum(cnt, stage);
    if (threadIdx.x == 0) {
        a.tile_q[tile] = q;
        a.tile_cnt[tile] = (long)(u64)cnt;
    }
}

__global__ __launch_bounds__(256) void post_sum_kernel(PostArgs a)
{
    __shared__ u64 stage[4][2];
    post_sum_body(a, (int)blockIdx.x, stage);
}

// the branches of a launch chain that want samples: slot blockIdx.y of `tab` (the grid's first dimension is sized for the
// bound N the chain's calls share; a workgroup beyond its branch's tiles in use leaves at once, as in the single call)
__global__ __launch_bounds__(256) void post_sum_chain_kernel(const PostArgs* __restrict__ tab)
{
    __shared__ u64 stage[4][2];
    const PostArgs a = tab[blockIdx.y];
    post_sum_body(a, (int)blockIdx.x, stage);
}

__device__ __forceinline__ void post_emit(const PostArgs& a, int j, long r)
{
    if (a.out_pos) a.out_pos[j] = r;
    if (!a.block) return;
    const long M = a.M, pos = a.twin ? a.N - 1 - r : r;
    double* rows = a.block + 8;
    for (int c = 0; c < 14; ++c) rows[c * M + j] = (c < a.ncol) ? a.cols[(long)c * a.N + pos] : 0.0;
    rows[14 * M + j] = (double)r;
    rows[15 * M + j] = post_x(a, r);
}

// c_lo / c_hi: inclusive sums of the chunk, [8][256]: row 8 t + k at k * 256 + t
__device__ __forceinline__ void post_select_body(const PostArgs& a, const int tile, u64 (*stage)[2], u64* c_lo, u64* c_hi)
{
    const long n = post_rows_of(a);
    int tiles, per_tile;
    post_geometry(n < a.n ? n : a.n, a.n, tiles, per_tile);
    const int tid = (int)threadIdx.x, M = a.M;
    if (tile >= tiles) return;
    const double X = a.xmax[0];
    // the tiles before this one, all of them, and the rows that carry weight
    u128 before = 0, Q = 0, cnt = 0;
    for (int i = tid; i < tiles; i += 256) {
        const u128 q = a.tile_q[i];
        Q += q;
        if (i < tile) before += q;
        cnt += (u128)(u64)a.tile_cnt[i];
    }
    Q = post_block_sum(Q, stage);
    before = post_block_sum(before, stage);
    cnt = post_block_sum(cnt, stage);
    const double u = post_uniform(a.seed, a.branch);
    const double Qd = post_to_double(Q);
    if (tile == 0) {
        if (tid == 0) {
            double* hdr = a.block ? a.block : a.out_hdr;
            hdr[0] = u;
            hdr[1] = X;
            hdr[2] = Q ? log(Qd) - (double)kPostFrac * 0.693147180559945309417232121458 : -INFINITY;
            hdr[3] = (double)(u64)cnt;
            if (a.block)
                for (int i = 4; i < 8; ++i) hdr[i] = 0.0;
        }
        if (!Q) {                                            // no row carries weight: nothing to draw from
            for (int j = tid; j < M; j += 256) {
                if (a.out_pos) a.out_pos[j] = -1;
                if (a.block)
                    for (int c = 0; c < 16; ++c) a.block[8 + (long)c * M + j] = NAN;
            }
        }
    }
    if (!Q) return;
    const u128 mine = a.tile_q[tile];
    int any = 0;
    for (int j = tid; j < M; j += 256) {
        const u128 t = post_target(u, j, M, Qd, Q);
        any |= (t >= before && t - before < mine) ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;

    u128 base = before;                                      // cumulative sum in front of the chunk
    for (int c = 0; c < per_tile; ++c) {
        const long lo = ((long)tile * per_tile + c) * kPostChunk;
        if (lo >= n) break;
        u128 run[8];
        u128 acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long r = lo + 8 * tid + k;
            if (r < n) acc += post_weight(post_x(a, r), X);
            run[k] = acc;
        }
        // exclusive prefix of the threads' totals: inclusive wave scan, then the waves in front
        u128 inc = acc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u128 up = post_shfl_up(inc, o);
            if ((tid & 63) >= o) inc += up;
        }
        __syncthreads();                                     // (the last chunk's searches are done with c_lo / c_hi / stage)
        if ((tid & 63) == 63) { stage[tid >> 6][0] = (u64)inc; stage[tid >> 6][1] = (u64)(inc >> 64); }
        __syncthreads();
        u128 front = base, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const u128 s = ((u128)stage[w][1] << 64) | stage[w][0];
            if (w < (tid >> 6)) front += s;
            total += s;
        }
        front += inc - acc;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const u128 v = front + run[k];
            c_lo[k * 256 + tid] = (u64)v;
            c_hi[k * 256 + tid] = (u64)(v >> 64);
        }
        __syncthreads();
        for (int j = tid; j < M; j += 256) {
            const u128 t = post_target(u, j, M, Qd, Q);
            if (t < base || t - base >= total) continue;
            // first thread whose last row's sum exceeds the target, then the first such row of its 8
            int a0 = 0, a1 = 255;
            while (a0 < a1) {
                const int mid = (a0 + a1) >> 1;
                const u128 v = ((u128)c_hi[7 * 256 + mid] << 64) | c_lo[7 * 256 + mid];
                if (v > t) a1 = mid; else a0 = mid + 1;
            }
            int k = 0;
            while (k < 7 && !((((u128)c_hi[k * 256 + a0] << 64) | c_lo[k * 256 + a0]) > t)) ++k;
            const long r = lo + 8 * a0 + k;                  // (a row that carries weight: r < n)
            post_emit(a, j, r < n ? r : n - 1);
        }
        base += total;
    }
}

__global__ __launch_bounds__(256) void post_select_kernel(PostArgs a)
{
    __shared__ u64 stage[4][2];
    __shared__ u64 c_lo[kPostChunk], c_hi[kPostChunk];
    post_select_body(a, (int)blockIdx.x, stage, c_lo, c_hi);
}

__global__ __launch_bounds__(256) void post_select_chain_kernel(const PostArgs* __restrict__ tab)
{
    __shared__ u64 stage[4][2];
    __shared__ u64 c_lo[kPostChunk], c_hi[kPostChunk];
    const PostArgs a = tab[blockIdx.y];
    post_select_body(a, (int)blockIdx.x, stage, c_lo, c_hi);
}

// the passes of one branch behind its evidence (X already in a.xmax) -- or, standalone, behind the search for X
int post_launch(const PostArgs& a, bool find_x, hipStream_t st)
{
    int tiles, per_tile;
    post_geometry(a.n, a.n, tiles, per_tile);
    if (find_x) {
        hipLaunchKernelGGL(post_max_kernel, dim3(tiles), dim3(256), 0, st, a);
        hipLaunchKernelGGL(post_x_kernel, dim3(1), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(post_sum_kernel, dim3(tiles), dim3(256), 0, st, a);
    hipLaunchKernelGGL(post_select_kernel, dim3(tiles), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? TRX_OK : TRX_ERR_HIP;
}

// ... and of the `slots` branches of a launch chain that want samples, behind the chain's evidence stage: two launches
// for the whole chain.  dev_tab: their PostArgs in device memory (every one with n = N, the bound the chain's calls share)
int post_launch_chain(const PostArgs* dev_tab, int slots, long N, hipStream_t st)
{
    int tiles, per_tile;
    post_geometry(N, N, tiles, per_tile);
    hipLaunchKernelGGL(post_sum_chain_kernel, dim3(tiles, slots), dim3(256), 0, st, dev_tab);
    hipLaunchKernelGGL(post_select_chain_kernel, dim3(tiles, slots), dim3(256), 0, st, dev_tab);
    return hipGetLastError() == hipSuccess ? TRX_OK : TRX_ERR_HIP;
}

}  // namespace
}  // namespace trx
