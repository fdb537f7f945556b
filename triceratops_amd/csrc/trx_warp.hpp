// The evidence's weight per (uniform, bin): the input of an adaptive importance map (trx_scenario_args.warp_hist,
// trx_draw_args.warp: include/trx.h).  Included by trx_scenario.hip only.
//
// The n masked draws of a branch, in list order, carry the evidence's own log-weights
//     x_i = -ln(sigma) - 0.5 ln(2 pi) - h_i (+ lnprior_i),      w_i = exp(x_i - X) where x_i - X > -80, else 0
// (X = the branch's largest x_i, left in the call's scratch by the evidence's final stage: ScenFinal.post_x -- the
// weights of trx_posterior.hpp).  For every slot d the scenario consumes from the kernel's own generator the draw's
// PRE-MAP uniform y is recomputed from (seed, draw index, slot) -- the draw index through the branch's index list -- and
// floor(w_i 2^32) is added to bin min((int)(y 64), 63) of row d.  Integer sums: exact, so every partition and order
// gives the same bits and no floating-point atomic is needed.  w <= 1 and n < 2^31 keep every sum below 2^63.
//
//   warp_hist_kernel        grid-stride over the rows; a [7][64] histogram of 64-bit integers per workgroup in LDS (LDS
//                           atomics), then ONE global atomic add per non-empty (slot, bin) and workgroup into the branch's
//                           block in device scratch (zeroed on the stream before the launch); the caller's block is a copy
//   warp_hist_chain_kernel  the same for every branch of a launch chain that wants a histogram: the branch is the grid's
//                           second dimension and picks its WarpHistArgs from a table in the chain's arena
// trxw_hist_from_halfchi2 (trx_scenario.hip) is warp_hist_kernel on a caller's chi^2/2 values: the row count by value
// (n_dev null), the draw indices as 64-bit integers (idx64), X found by post_max_kernel / post_x_kernel (trx_posterior.hpp).
//
// The bounded evaluation stays on, as for the posterior rows: a draw it abandoned reports a lower
// bound of its chi^2/2 that puts it more than 90 below X -- beyond the cut at -80, weight 0 with and without the flag.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/trx.h"

namespace trx {
namespace {

constexpr int kWarpHistBlocks = 256;       // workgroups per branch (256 threads each)

struct WarpHistArgs {
    const double* h;          // chi^2/2 of the masked draws, list order
    const double* lnprior;    // null, or per row: position r (twin: N - 1 - r)
    const long* n_dev;        // the number of rows on the device, or null: n
    long n;
    const int* idx;           // the rows' draw indices
    const long* idx64;        // ... or, when not null, the same as 64-bit integers (idx is not read then)
    long N;
    int twin;
    unsigned slots;           // bit d: slot d is consumed from the kernel's own generator
    double c0;                // -0.5 ln(2 pi) - ln(sigma)
    unsigned long long seed;
    const double* xmax;       // [1] X
    unsigned long long* out;  // TRX_WARP_BRANCH words, zero before the launch (device)
};

// Philox4x32-10 as the draw kernel's (trx_draw.hip): key = seed, counter = (draw index lo, hi, block, 0); two 53-bit
// uniforms per block (numpy's construction)
__device__ __forceinline__ void warp_uniform2(unsigned long long seed, long i, unsigned block, double& u0, double& u1)
{
    unsigned c0 = (unsigned)i, c1 = (unsigned)((unsigned long long)i >> 32), c2 = block, c3 = 0u;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    u0 = ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * (1.0 / 9007199254740992.0);
    u1 = ((double)(c2 >> 5) * 67108864.0 + (double)(c3 >> 6)) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ int warp_bin(double y)
{
    const int b = (int)(y * (double)TRX_WARP_BINS);
    return b < TRX_WARP_BINS - 1 ? b : TRX_WARP_BINS - 1;
}

// The slots a scenario takes from the kernel's own generator (draw_one, trx_draw.hip): the inputs it consumes less the
// staged ones.  0 without use_philox.
inline unsigned warp_consumed_slots(const trx_draw_args& a)
{
    if (!a.use_philox) return 0u;
    unsigned m = 0u;
    if (a.range_P && !a.uP) m |= 1u << 0;
    if (a.comp == TRX_COMP_BOUND && !a.qc_in && !a.uQc) m |= 1u << 1;
    if (a.planet && !a.uRp) m |= 1u << 2;
    if (!a.uInc) m |= 1u << 3;
    if (!a.planet && !a.uQ) m |= 1u << 4;
    if (a.planet ? !a.ecc_in : !a.uEcc) m |= 1u << 5;
    if (!a.uW) m |= 1u << 6;
    return m;
}

__device__ __forceinline__ void warp_hist_body(const WarpHistArgs& a, unsigned long long* lds)
{
    const double X = a.xmax[0];
    if (!(X == X) || X == INFINITY || X == -INFINITY) return;       // lnZ = +-inf or NaN: the block stays zero
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < TRX_WARP_DIMS * TRX_WARP_BINS; i += blockDim.x) lds[i] = 0ull;
    __syncthreads();
    const long n = a.n_dev ? *a.n_dev : a.n;
    unsigned long long rows = 0ull;
    for (long r = (long)blockIdx.x * blockDim.x + tid; r < n; r += (long)gridDim.x * blockDim.x) {
        double x = a.c0 - a.h[r];                                   // (lme_partial_body's expression: the same bits)
        if (a.lnprior) x += a.lnprior[a.twin ? a.N - 1 - r : r];
        const double d = x - X;
        if (!(d > -80.0)) continue;                                 // the evidence's cut; NaN, -inf
        rows += 1ull;
        const unsigned long long q = (unsigned long long)(fmin(exp(d), 1.0) * 4294967296.0);
        if (q == 0ull) continue;
        const long i = a.idx64 ? a.idx64[r] : (long)a.idx[r];
        double u0, u1;
        if (a.slots & (1u << 2 | 1u << 4 | 1u << 3)) {
            warp_uniform2(a.seed, i, 16u, u0, u1);
            if (a.slots & (1u << 2)) atomicAdd(&lds[2 * TRX_WARP_BINS + warp_bin(u0)], q);
            if (a.slots & (1u << 4)) atomicAdd(&lds[4 * TRX_WARP_BINS + warp_bin(u0)], q);
            if (a.slots & (1u << 3)) atomicAdd(&lds[3 * TRX_WARP_BINS + warp_bin(u1)], q);
        }
        if (a.slots & (1u << 5 | 1u << 6)) {
            warp_uniform2(a.seed, i, 17u, u0, u1);
            if (a.slots & (1u << 5)) atomicAdd(&lds[5 * TRX_WARP_BINS + warp_bin(u0)], q);
            if (a.slots & (1u << 6)) atomicAdd(&lds[6 * TRX_WARP_BINS + warp_bin(u1)], q);
        }
        if (a.slots & (1u << 1 | 1u << 0)) {
            warp_uniform2(a.seed, i, 18u, u0, u1);
            if (a.slots & (1u << 1)) atomicAdd(&lds[1 * TRX_WARP_BINS + warp_bin(u0)], q);
            if (a.slots & (1u << 0)) atomicAdd(&lds[0 * TRX_WARP_BINS + warp_bin(u1)], q);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o, 64);
    if ((tid & 63) == 0 && rows) atomicAdd(&a.out[1], rows);
    __syncthreads();
    for (int i = tid; i < TRX_WARP_DIMS * TRX_WARP_BINS; i += blockDim.x)
        if (lds[i]) atomicAdd(&a.out[8 + i], lds[i]);
    if (blockIdx.x == 0 && tid == 0) a.out[0] = (unsigned long long)__double_as_longlong(X);
}

__global__ __launch_bounds__(256) void warp_hist_kernel(WarpHistArgs a)
{
    __shared__ unsigned long long lds[TRX_WARP_DIMS * TRX_WARP_BINS];
    warp_hist_body(a, lds);
}

__global__ __launch_bounds__(256) void warp_hist_chain_kernel(const WarpHistArgs* __restrict__ tab)
{
    __shared__ unsigned long long lds[TRX_WARP_DIMS * TRX_WARP_BINS];
    const WarpHistArgs a = tab[blockIdx.y];
    warp_hist_body(a, lds);
}

int warp_hist_launch(const WarpHistArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(warp_hist_kernel, dim3(kWarpHistBlocks), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? TRX_OK : TRX_ERR_HIP;
}

int warp_hist_launch_chain(const WarpHistArgs* dev_tab, int slots, hipStream_t st)
{
    hipLaunchKernelGGL(warp_hist_chain_kernel, dim3(kWarpHistBlocks, slots), dim3(256), 0, st, dev_tab);
    return hipGetLastError() == hipSuccess ? TRX_OK : TRX_ERR_HIP;
}

}  // namespace
}  // namespace trx
