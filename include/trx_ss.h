/* libtrx.so, eighth header: reductions of a model grid under correlated noise with a two-dimensional state (DESIGN.md
 * section 14).  include/trx.h is the core ABI; what is declared here is exported by the same library under the prefix
 * trxs_ and follows the same conventions (device pointers, explicit stream, 0 = ok or TRX_ERR_*, no synchronisation
 * inside). */
#ifndef TRX_SS_H
#define TRX_SS_H
#include "trx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* trxn_chi2_grid_ou (include/trx_noise.h) for a light curve whose noise is white plus a stationary Gaussian process with
 * a state of dimension two, observed through its first component -- a Matern-3/2 term, the sum of two exponential terms
 * --, stamps in time order: out[r] (+)= 0.5 y^T K^-1 y, y_t = flux[t] - model_grid[r][t], by the O(n_time) innovation
 * form of the process' Kalman filter
 *     u_(-1) = 0,   z_n = y_n - u_(n-1)[0],   u_n = A[n] u_(n-1) + g[n] y_n,    0.5 sum_n omega[n] z_n^2.
 *   A       [n_time][4] in device memory: the 2 x 2 matrices by rows (A[n][0] A[n][1]; A[n][2] A[n][3])
 *   g       [n_time][2] in device memory
 *   omega   [n_time] in device memory
 *           the same for every row (the host forms them from sigma_t, the term's parameters and the stamps; A and g of
 *           the last stamp enter no innovation)
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's -- +inf where secdepth[r] >= sec_limit (false
 *   for a NaN depth), added to out_halfchi2[r] when accumulate != 0 (+inf stays +inf), a NaN in a row gives NaN.
 * The grid may start at any 8-byte boundary; a row's bits depend on n_time, the tables and its values alone.
 * NULL flux, model_grid, out_halfchi2, A, g or omega, n < 0, n_time < 1: TRX_ERR_ARG, nothing is enqueued;
 * n == 0 launches nothing.  No synchronisation inside. */
int trxs_chi2_grid_ss2(const double* flux, const double* model_grid, int n_time, long n,
                       const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                       const double* A /* [n_time][4] */, const double* g /* [n_time][2] */,
                       const double* omega /* [n_time] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_SS_H */
