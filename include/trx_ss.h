/* libtrx.so, eighth header: reductions of a model grid under correlated noise with a two-dimensional state (DESIGN.md
 * section 14) -- the noise alone (prefix trxs_), and with a linear baseline model marginalised under it (prefix trxk_).
 * include/trx.h is the core ABI; what is declared here is exported by the same library under these prefixes and follows
 * the same conventions (device pointers, explicit stream, 0 = ok or TRX_ERR_*, no synchronisation inside). */
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

#define TRXK_MAX_TERMS 4

/* The reduction above with a linear baseline sum_k c_k B_k[t], c_k ~ N(0, s_k^2), marginalised per row under the same
 * noise K (trxg_chi2_grid_ou_baseline of include/trx_gls.h for a state of dimension two):
 *     out[r] (+)= 0.5 max(S2 - sum_ij M_ij b_i b_j, 0),   S2 = sum_n omega[n] z_n^2,   b_k = sum_n columns[k][n] z_n,
 * z_n = y_n - u_(n-1)[0] the innovations of y_t = flux[t] - model_grid[r][t] as above.
 *   A, g, omega          as above
 *   columns              [n_terms][n_time] in device memory: omega[n] z[B_k]_n / sqrt(D_k), the innovations of the
 *                        baseline columns under the same recurrence, D_k = sum_n omega[n] z[B_k]_n^2 (the host forms them:
 *                        datasets.ss2_baseline_system)
 *   n_terms              1 .. TRXK_MAX_TERMS
 *   minv                 HOST memory, read before the call returns: the n_terms (n_terms + 1) / 2 entries of the upper
 *                        triangle, by rows, of M = (D^(-1/2) (B^T K^-1 B + diag(1 / s_k^2)) D^(-1/2))^-1; all zero gives
 *                        the bits of the reduction above
 *   coef_out             NULL, or [n][n_terms] in device memory: receives sum_j M_ij b_j, the scaled posterior-mean
 *                        coefficients (c_k = coef_out[r][k] / sqrt(D_k))
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's; a NaN in a row gives NaN.
 * The grid may start at any 8-byte boundary; a row's bits depend on n_time, its values and the tables alone.
 * NULL flux, model_grid, out_halfchi2, A, g, omega, columns or minv, n < 0, n_time < 1, n_terms outside
 * 1 .. TRXK_MAX_TERMS, an entry of minv that is not finite: TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing. */
int trxk_chi2_grid_ss2_baseline(const double* flux, const double* model_grid, int n_time, long n,
                                const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                                const double* A /* [n_time][4] */, const double* g /* [n_time][2] */,
                                const double* omega /* [n_time] */, const double* columns, int n_terms,
                                const double* minv, double* coef_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_SS_H */
