/* libtrx.so, seventh header: a linear baseline model marginalised under correlated noise.
 * include/trx.h is the core ABI; what is declared here is exported by the same library under the prefix trxg_ and
 * follows the same conventions (device pointers, explicit stream, 0 = ok or TRX_ERR_*, no synchronisation inside). */
#ifndef TRX_GLS_H
#define TRX_GLS_H
#include "trx.h"
#ifdef __cplusplus
extern "C" {
#endif

#define TRXG_MAX_TERMS 4

/* trxn_chi2_grid_ou (include/trx_noise.h) with a linear baseline sum_k c_k B_k[t], c_k ~ N(0, s_k^2), marginalised per
 * row under the same noise K = diag(sigma_t^2) + s_r^2 exp(-|t_i - t_j| / tau):
 *     out[r] (+)= 0.5 max(S2 - sum_ij M_ij b_i b_j, 0),   S2 = sum_n omega[n] z_n^2,   b_k = sum_n columns[k][n] z_n,
 * z_n = y_n - g_n the innovations of y_t = flux[t] - model_grid[r][t]: g_0 = 0, g_n = alpha[n] g_(n-1) + beta[n] y_(n-1).
 *   alpha, beta, omega   [n_time] in device memory, as for trxn_chi2_grid_ou
 *   columns              [n_terms][n_time] in device memory: omega[n] z[B_k]_n / sqrt(D_k), the innovations of the
 *                        baseline columns under the same recurrence, D_k = sum_n omega[n] z[B_k]_n^2 (the host forms them)
 *   n_terms              1 .. TRXG_MAX_TERMS
 *   minv                 HOST memory, read before the call returns: the n_terms (n_terms + 1) / 2 entries of the upper
 *                        triangle, by rows, of M = (D^(-1/2) (B^T K^-1 B + diag(1 / s_k^2)) D^(-1/2))^-1; all zero gives
 *                        trxn_chi2_grid_ou's bits
 *   coef_out             NULL, or [n][n_terms] in device memory: receives sum_j M_ij b_j, the scaled posterior-mean
 *                        coefficients (c_k = coef_out[r][k] / sqrt(D_k))
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's; a NaN in a row gives NaN.
 * The grid may start at any 8-byte boundary; a row's bits depend on n_time, its values and the tables alone.
 * NULL flux, model_grid, out_halfchi2, alpha, beta, omega, columns or minv, n < 0, n_time < 1, n_terms outside
 * 1 .. TRXG_MAX_TERMS, an entry of minv that is not finite: TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing. */
int trxg_chi2_grid_ou_baseline(const double* flux, const double* model_grid, int n_time, long n,
                               const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                               const double* alpha, const double* beta, const double* omega,
                               const double* columns, int n_terms, const double* minv, double* coef_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_GLS_H */
