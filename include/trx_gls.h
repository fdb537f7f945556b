/* libtrx.so, seventh header: a linear baseline model marginalised under a noise model --
 * correlated noise (prefix trxg_), white noise whose size is marginalised over candidates (prefix trxb_).
 * include/trx.h is the core ABI; what is declared here is exported by the same library under these prefixes and
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

#define TRXB_MAX_CANDIDATES 8
#define TRXB_MAX_TERMS 4

/* trx_chi2_grid_weighted (include/trx.h) for n_cand candidate white-noise models at once -- candidate j with the per-point
 * weights weights[j][t] = 1 / (k_j^2 sigma_t^2 + s_j^2), an error scale k_j and a jitter s_j -- with a linear baseline
 * sum_k c_k basis[k][t], c_k ~ N(0, s_k^2), marginalised per row under every candidate.  With d_t = flux[t] -
 * model_grid[r][t], j = 0 .. n_cand - 1, k = 0 .. n_terms - 1:
 *     S2_j = sum_t weights[j][t] d_t^2,   b_jk = sum_t weights[j][t] basis[k][t] d_t,   c_j = Ainv_j b_j,
 *     h_j = 0.5 max(S2_j - b_j . c_j, 0),
 *     out[r] (+)= T[r] = -ln sum_j exp(lnc[j] - h_j)   (a_j = h_j - lnc[j], m = min_j a_j, T = m - ln sum_j exp(m - a_j)),
 * a value that rounding drives below 0 stored as 0; T is not halved again.  One pass over the grid: every grid value is
 * read once, its residual serves all candidates and columns.
 *   weights              [n_cand][n_time] in device memory, row j the weights of candidate j
 *   basis                [n_terms][n_time] in device memory, the baseline columns as given (the same for every candidate)
 *   minv                 HOST memory, read before the call returns: [n_cand][n_terms (n_terms + 1) / 2], per candidate the
 *                        upper triangle, by rows, of Ainv_j = (basis W_j basis^T + diag(1 / s_k^2))^-1, in the units of the
 *                        b_jk; all zero gives h_j = 0.5 S2_j
 *   lnc                  [n_cand] in HOST memory, read before the call returns: ln(prior weight of j) + 0.5 sum_t ln
 *                        weights[j][t] - 0.5 ln det A_j, less their log-sum-exp (the host forms them:
 *                        datasets.white_baseline_system); -inf switches a candidate off
 *   cand_out             [n][n_cand] in device memory or NULL: cand_out[r][j] = h_j (no secondary rule, not accumulated)
 *   coef_out             [n][n_cand][n_terms] in device memory or NULL: coef_out[r][j][k] = c_jk, the posterior-mean
 *                        coefficients under candidate j
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's -- +inf where secdepth[r] >= sec_limit (false
 *   for a NaN depth), added to out_halfchi2[r] when accumulate != 0 (+inf stays +inf), a NaN in a row gives NaN there and
 *   leaves every other row alone.
 * The grid may start at any 8-byte boundary; a row's bits depend on n_time, n_cand, n_terms, its values and the tables
 * alone.  No condition on the order of the stamps.
 * NULL flux, model_grid, out_halfchi2, weights, basis, minv or lnc, n < 0, n_time < 1, n_cand outside
 * 1 .. TRXB_MAX_CANDIDATES, n_terms outside 1 .. TRXB_MAX_TERMS, a NaN or +inf in lnc, an entry of minv that is not
 * finite: TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing.  No synchronisation inside; no switches, no
 * environment. */
int trxb_chi2_grid_white_baseline(const double* flux, const double* model_grid, int n_time, long n,
                                  const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                                  const double* weights, const double* basis, int n_cand, int n_terms,
                                  const double* minv, const double* lnc, double* cand_out, double* coef_out,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_GLS_H */
