/* libtrx.so, fourth header: the reductions of a model grid that marginalise the noise model over a small grid of
 * candidates -- correlated noise of unknown amplitude and time scale (prefix trxm_), white noise of
 * unknown size (prefix trxv_).
 * include/trx.h is the core ABI; what is declared here is exported by the same library under these prefixes and
 * follows the same conventions (device pointers, explicit stream, 0 = ok or TRX_ERR_*, no synchronisation inside). */
#ifndef TRX_MIX_H
#define TRX_MIX_H
#include "trx.h"
#ifdef __cplusplus
extern "C" {
#endif

#define TRXM_MAX_CANDIDATES 8

/* trxn_chi2_grid_ou (include/trx_noise.h) for n_cand candidate noise models at once, K_j = diag(sigma_t^2) +
 * s_j^2 exp(-|t_i - t_k| / tau_j), j = 0 .. n_cand - 1: with h_j[r] = 0.5 y^T K_j^-1 y, y_t = flux[t] - model_grid[r][t],
 * by the recurrence of trxn_chi2_grid_ou on candidate j's alpha, beta, omega -- the bits that call gives --
 *     out[r] (+)= T[r] = -ln sum_j exp(lnc[j] - h_j[r])   (a_j = h_j - lnc[j], m = min_j a_j, T = m - ln sum_j exp(m - a_j)),
 * a value that rounding drives below 0 stored as 0.  One pass over the grid: every grid value is read once.
 *   alpha, beta, omega   [n_cand][n_time] in device memory, row j the tables of candidate j
 *   lnc                  [n_cand] in HOST memory, read before the call returns: ln(prior weight of j) - 0.5 ln det K_j, less
 *                        their log-sum-exp (the host forms them: datasets.ou_mix_system); -inf switches a candidate off
 *   cand_out             [n][n_cand] in device memory or NULL: cand_out[r][j] = h_j[r] (no secondary rule, not accumulated)
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's -- +inf where secdepth[r] >= sec_limit (false
 *   for a NaN depth), added to out_halfchi2[r] when accumulate != 0 (+inf stays +inf), a NaN in a row gives NaN.
 * n_cand == 1 with lnc[0] == 0 gives trxn_chi2_grid_ou's bits.  The grid may start at any 8-byte boundary; a row's bits
 * depend on n_time, n_cand and its values alone.
 * NULL flux, model_grid, out_halfchi2, alpha, beta, omega or lnc, n < 0, n_time < 1, n_cand outside
 * 1 .. TRXM_MAX_CANDIDATES, a NaN or +inf in lnc: TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing.  No
 * synchronisation inside. */
int trxm_chi2_grid_ou_mix(const double* flux, const double* model_grid, int n_time, long n,
                          const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                          const double* alpha, const double* beta, const double* omega,
                          int n_cand, const double* lnc, double* cand_out, void* stream);

#define TRXV_MAX_CANDIDATES 8

/* trx_chi2_grid_weighted (include/trx.h) for n_cand candidate white-noise models at once, candidate j with the per-point
 * weights weights[j][t] = 1 / (k_j^2 sigma_t^2 + s_j^2) -- an error scale k_j and a jitter s_j --, j = 0 .. n_cand - 1:
 * with h_j[r] = 0.5 sum_t weights[j][t] (flux[t] - model_grid[r][t])^2, summed as trx_chi2_grid_weighted sums it with
 * inv_var = weights[j] -- the bits that call gives --
 *     out[r] (+)= T[r] = -ln sum_j exp(lnc[j] - h_j[r])   (a_j = h_j - lnc[j], m = min_j a_j, T = m - ln sum_j exp(m - a_j)),
 * a value that rounding drives below 0 stored as 0; T is not halved again.  One pass over the grid: every grid value is
 * read once, its residual serves all candidates.
 *   weights              [n_cand][n_time] in device memory, row j the weights of candidate j
 *   lnc                  [n_cand] in HOST memory, read before the call returns: ln(prior weight of j) + 0.5 sum_t ln
 *                        weights[j][t], less their log-sum-exp (the host forms them: datasets.white_mix_system); -inf
 *                        switches a candidate off
 *   cand_out             [n][n_cand] in device memory or NULL: cand_out[r][j] = h_j[r] (no secondary rule, not accumulated)
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's -- +inf where secdepth[r] >= sec_limit (false
 *   for a NaN depth), added to out_halfchi2[r] when accumulate != 0 (+inf stays +inf), a NaN in a row gives NaN there and
 *   leaves every other row alone.
 * n_cand == 1 with lnc[0] == 0 gives trx_chi2_grid_weighted's bits.  The grid may start at any 8-byte boundary; a row's
 * bits depend on n_time, n_cand, its values and the tables alone.  No condition on the order of the stamps.
 * NULL flux, model_grid, out_halfchi2, weights or lnc, n < 0, n_time < 1, n_cand outside 1 .. TRXV_MAX_CANDIDATES, a NaN
 * or +inf in lnc: TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing.  No synchronisation inside; no switches, no
 * environment. */
int trxv_chi2_grid_white_mix(const double* flux, const double* model_grid, int n_time, long n,
                             const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                             const double* weights, int n_cand, const double* lnc, double* cand_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_MIX_H */
