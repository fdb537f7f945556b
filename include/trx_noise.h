/* libtrx.so, third header: reductions of a model grid under correlated noise.
 * include/trx.h is the core ABI; what is declared here is exported by the same library under the prefix trxn_ and
 * follows the same conventions (device pointers, explicit stream, 0 = ok or TRX_ERR_*, no synchronisation inside). */
#ifndef TRX_NOISE_H
#define TRX_NOISE_H
#include "trx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* trx_chi2_grid_weighted for a light curve whose noise is white plus one exponential (Ornstein-Uhlenbeck) term,
 * K = diag(sigma_t^2) + s_r^2 exp(-|t_i - t_j| / tau), stamps in time order: out[r] (+)= 0.5 y^T K^-1 y,
 * y_t = flux[t] - model_grid[r][t], by the O(n_time) recurrence
 *     g_0 = 0,  g_n = alpha[n] g_(n-1) + beta[n] y_(n-1),   0.5 sum_n omega[n] (y_n - g_n)^2.
 *   alpha, beta, omega   [n_time] in device memory, the same for every row (the host forms them from sigma_t, s_r, tau
 *                        and the stamps; alpha[0] and beta[0] are not read).  alpha in [0, 1)
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's -- +inf where secdepth[r] >= sec_limit (false
 *   for a NaN depth), added to out_halfchi2[r] when accumulate != 0 (+inf stays +inf), a NaN in a row gives NaN.
 * The grid may start at any 8-byte boundary; a row's bits depend on n_time and its values alone.
 * NULL flux, model_grid, out_halfchi2, alpha, beta or omega, n < 0, n_time < 1: TRX_ERR_ARG, nothing is enqueued;
 * n == 0 launches nothing.  No synchronisation inside. */
int trxn_chi2_grid_ou(const double* flux, const double* model_grid, int n_time, long n,
                      const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                      const double* alpha, const double* beta, const double* omega, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_NOISE_H */
