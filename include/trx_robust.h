/* libtrx.so, sixth header: the outlier-tolerant reduction of a model grid.
 * include/trx.h is the core ABI; what is declared here is exported by the same library under the prefix trxr_ and
 * follows the same conventions (device pointers, explicit stream, 0 = ok or TRX_ERR_*, no synchronisation inside). */
#ifndef TRX_ROBUST_H
#define TRX_ROBUST_H
#include "trx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* trx_chi2_grid_weighted for a light curve whose every point is, with probability eps, an outlier from a Gaussian kappa
 * times wider than its stated error, the membership integrated out per point: with d_t = flux[t] - model_grid[r][t],
 * a_t = 0.5 inv_var[t] d_t^2,
 *     out[r] (+)= h[r] = sum_t -ln[(1 - eps) exp(-a_t) + (eps / kappa) exp(-a_t / kappa^2)]
 *                      = sum_t (lo_t - log1p(exp(-|A_t - B_t|))),   A_t = a_t + c0,  B_t = a_t k2 + c1,  lo_t = min(A_t, B_t),
 * a total that rounding drives below 0 stored as 0.  The common factor prod_t (sigma_t sqrt(2 pi))^-1 is dropped, the wide
 * component's own 1 / kappa is kept in c1.  The total is not halved.
 *   c0, c1, k2   -log1p(-eps) >= 0,  ln kappa - ln eps,  1 / kappa^2 in (0, 1): the same for every row, formed by the host
 *   secdepth, sec_limit, accumulate, out_halfchi2: trx_chi2_grid_weighted's -- +inf where secdepth[r] >= sec_limit (false
 *   for a NaN depth), added to out_halfchi2[r] when accumulate != 0 (+inf stays +inf), a NaN in a row gives NaN.
 * The grid may start at any 8-byte boundary; a row's bits depend on n_time, the three constants and its values alone.
 * NULL flux, inv_var, model_grid or out_halfchi2, n < 0, n_time < 1, c0 not finite or < 0, c1 not finite, k2 outside
 * (0, 1): TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing.  No synchronisation inside. */
int trxr_chi2_grid_robust(const double* flux, const double* inv_var, const double* model_grid, int n_time, long n,
                          const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                          double c0, double c1, double k2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_ROBUST_H */
