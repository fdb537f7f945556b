/* libtrx.so, fifth header: the soft minimum over the nodes of a dataset's transit-time shift grid.
 * include/trx.h is the core ABI; what is declared here is exported by the same library under the prefix trxt_ and
 * follows the same conventions (device pointers, explicit stream, 0 = ok or TRX_ERR_*, no synchronisation inside). */
#ifndef TRX_SHIFT_H
#define TRX_SHIFT_H
#include "trx.h"
#ifdef __cplusplus
extern "C" {
#endif

#define TRXT_MAX_NODES 8

/* out[r] (+)= T[r] = -ln sum_j exp(lnc[j] - cand[j * stride + r]), r < n
 *     (a_j = cand[j * stride + r] - lnc[j], m = min_j a_j, T = m - ln sum_j exp(m - a_j); the minimum and the sum in
 *     ascending j), a value that rounding drives below 0 stored as 0.
 *   cand        n_cand rows of `stride` doubles in device memory, the first n of each used: row j holds node j's term of the
 *               log-weight of every draw (chi^2/2 from any of the grid reductions; +inf: an excluded draw)
 *   lnc         [n_cand] in HOST memory, read before the call returns: the nodes' log prior weights; -inf switches a node off
 *   accumulate  != 0: T is added to out[r] (+inf stays +inf), else stored
 * Every node +inf gives +inf (m = +inf or NaN is stored as it is); a NaN among a row's values gives NaN wherever another node
 * is finite or every node is NaN.  n_cand == 1 with lnc[0] == 0 returns cand's bits.  A
 * row's bits depend on its n_cand values and lnc alone, not on n, stride or its position.
 * NULL cand, lnc or out, n < 0, stride < n, n_cand outside 1 .. TRXT_MAX_NODES, a NaN or +inf in lnc: TRX_ERR_ARG, nothing
 * is enqueued; n == 0 launches nothing.  No synchronisation inside. */
int trxt_softmin_rows(const double* cand, long stride, long n, int n_cand, const double* lnc, int accumulate, double* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_SHIFT_H */
