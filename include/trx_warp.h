/* libtrx.so, second header: the weight histogram of an adaptive importance map on its own.
 * include/trx.h is the core ABI; what is declared here is exported by the same library under the prefix trxw_ and
 * follows the same conventions (device pointers, explicit workspace and stream, 0 = ok or TRX_ERR_*, no
 * synchronisation inside). */
#ifndef TRX_WARP_H
#define TRX_WARP_H
#include "trx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The histogram of trx_scenario_args.warp_hist for ONE branch on its own, on chi^2/2 values already on the device (the
 * counterpart of trx_lnz_from_halfchi2 / trx_posterior_from_halfchi2 for callers that evaluate the draws of
 * trx_draw_scenario themselves): halfchi2 [n], lnprior [n] or NULL and idx [n] -- the rows' draw indices, from which the
 * PRE-MAP uniforms are recomputed -- in list order, all in device memory.
 *   draw       HOST: read for `seed` and for the slots the scenario consumes from the kernel's own generator; nothing
 *              it points to is touched.  use_philox == 0: TRX_ERR_ARG
 *   out        TRX_WARP_BRANCH 64-bit words in device memory, the layout of trx_scenario_args.warp_hist: [0] X = max x_i
 *              as a double's bits (found here; NaN terms are ignored), [1] the rows with x_i - X > -80, [2..7] 0, then the bins.  Zeroed on the
 *              stream by the call itself; all zeros when n == 0 or X is +-inf or NaN (a +inf term included)
 *   workspace  trx_workspace_bytes() bytes of device scratch
 * Integer sums: the block repeats bit for bit.  NULL draw / out, NULL halfchi2 / idx with n > 0, n < 0, n > 2^31 - 1:
 * TRX_ERR_ARG; workspace too small: TRX_ERR_WORKSPACE; nothing is enqueued then.  No synchronisation inside. */
int trxw_hist_from_halfchi2(const trx_draw_args* draw, const double* halfchi2, const double* lnprior,
                            const long* idx, long n, double lnsigma, unsigned long long* out,
                            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_WARP_H */
