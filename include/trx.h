/*
 * trx.h -- C ABI of libtrx.so, the MI355X (gfx950) implementation of the
 * marginal-likelihood hot path of stevengiacalone/triceratops.
 *
 * The reference has no FFI: this path sits behind plain in-process Python functions
 * (triceratops/likelihoods.py, triceratops/marginal_likelihoods.py,
 * triceratops/_numerics.py) plus the third-party pytransit.QuadraticModel object.
 * Each entry point below names the reference interface it replaces; INTEGRATION.md
 * shows the ctypes binding a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no C++/torch types; every buffer is caller-owned;
 *   - pointers are DEVICE pointers (hipMalloc / torch.Tensor.data_ptr()) unless the
 *     function name ends in _host;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null
 *     stream) and the call returns without synchronising: safe to call concurrently on
 *     different streams / devices.  The entry points that evaluate the light-curve model
 *     (trx_lnl_batch, trx_lnl_batch_weighted, trx_flux_grid, trx_lnz_scenario, trx_scenario_evidence, trx_star_enqueue) keep scratch per
 *     (device, stream) inside the library -- 152 B per row for the per-row constants, the draw
 *     block of trx_scenario_evidence (~0.36 GB per stream at N = 1e6 draws), the arena of a launch chain of
 *     trx_star_enqueue (that much per call of the chain) -- which serves call after call on that stream and only
 *     grows (the stream is synchronised before a buffer is replaced by a larger one);
 *     trx_release_scratch() frees it all.  Two host threads that enqueue on ONE stream take turns (a
 *     per-stream lock is held while a call enqueues its kernels; the stream's order does the rest).
 *     trx_lnl_batch, trx_flux_grid, trx_lnz_scenario and the reductions can be captured
 *     into a hipGraph: while `stream` is capturing, a model call takes a scratch buffer of its own that the
 *     captured graph OWNS (a hipUserObject: it returns to the library's pool when the graph and its executable
 *     graphs are destroyed; rounds 2-5 used graph memory nodes, which intermittently handed a replay zeroed
 *     pages on this stack -- DESIGN.md 4.8).  Inputs must be resident before the capture begins.
 *     NO process-wide mutable state: the library's behaviour is a function of a call's arguments.  What it
 *     keeps besides the scratch are caches whose content cannot change a result -- a mutex-guarded table of the
 *     Gauss nodes per `nsupersample` (filled on first use, read-only afterwards), its device copy, and a
 *     per-light-curve hint whether the centre-value stencil applied (it only saves an empty launch) -- and the
 *     two monotonic row counters of trx_skipped_rows / trx_pruned_rows (statistics).  The tuning and
 *     diagnostics switches that rounds 1-5 exported from this library (trx_set_*) live in include/trx_debug.h
 *     and exist only in the TESTING build, libtrx_testing.so (-DTRX_TESTING); per-call choices are TRX_FLAG_* bits;
 *   - return value: 0 = ok, TRX_ERR_* otherwise (never throws); trx_last_error()
 *     gives a thread-local message for the last non-zero return on this thread;
 *   - numerical exclusions travel in-band exactly as in the reference:
 *     +inf in chi^2/2 = excluded draw, -inf / NaN log-weights = zero weight.
 */
#ifndef TRX_H
#define TRX_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* model families */
#define TRX_MODEL_TP       0  /* transiting planet:  simulate_TP_transit_p, likelihoods.py:302-358 */
#define TRX_MODEL_EB       1  /* eclipsing binary:   simulate_EB_transit_p, likelihoods.py:361-439;
                                 lnL +inf where secondary depth >= 1.5 sigma, :534-538 */
#define TRX_MODEL_EB_TWIN  2  /* twin EB (q>=0.95 at 2 P_orb): same light curve as EB, no secondary
                                 cut, likelihoods.py:542-587 */
#define TRX_MODEL_RAW      3  /* bare pytransit-shaped evaluate_pv (no unit conversion, no dilution);
                                 trx_flux_grid only */

/* flags (bit-or) */
#define TRX_FLAG_COMPANION_IS_HOST 1 /* `companion_is_host=True`, likelihoods.py:352, 427 */
#define TRX_FLAG_SCALAR_K          2 /* scalar-path radius-ratio rule `abs(k-1)<1e-6`, 1/k for the
                                        secondary (likelihoods.py:121-123, 137) instead of the vector
                                        path's `(k-1)<1e-6` on both (likelihoods.py:406, 418) */

#define TRX_FLAG_FP32_MODEL         4 /* mixed precision (BASELINE config 5): fp64 orbit and geometric
                                        differences, fp32 Mandel-Agol arithmetic, fp64 chi^2 and
                                        log-mean-exp accumulation; ~1e-7 absolute in flux */

#define TRX_FLAG_EVALUATE_EXCLUDED   8 /* trx_lnl_batch / trx_lnz_scenario: evaluate the light curve of a draw that
                                        lnL_EB_p's secondary-eclipse rule excludes anyway (+inf either way): for
                                        benchmarks that count every row.  Default: such a row (half of the EB draws
                                        of a typical run, likelihoods.py:535-538) is not evaluated at all;
                                        trx_skipped_rows counts them */
/* Result-neutral per-call choices (same numbers to rounding; for benchmarks and cross-checks): */
#define TRX_FLAG_ALL_SUBEXPOSURES   16 /* every cell evaluates all `nsupersample` sub-exposures, the reference's literal
                                        algorithm, instead of the 3-9 point Gauss rule of the same discrete measure
                                        where the model is analytic over the exposure (agree to ~1e-13 in flux) */
#define TRX_FLAG_NO_STENCIL         32 /* no centre-value stencil: on a uniform time grid of <= 0.3 exposures per cell
                                        (light curves of 320 points and more) a cell far from every limb contact
                                        otherwise takes its exposure average from the instantaneous flux at the
                                        centres of its 13 nearest cells (one evaluation per cell, error bound 1e-15)
                                        instead of 3-4 Gauss nodes (agree to ~2e-14 in flux) */
#define TRX_FLAG_COUNT_EVALUATIONS  64 /* trx_flux_grid: out_flux receives the NUMBER of model evaluations each cell
                                        cost instead of its flux (the census behind bench.py's roofline line) */
#define TRX_FLAG_FULL_EVALUATION   128 /* trx_scenario_* / trx_star_enqueue: every masked draw is evaluated to the end.
                                        Default: bounded evaluation -- a draw is abandoned once it is shown that it
                                        can neither be the best draw (its chi^2 exceeds the smallest finished one) nor
                                        carry weight in the evidence (its log-weight lies 90 below the largest
                                        finished one; the reduction drops everything 80 below the largest): from its
                                        constants alone when the model can never be as deep as the data, else from its
                                        chi^2 over ~16 probe cells and every cell outside its transit window.  lnZ
                                        agrees to rounding, the best draw is the same, results repeat bit for bit;
                                        light curves of fewer than 48 points are always evaluated in full;
                                        trx_pruned_rows counts the abandoned draws.  The per-row entry points
                                        (trx_lnl_batch, trx_lnz_scenario ...) always return the full chi^2. */
#define TRX_FLAG_WEIGHT_MOMENTS    256 /* trx_scenario_enqueue / trx_scenario_evidence / trx_star_enqueue: a branch record
                                        is TRX_SCENARIO_OUT_MOMENTS doubles wide -- the TRX_SCENARIO_OUT of today, then
                                        [18] lnM2 and [19] lnWmax of the evidence's weights (the definitions and special
                                        cases of trx_lnz_moments_from_halfchi2; both NaN when [17] status is 1) -- and
                                        the record of a call 2 * TRX_SCENARIO_OUT_MOMENTS + 1 doubles.  Every other slot,
                                        lnZ and the best draw are the same bits with and without the flag.  Calls with
                                        and without it may share a launch chain (each keeps its own record width). */

/* parameter-block rows, SoA [n_param][n] contiguous fp64 (reference argument order):
 *   TP  (10): R_p[R_earth] P_orb[d] inc[deg] a[cm] R_s[R_sun] u1 u2 ecc argp[deg] companion_fluxratio
 *   EB  (11): R_EB[R_sun] EB_fluxratio P_orb[d] inc[deg] a[cm] R_s[R_sun] u1 u2 ecc argp[deg] companion_fluxratio
 *   RAW  (9): k t0 p a(in stellar radii) i[rad] e w[rad] u1 u2      (pvp columns + ldc)            */
#define TRX_NPARAM_TP  10
#define TRX_NPARAM_EB  11
#define TRX_NPARAM_RAW 9

/* status codes */
#define TRX_OK              0
#define TRX_ERR_ARG         1  /* NULL pointer, negative size, unknown model ... */
#define TRX_ERR_HIP         2  /* a HIP runtime call failed (see trx_last_error) */
#define TRX_ERR_WORKSPACE   3  /* workspace too small */
#define TRX_ERR_NTOTAL      4  /* N_total != len(logw): the reference raises ValueError,
                                  _numerics.py:40-45 */

/* Replaces lnL_TP_p / lnL_EB_p / lnL_EB_twin_p (likelihoods.py:443-587), i.e. the light-curve
 * model + 0.5*sum((flux-model)^2/sigma^2, axis=1), fused: the (n x n_time) grid is never
 * materialised.  out_halfchi2[n] receives +chi^2/2 (+inf where model==EB and secondary depth
 * >= 1.5*sigma).  Unlike the reference it does not convert the caller's `inc` to radians in
 * place (likelihoods.py:344, 410). */
int trx_lnl_batch(int model, int flags,
                  const double* time, const double* flux, int n_time, double sigma,
                  const double* params, long n,
                  double exptime, int nsupersample,
                  double* out_halfchi2, void* stream);

/* Replaces simulate_TP_transit_p / simulate_EB_transit_p (likelihoods.py:302-439) and, with
 * model == TRX_MODEL_RAW, pytransit's QuadraticModel.set_data + evaluate_pv
 * (likelihoods.py:348-349, 414-415).  out_flux is (n, n_time) row-major; out_secdepth[n] may be
 * NULL (written for EB / EB_TWIN only). */
int trx_flux_grid(int model, int flags,
                  const double* time, int n_time,
                  const double* params, long n,
                  double exptime, int nsupersample,
                  double* out_flux, double* out_secdepth, void* stream);

/* The reference's reduction over a materialised model grid,
 * 0.5*np.sum((flux-model)**2/sigma**2, axis=1) (likelihoods.py:486, 537, 586): HBM-bound row
 * reduction over model_grid (n, n_time). */
int trx_chi2_grid(const double* flux, const double* model_grid, int n_time, long n, double sigma,
                  double* out_halfchi2, void* stream);

/* trx_chi2_grid with per-point weights, for light curves whose errors differ from point to point and for evidences
 * summed over several light curves (no reference counterpart):
 *   out[r] = (accumulate ? out[r] : 0) + 0.5 * sum_t inv_var[t] * (flux[t] - model_grid[r][t])^2
 * flux, inv_var [n_time], model_grid [n][n_time] row-major, secdepth [n] or NULL, out_halfchi2 [n]: device, 8-byte
 * aligned.  With secdepth != NULL out[r] = +inf where secdepth[r] >= sec_limit (false for a NaN depth, as numpy's
 * comparison); +inf stays +inf under accumulation.  HBM-bound: every grid value is read once.
 * Each row's sum has one fixed order that depends on n_time alone (csrc/trx_reduce.hpp): the result does not depend on
 * the launch geometry, on the row's position in the grid or on the alignment of any pointer (16-byte aligned rows are
 * read with 16-byte loads, the others with 8-byte loads -- same values, same arithmetic, same bits) and repeats bit for
 * bit.  NULL flux / inv_var / model_grid / out_halfchi2, n < 0 or n_time < 1: TRX_ERR_ARG, nothing is enqueued;
 * n == 0 launches nothing. */
int trx_chi2_grid_weighted(const double* flux, const double* inv_var, const double* model_grid,
                           int n_time, long n, const double* secdepth, double sec_limit,
                           int accumulate, double* out_halfchi2, void* stream);

/* trx_chi2_grid_weighted with a constant baseline offset of the light curve marginalised in closed form (no reference
 * counterpart).  With d_t = flux[t] - model_grid[r][t], S2 = sum_t inv_var[t] d_t^2 and
 * S1 = sum_t inv_var[t] d_t, for an offset c ~ N(0, s^2) added to the model,
 *   out[r] = (accumulate ? out[r] : 0) + 0.5 * (S2 - S1^2 / (sum_w + prior_prec)),
 *   offset_out[r] = S1 / (sum_w + prior_prec)                      (the posterior mean of c for row r; may be NULL)
 * sum_w = sum_t inv_var[t], given by the caller (it does not depend on the row); prior_prec = 1 / s^2: 0 is the flat prior
 * (the offset profiled out), +inf is no offset -- then out is trx_chi2_grid_weighted's, bit for bit.  The factor
 * (1 + s^2 sum_w)^(-1/2) of the marginal is NOT included: it is the same for every row.  A difference that rounding
 * drives below 0 is stored as 0; a NaN stays a NaN.  Buffers, the secondary rule, accumulation, the fixed order of
 * summation (S2 term for term that of trx_chi2_grid_weighted) and repeatability: as trx_chi2_grid_weighted.
 * NULL flux / inv_var / model_grid / out_halfchi2, n < 0, n_time < 1, sum_w not finite or <= 0, prior_prec < 0 or NaN:
 * TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing. */
int trx_chi2_grid_offset(const double* flux, const double* inv_var, const double* model_grid,
                         int n_time, long n, const double* secdepth, double sec_limit,
                         int accumulate, double* out_halfchi2,
                         double sum_w, double prior_prec, double* offset_out, void* stream);

/* trx_chi2_grid_weighted with a linear baseline model of the light curve marginalised in closed form (no reference
 * counterpart).  The data model is model_grid[r][t] + sum_k c_k B_k[t], k < n_terms <= 4, with
 * independent priors c_k ~ N(0, s_k^2) (s_k = inf: flat).  With d_t = flux[t] - model_grid[r][t], w = inv_var,
 * D_k = sum_t w_t B_k[t]^2, A~ = D^(-1/2) (B^T W B + diag(1 / s_k^2)) D^(-1/2) (unit diagonal) and M = A~^(-1), all
 * formed by the caller (they do not depend on the row),
 *   S2 = sum_t w_t d_t^2,   b_k = sum_t wbasis[k][t] d_t,   wbasis[k][t] = w_t B_k[t] / sqrt(D_k),
 *   out[r] = (accumulate ? out[r] : 0) + 0.5 * max(S2 - sum_ij M_ij b_i b_j, 0),
 *   coef_out[r][i] = sum_j M_ij b_j        (scaled: the posterior mean of c_i for row r is coef_out[r][i] / sqrt(D_i))
 * The factor det(I + diag(s^2) B^T W B)^(-1/2) of the marginal is NOT included: it is the same for every row.  A
 * difference that rounding drives below 0 is stored as 0; a NaN stays a NaN.  trx_chi2_grid_offset is the case of one
 * column of ones (in another order of operations: equal to rounding, not bit for bit).
 * Order of summation: S2 term for term that of trx_chi2_grid_weighted; every b_k as fma(wbasis[k][t], d_t, acc) over the
 * same stamps on the same lanes in the same order, then the same butterfly; c_i = sum_j fma(M_ij, b_j, .) for ascending
 * j, the quadratic form sum_i fma(b_i, c_i, .) for ascending i.  An all-zero minv therefore gives
 * trx_chi2_grid_weighted's bits (and coefficients 0).  Buffers, the secondary rule, accumulation and repeatability: as
 * trx_chi2_grid_weighted.  minv is read on the HOST before the call returns and passed to the kernel by value.
 * NULL flux / inv_var / model_grid / out_halfchi2 / wbasis / minv, n < 0, n_time < 1, n_terms outside 1 .. 4, an entry of
 * minv that is not finite: TRX_ERR_ARG, nothing is enqueued; n == 0 launches nothing.  No synchronisation inside. */
int trx_chi2_grid_baseline(const double* flux, const double* inv_var, const double* model_grid,
                           int n_time, long n, const double* secdepth, double sec_limit,
                           int accumulate, double* out_halfchi2,
                           const double* wbasis,   /* device [n_terms][n_time]: g_k[t] */
                           int n_terms,            /* 1 .. 4 */
                           const double* minv,     /* HOST, n_terms (n_terms + 1) / 2 doubles, packed upper
                                                      triangle by rows of M; read before the call returns */
                           double* coef_out,       /* device [n][n_terms] scaled coefficients, or NULL */
                           void* stream);

/* trx_lnl_batch with per-point weights: the light-curve model and its weighted chi^2 in one kernel, the (n x n_time)
 * grid never materialised (no reference counterpart):
 *   out[r] = (accumulate ? out[r] : 0) + 0.5 * sum_t inv_var[t] * (flux[t] - m_r(t))^2,
 * m_r the model trx_flux_grid evaluates for the same arguments (the fused kernel's own order of summation: it agrees
 * with trx_flux_grid + trx_chi2_grid_weighted to rounding, not bit for bit).  time, flux, inv_var [n_time], params
 * [n_param][n], out_halfchi2 [n]: device, 8-byte aligned.  inv_var entries are finite and >= 0; a zero drops the point.
 * The secondary-eclipse rule is trx_chi2_grid_weighted's, not trx_lnl_batch's: for TRX_MODEL_EB out[r] = +inf where
 * secdepth_r >= sec_limit -- the limit as given, the depth trx_flux_grid's out_secdepth holds; false for a NaN depth
 * (a depth that is NaN at some of the scan's points only is not told from one that is NaN at none).  sec_limit = +inf
 * switches the rule off (no secondary scan); +inf stays +inf under accumulation, and with `accumulate` a row whose
 * out[r] is +inf already is not evaluated.  Every row is evaluated in full whatever `flags` says about the bounded
 * evaluation; TRX_FLAG_FP32_MODEL and the result-neutral flags apply as in trx_lnl_batch.  Stream order, concurrency
 * and repeatability: as trx_lnl_batch.  No _host twin.
 * TRX_MODEL_RAW or an unknown model, a NULL pointer, n < 0, n_time < 1 or nsupersample < 1: TRX_ERR_ARG, nothing is
 * enqueued; n == 0 launches nothing. */
int trx_lnl_batch_weighted(int model, int flags,
                           const double* time, const double* flux, const double* inv_var, int n_time,
                           const double* params, long n, double exptime, int nsupersample,
                           double sec_limit, int accumulate,
                           double* out_halfchi2, void* stream);

/* Column quantiles of a row-major grid: out[i][c] = np.quantile(v[:, c], q[i]) (numpy's default "linear" method) over
 * the n_rows values v[r][c] of column c -- the pointwise credible band of the model curves trx_flux_grid wrote, one
 * curve per row (no reference counterpart: the reference draws the best-fit curve only).
 *   grid   [n_grid_rows][n_cols] (device)
 *   rows   [n_rows] (device) or NULL: the grid row each of the n_rows values comes from, every entry in
 *          [0, n_grid_rows), repeats allowed (an entry outside contributes a NaN); NULL: rows 0 .. n_rows - 1
 *   scale  [n_rows] (device) or NULL: v[r][c] = 1 - scale[r] * (1 - grid[rows[r]][c]), the inverse of renorm_flux
 *          (funcs.py:164-177: a model in its host star's normalisation back in the target's); NULL: the grid value
 *   q      [n_q] HOST, 0 <= q <= 1, 1 <= n_q <= 16 (copied into the launch: free to reuse on return)
 *   out    [n_q][n_cols] (device)
 * With h = (n_rows - 1) q, lo = floor(h), hi = min(lo + 1, n_rows - 1), t = h - lo and a <= b the order statistics lo
 * and hi of the column: a + (b - a) t for t < 0.5, b - (b - a) (1 - t) for t >= 0.5 (numpy's _lerp, every operation
 * rounded on its own), exactly a where a == b; NaN for every q of a column that holds a NaN.  The result does not
 * depend on the launch geometry and repeats bit for bit.  1 <= n_rows <= TRX_POST_MAX_ROWS.  NULL grid / q / out,
 * n_rows or n_q out of range, n_cols < 1, a q outside [0, 1] or NaN: TRX_ERR_ARG, nothing is enqueued. */
int trx_grid_quantiles(const double* grid, long n_grid_rows, int n_cols,
                       const long* rows, const double* scale, long n_rows,
                       const double* q, int n_q, double* out, void* stream);

/* Bytes of device scratch the reductions below need (a small constant: 64 KiB). */
size_t trx_workspace_bytes(void);

/* Replaces _log_mean_exp(logw, N_total=...) (_numerics.py:12-51): log(mean(exp(logw))) with
 * -inf / NaN = zero weight still counted in the denominator, any +inf -> +inf, no finite entry
 * -> -inf.  n_total must equal n (TRX_ERR_NTOTAL otherwise, nothing enqueued).  out: 1 double. */
int trx_log_mean_exp(const double* logw, long n, long n_total, double* out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Fused evidence of one scenario branch, the tail of every lnZ_* in marginal_likelihoods.py
 * (e.g. lnZ_TTP 117-154):  lnL_i = -0.5 ln(2 pi) - lnsigma - chi2half_i (+ lnprior_i),
 * lnZ = log( sum_i exp(lnL_i) / n_total ), where the n rows are the draws that passed the
 * geometry mask and the other n_total - n draws have weight zero.
 *   lnprior  [n] or NULL  (lnprior_companion of the P/S/D/B scenarios, already masked)
 *   out_halfchi2 [n]      chi^2/2 per masked draw (needed by the caller for the best-100 table)
 *   out_lnz  1 double */
int trx_lnz_scenario(int model, int flags,
                     const double* time, const double* flux, int n_time, double sigma,
                     const double* params, long n,
                     double exptime, int nsupersample,
                     const double* lnprior, long n_total, double lnsigma,
                     double* out_halfchi2, double* out_lnz,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The tail of trx_lnz_scenario on its own: lnZ from chi^2/2 values already on the device. */
int trx_lnz_from_halfchi2(const double* halfchi2, const double* lnprior, long n, long n_total,
                          double lnsigma, double* out_lnz,
                          void* workspace, size_t workspace_bytes, void* stream);

/* trx_lnz_from_halfchi2 with the Monte-Carlo moments of the same weights w_i = exp(lnL_i [+ lnprior_i]), one pass:
 *   out[0]  lnZ    = log(sum w / n_total): trx_lnz_from_halfchi2's value bit for bit (same partition, same fold)
 *   out[1]  lnM2   = log(sum w^2 / n_total), the log of the mean squared weight (the zero weights count in n_total)
 *   out[2]  lnWmax = log(max w / sum w), the largest single weight's share of the evidence (<= 0)
 * so that the effective sample size is (sum w)^2 / sum w^2 = n_total * exp(2 lnZ - lnM2) and the standard error of lnZ
 * sqrt(1 / ess - 1 / n_total).  Special cases: any +inf term -> lnZ = +inf, lnM2 = lnWmax = NaN; no finite term (or
 * n = 0) -> lnZ = lnM2 = -inf, lnWmax = NaN.  (In a record of TRX_FLAG_WEIGHT_MOMENTS a branch whose status is 1 --
 * a row no pass wrote -- has lnZ = lnM2 = lnWmax = NaN.)  Terms more than 80 below the largest are left out of both
 * sums, as of lnZ's.  out: 3 doubles (device). */
int trx_lnz_moments_from_halfchi2(const double* halfchi2, const double* lnprior, long n, long n_total,
                                  double lnsigma, double* out, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* The selection of trx_scenario_args.post_rows on its own, on chi^2/2 values already on the device (the counterpart of
 * trx_lnz_moments_from_halfchi2): post_rows = M systematic-resampling draws from the weights of the n rows.
 *   out_pos [M] (device)  the sampled list positions r_j, non-decreasing; -1 where there is none
 *   out_hdr [4] (device)  u, X, ln S, the number of rows with positive weight (0: no sample; also when a +inf term
 *                         makes the evidence +inf)
 *   workspace             trx_workspace_bytes() bytes of device scratch
 * M < 0, M > TRX_POST_MAX_ROWS, n < 0, NULL outputs: TRX_ERR_ARG; workspace too small: TRX_ERR_WORKSPACE; nothing is
 * enqueued then. */
int trx_posterior_from_halfchi2(const double* halfchi2, const double* lnprior, long n, double lnsigma,
                                int post_rows, unsigned long long post_seed, long* out_pos, double* out_hdr,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Host-pointer conveniences: stage host buffers to the current device, run the kernels above,
 * copy back and synchronise.  For callers without a device allocator (a ctypes binding on
 * numpy arrays).  They are GPU paths, not CPU fallbacks. */
int trx_lnl_batch_host(int model, int flags,
                       const double* time, const double* flux, int n_time, double sigma,
                       const double* params, long n,
                       double exptime, int nsupersample, double* out_halfchi2);
int trx_flux_grid_host(int model, int flags,
                       const double* time, int n_time,
                       const double* params, long n,
                       double exptime, int nsupersample,
                       double* out_flux, double* out_secdepth);
int trx_log_mean_exp_host(const double* logw, long n, long n_total, double* out);

/* Statistics (monotonic device counters, current device; reading synchronises the device; reset != 0 clears the one
 * read): rows of likelihood calls that were not evaluated because lnL_EB_p's secondary-eclipse rule excludes them
 * anyway (see TRX_FLAG_EVALUATE_EXCLUDED), and draws the bounded evaluation abandoned (see TRX_FLAG_FULL_EVALUATION).
 * They cannot change a result. */
int trx_skipped_rows(unsigned long long* out, int reset);
int trx_pruned_rows(unsigned long long* out, int reset);

/* ------------------------------------------------------------------------------------------
 * The per-draw half of one scenario evidence as ONE kernel (no reference counterpart as a single
 * function: it is the body of every lnZ_* between its np.random draws and its lnL_*_p call,
 * marginal_likelihoods.py:67-123 (TTP) ... 2064-2250 (BEB), with the samplers of priors.py:16-383,
 * the stellar / flux relations of funcs.py:54-140 and the companion priors of priors.py:580-1005).
 * Input: staged random numbers in the reference's draw order (device generator, or numpy's global
 * stream copied over); output: the SoA parameter block trx_lnl_batch takes (all N draws, not yet
 * compacted), the geometry mask(s) and lnprior_companion. */

#define TRX_HOST_TARGET     0   /* T, P, D scenarios: the target star hosts the transit */
#define TRX_HOST_COMPANION  1   /* S scenarios: an unresolved bound companion hosts it */
#define TRX_HOST_FIELD      2   /* B scenarios: a background (TRILEGAL) star hosts it */
#define TRX_COMP_NONE       0
#define TRX_COMP_BOUND      1   /* P, S: bound companion (mass ratio draw or MOLUSC table) */
#define TRX_COMP_FIELD      2   /* D, B: background star drawn from the TRILEGAL population */
#define TRX_PRIOR_NONE      0
#define TRX_PRIOR_BOUND_TP  1   /* lnprior_bound_TP, priors.py:580-782 */
#define TRX_PRIOR_BOUND_EB  2   /* lnprior_bound_EB, priors.py:784-984 */
#define TRX_PRIOR_FIELD     3   /* lnprior_background or its no-contrast-curve constant, :986-1005 */

#define TRX_DRAW_MAX_KNOTS      16
#define TRX_DRAW_SPLINE_DOUBLES (1 + 5 * TRX_DRAW_MAX_KNOTS)  /* m, knots[16], c0..c3[16] */
#define TRX_DRAW_N_SPLINES      6
#define TRX_SPL_R_HOT   0   /* funcs.py:19-51: mass -> radius / Teff, Torres et al. branch */
#define TRX_SPL_T_HOT   1
#define TRX_SPL_R_COOL  2   /*                                         cool-dwarf branch   */
#define TRX_SPL_T_COOL  3
#define TRX_SPL_F_TESS  4   /* funcs.py:81-119: mass -> log10 flux, TESS band */
#define TRX_SPL_F_BAND  5   /*                  ... band of the contrast curve */
#define TRX_DRAW_MAX_CC   256   /* contrast-curve points */
#define TRX_DRAW_MAX_LUT  160   /* (Teff / 250 K) x (logg / 0.5 dex) cells of the companion LDC table */

/* inverse CDF of a broken power law (sample_rp, sample_q, sample_q_companion); the constants are
 * computed on the host in the arithmetic of priors.py: segment j covers lo[j] < x <= hi[j] and maps
 * x to ((x / norm - cum[j]) * p1[j] / amp[j] + base[j]) ** ip[j]   (amp[j] == 0: no division) */
typedef struct {
    int nseg, ones;              /* ones: degenerate law (M_s <= 0.1): every draw is 1 */
    double norm;
    double hi[3], lo[3], cum[3], p1[3], amp[3], base[3], ip[3];
} trx_power_law;

typedef struct {
    long N;
    int planet;                  /* 1: *TP scenario (10-column block), 0: *EB (11 columns + twin) */
    int host, comp, prior;       /* TRX_HOST_*, TRX_COMP_*, TRX_PRIOR_* */
    int parallel;                /* 1: vector-path mask semantics, 0: per-draw-loop semantics */
    int flat;                    /* flatpriors */
    int use_cc;                  /* a contrast curve was given */
    int n_cc, n_lut;
    double P_lo, P_hi;           /* period range (uP != NULL) or the fixed period in P_lo */
    double M_s, R_s, Teff, u1, u2;        /* target star and its limb darkening */
    double ecc_pow;              /* binaries: ecc = uEcc ** ecc_pow (priors.py:152-154) */
    double teff_cap;             /* companion LDC lookup: 10000 (STP) or 13000 (SEB) */
    double f0_tess, f0_band;     /* flux_relation(M_s) in the TESS band / contrast-curve band */
    double dist_pc, kepler_c;    /* 1000 / plx;  4 pi^2 / (G M_ref Msun)        (priors.py:601-640) */
    double f1, f2, f3, t2, t3, t4, t5;     /* Moe & Di Stefano rate constants for M_ref */
    double bg_const, bg_amp;     /* ln((N_comp/0.1)(1/3600)^2 2.2^2);  (N_comp/0.1)(1/3600)^2 */
    trx_power_law law_rp_hi, law_rp_lo, law_q, law_qc;
    /* tables (device) */
    const double* splines;       /* [TRX_DRAW_N_SPLINES][TRX_DRAW_SPLINE_DOUBLES] */
    const double* cc_seps;       /* [n_cc] separations, */
    const double* cc_cons;       /* [n_cc] contrasts (increasing) */
    const double* lut;           /* [2][n_lut] companion limb darkening, NaN = cell absent */
    /* TRILEGAL population (device), indexed by idx */
    const double *f_mass, *f_radius, *f_teff, *f_logg, *f_fr, *f_delta, *f_frband, *f_u1, *f_u2;
    /* staged random numbers (device), [N] each; NULL where the scenario does not draw */
    const double *uP, *uQc, *uRp, *uInc, *uQ, *uEcc, *uW;
    const double* ecc_in;        /* planets: Beta(0.867, 3.03) draws */
    const double* qc_in;         /* MOLUSC mass ratios instead of uQc */
    const long* idx;             /* field-star index per draw */
    /* outputs (device) */
    double* cols;                /* [11][N] planet: R_p P inc a R_s u1 u2 ecc argp comp_fr M_host;
                                    [14][N] binary: R_EB EB_fr P inc a R_s u1 u2 ecc argp comp_fr
                                                    a_twin M_EB M_host */
    unsigned char* mask;         /* [N] geometry mask (binary: the q < 0.95 branch) */
    unsigned char* mask_twin;    /* [N] binary: the q >= 0.95 branch at 2 P_orb */
    double* lnprior;             /* [N] or NULL */
    int* flag;                   /* [1]: bit 0 set when a draw needs a limb-darkening cell the grid
                                    lacks (the reference raises ValueError) */
    /* in-kernel random numbers: with use_philox = 1 every random input left NULL above is generated
     * in the kernel by Philox4x32-10, key = seed, counter = (draw index, slot, sub-draw): slot 0 P,
     * 1 q_companion, 2 R_p, 3 inc, 4 q, 5 ecc (binaries), 6 argp, 7 field-star index (two slots share
     * one counter block: (2 | 4, 3), (5, 6), (1 | 7, 0)).  The planets' Beta(0.867, 3.030) eccentricity is
     * the inverse CDF of the slot-5 uniform (tabulated, fp32, within 1e-6 of the exact quantile).  A draw's
     * numbers depend on (seed, draw index) only, not on N or on the launch geometry. */
    int use_philox;
    int range_P;                 /* the period is drawn from [P_lo, P_hi] (implied by uP != NULL) */
    long n_field_draw;           /* field-star index drawn from [0, n_field_draw) */
    int pretest;                 /* trx_scenario_enqueue only: 1 = the geometry masks of the draws that fail a cheap fp32
                                  * necessary condition are written as 0 without the fp64 evaluation (same masks) */
    unsigned long long seed;
    double* dump;                /* [9][N] or NULL (tests): the random numbers each draw used, rows =
                                    P q_c R_p inc q ecc_u argp index ecc_beta (as uniforms / values) */
    /* Replaying the reference's own interpolation of the contrast curve (funcs.py:222-238: np.interp).  On a curve whose
     * contrasts are NOT monotonic np.interp returns the interval its search ends in, and numpy starts that search from
     * the PREVIOUS draw's interval: the value of draw i depends on draw i - 1.  The kernel bisects (no such memory).  A
     * caller that must reproduce the reference draw for draw -- the seeded validation mode -- asks trx_draw_scenario for
     * every draw's contrast (dm_out [N]: the signed delta magnitude the prior is evaluated at, NaN where the scenario
     * has none), runs np.interp over |dm| itself, in draw order, and hands the separations back (sep_in [N], arcsec):
     * where sep_in is given the kernel takes sep_in[i] instead of interpolating.  Both NULL: the kernel's own search. */
    const double* sep_in;
    double* dm_out;
    /* Importance map of the kernel's own uniforms, NULL = none: [TRX_WARP_DIMS][TRX_WARP_BINS + 1]
     * doubles (device), row d = the edges of slot d (0 P, 1 q_companion, 2 R_p, 3 inc, 4 q, 5 ecc, 6 argp; slot 7, the
     * field-star index, is never mapped), e[0] = 0, e[TRX_WARP_BINS] = 1, strictly increasing.  A uniform y the kernel
     * generated itself for slot d becomes  b = min((int)(y 64), 63), t = y 64 - b, u = e[b] + t (e[b+1] - e[b])  (kept
     * below 1), and the draw's lnprior gains ln J = sum over the slots the scenario consumes of log(64 (e[b+1] - e[b])),
     * added AFTER the prior's clamp: the evidence E_y[L prior J] is that of the unmapped draws for any valid grid.  The
     * fp32 pre-test, the mask pass and the fill pass see the same u; `dump` reports u.  A staged input is never mapped;
     * warp with use_philox == 0 is TRX_ERR_ARG.  With the identity grid e[b] = b / 64: u == y and ln J == 0 exactly.
     * A scenario without a prior (TRX_PRIOR_NONE) gets a prior column that holds ln J: trx_scenario_enqueue and
     * trx_star_enqueue force want_prior on for a call with a map.  The mapped kernels are template instantiations of
     * their own; a call without a map runs the code it ran before.  In trx_star_enqueue a call with a map and a call
     * without one do not share a launch chain: the chain is SPLIT there (calls with maps chain among themselves). */
    const double* warp;
} trx_draw_args;
#define TRX_WARP_DIMS 7
#define TRX_WARP_BINS 64

int trx_draw_scenario(const trx_draw_args* args, void* stream);
size_t trx_draw_args_size(void);   /* sizeof(trx_draw_args): lets a foreign binding check its layout */

/* One lnZ_* call of calc_probs end to end (the body of e.g. lnZ_TTP, marginal_likelihoods.py:39-172,
 * as calc_probs uses it, triceratops.py:797-817: it keeps the best draw and lnZ of each scenario):
 * draw kernel -> ordered compaction of the geometry mask(s) -> lnL_*_p of the masked draws ->
 * _log_mean_exp(lnL [+ lnprior_companion], N_total = N) -> the draw with the smallest chi^2
 * (first of equals, NaN first: numpy's / torch's argmin).  Planet scenarios give one branch, binary
 * scenarios two (q < 0.95 at P_orb, q >= 0.95 at 2 P_orb).
 *   draw      as for trx_draw_scenario; its output pointers (cols, mask, mask_twin, lnprior, flag,
 *             dump) are ignored: the buffers are stream-ordered scratch of the call
 *   out       HOST, [branches][TRX_SCENARIO_OUT] ([branches][TRX_SCENARIO_OUT_MOMENTS] with TRX_FLAG_WEIGHT_MOMENTS):
 *             the best draw's columns (11 or 14, the layout
 *             of trx_draw_args.cols; draw 0 when no draw passes the mask), then lnZ, then the
 *             number of draws that passed the mask; [16] the number of masked draws that hold the smallest
 *             chi^2 (> 1: the best draw is the FIRST of an exact tie -- numpy's argmin; the reference's
 *             argsort, marginal_likelihoods.py:152, may pick another of them); [17] status: 0, or 1 when a
 *             masked draw's chi^2 was never written by any pass of the likelihood (an internal error:
 *             lnZ is NaN then and the caller must not use the record)
 *   out_flag  HOST, [1]: trx_draw_args.flag
 * Nothing inside the call waits for the device: the masked counts stay there (the likelihood kernels
 * read them from device memory and their grids are sized for a guess), so trx_scenario_evidence is the
 * enqueue below followed by ONE hipStreamSynchronize, after which `out` is filled. */
#define TRX_SCENARIO_OUT 18
#define TRX_SCENARIO_OUT_MOMENTS 20  /* with TRX_FLAG_WEIGHT_MOMENTS: + [18] lnM2, [19] lnWmax */
typedef struct {
    const trx_draw_args* draw;
    const double* time;          /* [n_time] device */
    const double* flux;          /* [n_time] device */
    int n_time, nsupersample;
    double sigma, lnsigma, exptime;
    int flags;                   /* TRX_FLAG_* of trx_lnl_batch */
    int want_prior;              /* lnprior_companion enters the evidence (P, S, D, B scenarios) */
    double* out;
    int* out_flag;
    /* The reference's table of the best draws (marginal_likelihoods.py:152-171: `(-lnL).argsort()[:100]` and the 14
     * columns gathered at those draws), for callers of lnZ_* themselves (calc_probs reads row 0 only: leave table_rows
     * at 0 or 1).  table_rows = K > 1: `table` receives, per branch b, TRX_TABLE_BRANCH(K) doubles at
     * table + b * TRX_TABLE_BRANCH(K): column c of trx_draw_args.cols at [c * (K + 1), c * (K + 1) + K) -- row j = the
     * masked draw with the j-th smallest chi^2 (NaN last; exact ties: the earlier draw first) --, then at
     * [14 * (K + 1), 15 * (K + 1)) the K + 1 smallest chi^2/2 values themselves (a caller that must reproduce numpy's
     * order among exact ties can see from them whether there are any).  Fewer than K masked draws: the rows beyond
     * them hold draws 0, 1, 2 ... (of all N draws, whatever their mask), as the reference's argsort of equal -inf
     * log-likelihoods may.  Such a call evaluates EVERY masked draw to the end (TRX_FLAG_FULL_EVALUATION is implied:
     * the bounded evaluation leaves only the best draw and the evidence exact) and is enqueued on its own, not in a
     * launch chain.  `table`: pinned host memory (written by the device, valid once the stream has passed the call)
     * or device memory.  K <= TRX_TABLE_MAX_ROWS. */
    int table_rows;
    double* table;
    /* Histogram of the evidence's weight over the bins of the draws' uniforms (the input of an adaptive importance map,
     * trx_draw_args.warp), NULL = none; pinned host or device memory, as `post`.  Per branch b, TRX_WARP_BRANCH 64-bit
     * words at warp_hist + b * TRX_WARP_BRANCH:
     *   [0] X, the branch's largest log-weight, as a double's bits   [1] the number of rows with x_i - X > -80   [2..7] 0
     *   [8 + d * TRX_WARP_BINS + k]  the sum of floor(w_i 2^32) over the branch's masked draws whose PRE-MAP uniform y of
     *                                slot d (recomputed from seed, draw index and slot) falls into bin k = min((int)(y 64), 63);
     *                                w_i = exp(x_i - X) where x_i - X > -80, else 0 -- the weights of `post`
     * Only the slots the scenario consumes from the kernel's own generator are filled (the others stay 0); needs
     * use_philox (TRX_ERR_ARG otherwise).  Integer sums: exact, independent of order, the block repeats bit for bit.  A
     * branch whose lnZ is +-inf or NaN gets TRX_WARP_BRANCH zeros.  The bounded evaluation stays on (an abandoned draw
     * lies more than 90 below X: weight 0 either way); the record is that of the call without warp_hist, bit for bit.
     * In trx_star_enqueue such a call joins a launch chain like any other (one more launch per chain).  The same block
     * from chi^2/2 values a caller computed outside this chain: trxw_hist_from_halfchi2 (include/trx_warp.h). */
    unsigned long long* warp_hist;
    /* Posterior samples: post_rows = M > 0 draws M of the branch's masked draws in proportion to their weight in the
     * evidence, w_i = exp(x_i - X) with x_i = -ln(sigma) - 0.5 ln(2 pi) - chi2half_i (+ lnprior_i), X = max x_i, and
     * w_i = 0 where x_i - X <= -80 (the evidence's own cut; NaN and -inf: 0) -- by systematic resampling: S = sum w_i,
     * C_i = w_0 + ... + w_i over the masked draws in list order, one uniform u in [0, 1), and sample j = the first list
     * position r_j with C_{r_j} > (u + j) / M * S.  The r_j come out in non-decreasing order; draw i appears
     * floor(M w_i / S) or ceil(M w_i / S) times; a draw of zero weight never appears.  The sums are taken in 128-bit fixed
     * point (w 2^96), so S and C are exact to n 2^-96 S and the result repeats bit for bit.  `post` receives, per branch
     * b, TRX_POST_BRANCH(M) doubles at post + b * TRX_POST_BRANCH(M):
     *   [0] u  [1] X  [2] ln S  [3] the number of rows with w > 0  [4..7] 0
     *   [8 + c * M, 8 + (c + 1) * M)  row c: column c of trx_draw_args.cols at the sampled draws for c < 11 (planet) or
     *                                 14 (binary), 0 for the rows up to 13; row 14 the list positions r_j; row 15 the
     *                                 log-weights x_{r_j}
     * A branch without a positive weight (lnZ = -inf), or with lnZ = +inf / NaN: [3] = 0 and every one of the 16 rows NaN.
     * u is Philox4x32-10 with key post_seed and counter (b, 0, 0x504f5354, 0): no random stream of the draws is touched.
     * Such a call keeps the bounded evaluation (an abandoned draw lies more than 90 below X: weight 0 either way) and
     * may be combined with table_rows and TRX_FLAG_WEIGHT_MOMENTS; its record is bit for bit that of the call without
     * post_rows.  In trx_star_enqueue it joins a launch chain like a call without post_rows (the calls of a chain may
     * ask for different M, 0 included, and name different `post` blocks; the block is that of the call enqueued on its
     * own, bit for bit: key and counter are the call's own) -- unless it also asks for a table: table_rows > 1 takes a
     * call out of the chains, with or without post_rows.  `post`: pinned host or device memory, as `table`.
     * M <= TRX_POST_MAX_ROWS.  post_rows = 0: no posterior. */
    int post_rows;
    double* post;
    unsigned long long post_seed;
} trx_scenario_args;
#define TRX_WARP_BRANCH (8 + TRX_WARP_DIMS * TRX_WARP_BINS)
#define TRX_TABLE_MAX_ROWS 127
#define TRX_TABLE_BRANCH(K) (15 * ((K) + 1))
#define TRX_POST_MAX_ROWS 4096
#define TRX_POST_BRANCH(M) (8 + 16 * (M))
int trx_scenario_evidence(const trx_scenario_args* args, void* stream);
/* The same call without the final synchronisation: everything is enqueued on `stream` and the function
 * returns.  args->out / args->out_flag are ignored; the record arrives in
 *   out   HOST, [2 * TRX_SCENARIO_OUT + 1] doubles: the branch records as above, then the flag as a double
 *         ([2 * TRX_SCENARIO_OUT_MOMENTS + 1] with TRX_FLAG_WEIGHT_MOMENTS in args->flags).
 * Give pinned memory (hipHostMalloc / torch pin_memory) so that the copy is asynchronous; `out` is valid once
 * the stream has passed the call (hipStreamSynchronize, an event).  `args` and everything it points to on the
 * host may be reused as soon as the function returns; the device tables it names must stay alive until the
 * stream has passed the call.  A caller can enqueue every lnZ_* call of a calc_probs on a few streams and wait
 * once. */
int trx_scenario_enqueue(const trx_scenario_args* args, double* out, void* stream);
size_t trx_scenario_args_size(void);

/* The lnZ_* calls of one star of calc_probs (triceratops.py:784-1340: TP, EB, PTP, PEB, STP, SEB, DTP, DEB, BTP,
 * BEB for the target; TP, EB for a nearby star) -- or any other group of calls -- in ONE library call:
 * trx_scenario_enqueue(&calls[i], out[i], streams[i]) for i = 0 .. n_calls - 1, in that order.  A host binding
 * builds the argument blocks of a star once and crosses the FFI once instead of ten times.
 *   calls    HOST, [n_calls]
 *   out      HOST, [n_calls] pointers to pinned records of 2 * TRX_SCENARIO_OUT + 1 doubles (of
 *            2 * TRX_SCENARIO_OUT_MOMENTS + 1 for a call with TRX_FLAG_WEIGHT_MOMENTS)
 *   streams  HOST, [n_calls] hipStream_t handles (they may repeat; calls on one stream run in order)
 * Returns the status of the first call that failed (the later ones are not enqueued; *n_done, if given, receives
 * the number of calls that were). */
int trx_star_enqueue(const trx_scenario_args* calls, int n_calls, double* const* out, void* const* streams,
                     int* n_done);
/* Consecutive calls of a trx_star_enqueue that sit on ONE stream and share N, the time stamps (pointer and length),
 * exptime, nsupersample and the precision flag are enqueued as one LAUNCH CHAIN: every kernel of the path once, with
 * the call / branch as a further grid dimension (up to 16 calls or 24 branches per chain; ~11 launches instead of
 * 9-17 per call, and two more for all the posterior rows of a chain's calls together).  A call with a table
 * (table_rows > 1) is enqueued on its own and splits the chain there; post_rows does not.  Same records and posterior
 * blocks, bit for bit.  The calls of a chain run side by side: `out` (and `post`) of all of them is valid once the
 * stream has passed the call.  (The testing library can switch chains off: trx_debug.h.) */

/* Frees the per-stream scratch described above (every device); all streams must be idle. */
int trx_release_scratch(void);

const char* trx_version(void);
const char* trx_last_error(void);
int trx_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* TRX_H */
