/*
 * trx_debug.h -- switches and probes of the TESTING build of libtrx (libtrx_testing.so: the sources of libtrx.so
 * compiled with -DTRX_TESTING by __graft_entry__.build()).
 *
 * NOT part of the production ABI: libtrx.so exports none of these symbols, reads nothing from the environment and
 * has no process-wide mutable state (include/trx.h, Conventions).  Everything here is process-wide: a switch flipped
 * by one host thread changes what another thread's in-flight call enqueues.  That is acceptable for tests/ and the
 * A/B scripts under profiles/, which use them to force a code path -- a number of rows per wave, the one-row kernel on
 * a short light curve, a re-enabled bug for the "never written" guard -- and for nothing else.  With every switch at
 * its default the testing library enqueues exactly what the production library does.
 *
 * Environment variables (testing build only; read once): TRX_PROBE_ROWS, TRX_BOUNDED, TRX_STAR_CHAIN give three of
 * the switches below their initial value; TRX_PROBE_CELLS, TRX_THIRD_STRIDE, TRX_GRID_CAP, TRX_GRID_CAP_PLAIN,
 * TRX_GRID_CAP_LONG, TRX_ROWC_CAP, TRX_SCAN_CAP, TRX_WAVE_FLOOR, TRX_WAVE_FLOOR3, TRX_CHAIN_DRAWS override launch
 * geometry constants (experiments; the values the production library has compiled in are the measured best).
 */
#ifndef TRX_DEBUG_H
#define TRX_DEBUG_H

#include "trx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows staged per wavefront of the batched kernel (light curves below trx_set_cell_packing_below's threshold),
 * 1..22; 0 = automatic (default) */
int trx_set_rows_per_wave(int rows);
/* light curves with fewer than n points (default 320) are processed in batches of rows per wave, longer ones one row
 * per wave; 0 = never.  Model values agree to rounding between the two; chi^2 differs by summation order. */
int trx_set_cell_packing_below(int n_time);
/* (host only, touches no device) checks the plan by which the batched likelihood kernel deals `rows` rows to its
 * waves at `rows_per_wave` rows each -- tapered towards the end of the launch when `taper` is set --: every row in
 * exactly one batch.  *positions: wave positions per XCD; *rows_min: the smallest batch. */
int trx_debug_batch_plan(long rows, int rows_per_wave, int taper, long* positions, int* rows_min);

/* process-wide forms of TRX_FLAG_ALL_SUBEXPOSURES (0), TRX_FLAG_NO_STENCIL (0), TRX_FLAG_EVALUATE_EXCLUDED (0),
 * TRX_FLAG_COUNT_EVALUATIONS (1); defaults 1 / 1 / 1 / 0 */
int trx_set_supersample_tiers(int on);
int trx_set_stencil(int on);
int trx_set_skip_excluded(int on);
int trx_set_debug_node_counts(int on);
/* 0 = a full Kepler solve at every node instead of Newton steps from the exposure centre's solution (default 1) */
int trx_set_kepler_stepping(int on);

/* bounded evaluation of the scenario entry points: 0 = never (TRX_FLAG_FULL_EVALUATION for every call), 1 = light
 * curves of one row per wave only, 2 = always (default) */
int trx_set_bounded_evaluation(int mode);
/* 1: trx_lnl_batch / trx_lnz_scenario treat their rows the bounded way too, as for an evidence without prior: a row
 * then holds its chi^2/2 or, if abandoned, a lower bound of it that exceeds the call's smallest by more than 90 */
int trx_set_debug_bounded_lnl(int on);
/* 1: trx_scenario_enqueue / trx_star_enqueue zero the chi^2 arrays of a call before its likelihood kernels run, so
 * that a row no kernel writes shows as a perfect fit instead of as whatever the stream's previous call left there */
int trx_set_debug_poison(int on);
/* 1: re-enables a bug of round 4 (the third pass of the bounded evaluation skipped its last batches when nothing was
 * probed), so that a test can show the "never written" status of the record catching it */
int trx_set_debug_bug(int on);
/* rows per wave of the probe pass of the bounded evaluation of batched light curves: 0 = as many as its LDS layout
 * holds (default), 1 = as many as the other passes take, n > 1 = n (at most 22).  Results do not depend on it. */
int trx_set_probe_rows(int rows);
/* 0: trx_star_enqueue enqueues its calls one by one instead of in launch chains (same records, bit for bit) */
int trx_set_star_chain(int on);
/* 0: a likelihood launch of one row per wave hands its rows to the waves as they come instead of dearest first
 * (default 1).  No output depends on it, bit for bit: a row is evaluated by its own wave from its own block. */
int trx_set_row_order(int on);
/* The cost order of the last likelihood launch of this thread that built one (it waits for the device): *n_rows its
 * rows, *segment_capacity the entries a segment's list can hold; counts[64]: the rows filed in segment s = 4 bucket +
 * shard, bucket 0 the dearest of 16; lists[64 * capacity]: the row numbers of segment s in its first counts[s] entries
 * from s * capacity on; row_blocks[19 * n_rows]: the rows' constant blocks as the kernels read them (t0 and nmot are
 * doubles 1 and 2 of a block, the window doubles 10 and 11, the secondary rule's verdict double 18).  Array pointers may be NULL;
 * called with all of them NULL it tells the sizes.  TRX_ERR_ARG when there has been no such launch. */
int trx_debug_row_order(long* n_rows, long* segment_capacity, int* counts, int* lists, double* row_blocks);
/* 0: pass 1 of the stencil instantiation of the one-row kernel tests every cell of a walked 64-cell trip instead of
 * filing the trips that lie wholly inside a transit window as they stand (default 1).  No output depends on it, bit
 * for bit: the in-window list holds the same cells in the same order. */
int trx_set_whole_trips(int on);
/* How the one-row kernels of the full evaluation (with and without the stencil) take the cells next to a limb contact:
 * 1 (default, what the production library does): the likelihood kernels evaluate them in the chunk that planned them,
 * the flux grid files them for a second sweep over the in-window list, as the bounded and the batched kernels do;
 * 0: the likelihood kernels take the second sweep too; 2: the flux grid and its evaluation census take the one sweep
 * too.  The evaluations per cell do not depend on it; a contact cell's value and chi^2/2 may move in the last bits (its
 * centre solution comes from another plan trip, and its chi^2 term is added by another lane).  TRX_ERR_ARG for another
 * value. */
int trx_set_one_sweep(int mode);
/* How the stencil instantiation of the one-row kernels chunks the in-window list where it takes the one sweep:
 * 1 (default, what the production library does): a chunk of the likelihood kernels takes 64 new list entries; a stencil
 * cell of its last 8 lanes is finalised by the next chunk, which owes it the centre values of its first cells.  The flux
 * grid keeps the one-sided halo (56 new cells per chunk, the last 8 lanes lent), as the bounded and batched kernels do;
 * 0: the likelihood kernels keep the halo too; 2: the flux grid and its evaluation census take full chunks too (only
 * together with trx_set_one_sweep(2)).  A cell's value and chi^2/2 may move in the last bits (other trip-mates in the plan,
 * another lane and order for its chi^2 term); a cell within 8 lanes of a chunk edge may change between the stencil and
 * its own nodes.  TRX_ERR_ARG for another value. */
int trx_set_full_chunks(int mode);
/* bytes of LDS a workgroup of the one-row kernels (one wave) is launched with, from the function the launch plan uses;
 * sixteen of them have to fit a CU's 160 KB.  No device is touched. */
long trx_debug_cells_lds_one_row(void);
/* the 64-cell trips of pass 1 that the stencil instantiation's waves on the current device filed whole and those they
 * walked cell by cell since the library was loaded (or since the last call with reset != 0, which returns the counts and
 * then zeroes them); the trips that cannot hold an in-window cell are in neither.  It waits for the device.  Device
 * counters of the testing library; they cannot change a result.  Either pointer may be NULL. */
int trx_debug_whole_trips(long* whole, long* walked, int reset);
/* 0: with full chunks (trx_set_full_chunks) every chunk of pass 2 runs the stencil tests of the chunk loop's body; 1
 * (default, what the production library does): a chunk in the interior of a row's stencil zone -- 64 consecutive cells
 * in step with the list before and behind them, every one planned for the stencil on the disc, the previous chunk's last
 * 8 cells pending -- skips the stencil tests, whose outcome is known for it, and goes on with the centre values and the
 * finalisation of the same body.  No output depends on it, bit for bit: the same terms in the same lanes and order. */
int trx_set_zone_loop(int on);
/* the chunks of pass 2 that skipped the stencil tests in this way on the current device since the library was loaded (or since the last call
 * with reset != 0, which returns the count and then zeroes it).  It waits for the device.  A device counter of the testing
 * library; it cannot change a result.  The pointer may be NULL. */
int trx_debug_zone_chunks(long* chunks, int reset);
/* what trx_star_enqueue has put into launch chains since the library was loaded (or since the last call with
 * reset != 0, which returns the counts and then zeroes them): chains, the calls in them, and those of these calls that
 * had post_rows > 0.  Host counters; they cannot change a result.  Any pointer may be NULL. */
int trx_debug_chain_counts(long* chains, long* calls_in_chains, long* posterior_calls_in_chains, int reset);

/* The selection stage of ONE branch of a scenario call on the caller's numbers: exactly what trx_scenario_enqueue runs
 * behind the branch's likelihood kernels -- lme_partial_kernel<SCEN> with the branch's final stage (the evidence, the
 * best draw and its columns, the masked count, the tie count, the status, the moments, the largest log-weight for the
 * posterior resampler), then, for K > 1, table_kernel -- with the arguments a real call builds, on the stream's scenario
 * scratch behind its persistent block, which is left at zero.  No kernel of its own; it waits for the stream.
 *   halfchi2   DEVICE [n], chi^2/2 of the masked draws in list order; 16-byte aligned (TRX_ERR_ARG otherwise)
 *   lnprior    DEVICE [N] or NULL, stored densely like the columns: row r at r, with twin != 0 at N - 1 - r
 *   cols       DEVICE [ncol][N], the masked draws' columns, stored the same way
 *   cols_pad   DEVICE [ncol][max(K, 1)]: the stand-in draws 0 .. K - 1 (the record of a branch without rows, the table's
 *              spare rows)
 *   n, N       the masked count -- handed to the kernels through a `long` on the device, as in a real call -- and the
 *              draws the launch is sized for (n_upper = N: the blocks beyond lme_blocks(n) exist and leave);
 *              N >= max(n, K, 1)
 *   n_total    the divisor of the evidence (>= 1); ncol 11 or 14; twin 0 / 1 (ScenFinal.branch, TableArgs.branch)
 *   K          0: no table, or 2 .. TRX_TABLE_MAX_ROWS; moments 0 / 1: a record of TRX_SCENARIO_OUT /
 *              TRX_SCENARIO_OUT_MOMENTS doubles
 *   out_record   HOST, the branch record (include/trx.h); slots no kernel writes read 0x7f7f7f7f7f7f7f7f (1.38e306)
 *   out_post_x   HOST [1], the largest log-weight the final stage leaves in the scratch
 *   out_table    HOST [TRX_TABLE_BRANCH(K)] (K > 1; else may be NULL)
 * No bounded evaluation (no row-constant header: the -90 floor is not applied). */
int trx_debug_select_from_halfchi2(const double* halfchi2, const double* lnprior, const double* cols,
                                   const double* cols_pad, long n, long N, long n_total, int ncol, int twin, int K,
                                   int moments, double lnsigma, double* out_record, double* out_post_x,
                                   double* out_table, void* stream);

/* scratch buffers of calls captured into hipGraphs: how many a live graph still owns, how many wait in the library's
 * pool for reuse (trx_release_scratch frees those) */
int trx_debug_capture_buffers(long* live, long* idle);

#ifdef __cplusplus
}
#endif
#endif /* TRX_DEBUG_H */
