// libtrx.so: the host side of the likelihood path and the C ABI (include/trx.h) for gfx950.
//
// The kernels live in eleven headers that only this file includes:
//   trx_cells.hpp    rowc_kernel (per-row constants, 152 B per row of scratch; the EB rows' secondary-eclipse verdict),
//                    sec_scan_kernel, cells_kernel<MODE, STEP, FP32, LONG, ST, PRUNE, WT> (the light-curve model and its
//                    chi^2: one wavefront per row or per batch of rows, in-window cells filed in LDS, each lane plans a
//                    cell, the (cell, node) pairs dealt to all lanes; centre-value stencil on dense uniform grids; the
//                    passes of the bounded evaluation), pilot_stats_kernel, depth_screen_kernel, and what host and
//                    device share (RowsArgs, batch_rows, batch_plan, set_scratch)
//   trx_reduce.hpp   chi2_grid_kernel, chi2_rows_kernel<STAGE, Terms> (row reductions over a materialised grid; one launcher
//                    here, chi2_rows_launch) and the log-mean-exp kernels, HBM bound
//   trx_scan.hpp     scan_rows_kernel<ONE, Filter> (the row reductions under correlated noise: a scan along the row, what
//                    differs in a Filter; one launcher here, scan_rows_launch) and the pieces its filters and ou_mix_kernel
//                    share
//   trx_noise.hpp    OuFilter (one exponential term; include/trx_noise.h)
//   trx_noise_mix.hpp  ou_mix_kernel<ONE, J> (the same for J candidate noise models in one pass, their soft minimum per
//                    row: a kernel of its own through scan_rows_launch; include/trx_mix.h)
//   trx_softmin.hpp  softmin_rows_kernel<J> (the soft minimum of J candidate values per row, one lane a row;
//                    softmin_launch here; include/trx_shift.h)
//   trx_robust.hpp   chi2_robust_kernel<STAGE> (the outlier-tolerant row reduction: a two-component mixture per point, one
//                    exp and one log1p a value; chi2_robust_launch here; include/trx_robust.h)
//   trx_white_mix.hpp  chi2_white_mix_kernel<STAGE, J> (the weighted row reduction for J candidate white-noise models in
//                    one pass, their soft minimum per row; chi2_white_mix_launch here; include/trx_mix.h)
//   trx_white_lin.hpp  chi2_white_lin_kernel<STAGE, J, K> (white_mix's reduction with K baseline columns marginalised per
//                    candidate, the J (1 + K) sums of a row folded together; chi2_white_lin_launch here; include/trx_gls.h)
//   trx_gls.hpp      OuColsFilter<K> (the OU filter with K baseline columns marginalised under the same noise;
//                    include/trx_gls.h)
//   trx_ss2.hpp      Ss2Filter (noise with a two-dimensional state: 2 x 2 affine maps in the scan; include/trx_ss.h)
//   trx_ss2_cols.hpp Ss2ColsFilter<K> (that filter with K baseline columns marginalised under the same noise, and the
//                    blocks a CU of each instantiation; include/trx_ss.h)
//   (+ trx_device.hpp: the fp64 device math; trx_draw.hip / trx_scenario.hip: the per-draw kernel and the scenario calls)
// Here: the launch plan (plan_cells; probe_pass: what its probe pass changes), the launchers (launch_cells for one call,
// lnl_lme_chain for a chain's branches; launch_cells_kernel is the one place that names cells_kernel instantiations), the
// per-stream scratch and the scratch of captured calls, the node tables, the entry points of include/trx.h and -- testing
// build only -- of include/trx_debug.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/trx.h"
#include "../../include/trx_noise.h"
#include "../../include/trx_mix.h"
#include "../../include/trx_shift.h"
#include "../../include/trx_robust.h"
#include "../../include/trx_gls.h"
#include "../../include/trx_ss.h"
#include "trx_device.hpp"
#include "trx_internal.hpp"
#include "trx_knobs.hpp"

namespace {

using namespace trx;
static_assert(kTwoPiHost == kTwoPi, "lnl_c0 (trx_internal.hpp)");

thread_local char g_err[256] = "";

int fail(int code, const char* fmt, const char* a = "", long b = 0)
{
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return code;
}

#define TRX_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) return fail(TRX_ERR_HIP, "%s (hip error %ld)", hipGetErrorString(e_), (long)e_); \
    } while (0)

}  // namespace

#include "trx_cells.hpp"
#include "trx_reduce.hpp"
#include "trx_scan.hpp"
#include "trx_noise.hpp"
#include "trx_noise_mix.hpp"
#include "trx_softmin.hpp"
#include "trx_robust.hpp"
#include "trx_white_mix.hpp"
#include "trx_gls.hpp"
#include "trx_white_lin.hpp"
#include "trx_ss2.hpp"
#include "trx_ss2_cols.hpp"
#include "trx_bands.hpp"

namespace {

// ---------------------------------------------------------------------------------------
// Tuning and diagnostics switches: trx_knobs.hpp.  Compile-time constants in the production library; process-wide
// atomics with setters (include/trx_debug.h) in the testing build, read once per enqueue.

int n_params(int model)
{
    switch (model) {
        case TRX_MODEL_TP: return TRX_NPARAM_TP;
        case TRX_MODEL_EB:
        case TRX_MODEL_EB_TWIN: return TRX_NPARAM_EB;
        case TRX_MODEL_RAW: return TRX_NPARAM_RAW;
        default: return -1;
    }
}

// Node sets for the exposure average: the n-point GAUSS rule of the discrete measure the reference
// averages over (S equally spaced points, weight 1/S each).  It reproduces the S-point average of
// every polynomial of degree <= 2n-1, so for a model that is analytic over the exposure its error
// falls like rho^(-2n) with the distance to the nearest limb contact -- half the nodes of an
// interpolatory rule of the same accuracy.  Nodes = roots of the degree-n orthogonal polynomial
// of the measure (Stieltjes recurrence, roots by bisection between the roots of degree n-1),
// weights = Christoffel numbers; long double, once per launch.  Radii from the measured error
// decay (profiles/r01/q_tier_error.txt): <= ~2e-14 per tier.
bool compute_tiers(TierTable& T, int S)
{
    static const int nn[kTiers] = {3, 4, 5, 6, 7, 8, 9};
    static const double rad[kTiers] = {60.0, 13.0, 6.0, 3.5, 2.7, 2.1, 1.8};
    typedef long double ld;
    static ld xs[4096];               // callers hold fill_tiers' mutex
    const bool usable = S <= 4096;
    for (int s = 1; usable && s <= S; ++s) xs[s - 1] = ((ld)s - 0.5L) / S - 0.5L;
    // recurrence p_{k+1} = (x - al[k]) p_k - be[k] p_{k-1}, norms h[k] = <p_k, p_k>
    ld al[kTierMaxNodes + 1], be[kTierMaxNodes + 1], h[kTierMaxNodes + 1];
    auto poly = [&](int deg, ld x) -> ld {            // monic orthogonal polynomial of degree deg
        ld pm = 0.0L, p = 1.0L;
        for (int k = 0; k < deg; ++k) {
            const ld pn = (x - al[k]) * p - (k > 0 ? be[k] : 0.0L) * pm;
            pm = p;
            p = pn;
        }
        return p;
    };
    const int nmax = nn[kTiers - 1];
    if (usable) {
        for (int k = 0; k <= nmax && k < S; ++k) {
            ld num = 0.0L, den = 0.0L;
            for (int s = 0; s < S; ++s) {
                const ld p = poly(k, xs[s]);
                num += xs[s] * p * p;
                den += p * p;
            }
            h[k] = den / S;
            al[k] = num / den;
            be[k] = (k > 0) ? h[k] / h[k - 1] : h[0];
        }
    }
    bool any = false;
    for (int q = 0; q < kTiers; ++q) {
        const int n = nn[q];
        T.n[q] = 0;
        T.radius[q] = rad[q];
        for (int j = 0; j < kTierMaxNodes; ++j) T.x[q * kTierMaxNodes + j] = T.w[q * kTierMaxNodes + j] = 0.0;
        if (!usable || 2 * n + 2 > S) continue;       // needs degree 2n-1 well below S
        // roots of p_m interlace those of p_{m-1}: build them degree by degree
        ld roots[kTierMaxNodes + 2], prev[kTierMaxNodes + 2];
        int np_ = 0;
        for (int m = 1; m <= n; ++m) {
            ld edges[kTierMaxNodes + 3];
            edges[0] = -0.5L;
            for (int i = 0; i < np_; ++i) edges[i + 1] = prev[i];
            edges[np_ + 1] = 0.5L;
            for (int i = 0; i < m; ++i) {
                ld lo = edges[i], hi = edges[i + 1];
                const bool up = poly(m, hi) > 0.0L;
                for (int it = 0; it < 200; ++it) {
                    const ld mid = 0.5L * (lo + hi);
                    if ((poly(m, mid) > 0.0L) == up) hi = mid; else lo = mid;
                }
                roots[i] = 0.5L * (lo + hi);
            }
            np_ = m;
            for (int i = 0; i < m; ++i) prev[i] = roots[i];
        }
        ld w[kTierMaxNodes], sum = 0.0L;
        for (int j = 0; j < n; ++j) {
            ld acc = 0.0L;
            for (int k = 0; k < n; ++k) {
                const ld p = poly(k, roots[j]);
                acc += p * p / h[k];
            }
            w[j] = 1.0L / acc;
            sum += w[j];
        }
        for (int j = 0; j < n; ++j) {
            T.x[q * kTierMaxNodes + j] = (double)roots[j];
            T.w[q * kTierMaxNodes + j] = (double)(w[j] / sum);
        }
        T.n[q] = n;
        any = true;
    }
    return any;
}

// The table depends on S only and costs ~0.8 ms of long-double work at S = 20 (as much as a small
// kernel): computed once per S and kept (S = 20, the reference's default, and the few other
// values a process ever uses).  The cache is the library's only state besides the diagnostics
// switches; a mutex makes concurrent first calls safe.
bool fill_tiers(TierTable& T, int S)
{
    constexpr int kSlots = 16;
    static std::mutex mu;
    static int keys[kSlots];
    static bool oks[kSlots];
    static TierTable tabs[kSlots];
    static int used = 0, next = 0;
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < used; ++i)
        if (keys[i] == S) { T = tabs[i]; return oks[i]; }
    const bool ok = compute_tiers(T, S);
    const int slot = (used < kSlots) ? used++ : (next++ % kSlots);
    keys[slot] = S;
    oks[slot] = ok;
    tabs[slot] = T;
    return ok;
}

// The part of the table a kernel takes by value (TierHead) and a device copy of its (node, weight) pairs, one per
// (device, S), uploaded on first use and kept for the life of the process (1.1 KB).  Returns 0, or -1 when HIP fails;
// *usable: S is large enough for at least one tier.
int tier_device(int S, TierHead& head, const double** xw, bool* usable)
{
    TierTable T;
    *usable = fill_tiers(T, S);
    for (int q = 0; q < kTiers; ++q) { head.n[q] = T.n[q]; head.radius[q] = T.radius[q]; }
    static std::mutex mu;
    static std::map<std::pair<int, int>, double*> dev_tabs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    std::lock_guard<std::mutex> lock(mu);
    auto it = dev_tabs.find(std::make_pair(dev, S));
    if (it == dev_tabs.end()) {
        double pairs[2 * kTiers * kTierMaxNodes];
        for (int i = 0; i < kTiers * kTierMaxNodes; ++i) { pairs[2 * i] = T.x[i]; pairs[2 * i + 1] = T.w[i]; }
        // (legal while another stream of this thread is being captured into a graph: nothing here touches that stream)
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        double* p = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), sizeof(pairs));
        if (e == hipSuccess) e = hipMemcpy(p, pairs, sizeof(pairs), hipMemcpyHostToDevice);
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        if (e != hipSuccess) { (void)hipGetLastError(); if (p) (void)hipFree(p); return -1; }
        it = dev_tabs.emplace(std::make_pair(dev, S), p).first;
    }
    *xw = it->second;
    return 0;
}

// ---- stencil memo (see cells_kernel) ------------------------------------------------------
struct StencilMemo {
    static constexpr int kSlots = 256;
    struct Key { const void* time; int n_time, S, dev; double exptime; };
    std::mutex mu;
    int* flags = nullptr;            // pinned, host- and device-visible: 0 unknown, 1 no stencil, 2 stencil
    Key keys[kSlots];
    int used = 0, next = 0;
    // the slot of this light curve (a fresh one starts as unknown), or null if pinned memory is not to be had
    int* slot(const Key& k)
    {
        std::lock_guard<std::mutex> lock(mu);
        if (!flags) {
            if (hipHostMalloc(reinterpret_cast<void**>(&flags), kSlots * sizeof(int),
                              hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
                (void)hipGetLastError();
                flags = nullptr;
                return nullptr;
            }
            for (int i = 0; i < kSlots; ++i) flags[i] = 0;
        }
        for (int i = 0; i < used; ++i)
            if (keys[i].time == k.time && keys[i].n_time == k.n_time && keys[i].S == k.S && keys[i].dev == k.dev &&
                keys[i].exptime == k.exptime)
                return flags + i;
        const int i = (used < kSlots) ? used++ : (next++ % kSlots);
        keys[i] = k;
        flags[i] = 0;
        return flags + i;
    }
};
StencilMemo g_stencil_memo;


// what the last launch_cells of this thread did (trx::lnl_draws hands it to the reduction that follows)
thread_local const double* t_last_rowc = nullptr;
thread_local bool t_last_pruned = false;
// the cost order of this thread's last launch that built one (trx_debug_row_order; the testing build reads it back)
thread_local const int* t_last_order = nullptr;
thread_local long t_last_order_rows = 0;


// THE place that picks a cells_kernel instantiation; these are all there are.  The call site fixes the variant (LONG: one
// row per wave, a workgroup of one wave; ST: the centre-value stencil; PRUNE: the passes of the bounded evaluation; WT: one
// weight per time stamp), the launch chooses among
//   full evaluation, MODE_LNL and MODE_GRID: {no Kepler stepping, stepping fp64, stepping fp32} x {batched, LONG, LONG + ST}
//   PRUNE, MODE_LNL only:                    stepping {fp64, fp32} x {batched, LONG}
//   WT, MODE_LNL only:                       stepping {fp64, fp32} x {batched, LONG, LONG + ST}
template <int MODE, bool LONG, bool ST, bool PRUNE, bool WT>
void launch_cells_kernel(bool step, bool fp32, unsigned grid, size_t lds, hipStream_t st, const RowsArgs& a)
{
    static_assert(MODE == MODE_LNL || !(PRUNE || WT), "PRUNE and WT exist for the likelihood mode only");
    static_assert(!ST || (LONG && !PRUNE), "the stencil: one row per wave, full evaluation");
    static_assert(!(PRUNE && WT), "a weighted launch is evaluated in full");
    const dim3 g(grid), block(LONG ? 64 : 64 * kBatchWaves);
    if constexpr (!PRUNE && !WT) {         // (a full Kepler solve per sub-exposure: testing build's switch, fp64 only)
        if (!step) {
            hipLaunchKernelGGL((cells_kernel<MODE, false, false, LONG, ST, false, false>), g, block, lds, st, a);
            return;
        }
    }
    if (fp32) hipLaunchKernelGGL((cells_kernel<MODE, true, true, LONG, ST, PRUNE, WT>), g, block, lds, st, a);
    else      hipLaunchKernelGGL((cells_kernel<MODE, true, false, LONG, ST, PRUNE, WT>), g, block, lds, st, a);
}

// a pass of the bounded evaluation (launch_cells of MODE_GRID never takes it: plan_cells)
template <int MODE>
void launch_pruned(const RowsArgs& a, hipStream_t st, bool long_rows, bool fp32, unsigned grid, size_t lds)
{
    if constexpr (MODE == MODE_LNL) {
        if (long_rows) launch_cells_kernel<MODE_LNL, true, false, true, false>(true, fp32, grid, lds, st, a);
        else           launch_cells_kernel<MODE_LNL, false, false, true, false>(true, fp32, grid, lds, st, a);
    }
}

// light curves below the packing threshold go through the batched variant: several rows per wave
bool short_rows(int n_time) { return n_time > 0 && n_time < knob_cells_below(); }

// What launch_cells and the chain launcher decide before anything is enqueued: the rows per wave and the LDS layout, the
// node tables, whether the bounded evaluation applies, the grids.
struct CellsPlan {
    bool long_rows, prune, split, fp32, step;
    size_t lds;
    unsigned grid_main;        // cells_kernel: the full evaluation, or the passes behind the pilot
    unsigned grid_pilot;
    unsigned grid_rowc;        // rowc_kernel (+ 1 header workgroup)
    unsigned grid_scan;        // sec_scan_kernel<8>
    unsigned grid_screen;      // depth_screen_kernel
    bool passes;               // prune: there may be rows behind the pilot (pilot_stats_kernel and the later passes run)
    int probe_B;               // split: rows per wave of the probe pass (its own LDS layout: probe_lds, probe_wave_doubles)
    size_t probe_lds;
    int probe_wave_doubles;
};

// The probe pass of a split launch (batches of short light curves; bounded evaluation) evaluates its ~16 cells per row with
// the fp32 flux model whatever the call's precision: a row leaves it abandoned -- reporting a lower bound that allows for
// the model's error, fp32_model_slack in trx_cells.hpp -- or on the survivors' list, and the survivors' pass evaluates
// those again from the start in the call's own precision.  No result of the call carries fp32 arithmetic; what changes
// is which rows are abandoned at the margin (a few more survive).
#ifndef TRX_PROBE_FP32
#define TRX_PROBE_FP32 1
#endif
constexpr bool kProbeFp32 = TRX_PROBE_FP32 != 0;

// LDS of cells_kernel: [node tables | atan constants | tier head] shared by the workgroup's waves (then, short curves,
// the staged light curve), and per wave [rows, accumulators | pair table | in-window list | cell state (| stencil state)]
constexpr size_t cells_tables_bytes()
{
    return (size_t)(2 * kTiers * kTierMaxNodes + kAtanRanges * kAtanCols + kTierHeadDoubles) * sizeof(double);
}
constexpr size_t cells_wave_bytes(int B, bool long_variant)
{
    return (size_t)B * (kRowDoubles + 4) * sizeof(double)
         + (kCellsPairs + cells_window(long_variant)) * sizeof(unsigned short) + sizeof(CellState)
         + (long_variant ? sizeof(StencilState) : 0);
}
// one row per wave: sixteen one-wave workgroups per CU (four waves per SIMD) share its 160 KB
static_assert(cells_tables_bytes() + cells_wave_bytes(1, true) <= 160 * 1024 / 16, "LDS of the one-row workgroup");

template <int MODE>
int plan_cells(RowsArgs& a, bool long_rows, CellsPlan& P)
{
    // rows per wave (batch_rows); with the row count on the device the LDS layout takes the largest value
    a.forced_B = knob_rows_per_wave();
    a.B = long_rows ? 1 : batch_rows(a.n_dev ? -1 : a.n, a.n_time, a.forced_B);
    a.s2 = a.sigma * a.sigma;
    a.rs2 = 1.0 / a.s2;
    a.dS = (double)a.S;
    a.rS = 1.0 / a.dS;
    a.nbatch = 8 * batch_plan(a.n, a.B).P;          // wave positions of the launch (batch_plan)
    a.debug_bug = knob_debug_bug();
    a.whole_trips = knob_whole_trips();
    a.one_sweep = knob_one_sweep();
    a.full_chunks = knob_full_chunks() | (knob_zone_loop() ? 4 : 0);     // (one field for both: zone_loop_on, trx_cells.hpp)
    a.mark_unwritten = (MODE == MODE_LNL && !a.inv_var) ? 1 : 0;     // (a weighted launch may ADD to out[]: never marked)
    bool tiers_ok = false;
    if (tier_device(a.S, a.tiers, &a.tier_xw, &tiers_ok)) return fail(TRX_ERR_HIP, "tier table upload failed%s", "", 0);
    a.use_tiers = tiers_ok && knob_tiers() && !(a.flags & TRX_FLAG_ALL_SUBEXPOSURES);
    // bounded evaluation (trx_scenario_evidence): ~16 probe cells per row; its instantiations carry no stencil
    // (default: light curves of one row per wave only -- measured on calc_probs at N = 1e6: Kepler-10b, 478 points,
    // 46 -> 39 ms; at 100 binned points the batched variant gains or loses ~3 % (the probe phase, the pilot
    // launch and the second window pass eat what the abandoned rows save): profiles/r03/bounded_e2e.txt)
    const int prune_mode = (a.flags & TRX_FLAG_FULL_EVALUATION) ? 0 : (a.prune == 2 ? 2 : knob_bounded());
    // (batched variant: the verdict after the probe phase reads flat + corrections - hrem, and hrem holds only the
    // in-window cells of the window passes done so far -- a valid bound only when the batch's cells fit ONE window;
    // a forced rows-per-wave or a raised trx_set_cell_packing_below can exceed it: those launches evaluate in full)
    const bool prune = MODE == MODE_LNL && a.prune && knob_kepler_stepping() &&
                       (prune_mode == 2 || (prune_mode == 1 && long_rows)) &&
                       (long_rows || (long)a.B * a.n_time <= (long)kCellsWindowBatch) &&
                       a.n_time >= kProbeMinPoints;
    a.prune = prune ? 1 : 0;
    // probe cells per row: every (n_time / kProbeCells)-th stamp (TRX_PROBE_CELLS in the environment: experiments)
    static const int probe_cells = (int)env_long("TRX_PROBE_CELLS", kProbeCells);
    a.pstride = prune ? (a.n_time / probe_cells > 1 ? a.n_time / probe_cells : 2) : 1;
    static const int third_stride = (int)env_long("TRX_THIRD_STRIDE", kThirdStride);
    a.pstride3 = (prune && third_stride > 1 && a.n_time >= 4 * third_stride) ? third_stride : 0;
    a.use_stencil = (!prune && long_rows && a.use_tiers && a.exptime > 0.0 && a.S >= 8 && a.n_time >= 64 &&
                     knob_stencil() && !(a.flags & TRX_FLAG_NO_STENCIL)) ? 1 : 0;
    a.skip_excl = knob_skip_excluded() && !(a.flags & TRX_FLAG_EVALUATE_EXCLUDED);
    a.need_sec = (a.model == TRX_MODEL_EB && MODE == MODE_LNL) ||
                 ((a.model == TRX_MODEL_EB || a.model == TRX_MODEL_EB_TWIN) && a.out_sec != nullptr);
    // (per-point weights: the limit is the caller's; +inf or NaN excludes no depth, so nothing is scanned)
    if (a.inv_var && !(a.sec_limit < INFINITY)) a.need_sec = 0;
    // LDS: [node tables | atan constants | the staged light curve (short curves): time, flux and -- per-point weights --
    // inv_var] shared by the workgroup's waves, then per wave [rows, accumulators | pair table | in-window list | cell
    // state (| stencil state)]
    static_assert((kCellsPairs + kCellsWindowLong) % 4 == 0 && (kCellsPairs + kCellsWindowBatch) % 4 == 0 &&
                  sizeof(CellState) % 8 == 0 && sizeof(StencilState) % 8 == 0, "8-byte alignment of the LDS arrays");
    const size_t tables = cells_tables_bytes();
    auto wave_bytes = [&](bool long_variant) -> size_t { return cells_wave_bytes(a.B, long_variant); };
    a.tl_off = (int)(tables / sizeof(double));
    size_t shared = tables + (long_rows ? 0 : (size_t)(a.inv_var ? 3 : 2) * a.n_time * sizeof(double));
    size_t lds = shared + cells_waves(long_rows) * wave_bytes(long_rows);
    if (lds > 64 * 1024) {             // a long curve forced through the batched variant by a test knob
        long_rows = true;
        a.B = 1;
        a.nbatch = a.n;
        shared = tables;
        lds = shared + wave_bytes(true);
    }
    a.wave_off = (int)(shared / sizeof(double));
    a.wave_doubles = (int)(wave_bytes(long_rows) / sizeof(double));
#ifdef TRX_NO_SPLIT
    const bool split = false;              // (A/B builds: batches probe and finish in one kernel, as in round 3)
#else
    const bool split = prune && !long_rows;
#endif
    a.split = split ? 1 : 0;
    // The probe pass of a split launch looks at ~16 cells of a row: with the 3 rows per wave that 200 points allow the
    // other passes, a batch has ~24 in-window probe cells -- one chunk on a third of its lanes, two trips of pairs two
    // thirds full (SQ_THREAD_CYCLES_VALU: 0.48 of the lanes active over the pass, profiles/r05/pmc_chain.sh).  Only the
    // probe cells are filed, so the pass needs no room for a batch's every cell in the in-window list: it takes as many
    // rows per wave as the LDS of five waves per SIMD has room for row blocks (9 at 200 points, 11 at 100), its "window"
    // is the whole batch, and its chunks and trips fill up.
    P.probe_B = a.B;
    P.probe_lds = lds;
    P.probe_wave_doubles = a.wave_doubles;
    a.probe_rows = 0;
    a.wave_floor = a.wave_floor3 = 3200;
    if (split && knob_probe_rows() != 1) {
        const int forced = knob_probe_rows();
        const int per_row = a.n_time / a.pstride + 1;                      // probe cells of a row
        const size_t fixed = (kCellsPairs + cells_window(false)) * sizeof(unsigned short) + sizeof(CellState);
        const size_t room = (32 * 1024 - shared) / cells_waves(false);       // five workgroups per CU
        int B2 = room > fixed ? (int)((room - fixed) / ((kRowDoubles + 4) * sizeof(double))) : a.B;
        if (forced > 1) B2 = forced;
        if (B2 > kCellsMaxRows) B2 = kCellsMaxRows;
        if (B2 * per_row > cells_window(false)) B2 = cells_window(false) / per_row;
        if ((long)B2 * a.n_time > 65535) B2 = 65535 / a.n_time;               // (list entries are 16-bit cell numbers)
        if (B2 > a.B) {
            P.probe_B = B2;
            P.probe_wave_doubles = (int)(((size_t)B2 * (kRowDoubles + 4) * sizeof(double) + fixed) / sizeof(double));
            P.probe_lds = shared + cells_waves(false) * (size_t)P.probe_wave_doubles * sizeof(double);
        }
    }
    P.long_rows = long_rows;
    P.prune = prune;
    P.split = split;
    P.lds = lds;
    P.fp32 = (a.flags & TRX_FLAG_FP32_MODEL) != 0;
    P.step = knob_kepler_stepping() != 0;
    // Row count on the device: `n` is its upper bound (every draw of the scenario), the geometry mask
    // keeps 2-11 % of them, so the grid takes a quarter of the bound -- blocks
    // beyond the batches leave at once, batches beyond the grid are reached by the grid-stride loop.
    // (a workgroup is cells_waves() waves, each with its own batches; a multiple of 8 workgroups: one per XCD)
    const long max_grid = 1L << 20;
    auto grid_for = [&](long batches, bool long_variant, long cap) -> unsigned {
        if (a.n_dev) {
            batches = (batches + 3) / 4;
            batches = batches < 4096 ? 4096 : batches;
        }
        const long groups = (batches + cells_waves(long_variant) - 1) / cells_waves(long_variant);
        long want = 8 * ((groups + 7) / 8);
        if (cap > 0 && want > cap) want = cap;
        return (unsigned)(want < max_grid ? want : max_grid);
    };
    // Workgroups beyond the batches are not free: ~2.4 ns each to dispatch and leave, and while they are dealt out they
    // hold back the workgroups of the other streams' kernels.  A grid sized for the upper bound of a row count that
    // only the device knows is mostly such workgroups (a quarter of the bound: 10 000 of them per launch at N = 10^6,
    // three launches per call; 250 000 one-wave workgroups with one row per wave).  So the grid is capped and the waves
    // stride over the positions beyond it: one workgroup per slot of the chip (1280) for the passes of the bounded
    // evaluation, four per slot for a full evaluation -- which loses nothing against one workgroup per four batches
    // when a launch runs alone (static striding below that does: +6 % at two per slot, +18 % at one) --, four waves
    // per slot with one row per wave.  Measured in one job each (profiles/r04/ab_cap.txt): 64 TOIs on three streams
    // 0.265 -> 0.185 s per step (four streams 0.175), the 75-scenario calc_probs 22.0 -> 20.4 ms, 15 scenarios
    // 3.8 -> 3.1 ms, Kepler-10b 12.0 -> 10.6 ms.  (Environment: experiments only.)
    static const long cap_probe = env_long("TRX_GRID_CAP", 1280);
    static const long cap_plain = env_long("TRX_GRID_CAP_PLAIN", 5120);
    static const long cap_long = env_long("TRX_GRID_CAP_LONG", 16384);
    const long cap = (a.n_dev || prune) ? (long_rows ? cap_long : (prune ? cap_probe : cap_plain)) : 0;
    P.grid_main = grid_for(long_rows ? a.n : a.nbatch, long_rows, cap);
    {
        // pilot rows (evaluated to the end; first values of the running bounds)
        const long np = a.n < kPilotRows ? a.n : kPilotRows;
        const int pilot_B = kPilotB < a.B ? kPilotB : a.B;
        const long pilot_batches = long_rows ? np : (split ? (np + pilot_B - 1) / pilot_B : (np + a.B - 1) / a.B);   // (split: kPilotB pilot rows per wave)
        const long pilot_groups = (pilot_batches + cells_waves(long_rows) - 1) / cells_waves(long_rows);
        P.grid_pilot = (unsigned)(8 * ((pilot_groups + 7) / 8));
        P.passes = a.n_dev || a.n > kPilotRows;
    }
    {
        // (with the row count on the device the grids are guesses, and a workgroup that finds nothing to do still costs
        // its dispatch: a chain's rowc_kernel_star was 70 000 one-wave workgroups for 15 000 blocks of rows -- capped,
        // the workgroups stride: 149 -> 106 us per chain at 512 per branch (1024: 116, 256: 110, 160: 124).  The scan
        // of the open rows is the opposite case: serial chains of ~1000 fp64 instructions, eight rows a workgroup -- 61 us
        // with the guessed grid, 123 at 512 workgroups a branch, 373 at 128 (profiles/r05/trace_env.sh).  Environment:
        // experiments.)
        static const long rowc_cap = env_long("TRX_ROWC_CAP", 512);
        static const long scan_cap = env_long("TRX_SCAN_CAP", 1L << 30);
        long rb = (a.n + 63) / 64;
        if (a.n_dev) rb = (rb + 3) / 4 < 64 ? 64 : (rb + 3) / 4;      // see grid_for; rowc_kernel strides over the rest
        if (a.n_dev && rb > rowc_cap) rb = rowc_cap;
        P.grid_rowc = (unsigned)rb + 1;
        // every row when the depth is asked for; else the open rows, ~3 % of the rows of a likelihood call (which
        // are themselves ~10 % of `n` when that is only the upper bound): workgroups stride over the list
        long sb = (a.n + 63) / 64;
        if (!a.out_sec && a.n_dev) sb = (sb + 3) / 4;
        if (!a.out_sec && a.n_dev && sb > scan_cap) sb = scan_cap;
        P.grid_scan = (unsigned)(sb < 64 ? 64 : (sb > 8192 ? 8192 : sb));
        // the depth screen of the rows behind the pilot, lanes = rows; what it leaves goes to the probe pass
        long sg = (a.n + kScreenRows - 1) / kScreenRows;
        if (a.n_dev) sg = (sg + 3) / 4;
        P.grid_screen = (unsigned)(sg < 8 ? 8 : (sg > 512 ? 512 : sg));
    }
    return TRX_OK;
}

// Pass `part` of the bounded evaluation as launch_cells and lnl_lme_chain launch it: the arguments, the LDS size and the
// flux model's precision.  They are the launch's own except in the probe pass (part 2) of a split launch: its rows end
// abandoned or on the survivors' list, so it takes the fp32 flux model (kProbeFp32) and, where plan_cells found room for
// more rows per wave, its own LDS layout.
struct ProbePass { RowsArgs a; size_t lds; bool fp32; };
ProbePass probe_pass(const RowsArgs& a, const CellsPlan& P, int part)
{
    ProbePass p{a, P.lds, P.fp32};
    if (part == 2 && P.split) {
        p.fp32 = P.fp32 || kProbeFp32;
        if (P.probe_B > a.B) {
            p.a.B = P.probe_B; p.a.probe_rows = P.probe_B; p.a.wave_doubles = P.probe_wave_doubles;
            p.lds = P.probe_lds;
        }
    }
    return p;
}

// WT: the instantiations with one weight per time stamp (trx_lnl_batch_weighted: a.inv_var, a.sec_limit, a.accumulate)
template <int MODE, bool WT = false>
int launch_cells(const RowsArgs& a0, hipStream_t st, bool long_rows)
{
    trx::StreamLock turn(st);            // rowc_kernel and cells_kernel of one call share the stream's scratch
    RowsArgs a = a0;
    CellsPlan P;
    if (int rc = plan_cells<MODE>(a, long_rows, P)) return rc;
    long_rows = P.long_rows;
    const bool prune = P.prune && !WT, split = P.split, fp32 = P.fp32, step = P.step;      // (a weighted launch: always in full)
    const size_t lds = P.lds;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &capture) != hipSuccess) { (void)hipGetLastError(); capture = hipStreamCaptureStatusNone; }
    const bool capturing = capture == hipStreamCaptureStatusActive;
    int verdict = 0;                       // of an earlier launch on this light curve: 1 no stencil, 2 stencil
    if (a.use_stencil && !capturing) {     // (a captured launch always carries both instantiations)
        int dev = 0;
        TRX_HIP(hipGetDevice(&dev));
        a.memo = g_stencil_memo.slot({a.time, a.n_time, a.S, dev, a.exptime});
        if (a.memo) verdict = *static_cast<volatile int*>(a.memo);
        if (verdict == 1 || verdict == 2) a.use_stencil = 2;
    }
    // the row constants: 152 B per row of the stream's scratch (+ the flat-model chi^2), filled 64 rows
    // per wave.  While the stream is being captured into a hipGraph the scratch is a buffer of its own that the
    // GRAPH owns (trx::capture_scratch: the stream's buffer must not be grown, nor baked into a graph).
    void* scratch = nullptr;
    const size_t launch_doubles = launch_scratch_doubles(a.n, split, a.use_stencil ? a.n_time : 0);
    // Cost-ordered rows (RowsArgs::order): a full evaluation of a likelihood launch at one row per wave whose row count
    // the host knows; the counters and lists sit behind everything else in the call's scratch
    // (a workgroup per row: the grid's 2^20 bounds the launches that are ordered -- beyond it the waves stride, and the
    // tail of a launch of so many rounds over the chip is a smaller share of it anyway)
    const bool ordered = MODE == MODE_LNL && !WT && long_rows && !prune && !a.n_dev && a.n_time > 0 && a.n <= (1L << 20) &&
                         (long)P.grid_main >= a.n && knob_row_order();
    const size_t scratch_bytes = (launch_doubles + (ordered ? order_doubles(a.n) : 0)) * sizeof(double);
#ifdef TRX_CAPTURE_GRAPH_MEM
    // (A/B builds only, profiles/r06/graph_stress.py: rounds 2-5 took a pair of graph memory nodes here)
    if (capturing) TRX_HIP(hipMallocAsync(&scratch, scratch_bytes, st));
#else
    if (capturing) TRX_HIP(trx::capture_scratch(st, scratch_bytes, &scratch));
#endif
    else TRX_HIP(trx::stream_scratch(st, 0, scratch_bytes, &scratch));
    set_scratch(a, static_cast<double*>(scratch));
    if (ordered) {
        // (the counters' place depends on the row count and the scratch holds whatever the stream's last call left:
        // cleared here, 4 KB, before rowc_kernel counts)
        a.order = reinterpret_cast<int*>(static_cast<double*>(scratch) + launch_doubles);
        TRX_HIP(hipMemsetAsync(a.order, 0, order_counter_bytes(), st));
        t_last_order = a.order;
        t_last_order_rows = a.n;
    }
    // From here on a failure may leave the scan's counter non-zero in the stream's scratch (rowc_kernel<true> counts,
    // the cells_kernel behind it resets): cleared on the way out, or the next call's list would start beyond its end
    auto fail_launch = [&](hipError_t e) {
        if (!capturing) (void)hipMemsetAsync(a.scan_count, 0, sizeof(unsigned long long), st);
        return fail(TRX_ERR_HIP, "%s (hip error %ld)", hipGetErrorString(e), (long)e);
    };
    if (a.need_sec) {
        // (the scan's counter is zero in the stream's scratch: cleared at allocation, then by every cells_kernel
        // that follows a scan; a captured call's own buffer holds anything)
        if (capturing) TRX_HIP(hipMemsetAsync(a.scan_count, 0, sizeof(unsigned long long), st));
        if (ordered) hipLaunchKernelGGL((rowc_kernel<true, false, true>), dim3(P.grid_rowc), dim3(64), 0, st, a);
        else         hipLaunchKernelGGL((rowc_kernel<true, WT>), dim3(P.grid_rowc), dim3(64), 0, st, a);
        if (a.out_sec) hipLaunchKernelGGL(sec_scan_kernel<64>, dim3(P.grid_scan), dim3(64), 0, st, a);
        else           hipLaunchKernelGGL((sec_scan_kernel<8, WT>), dim3(P.grid_scan), dim3(64), 0, st, a);
    } else {
        if (ordered) hipLaunchKernelGGL((rowc_kernel<false, false, true>), dim3(P.grid_rowc), dim3(64), 0, st, a);
        else         hipLaunchKernelGGL((rowc_kernel<false, WT>), dim3(P.grid_rowc), dim3(64), 0, st, a);
    }
    const unsigned g2 = P.grid_main;
    t_last_rowc = a.rowc;
    t_last_pruned = prune;
    if (prune) {
        // pilot rows (evaluated to the end; first values of the running bounds), verdict on probing, the rest
        RowsArgs ap = a;
        ap.part = 1;
        launch_pruned<MODE>(ap, st, long_rows, fp32, P.grid_pilot, lds);
        if (P.passes) {
            hipLaunchKernelGGL(pilot_stats_kernel, dim3(1), dim3(256), 0, st, a.out, a.n, a.n_dev, a.rowc, a.surv_count, a.pstride,
                               a.probe_count);
            if (split) hipLaunchKernelGGL(depth_screen_kernel, dim3(P.grid_screen), dim3(256), 0, st, a);
            ap.part = 2;
            const ProbePass probe = probe_pass(ap, P, 2);
            launch_pruned<MODE>(probe.a, st, long_rows, probe.fp32, g2, probe.lds);
            if (split) {
                // batches of short light curves: the launch above was the probe pass; the rows it left alive, compacted
                // across workgroups, are evaluated to the end here
                ap.part = 3;
                launch_pruned<MODE>(ap, st, long_rows, fp32, g2, lds);
            }
        }
    } else if (long_rows) {
        // (WT: full evaluation with Kepler stepping, the production path -- trx_lnl_batch_weighted refuses anything else)
        if (verdict != 2) launch_cells_kernel<MODE, true, false, false, WT>(step, fp32, g2, lds, st, a);
        if (a.use_stencil && verdict != 1) launch_cells_kernel<MODE, true, true, false, WT>(step, fp32, g2, lds, st, a);
    } else {
        launch_cells_kernel<MODE, false, false, false, WT>(step, fp32, g2, lds, st, a);
    }
    const hipError_t launched = hipGetLastError();
#ifdef TRX_CAPTURE_GRAPH_MEM
    if (capturing) TRX_HIP(hipFreeAsync(scratch, st));
#endif
    if (launched != hipSuccess) return fail_launch(launched);
    return TRX_OK;
}

template <int MODE>
int launch_rows(const RowsArgs& a0, hipStream_t st) { return launch_cells<MODE>(a0, st, !short_rows(a0.n_time)); }

int launch_lme(const double* logw, const double* h, const double* lnprior, double c0, long n,
               long n_total, double* out, void* workspace, size_t workspace_bytes, hipStream_t st, int moments = 0)
{
    if (workspace_bytes < trx_workspace_bytes() || !workspace)
        return fail(TRX_ERR_WORKSPACE, "workspace too small%s (need %ld bytes)", "", (long)trx_workspace_bytes());
    const int blocks = lme_blocks(n);
    static_assert(kLmeMaxBlocks == 2048, "lme_blocks");
    double* ws = static_cast<double*>(workspace);
    const uintptr_t al = (uintptr_t)(h ? h : logw) | (uintptr_t)lnprior;
    const int vec_ok = (al % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(lme_partial_kernel<false>, dim3(blocks), dim3(256), 0, st, logw, h, lnprior, c0, n,
                       vec_ok, ws, (const long*)nullptr, (const int*)nullptr, (double*)nullptr, (long*)nullptr,
                       (const double*)nullptr, ScenFinal{});
    TRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(lme_final_kernel, dim3(1), dim3(64), 0, st, ws, blocks, n_total, out, moments);
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int check_rows(int model, const double* time, int n_time, const double* params, long n, int S)
{
    if (n_params(model) < 0) return fail(TRX_ERR_ARG, "unknown model%s %ld", "", (long)model);
    if (n < 0 || n_time < 0) return fail(TRX_ERR_ARG, "negative size%s (n=%ld)", "", n);
    if (S < 1) return fail(TRX_ERR_ARG, "nsupersample must be >= 1%s (got %ld)", "", (long)S);
    if (n > 0 && n_time > 0 && (!time || !params)) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    return TRX_OK;
}

}  // namespace

// ---- per-stream scratch (trx_internal.hpp) ------------------------------------------------
namespace trx {
namespace {
constexpr int kStageRing = 32;           // pinned blocks per stream for small uploads (pinned_stage_begin)
struct ScratchEntry {
    void* p[kScratchSlots] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[kScratchSlots] = {0, 0, 0, 0};
    std::recursive_mutex mu;             // StreamLock: one call at a time enqueues on the stream
    // ring of pinned staging blocks: a block is reused once the event recorded behind its copy has passed
    void* stage[kStageRing] = {};
    size_t stage_cap[kStageRing] = {};
    hipEvent_t stage_ev[kStageRing] = {};
    bool stage_busy[kStageRing] = {};
    int stage_next = 0;
};
std::mutex g_scratch_mu;
std::map<std::pair<int, hipStream_t>, ScratchEntry> g_scratch;      // (node addresses are stable)

ScratchEntry* scratch_entry(hipStream_t st)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; }
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    return &g_scratch[std::make_pair(dev, st)];
}
}  // namespace

StreamLock::StreamLock(hipStream_t st) : mu_(&scratch_entry(st)->mu) { static_cast<std::recursive_mutex*>(mu_)->lock(); }
StreamLock::~StreamLock() { static_cast<std::recursive_mutex*>(mu_)->unlock(); }

hipError_t stream_scratch(hipStream_t st, int slot, size_t bytes, void** out)
{
    ScratchEntry& en = *scratch_entry(st);
    std::lock_guard<std::recursive_mutex> lock(en.mu);
    hipError_t e = hipSuccess;
    if (en.cap[slot] < bytes) {
        // earlier launches on this stream may still read the old buffer
        if (en.p[slot]) {
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            (void)(slot == 3 ? hipHostFree(en.p[slot]) : hipFree(en.p[slot]));
            en.p[slot] = nullptr;
            en.cap[slot] = 0;
        }
        const size_t want = bytes + bytes / 4 + 256;
        e = (slot == 3) ? hipHostMalloc(&en.p[slot], want, hipHostMallocDefault) : hipMalloc(&en.p[slot], want);
        if (e != hipSuccess) return e;
        en.cap[slot] = want;
        if (slot != 3 && (e = hipMemsetAsync(en.p[slot], 0, kScratchZeroed < want ? kScratchZeroed : want, st)) != hipSuccess)
            return e;
    }
    *out = en.p[slot];
    return hipSuccess;
}

// ---- scratch of a call captured into a hipGraph -----------------------------------------------------------------
// Rounds 2-5 took graph memory nodes (hipMallocAsync / hipFreeAsync on the capturing stream).  On this stack (ROCm 7.2,
// gfx950) a replay enqueued behind work still in flight then intermittently runs cells_kernel on row blocks that read as
// ZERO from a 4-KiB page boundary of the node's allocation to its end -- the rows there come back with the flat-model
// chi^2 (profiles/r06/graph_stress_*.txt: 1 replay in ~2000 without a host synchronisation before it, none with one;
// the once-in-twenty-suite-runs failure of test_entry_points_capture_into_a_hip_graph_and_replay).  The runtime maps a
// node's physical memory when the graph is launched, from the host, whatever the GPU is doing.  So a captured call now
// gets a plain hipMalloc'ed buffer of its own -- allocated under the relaxed capture mode, like the node table of
// tier_device -- that belongs to the graph being captured: a hipUserObject retained by that graph hands the buffer back
// to the pool below when the last graph / executable graph that refers to it is destroyed (the callback may not call
// HIP: it only files the buffer), and a later capture takes a filed buffer that is large enough before allocating.
// trx_release_scratch() frees the filed ones.  If the runtime refuses the user object the buffer simply stays with the
// library until trx_release_scratch().
namespace {
struct CaptureBuf {
    void* p;
    size_t bytes;
    int dev;
};
std::mutex g_capture_mu;
std::vector<CaptureBuf*> g_capture_idle;      // handed back by their graphs (or never owned by one): reusable
std::vector<CaptureBuf*> g_capture_orphans;   // the runtime refused the user object: kept until trx_release_scratch()
long g_capture_live = 0;                      // buffers that a graph still owns
void capture_buf_release(void* ud)
{
    std::lock_guard<std::mutex> lock(g_capture_mu);
    g_capture_idle.push_back(static_cast<CaptureBuf*>(ud));
    --g_capture_live;
}
}  // namespace

hipError_t capture_scratch(hipStream_t st, size_t bytes, void** out)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    hipGraph_t graph = nullptr;
    unsigned long long id = 0;
    if ((e = hipStreamGetCaptureInfo_v2(st, &status, &id, &graph, nullptr, nullptr)) != hipSuccess) return e;
    if (status != hipStreamCaptureStatusActive || !graph) return hipErrorStreamCaptureInvalidated;
    CaptureBuf* buf = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_capture_mu);
        size_t best = 0;
        for (size_t i = 0; i < g_capture_idle.size(); ++i) {
            CaptureBuf* c = g_capture_idle[i];
            if (c->dev == dev && c->bytes >= bytes && (!buf || c->bytes < buf->bytes)) { buf = c; best = i; }
        }
        if (buf) g_capture_idle.erase(g_capture_idle.begin() + (long)best);
    }
    if (!buf) {
        // (legal while this thread captures in the global mode: nothing here touches the capturing stream)
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        void* p = nullptr;
        e = hipMalloc(&p, bytes);
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        if (e != hipSuccess) return e;
        buf = new CaptureBuf{p, bytes, dev};
    }
    hipUserObject_t obj = nullptr;
    bool owned = false;
    if (hipUserObjectCreate(&obj, buf, capture_buf_release, 1, hipUserObjectNoDestructorSync) == hipSuccess) {
        {
            std::lock_guard<std::mutex> lock(g_capture_mu);
            ++g_capture_live;
        }
        if (hipGraphRetainUserObject(graph, obj, 1, hipGraphUserObjectMove) == hipSuccess) owned = true;
        else { (void)hipGetLastError(); (void)hipUserObjectRelease(obj, 1); }      // (the callback files the buffer)
    } else {
        (void)hipGetLastError();
    }
    if (!owned) {
        // no owner: the buffer must outlive a graph whose lifetime the library cannot see -- it is kept out of the pool
        // (never reused) until trx_release_scratch()
        std::lock_guard<std::mutex> lock(g_capture_mu);
        for (size_t i = 0; i < g_capture_idle.size(); ++i)
            if (g_capture_idle[i] == buf) { g_capture_idle.erase(g_capture_idle.begin() + (long)i); break; }
        g_capture_orphans.push_back(buf);
    }
    *out = buf->p;
    return hipSuccess;
}

void capture_scratch_stats(long* live, long* idle)
{
    std::lock_guard<std::mutex> lock(g_capture_mu);
    *live = g_capture_live;
    *idle = (long)g_capture_idle.size();
}

hipError_t capture_scratch_release_idle()
{
    std::lock_guard<std::mutex> lock(g_capture_mu);
    int cur = 0;
    hipError_t e = hipGetDevice(&cur);
    if (e != hipSuccess) return e;
    for (CaptureBuf* c : g_capture_idle) {
        (void)hipSetDevice(c->dev);
        (void)hipFree(c->p);
        delete c;
    }
    g_capture_idle.clear();
    for (CaptureBuf* c : g_capture_orphans) {
        (void)hipSetDevice(c->dev);
        (void)hipFree(c->p);
        delete c;
    }
    g_capture_orphans.clear();
    return hipSetDevice(cur);
}

int fail_hip(hipError_t e) { return fail(TRX_ERR_HIP, "%s (hip error %ld)", hipGetErrorString(e), (long)e); }

hipError_t pinned_stage_begin(hipStream_t st, size_t bytes, void** block, void** ticket)
{
    ScratchEntry& en = *scratch_entry(st);
    std::lock_guard<std::recursive_mutex> lock(en.mu);
    const int k = en.stage_next;
    en.stage_next = (k + 1) % kStageRing;
    hipError_t e = hipSuccess;
    if (en.stage_busy[k]) {
        // (32 uploads ahead of the device on this stream: wait for the oldest to have been copied)
        if ((e = hipEventSynchronize(en.stage_ev[k])) != hipSuccess) return e;
        en.stage_busy[k] = false;
    }
    if (en.stage_cap[k] < bytes) {
        if (en.stage[k]) (void)hipHostFree(en.stage[k]);
        en.stage[k] = nullptr;
        en.stage_cap[k] = 0;
        const size_t want = bytes + bytes / 2 + 256;
        if ((e = hipHostMalloc(&en.stage[k], want, hipHostMallocDefault)) != hipSuccess) return e;
        en.stage_cap[k] = want;
    }
    if (!en.stage_ev[k] && (e = hipEventCreateWithFlags(&en.stage_ev[k], hipEventDisableTiming)) != hipSuccess) return e;
    *block = en.stage[k];
    *ticket = reinterpret_cast<void*>((intptr_t)(k + 1));
    return hipSuccess;
}

void pinned_stage_end(hipStream_t st, void* ticket)
{
    ScratchEntry& en = *scratch_entry(st);
    std::lock_guard<std::recursive_mutex> lock(en.mu);
    const int k = (int)(intptr_t)ticket - 1;
    if (k < 0 || k >= kStageRing) return;
    if (hipEventRecord(en.stage_ev[k], st) == hipSuccess) en.stage_busy[k] = true;
    else (void)hipGetLastError();
}

bool lnl_chain_applicable(int flags, int n_time, long N, int S)
{
    if (N < 1 || n_time < 1 || S < 1) return false;
    RowsArgs a{};
    a.model = TRX_MODEL_TP; a.flags = flags; a.n_time = n_time; a.sigma = 1.0; a.n = N; a.S = S; a.exptime = 0.0;
    static const long dummy_n = 0;
    a.n_dev = &dummy_n;              // (never read on the host: "the row count lives on the device")
    a.prune = 1;
    CellsPlan P;
    if (plan_cells<MODE_LNL>(a, !short_rows(n_time), P) != TRX_OK) return false;
    return P.prune && P.step && P.passes;
}

size_t chain_branch_scratch_bytes(long n_upper) { return launch_scratch_doubles(n_upper, true) * sizeof(double); }

// The likelihood and the reduction of every branch of a chain, one launch per stage with the branch as the grid's
// second dimension (trx_internal.hpp).  Returns kChainNotApplicable -- nothing enqueued -- when the launch would not
// take the bounded evaluation's passes (switched off, fewer than 48 points, a batch beyond one window): the caller
// then enqueues the branches one by one.
int lnl_lme_chain(const ChainBranch* br, int nbr, const double* time, int n_time, long N, double exptime, int S,
                  hipStream_t st)
{
    if (!br || nbr < 1 || nbr > kChainMaxBranches) return fail(TRX_ERR_ARG, "lnl_lme_chain: bad branch count%s %ld", "", (long)nbr);
    if (int rc = check_rows(br[0].model, time, n_time, br[0].cols, N, S)) return rc;
    RowsArgs a{};
    a.model = br[0].model; a.flags = br[0].flags; a.time = time; a.flux = br[0].flux; a.n_time = n_time; a.sigma = br[0].sigma;
    a.params = br[0].cols; a.n = N; a.exptime = exptime; a.S = S; a.out = br[0].h;
    a.n_dev = br[0].n_dev; a.src_idx = br[0].src_idx; a.src_stride = N; a.twin_cols = br[0].twin;
    a.dense = 1;
    a.prune = 1;
    CellsPlan P;
    if (int rc = plan_cells<MODE_LNL>(a, !short_rows(n_time), P)) return rc;
    if (!P.prune || !P.step || !P.passes) return kChainNotApplicable;
    BranchTab bt{};
    LmeTab lt{};
    bool any_sec = false;
    for (int i = 0; i < nbr; ++i) {
        const ChainBranch& c = br[i];
        if (c.model == TRX_MODEL_RAW || !c.n_dev || !c.src_idx || !c.h || !c.cols || !c.flux || !c.scratch || !c.scan_count ||
            !c.ws || !c.amin_pv || !c.amin_pi || ((uintptr_t)c.h % 16) != 0 ||
            ((c.flags ^ br[0].flags) & kChainSharedFlags))
            return fail(TRX_ERR_ARG, "lnl_lme_chain: bad argument in branch%s %ld", "", (long)i);
        BranchArgs& b = bt.b[i];
        b.model = c.model; b.flags = c.flags; b.twin_cols = c.twin; b.need_sec = (c.model == TRX_MODEL_EB) ? 1 : 0;
        any_sec = any_sec || b.need_sec;
        b.flux = c.flux; b.sigma = c.sigma; b.s2 = c.sigma * c.sigma; b.rs2 = 1.0 / b.s2;
        b.prune_c0 = lnl_c0(c.lnsigma);
        b.params = c.cols; b.out = c.h; b.n_dev = c.n_dev; b.src_idx = c.src_idx; b.prune_lp = c.lnprior;
        b.scratch = c.scratch; b.scan_count = c.scan_count;
        RowsArgs tmp = a;                       // (where set_scratch puts this branch's row blocks and header)
        set_scratch(tmp, c.scratch);
        LmeBranch& l = lt.b[i];
        l.h = c.h; l.lnprior = c.lnprior; l.c0 = b.prune_c0; l.ws = c.ws; l.n_dev = c.n_dev;
        l.amin_pv = c.amin_pv; l.amin_pi = c.amin_pi; l.bounds_base = tmp.rowc; l.fin = *c.fin;
    }
    const unsigned y = (unsigned)nbr;
    hipLaunchKernelGGL(rowc_kernel_star, dim3(P.grid_rowc, y), dim3(64), 0, st, a, bt);
    if (any_sec) {
        BranchMap map{};
        unsigned n_sec = 0;
        for (int i = 0; i < nbr; ++i)
            if (bt.b[i].need_sec) map.id[n_sec++] = (unsigned char)i;
        hipLaunchKernelGGL(sec_scan_kernel_star, dim3(P.grid_scan, n_sec), dim3(64), 0, st, a, bt, map);
    }
    // (the few-rows rule of the listed passes asks for ~3200 waves a launch: a chain's launch is all its branches'.  The
    // survivors' pass of a 64-target step ran one row per wave in most branches under the per-launch rule -- lanes 0.65
    // active: same job, 0.114 -> 0.107-0.109 s per step with the floor divided; any value from 1 to 300 does the same,
    // profiles/r05/ab_probe_rows.txt.  Environment: experiments.)
    static const int floor_env = (int)env_long("TRX_WAVE_FLOOR", 0);
    static const int floor3_env = (int)env_long("TRX_WAVE_FLOOR3", 0);
    a.wave_floor = floor_env > 0 ? floor_env : (3200 / nbr > 256 ? 3200 / nbr : 256);
    a.wave_floor3 = floor3_env > 0 ? floor3_env : a.wave_floor;
    auto cells = [&](unsigned grid, int part) {
        const ProbePass p = probe_pass(a, P, part);
        if (P.long_rows) {
            if (p.fp32) hipLaunchKernelGGL((cells_kernel_star<true, true>), dim3(grid, y), dim3(64), p.lds, st, p.a, bt, part);
            else        hipLaunchKernelGGL((cells_kernel_star<false, true>), dim3(grid, y), dim3(64), p.lds, st, p.a, bt, part);
        } else {
            if (p.fp32) hipLaunchKernelGGL((cells_kernel_star<true, false>), dim3(grid, y), dim3(64 * kBatchWaves), p.lds, st, p.a, bt, part);
            else        hipLaunchKernelGGL((cells_kernel_star<false, false>), dim3(grid, y), dim3(64 * kBatchWaves), p.lds, st, p.a, bt, part);
        }
    };
    cells(P.grid_pilot, 1);
    hipLaunchKernelGGL(pilot_stats_kernel_star, dim3(1, y), dim3(256), 0, st, a, bt);
    if (P.split) hipLaunchKernelGGL(depth_screen_kernel_star, dim3(P.grid_screen, y), dim3(256), 0, st, a, bt);
    cells(P.grid_main, 2);
    if (P.split) cells(P.grid_main, 3);
    hipLaunchKernelGGL(lme_partial_kernel_star, dim3((unsigned)lme_blocks(N), y), dim3(256), 0, st, lt, N);
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int lnl_draws(int model, int flags, const double* time, const double* flux, int n_time, double sigma,
              const double* cols, long n_upper, const long* n_dev, const int* src_idx, long src_stride,
              int twin, double exptime, int nsupersample, double* out_halfchi2, const double* lnprior,
              double lnsigma, const double** bounds_base, hipStream_t st)
{
    *bounds_base = nullptr;
    if (int rc = check_rows(model, time, n_time, cols, n_upper, nsupersample)) return rc;
    if (model == TRX_MODEL_RAW || !n_dev || !src_idx || !out_halfchi2 || n_upper < 1 || (n_time > 0 && !flux))
        return fail(TRX_ERR_ARG, "lnl_draws: bad argument%s", "", 0);
    RowsArgs a{};
    a.model = model; a.flags = flags; a.time = time; a.flux = flux; a.n_time = n_time; a.sigma = sigma;
    a.params = cols; a.n = n_upper; a.exptime = exptime; a.S = nsupersample; a.out = out_halfchi2;
    a.n_dev = n_dev; a.src_idx = src_idx; a.src_stride = src_stride; a.twin_cols = twin;
    a.dense = 1;              // compact_fill_kernel stored the masked draws' columns and priors densely, in list order
    // the caller keeps only lnZ and the best draw of these rows: bounded evaluation (cells_body, PRUNE)
    a.prune = 1;
    a.prune_c0 = lnl_c0(lnsigma);
    a.prune_lp = lnprior;
    const int rc = launch_rows<MODE_LNL>(a, st);
    if (rc == TRX_OK && t_last_pruned) *bounds_base = t_last_rowc;
    return rc;
}

int lme_draws(const double* halfchi2, const double* lnprior, double lnsigma, long n_upper, const long* n_dev,
              const int* src_idx, double* ws, double* amin_pv, long* amin_pi, const double* bounds_base,
              const ScenFinal& fin, hipStream_t st)
{
    if (!halfchi2 || !n_dev || !src_idx || !ws || !amin_pv || !amin_pi || ((uintptr_t)halfchi2 % 16) != 0)
        return fail(TRX_ERR_ARG, "lme_draws: bad argument%s", "", 0);
    const double c0 = lnl_c0(lnsigma);   // marginal_likelihoods.py:130 etc.
    hipLaunchKernelGGL(lme_partial_kernel<true>, dim3(lme_blocks(n_upper)), dim3(256), 0, st, (const double*)nullptr,
                       halfchi2, lnprior, c0, n_upper, 1, ws, n_dev, src_idx, amin_pv, amin_pi, bounds_base, fin);
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}
}  // namespace trx

namespace {
// One launch of chi2_rows_kernel<STAGE, Terms> (trx_chi2_grid_weighted, _offset, _baseline): STAGE while flux, inv_var
// and the policy's columns fit the LDS budget, and as many blocks as stay resident -- 8 of 256 threads a CU, fewer where
// the staged vectors fill the 160 KB of LDS -- on 256 CUs.
template <class Terms>
void chi2_rows_launch(const double* flux, const double* inv_var, const double* model_grid, int n_time, long n,
                      const double* secdepth, double sec_limit, int accumulate, double* out, const Terms& terms,
                      hipStream_t st)
{
    const bool stage = n_time <= chi2b_stage_max(Terms::kCols);
    const size_t lds = stage ? (2 + Terms::kCols) * (size_t)((n_time + 1) & ~1) * sizeof(double) : 0;
    long per_cu = lds ? (long)((160u * 1024u) / lds) : 8;
    per_cu = per_cu > 8 ? 8 : per_cu;
    long blocks = (n + 3) / 4;
    if (blocks > 256L * per_cu) blocks = 256L * per_cu;
    const auto kernel = stage ? chi2_rows_kernel<true, Terms> : chi2_rows_kernel<false, Terms>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, st, flux, inv_var, model_grid, n_time, n, secdepth,
                       sec_limit, accumulate, out, terms);
}

// One launch of the red-noise row reductions (trxn_chi2_grid_ou, trxs_chi2_grid_ss2, trxg_chi2_grid_ou_baseline,
// trxm_chi2_grid_ou_mix): `one` -- scan_rows_kernel<true, Filter>, ou_mix_kernel<true, J> -- while a row is a single trip
// of kOuTrip stamps, `trips` past that; p: the filter, or ou_mix_kernel's OuMix.  No dynamic LDS, so the registers bound
// what stays resident: blocks_per_cu = 4 blocks of 256 threads a CU at up to 128 VGPRs, 3 at up to 168
// (trxk_chi2_grid_ss2_baseline alone asks for that step), 2 at up to 256 (two waves a SIMD;
// ou_mix_kernel's up to 52 KB of LDS a block fit as well), on 256 CUs.  The rows behind that cap are the second row of a
// wave's pass and its further passes.
template <class P>
using ScanKernel = void (*)(const double*, const double*, int, long, const double*, double, int, double*, P);

template <class P>
void scan_rows_launch(ScanKernel<P> one, ScanKernel<P> trips, const double* flux, const double* model_grid, int n_time,
                      long n, const double* secdepth, double sec_limit, int accumulate, double* out, const P& p,
                      int blocks_per_cu, hipStream_t st)
{
    long blocks = (n + 3) / 4;
    if (blocks > 256L * blocks_per_cu) blocks = 256L * blocks_per_cu;
    hipLaunchKernelGGL(n_time <= kOuTrip ? one : trips, dim3((unsigned)blocks), dim3(256), 0, st, flux, model_grid, n_time,
                       n, secdepth, sec_limit, accumulate, out, p);
}

// f(std::integral_constant<int, N>{}) with N = n, for the instantiations of LO .. HI (the callers have checked the range;
// an n outside it takes HI)
template <int LO, int HI, class F>
void dispatch_int(int n, const F& f)
{
    if constexpr (LO < HI) {
        if (n != LO) return dispatch_int<LO + 1, HI>(n, f);
    }
    f(std::integral_constant<int, LO>{});
}

// The packed upper triangle of the n_terms x n_terms matrix M from the caller's array, and the log-weights of n_cand
// candidates (`what`: the caller's word for one): by value in the kernel arguments, so they are checked on the way.
int pack_minv(const double* minv, int n_terms, Chi2bM& M)
{
    M = Chi2bM{};
    for (int i = 0; i < n_terms * (n_terms + 1) / 2; ++i) {
        if (!(minv[i] - minv[i] == 0.0))                    // (NaN or +-inf)
            return fail(TRX_ERR_ARG, "minv must be finite%s (entry %ld)", "", (long)i);
        M.m[i] = minv[i];
    }
    return TRX_OK;
}

int pack_lnc(const double* lnc, int n_cand, const char* what, Lnc8& c)
{
    c = Lnc8{};
    for (int j = 0; j < n_cand; ++j) {
        if (!(lnc[j] < INFINITY)) return fail(TRX_ERR_ARG, "lnc is NaN or +inf (%s %ld)", what, j);
        c.v[j] = lnc[j];
    }
    return TRX_OK;
}

// One launch of chi2_robust_kernel<STAGE> (trxr_chi2_grid_robust): STAGE while flux and inv_var fit the LDS budget of
// chi2_rows_kernel, and chi2_rows_launch's cap of blocks -- 8 of 256 threads a CU, fewer where the staged vectors fill the
// 160 KB of LDS, on 256 CUs.  The registers decide how many of them are resident at once (six at the 80 VGPRs the kernel
// takes, four at the 128 its test allows); the others wait their turn, which measured faster than a cap of 4 at 100 stamps
// (0.48 - 0.49 against 0.54 ms of a 512 MiB grid) and the same at 2048 (0.35 - 0.36 ms).  The rows behind the cap are the second row of a
// wave's pass and its further passes.
void chi2_robust_launch(const double* flux, const double* inv_var, const double* model_grid, int n_time, long n,
                        const double* secdepth, double sec_limit, int accumulate, double* out, const RobustC& c,
                        hipStream_t st)
{
    const bool stage = n_time <= kChi2wStageMax;
    const size_t lds = stage ? 2 * (size_t)((n_time + 1) & ~1) * sizeof(double) : 0;
    long per_cu = lds ? (long)((160u * 1024u) / lds) : 8;
    per_cu = per_cu > 8 ? 8 : per_cu;
    long blocks = (n + 3) / 4;
    if (blocks > 256L * per_cu) blocks = 256L * per_cu;
    const auto kernel = stage ? chi2_robust_kernel<true> : chi2_robust_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, st, flux, inv_var, model_grid, n_time, n, secdepth,
                       sec_limit, accumulate, out, c);
}

// One launch of chi2_white_mix_kernel<STAGE, J> (trxv_chi2_grid_white_mix), J = n_cand: STAGE while flux and the J weight
// vectors fit the LDS budget of chi2_rows_kernel, and chi2_rows_launch's cap of blocks -- 8 of 256 threads a CU, fewer where
// the staged vectors fill the 160 KB of LDS, on 256 CUs.  The rows behind the cap are the second row of a wave's pass and
// its further passes.
void chi2_white_mix_launch(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                           double sec_limit, int accumulate, double* out, const WhiteMix& mix, int n_cand, hipStream_t st)
{
    dispatch_int<1, kWhiteMixMax>(n_cand, [&](auto j) {
        constexpr int J = decltype(j)::value;
        const bool stage = n_time <= white_stage_max(J);
        const size_t lds = stage ? (1 + J) * (size_t)((n_time + 1) & ~1) * sizeof(double) : 0;
        long per_cu = lds ? (long)((160u * 1024u) / lds) : 8;
        per_cu = per_cu > 8 ? 8 : per_cu;
        long blocks = (n + 3) / 4;
        if (blocks > 256L * per_cu) blocks = 256L * per_cu;
        const auto kernel = stage ? chi2_white_mix_kernel<true, J> : chi2_white_mix_kernel<false, J>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, st, flux, model_grid, n_time, n, secdepth,
                           sec_limit, accumulate, out, mix);
    });
}

// One launch of chi2_white_lin_kernel<STAGE, J, K> (trxb_chi2_grid_white_baseline), J = n_cand, K = n_terms: STAGE while
// flux, the J weight vectors and the K columns fit the LDS budget of chi2_rows_kernel; the candidates' packed A^-1 sit in
// front of them in either case.  The cap of blocks is what is
// resident at once: a block is one wave a SIMD, a SIMD holds 512 / wlin_vgpr_bound(J, K) of them -- 4 up to 24 sums a row,
// 3 up to 35, 2 at 40 --, fewer where the staged vectors fill the 160 KB of LDS, on 256 CUs.  The rows behind the
// cap are a wave's further passes.
void chi2_white_lin_launch(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                           double sec_limit, int accumulate, double* out, const WhiteLin& lin, int n_cand, int n_terms,
                           hipStream_t st)
{
    dispatch_int<1, kWlinMaxCands>(n_cand, [&](auto j) {
        dispatch_int<1, kWlinMaxTerms>(n_terms, [&](auto k) {
            constexpr int J = decltype(j)::value, K = decltype(k)::value;
            const bool stage = n_time <= wlin_stage_max(J, K);
            const size_t lds = (wlin_minv_doubles(J, K) + (stage ? (1 + J + K) * (size_t)((n_time + 1) & ~1) : 0)) * sizeof(double);
            constexpr long by_regs = 512 / wlin_vgpr_bound(J, K);
            long per_cu = (long)((160u * 1024u) / lds);
            per_cu = per_cu > by_regs ? by_regs : per_cu;
            long blocks = (n + 3) / 4;
            if (blocks > 256L * per_cu) blocks = 256L * per_cu;
            const auto kernel = stage ? chi2_white_lin_kernel<true, J, K> : chi2_white_lin_kernel<false, J, K>;
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, st, flux, model_grid, n_time, n, secdepth,
                               sec_limit, accumulate, out, lin);
        });
    });
}

// One launch of softmin_rows_kernel<J> (trxt_softmin_rows), J = n_cand: one lane per row, and as many blocks as the draw
// kernel's cap -- 16 of 256 threads a CU, on 256 CUs; the rows behind that cap are a lane's further trips.
void softmin_launch(const double* cand, long stride, long n, int n_cand, const Lnc8& lnc, int accumulate, double* out,
                    hipStream_t st)
{
    long blocks = (n + 255) / 256;
    if (blocks > 256L * 16) blocks = 256L * 16;
    dispatch_int<1, kSoftminMax>(n_cand, [&](auto j) {
        hipLaunchKernelGGL(softmin_rows_kernel<decltype(j)::value>, dim3((unsigned)blocks), dim3(256), 0, st, cand, stride,
                           n, lnc, accumulate, out);
    });
}
}  // namespace

// =========================================================================================
extern "C" {

int trx_lnl_batch(int model, int flags, const double* time, const double* flux, int n_time,
                  double sigma, const double* params, long n, double exptime, int nsupersample,
                  double* out_halfchi2, void* stream)
{
    if (int rc = check_rows(model, time, n_time, params, n, nsupersample)) return rc;
    if (model == TRX_MODEL_RAW) return fail(TRX_ERR_ARG, "TRX_MODEL_RAW has no likelihood%s", "", 0);
    if (n == 0) return TRX_OK;
    if (!out_halfchi2 || (n_time > 0 && !flux)) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    RowsArgs a{};
    a.model = model; a.flags = flags; a.time = time; a.flux = flux; a.n_time = n_time; a.sigma = sigma;
    a.params = params; a.n = n; a.exptime = exptime; a.S = nsupersample; a.out = out_halfchi2;
    if (knob_bounded_lnl()) { a.prune = 2; a.prune_c0 = 0.0; a.prune_lp = nullptr; }
    return launch_rows<MODE_LNL>(a, static_cast<hipStream_t>(stream));
}

int trx_lnl_batch_weighted(int model, int flags, const double* time, const double* flux, const double* inv_var,
                           int n_time, const double* params, long n, double exptime, int nsupersample,
                           double sec_limit, int accumulate, double* out_halfchi2, void* stream)
{
    if (n_params(model) < 0) return fail(TRX_ERR_ARG, "unknown model%s %ld", "", (long)model);
    if (model == TRX_MODEL_RAW) return fail(TRX_ERR_ARG, "TRX_MODEL_RAW has no likelihood%s", "", 0);
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (nsupersample < 1) return fail(TRX_ERR_ARG, "nsupersample must be >= 1%s (got %ld)", "", (long)nsupersample);
    if (!time || !flux || !inv_var || !params || !out_halfchi2) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (n == 0) return TRX_OK;
    // (the testing build's switch for a full Kepler solve per sub-exposure has no weighted instantiation)
    if (!knob_kepler_stepping()) return fail(TRX_ERR_ARG, "trx_lnl_batch_weighted needs Kepler stepping%s", "", 0);
    RowsArgs a{};
    a.model = model; a.flags = flags | TRX_FLAG_FULL_EVALUATION; a.time = time; a.flux = flux; a.n_time = n_time; a.sigma = 1.0;
    a.params = params; a.n = n; a.exptime = exptime; a.S = nsupersample; a.out = out_halfchi2;
    a.inv_var = inv_var; a.sec_limit = sec_limit; a.accumulate = accumulate ? 1 : 0;
    return launch_cells<MODE_LNL, true>(a, static_cast<hipStream_t>(stream), !short_rows(n_time));
}

int trx_flux_grid(int model, int flags, const double* time, int n_time, const double* params,
                  long n, double exptime, int nsupersample, double* out_flux, double* out_secdepth,
                  void* stream)
{
    if (int rc = check_rows(model, time, n_time, params, n, nsupersample)) return rc;
    if (n == 0) return TRX_OK;
    if (n_time > 0 && !out_flux) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    RowsArgs a{};
    a.model = model; a.flags = flags; a.time = time; a.n_time = n_time; a.sigma = 1.0;
    a.params = params; a.n = n; a.exptime = exptime; a.S = nsupersample; a.out = out_flux; a.out_sec = out_secdepth;
    a.debug_nodes = (knob_debug_nodes() || (flags & TRX_FLAG_COUNT_EVALUATIONS)) ? 1 : 0;
    return launch_rows<MODE_GRID>(a, static_cast<hipStream_t>(stream));
}

int trx_chi2_grid(const double* flux, const double* model_grid, int n_time, long n, double sigma,
                  double* out_halfchi2, void* stream)
{
    if (n < 0 || n_time < 0) return fail(TRX_ERR_ARG, "negative size%s (n=%ld)", "", n);
    if (n == 0) return TRX_OK;
    if (!out_halfchi2 || (n_time > 0 && (!flux || !model_grid))) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    const int vec_ok = (n_time % 2 == 0) && (((uintptr_t)flux | (uintptr_t)model_grid) % 16 == 0);
    long blocks = (n + 3) / 4;
    if (blocks > 256L * 64) blocks = 256L * 64;
    hipLaunchKernelGGL(chi2_grid_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), flux, model_grid, n_time, n, sigma,
                       out_halfchi2, vec_ok);
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trx_chi2_grid_weighted(const double* flux, const double* inv_var, const double* model_grid, int n_time, long n,
                           const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (!flux || !inv_var || !model_grid || !out_halfchi2) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (n == 0) return TRX_OK;
    chi2_rows_launch(flux, inv_var, model_grid, n_time, n, secdepth, sec_limit, accumulate, out_halfchi2, Chi2Plain{},
                     static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trx_chi2_grid_offset(const double* flux, const double* inv_var, const double* model_grid, int n_time, long n,
                         const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2, double sum_w,
                         double prior_prec, double* offset_out, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (!flux || !inv_var || !model_grid || !out_halfchi2) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (!(sum_w > 0.0) || sum_w == INFINITY) return fail(TRX_ERR_ARG, "sum_w must be finite and > 0%s", "", 0);
    if (!(prior_prec >= 0.0)) return fail(TRX_ERR_ARG, "prior_prec must be >= 0 (+inf allowed)%s", "", 0);
    if (n == 0) return TRX_OK;
    chi2_rows_launch(flux, inv_var, model_grid, n_time, n, secdepth, sec_limit, accumulate, out_halfchi2,
                     Chi2Offset{sum_w, prior_prec, offset_out}, static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxn_chi2_grid_ou(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                      double sec_limit, int accumulate, double* out_halfchi2, const double* alpha, const double* beta,
                      const double* omega, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (!flux || !model_grid || !out_halfchi2 || !alpha || !beta || !omega) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (n == 0) return TRX_OK;
    scan_rows_launch(scan_rows_kernel<true, OuFilter>, scan_rows_kernel<false, OuFilter>, flux, model_grid, n_time, n,
                     secdepth, sec_limit, accumulate, out_halfchi2, OuFilter{alpha, beta, omega}, 4,
                     static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxm_chi2_grid_ou_mix(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                          double sec_limit, int accumulate, double* out_halfchi2, const double* alpha, const double* beta,
                          const double* omega, int n_cand, const double* lnc, double* cand_out, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (n_cand < 1 || n_cand > TRXM_MAX_CANDIDATES) return fail(TRX_ERR_ARG, "n_cand outside 1 .. 8%s (n_cand=%ld)", "", n_cand);
    if (!flux || !model_grid || !out_halfchi2 || !alpha || !beta || !omega || !lnc)
        return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    static_assert(TRXM_MAX_CANDIDATES == kOuMixMax, "the header's limit is the kernel's");
    OuMix mix{alpha, beta, omega, {}, cand_out};
    if (int rc = pack_lnc(lnc, n_cand, "candidate", mix.lnc)) return rc;
    if (n == 0) return TRX_OK;
    // (up to J = 2 the kernel stays within 128 VGPRs, as the OU filter's; past that it holds two waves a SIMD)
    dispatch_int<1, kOuMixMax>(n_cand, [&](auto j) {
        constexpr int J = decltype(j)::value;
        scan_rows_launch(ou_mix_kernel<true, J>, ou_mix_kernel<false, J>, flux, model_grid, n_time, n, secdepth, sec_limit,
                         accumulate, out_halfchi2, mix, J <= 2 ? 4 : 2, static_cast<hipStream_t>(stream));
    });
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxv_chi2_grid_white_mix(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                             double sec_limit, int accumulate, double* out_halfchi2, const double* weights, int n_cand,
                             const double* lnc, double* cand_out, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (n_cand < 1 || n_cand > TRXV_MAX_CANDIDATES) return fail(TRX_ERR_ARG, "n_cand outside 1 .. 8%s (n_cand=%ld)", "", n_cand);
    if (!flux || !model_grid || !out_halfchi2 || !weights || !lnc) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    static_assert(TRXV_MAX_CANDIDATES == kWhiteMixMax, "the header's limit is the kernel's");
    WhiteMix mix{weights, {}, cand_out};
    if (int rc = pack_lnc(lnc, n_cand, "candidate", mix.lnc)) return rc;
    if (n == 0) return TRX_OK;
    chi2_white_mix_launch(flux, model_grid, n_time, n, secdepth, sec_limit, accumulate, out_halfchi2, mix, n_cand,
                          static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxg_chi2_grid_ou_baseline(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                               double sec_limit, int accumulate, double* out_halfchi2, const double* alpha,
                               const double* beta, const double* omega, const double* columns, int n_terms,
                               const double* minv, double* coef_out, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (n_terms < 1 || n_terms > TRXG_MAX_TERMS)
        return fail(TRX_ERR_ARG, "n_terms must lie in [1, 4]%s (got %ld)", "", (long)n_terms);
    if (!flux || !model_grid || !out_halfchi2 || !alpha || !beta || !omega || !columns || !minv)
        return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    static_assert(TRXG_MAX_TERMS == kChi2bMaxTerms, "the header's limit is the kernel's");
    Chi2bM M;
    if (int rc = pack_minv(minv, n_terms, M)) return rc;
    if (n == 0) return TRX_OK;
    // (below kGlsWideFrom columns the kernel stays within 128 VGPRs, from there on it would hold two waves a SIMD; as built
    // every K = 1 .. 4 is within 128: trx_gls.hpp)
    dispatch_int<1, kChi2bMaxTerms>(n_terms, [&](auto k) {
        constexpr int K = decltype(k)::value;
        using Filter = OuColsFilter<K>;
        scan_rows_launch(scan_rows_kernel<true, Filter>, scan_rows_kernel<false, Filter>, flux, model_grid, n_time, n,
                         secdepth, sec_limit, accumulate, out_halfchi2,
                         Filter{alpha, beta, omega, columns, {nullptr, M, coef_out}}, K < kGlsWideFrom ? 4 : 2,
                         static_cast<hipStream_t>(stream));
    });
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxb_chi2_grid_white_baseline(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                                  double sec_limit, int accumulate, double* out_halfchi2, const double* weights,
                                  const double* basis, int n_cand, int n_terms, const double* minv, const double* lnc,
                                  double* cand_out, double* coef_out, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (n_cand < 1 || n_cand > TRXB_MAX_CANDIDATES) return fail(TRX_ERR_ARG, "n_cand outside 1 .. 8%s (n_cand=%ld)", "", n_cand);
    if (n_terms < 1 || n_terms > TRXB_MAX_TERMS)
        return fail(TRX_ERR_ARG, "n_terms must lie in [1, 4]%s (got %ld)", "", (long)n_terms);
    if (!flux || !model_grid || !out_halfchi2 || !weights || !basis || !minv || !lnc)
        return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    static_assert(TRXB_MAX_CANDIDATES == kWlinMaxCands && TRXB_MAX_TERMS == kWlinMaxTerms, "the header's limits are the kernel's");
    WhiteLin lin{weights, basis, {}, {}, cand_out, coef_out};
    if (int rc = pack_lnc(lnc, n_cand, "candidate", lin.lnc)) return rc;
    const int packed = n_terms * (n_terms + 1) / 2;
    for (int j = 0; j < n_cand; ++j) {
        Chi2bM M;
        if (int rc = pack_minv(minv + (size_t)j * packed, n_terms, M)) return rc;
        for (int i = 0; i < packed; ++i) lin.minv[j][i] = M.m[i];
    }
    if (n == 0) return TRX_OK;
    chi2_white_lin_launch(flux, model_grid, n_time, n, secdepth, sec_limit, accumulate, out_halfchi2, lin, n_cand, n_terms,
                          static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxs_chi2_grid_ss2(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                       double sec_limit, int accumulate, double* out_halfchi2, const double* A, const double* g,
                       const double* omega, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (!flux || !model_grid || !out_halfchi2 || !A || !g || !omega) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (n == 0) return TRX_OK;
    scan_rows_launch(scan_rows_kernel<true, Ss2Filter>, scan_rows_kernel<false, Ss2Filter>, flux, model_grid, n_time, n,
                     secdepth, sec_limit, accumulate, out_halfchi2, Ss2Filter{A, g, omega}, 4,
                     static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxk_chi2_grid_ss2_baseline(const double* flux, const double* model_grid, int n_time, long n, const double* secdepth,
                                double sec_limit, int accumulate, double* out_halfchi2, const double* A, const double* g,
                                const double* omega, const double* columns, int n_terms, const double* minv,
                                double* coef_out, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (n_terms < 1 || n_terms > TRXK_MAX_TERMS)
        return fail(TRX_ERR_ARG, "n_terms must lie in [1, 4]%s (got %ld)", "", (long)n_terms);
    if (!flux || !model_grid || !out_halfchi2 || !A || !g || !omega || !columns || !minv)
        return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    static_assert(TRXK_MAX_TERMS == kChi2bMaxTerms, "the header's limit is the kernel's");
    Chi2bM M;
    if (int rc = pack_minv(minv, n_terms, M)) return rc;
    if (n == 0) return TRX_OK;
    // (the registers of an instantiation decide how many blocks a CU are resident: kSs2ColsBlocksPerCu, trx_ss2_cols.hpp)
    dispatch_int<1, kChi2bMaxTerms>(n_terms, [&](auto k) {
        constexpr int K = decltype(k)::value;
        using Filter = Ss2ColsFilter<K>;
        scan_rows_launch(scan_rows_kernel<true, Filter>, scan_rows_kernel<false, Filter>, flux, model_grid, n_time, n,
                         secdepth, sec_limit, accumulate, out_halfchi2,
                         Filter{A, g, omega, columns, {nullptr, M, coef_out}}, ss2_cols_blocks_per_cu(n_time <= kOuTrip, K),
                         static_cast<hipStream_t>(stream));
    });
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxt_softmin_rows(const double* cand, long stride, long n, int n_cand, const double* lnc, int accumulate, double* out,
                      void* stream)
{
    if (!cand || !lnc || !out) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (n < 0 || stride < n) return fail(TRX_ERR_ARG, "n < 0 or stride < n%s (n=%ld)", "", n);
    if (n_cand < 1 || n_cand > TRXT_MAX_NODES) return fail(TRX_ERR_ARG, "n_cand outside 1 .. 8%s (n_cand=%ld)", "", n_cand);
    static_assert(TRXT_MAX_NODES == kSoftminMax, "the header's limit is the kernel's");
    Lnc8 c;
    if (int rc = pack_lnc(lnc, n_cand, "node", c)) return rc;
    if (n == 0) return TRX_OK;
    softmin_launch(cand, stride, n, n_cand, c, accumulate, out, static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trxr_chi2_grid_robust(const double* flux, const double* inv_var, const double* model_grid, int n_time, long n,
                          const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2, double c0,
                          double c1, double k2, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (!flux || !inv_var || !model_grid || !out_halfchi2) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (!(c0 >= 0.0) || c0 == INFINITY) return fail(TRX_ERR_ARG, "c0 must be finite and >= 0%s", "", 0);     // (also NaN)
    if (!(c1 - c1 == 0.0)) return fail(TRX_ERR_ARG, "c1 must be finite%s", "", 0);                            // (NaN or +-inf)
    if (!(k2 > 0.0 && k2 < 1.0)) return fail(TRX_ERR_ARG, "k2 must lie in (0, 1)%s", "", 0);
    if (n == 0) return TRX_OK;
    chi2_robust_launch(flux, inv_var, model_grid, n_time, n, secdepth, sec_limit, accumulate, out_halfchi2,
                       RobustC{c0, c1, k2}, static_cast<hipStream_t>(stream));
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trx_chi2_grid_baseline(const double* flux, const double* inv_var, const double* model_grid, int n_time, long n,
                           const double* secdepth, double sec_limit, int accumulate, double* out_halfchi2,
                           const double* wbasis, int n_terms, const double* minv, double* coef_out, void* stream)
{
    if (n < 0 || n_time < 1) return fail(TRX_ERR_ARG, "n < 0 or n_time < 1%s (n=%ld)", "", n);
    if (!flux || !inv_var || !model_grid || !out_halfchi2 || !wbasis || !minv)
        return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (n_terms < 1 || n_terms > kChi2bMaxTerms)
        return fail(TRX_ERR_ARG, "n_terms must lie in [1, 4]%s (got %ld)", "", (long)n_terms);
    Chi2bM M;
    if (int rc = pack_minv(minv, n_terms, M)) return rc;
    if (n == 0) return TRX_OK;
    dispatch_int<1, kChi2bMaxTerms>(n_terms, [&](auto k) {
        chi2_rows_launch(flux, inv_var, model_grid, n_time, n, secdepth, sec_limit, accumulate, out_halfchi2,
                         Chi2Baseline<decltype(k)::value>{wbasis, M, coef_out}, static_cast<hipStream_t>(stream));
    });
    TRX_HIP(hipGetLastError());
    return TRX_OK;
}

int trx_grid_quantiles(const double* grid, long n_grid_rows, int n_cols, const long* rows, const double* scale,
                       long n_rows, const double* q, int n_q, double* out, void* stream)
{
    if (!grid || !q || !out) return fail(TRX_ERR_ARG, "null pointer%s", "", 0);
    if (n_rows < 1 || n_rows > TRX_POST_MAX_ROWS)
        return fail(TRX_ERR_ARG, "n_rows must lie in [1, TRX_POST_MAX_ROWS]%s (got %ld)", "", n_rows);
    if (n_cols < 1 || n_grid_rows < 1) return fail(TRX_ERR_ARG, "empty grid%s (n_cols=%ld)", "", (long)n_cols);
    if (!rows && n_rows > n_grid_rows) return fail(TRX_ERR_ARG, "more rows than the grid holds%s (n_rows=%ld)", "", n_rows);
    if (n_q < 1 || n_q > kBandMaxQ) return fail(TRX_ERR_ARG, "n_q must lie in [1, 16]%s (got %ld)", "", (long)n_q);
    BandArgs a{};
    for (int i = 0; i < n_q; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(TRX_ERR_ARG, "quantile levels must lie in [0, 1]%s (entry %ld)", "", (long)i);
        a.q[i] = q[i];
    }
    a.g = grid; a.n_grid_rows = n_grid_rows; a.n_cols = n_cols; a.rows = rows; a.scale = scale; a.n_rows = (int)n_rows;
    a.n_q = n_q; a.out = out;
    TRX_HIP(band_launch(a, static_cast<hipStream_t>(stream)));
    return TRX_OK;
}

size_t trx_workspace_bytes(void) { return (size_t)kLmeMaxBlocks * kLmePart * sizeof(double); }

int trx_log_mean_exp(const double* logw, long n, long n_total, double* out, void* workspace,
                     size_t workspace_bytes, void* stream)
{
    if (n < 0 || !out || (n > 0 && !logw)) return fail(TRX_ERR_ARG, "bad argument%s", "", 0);
    if (n_total != n)
        return fail(TRX_ERR_NTOTAL, "N_total must equal len(logw)%s (len=%ld)", "", n);
    return launch_lme(logw, nullptr, nullptr, 0.0, n, n_total, out, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream));
}

int trx_lnz_from_halfchi2(const double* halfchi2, const double* lnprior, long n, long n_total,
                          double lnsigma, double* out_lnz, void* workspace,
                          size_t workspace_bytes, void* stream)
{
    if (!out_lnz || n < 0 || (n > 0 && !halfchi2)) return fail(TRX_ERR_ARG, "bad argument%s", "", 0);
    if (n_total < n || n_total < 1) return fail(TRX_ERR_NTOTAL, "n_total must be >= n%s (n=%ld)", "", n);
    const double c0 = lnl_c0(lnsigma);   // marginal_likelihoods.py:130 etc.
    return launch_lme(nullptr, halfchi2, lnprior, c0, n, n_total, out_lnz, workspace,
                      workspace_bytes, static_cast<hipStream_t>(stream));
}

int trx_lnz_moments_from_halfchi2(const double* halfchi2, const double* lnprior, long n, long n_total,
                                  double lnsigma, double* out, void* workspace, size_t workspace_bytes,
                                  void* stream)
{
    if (!out || n < 0 || (n > 0 && !halfchi2)) return fail(TRX_ERR_ARG, "bad argument%s", "", 0);
    if (n_total < n || n_total < 1) return fail(TRX_ERR_NTOTAL, "n_total must be >= n%s (n=%ld)", "", n);
    const double c0 = lnl_c0(lnsigma);   // (the partition and the fold of trx_lnz_from_halfchi2)
    return launch_lme(nullptr, halfchi2, lnprior, c0, n, n_total, out, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream), 1);
}

int trx_lnz_scenario(int model, int flags, const double* time, const double* flux, int n_time,
                     double sigma, const double* params, long n, double exptime, int nsupersample,
                     const double* lnprior, long n_total, double lnsigma, double* out_halfchi2,
                     double* out_lnz, void* workspace, size_t workspace_bytes, void* stream)
{
    if (int rc = trx_lnl_batch(model, flags, time, flux, n_time, sigma, params, n, exptime,
                               nsupersample, out_halfchi2, stream))
        return rc;
    return trx_lnz_from_halfchi2(out_halfchi2, lnprior, n, n_total, lnsigma, out_lnz, workspace,
                                 workspace_bytes, stream);
}

// ---- host-pointer conveniences -----------------------------------------------------------
namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    double* d() { return static_cast<double*>(p); }
};
}  // namespace

int trx_lnl_batch_host(int model, int flags, const double* time, const double* flux, int n_time,
                       double sigma, const double* params, long n, double exptime,
                       int nsupersample, double* out_halfchi2)
{
    if (int rc = check_rows(model, time, n_time, params, n, nsupersample)) return rc;
    if (n == 0) return TRX_OK;
    if (model == TRX_MODEL_RAW) return fail(TRX_ERR_ARG, "TRX_MODEL_RAW has no likelihood%s", "", 0);
    const int np = n_params(model);
    DevBuf dt, df, dp, dout;
    TRX_HIP(dt.alloc(sizeof(double) * n_time));
    TRX_HIP(df.alloc(sizeof(double) * n_time));
    TRX_HIP(dp.alloc(sizeof(double) * np * n));
    TRX_HIP(dout.alloc(sizeof(double) * n));
    TRX_HIP(hipMemcpy(dt.p, time, sizeof(double) * n_time, hipMemcpyHostToDevice));
    TRX_HIP(hipMemcpy(df.p, flux, sizeof(double) * n_time, hipMemcpyHostToDevice));
    TRX_HIP(hipMemcpy(dp.p, params, sizeof(double) * np * n, hipMemcpyHostToDevice));
    if (int rc = trx_lnl_batch(model, flags, dt.d(), df.d(), n_time, sigma, dp.d(), n, exptime,
                               nsupersample, dout.d(), nullptr))
        return rc;
    TRX_HIP(hipMemcpy(out_halfchi2, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return TRX_OK;
}

int trx_flux_grid_host(int model, int flags, const double* time, int n_time, const double* params,
                       long n, double exptime, int nsupersample, double* out_flux,
                       double* out_secdepth)
{
    if (int rc = check_rows(model, time, n_time, params, n, nsupersample)) return rc;
    if (n == 0) return TRX_OK;
    const int np = n_params(model);
    DevBuf dt, dp, dout, dsec;
    TRX_HIP(dt.alloc(sizeof(double) * n_time));
    TRX_HIP(dp.alloc(sizeof(double) * np * n));
    TRX_HIP(dout.alloc(sizeof(double) * n * n_time));
    TRX_HIP(dsec.alloc(sizeof(double) * n));
    TRX_HIP(hipMemcpy(dt.p, time, sizeof(double) * n_time, hipMemcpyHostToDevice));
    TRX_HIP(hipMemcpy(dp.p, params, sizeof(double) * np * n, hipMemcpyHostToDevice));
    TRX_HIP(hipMemset(dsec.p, 0, sizeof(double) * n));
    if (int rc = trx_flux_grid(model, flags, dt.d(), n_time, dp.d(), n, exptime, nsupersample,
                               dout.d(), dsec.d(), nullptr))
        return rc;
    TRX_HIP(hipMemcpy(out_flux, dout.p, sizeof(double) * n * n_time, hipMemcpyDeviceToHost));
    if (out_secdepth) TRX_HIP(hipMemcpy(out_secdepth, dsec.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return TRX_OK;
}

int trx_log_mean_exp_host(const double* logw, long n, long n_total, double* out)
{
    if (n < 0 || !out || (n > 0 && !logw)) return fail(TRX_ERR_ARG, "bad argument%s", "", 0);
    if (n_total != n)
        return fail(TRX_ERR_NTOTAL, "N_total must equal len(logw)%s (len=%ld)", "", n);
    DevBuf dx, dws, dout;
    TRX_HIP(dx.alloc(sizeof(double) * n));
    TRX_HIP(dws.alloc(trx_workspace_bytes()));
    TRX_HIP(dout.alloc(sizeof(double)));
    TRX_HIP(hipMemcpy(dx.p, logw, sizeof(double) * n, hipMemcpyHostToDevice));
    if (int rc = trx_log_mean_exp(dx.d(), n, n_total, dout.d(), dws.p, trx_workspace_bytes(), nullptr))
        return rc;
    TRX_HIP(hipMemcpy(out, dout.p, sizeof(double), hipMemcpyDeviceToHost));
    return TRX_OK;
}

/* statistics (include/trx.h): rows skipped on the current device since the last reset */
static int read_row_stat(int which, unsigned long long* out, int reset)
{
    static unsigned long long host[kStatShards][kStatPad];
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    constexpr size_t slice = sizeof(host);                 // one counter's shards
    TRX_HIP(hipDeviceSynchronize());
    TRX_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_row_stats), slice, (size_t)which * slice));
    if (out) {
        unsigned long long sum = 0;
        for (int i = 0; i < kStatShards; ++i) sum += host[i][0];
        *out = sum;
    }
    if (reset) {
        // only this counter's slice is cleared (a copy of the WHOLE table written back would roll back what kernels of
        // another host thread added to the other counter between the read and the write: advisor, round 4)
        memset(host, 0, slice);
        TRX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_row_stats), host, slice, (size_t)which * slice));
    }
    return TRX_OK;
}

int trx_skipped_rows(unsigned long long* out, int reset) { return read_row_stat(0, out, reset); }

/* statistics (include/trx.h): rows abandoned by the bounded evaluation on the current device since the last reset */
int trx_pruned_rows(unsigned long long* out, int reset) { return read_row_stat(1, out, reset); }

#ifdef TRX_TESTING
// ---- include/trx_debug.h: the testing library only ---------------------------------------------------------
// (tests, host only: no device is touched) the plan the batched cells_kernel deals its rows by -- walks every position
// of the eight XCDs exactly as cells_body does and checks that the batches tile [0, rows) once, in order within an
// XCD, none larger than rows_per_wave; *positions = positions per XCD, *waves_min = the smallest batch met
int trx_debug_batch_plan(long rows, int rows_per_wave, int taper, long* positions, int* rows_min)
{
    if (rows < 0 || rows_per_wave < 1 || rows_per_wave > kCellsMaxRows) return fail(TRX_ERR_ARG, "bad plan request%s (%ld rows)", "", rows);
    const BatchPlan p = batch_plan(rows, rows_per_wave, taper != 0);
    long covered = 0;
    int smallest = rows_per_wave;
    for (long xcd = 0; xcd < 8; ++xcd) {
        long expect = xcd * p.R;                         // an XCD's batches follow one another in its share
        for (long pos = 0; pos < p.P; ++pos) {
            long base;
            int nb;
            batch_at(p, xcd, pos, base, nb);
            if (base >= rows) continue;
            if (rows - base < nb) nb = (int)(rows - base);
            if (nb < 1 || nb > rows_per_wave || base != expect)
                return fail(TRX_ERR_ARG, "batch plan broken%s (at row %ld)", "", base);
            expect = base + nb;
            covered += nb;
            if (nb < smallest) smallest = nb;
        }
        const long share_end = (xcd + 1) * p.R < rows ? (xcd + 1) * p.R : rows;
        if (xcd * p.R < rows && expect != share_end) return fail(TRX_ERR_ARG, "batch plan leaves rows out%s (after row %ld)", "", expect);
    }
    if (covered != rows) return fail(TRX_ERR_ARG, "batch plan covers the wrong number of rows%s (%ld)", "", covered);
    if (positions) *positions = p.P;
    if (rows_min) *rows_min = smallest;
    return TRX_OK;
}

int trx_set_rows_per_wave(int rows)
{
    if (rows < 0 || rows > kCellsMaxRows)
        return fail(TRX_ERR_ARG, "rows per wave must be 0 (automatic) .. 22%s (got %ld)", "", (long)rows);
    g_knob_rows_per_wave = rows;
    return TRX_OK;
}

/* diagnostics (include/trx.h): light curves with fewer points than this are processed in batches of rows per wave */
int trx_set_cell_packing_below(int n_time)
{
    if (n_time < 0) return fail(TRX_ERR_ARG, "n_time threshold must be >= 0%s (got %ld)", "", (long)n_time);
    g_knob_cells_below = n_time;
    return TRX_OK;
}

/* diagnostics (include/trx.h): 0 = evaluate the light curve of every row, also of those the EB rule excludes */
int trx_set_skip_excluded(int on)
{
    g_knob_skip_excluded = on ? 1 : 0;
    return TRX_OK;
}

/* diagnostics (include/trx.h): 0 = trx_scenario_evidence evaluates every masked draw to the end */
int trx_set_bounded_evaluation(int mode)
{
    if (mode < 0 || mode > 2) return fail(TRX_ERR_ARG, "bounded evaluation mode must be 0, 1 or 2%s (got %ld)", "", (long)mode);
    g_knob_bounded = mode;
    return TRX_OK;
}

/* tests (include/trx.h): trx_lnl_batch / trx_lnz_scenario evaluate their rows the bounded way, too */
int trx_set_debug_bug(int on)
{
    g_knob_debug_bug = on ? 1 : 0;
    return TRX_OK;
}

/* tests, A/B runs (include/trx.h): rows per wave of the probe pass of a split launch */
int trx_set_probe_rows(int rows)
{
    if (rows < 0 || rows > kCellsMaxRows) return fail(TRX_ERR_ARG, "probe rows must be 0 (automatic) .. 22%s (got %ld)", "", (long)rows);
    g_knob_probe_rows = rows;
    return TRX_OK;
}

int trx_set_debug_bounded_lnl(int on)
{
    g_knob_bounded_lnl = on ? 1 : 0;
    return TRX_OK;
}

/* diagnostics (include/trx.h): 0 = Gauss nodes everywhere, no centre-value stencil */
int trx_set_stencil(int on)
{
    g_knob_stencil = on ? 1 : 0;
    return TRX_OK;
}

/* diagnostics (include/trx.h): 0 = full Kepler solve per sub-exposure */
int trx_set_kepler_stepping(int on)
{
    g_knob_kepler_stepping = on ? 1 : 0;
    return TRX_OK;
}

/* diagnostics (include/trx.h): 0 = evaluate all S sub-exposures of every cell */
int trx_set_supersample_tiers(int on)
{
    g_knob_tiers = on ? 1 : 0;
    return TRX_OK;
}

/* diagnostics (include/trx.h): trx_flux_grid writes the number of model
   evaluations planned for each cell (0, a reduced node count, or nsupersample) instead of the flux */
int trx_set_debug_node_counts(int on)
{
    g_knob_debug_nodes = on ? 1 : 0;
    return TRX_OK;
}

/* (tests) 0: one row per wave takes its rows as they come, not dearest first */
int trx_set_row_order(int on)
{
    g_knob_row_order = on ? 1 : 0;
    return TRX_OK;
}

/* (tests) 0: pass 1 of the stencil instantiation tests every cell of a walked trip */
int trx_set_whole_trips(int on)
{
    g_knob_whole_trips = on ? 1 : 0;
    return TRX_OK;
}

/* (tests) 0: the one-row likelihood kernels take their contact cells in a second sweep; 2: one sweep in the flux grid too */
int trx_set_one_sweep(int mode)
{
    if (mode < 0 || mode > 2) return fail(TRX_ERR_ARG, "trx_set_one_sweep: mode must be 0, 1 or 2%s (got %ld)", "", (long)mode);
    g_knob_one_sweep = mode;
    return TRX_OK;
}

/* (tests) 0: the one-row likelihood kernels keep the stencil's one-sided halo (56 new cells per chunk); 2: full chunks in
   the flux grid too, where it takes the one sweep (trx_set_one_sweep(2)) */
int trx_set_full_chunks(int mode)
{
    if (mode < 0 || mode > 2) return fail(TRX_ERR_ARG, "trx_set_full_chunks: mode must be 0, 1 or 2%s (got %ld)", "", (long)mode);
    g_knob_full_chunks = mode;
    return TRX_OK;
}

/* (tests) 0: every chunk of the full chunks takes the chunk loop's body, the ones inside a stencil zone too */
int trx_set_zone_loop(int on)
{
    g_knob_zone_loop = on ? 1 : 0;
    return TRX_OK;
}

/* (tests) the pass-2 chunks the zone loop took on the current device since the last reset */
int trx_debug_zone_chunks(long* chunks, int reset)
{
    static unsigned long long host[kStatShards][kStatPad];
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    TRX_HIP(hipDeviceSynchronize());
    TRX_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_zone_stats), sizeof(host), 0));
    long sum = 0;
    for (int i = 0; i < kStatShards; ++i) sum += (long)host[i][0];
    if (chunks) *chunks = sum;
    if (reset) {
        memset(host, 0, sizeof(host));
        TRX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_zone_stats), host, sizeof(host), 0));
    }
    return TRX_OK;
}

/* (tests) the LDS a workgroup of the one-row cells_kernel is launched with, as plan_cells computes it */
long trx_debug_cells_lds_one_row(void)
{
    return (long)(cells_tables_bytes() + cells_wave_bytes(1, true));
}

/* (tests) the pass-1 trips filed whole / walked cell by cell on the current device since the last reset */
int trx_debug_whole_trips(long* whole, long* walked, int reset)
{
    static unsigned long long host[2][kStatShards][kStatPad];
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    TRX_HIP(hipDeviceSynchronize());
    TRX_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_trip_stats), sizeof(host), 0));
    long sum[2] = {0, 0};
    for (int w = 0; w < 2; ++w)
        for (int i = 0; i < kStatShards; ++i) sum[w] += (long)host[w][i][0];
    if (whole) *whole = sum[0];
    if (walked) *walked = sum[1];
    if (reset) {
        memset(host, 0, sizeof(host));
        TRX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_trip_stats), host, sizeof(host), 0));
    }
    return TRX_OK;
}

/* (tests) the cost order the last likelihood launch of this thread built, and the row blocks it was built from */
int trx_debug_row_order(long* n_rows, long* segment_capacity, int* counts, int* lists, double* row_blocks)
{
    if (!t_last_order || !t_last_rowc) return fail(TRX_ERR_ARG, "trx_debug_row_order: no ordered launch yet%s", "", 0);
    const long n = t_last_order_rows, cap = order_cap(n);
    if (n_rows) *n_rows = n;
    if (segment_capacity) *segment_capacity = cap;
    if (!counts && !lists && !row_blocks) return TRX_OK;
    TRX_HIP(hipDeviceSynchronize());
    if (counts) {
        std::vector<int> raw((size_t)kOrderSegs * kOrderStride);
        TRX_HIP(hipMemcpy(raw.data(), t_last_order, raw.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int sgm = 0; sgm < kOrderSegs; ++sgm) counts[sgm] = raw[(size_t)sgm * kOrderStride];
    }
    if (lists)
        TRX_HIP(hipMemcpy(lists, t_last_order + kOrderSegs * kOrderStride, (size_t)kOrderSegs * cap * sizeof(int), hipMemcpyDeviceToHost));
    if (row_blocks)
        TRX_HIP(hipMemcpy(row_blocks, t_last_rowc, (size_t)n * kRowDoubles * sizeof(double), hipMemcpyDeviceToHost));
    return TRX_OK;
}

/* (tests) scratch buffers of captured calls: how many a live graph still owns, how many wait in the pool for reuse */
int trx_debug_capture_buffers(long* live, long* idle)
{
    long a = 0, b = 0;
    trx::capture_scratch_stats(&a, &b);
    if (live) *live = a;
    if (idle) *idle = b;
    return TRX_OK;
}

#endif  // TRX_TESTING

#ifdef TRX_CENSUS
int trx_debug_census(unsigned long long* out32, int reset)
{
    TRX_HIP(hipDeviceSynchronize());
    if (out32) TRX_HIP(hipMemcpyFromSymbol(out32, HIP_SYMBOL(trx::g_census), 32 * sizeof(unsigned long long)));
    if (reset) {
        static const unsigned long long zeros[32] = {};
        TRX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(trx::g_census), zeros, sizeof(zeros)));
    }
    return TRX_OK;
}
#endif

#ifdef TRX_PHASE_TIMERS
/* debug builds only: read (and clear) the phase cycle counters */
int trx_debug_phase_cycles(unsigned long long* out8)
{
    TRX_HIP(hipDeviceSynchronize());
    TRX_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_phase_cycles), 8 * sizeof(unsigned long long)));
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    TRX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), zero, sizeof(zero)));
    return TRX_OK;
}
#endif

#ifdef TRX_TAIL_TIMERS
/* debug builds only: read (and clear) the tail timers of the one-row kernels run since the last call -- out4: earliest
   start, latest start, latest finish, sum of (finish - start), in ticks of the device's wall clock; finish[n]: the
   finish of the waves at the first n positions (n <= 131072; may be NULL) */
int trx_debug_tail(unsigned long long* out4, unsigned long long* finish, long n)
{
    TRX_HIP(hipDeviceSynchronize());
    if (n < 0 || n > kTailWaves) return fail(TRX_ERR_ARG, "trx_debug_tail: n out of range%s (n=%ld)", "", n);
    if (out4) TRX_HIP(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_tail), 4 * sizeof(unsigned long long)));
    if (finish && n > 0) TRX_HIP(hipMemcpyFromSymbol(finish, HIP_SYMBOL(g_tail_finish), (size_t)n * sizeof(unsigned long long)));
    const unsigned long long fresh[4] = {~0ull, 0ull, 0ull, 0ull};
    TRX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_tail), fresh, sizeof(fresh)));
    return TRX_OK;
}
#endif

/* frees every per-stream scratch buffer of the library (all devices); the streams must be idle */
int trx_release_scratch(void)
{
    std::lock_guard<std::mutex> lock(trx::g_scratch_mu);
    int cur = 0;
    TRX_HIP(hipGetDevice(&cur));
    for (auto& kv : trx::g_scratch) {
        TRX_HIP(hipSetDevice(kv.first.first));
        for (int sl = 0; sl < trx::kScratchSlots; ++sl)
            if (kv.second.p[sl]) (void)(sl == 3 ? hipHostFree(kv.second.p[sl]) : hipFree(kv.second.p[sl]));
        for (int k = 0; k < trx::kStageRing; ++k) {
            if (kv.second.stage[k]) (void)hipHostFree(kv.second.stage[k]);
            if (kv.second.stage_ev[k]) (void)hipEventDestroy(kv.second.stage_ev[k]);
        }
    }
    trx::g_scratch.clear();
    TRX_HIP(hipSetDevice(cur));
    TRX_HIP(trx::capture_scratch_release_idle());
    return TRX_OK;
}

const char* trx_version(void) { return "triceratops_amd libtrx 0.2.0 (gfx950)"; }
const char* trx_last_error(void) { return g_err; }

int trx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
