// trx_scenario_evidence / trx_scenario_enqueue / trx_star_enqueue (include/trx.h): one lnZ_* call of calc_probs, end
// to end on the device, with no host synchronisation inside the call.
//
// Round 2's version strung the call together from 12 (planet) or 23 (binary) launches and synchronised the stream
// twice: the number of draws that pass the geometry mask sized the likelihood launch, so the host had to read it.
// Here the count never leaves the device:
//   draw_kernel          the geometry mask(s) of every draw (trx_draw.hip: what does not feed a mask is not computed,
//                        no column is written); workgroup b takes draws [b per, (b + 1) per) and leaves its mask counts
//   compact_fill_kernel  ordered compaction of the mask(s) -- a workgroup sums the counts of the workgroups before it
//                        and appends the indices of its own masked draws, ascending (the order numpy's / torch's
//                        nonzero gives) -> idx[branch][], n[branch] -- and, in the same kernel, the parameter columns
//                        and the prior of those draws (the 5-10 % that passed), recomputed from the same counter-based
//                        random numbers and stored DENSELY, in list order (branch 0 from position 0 up, the twin branch
//                        from position N - 1 down: a draw passes at most one of the two masks)
//   rowc_kernel          } the likelihood of the masked draws: coalesced reads of those dense columns; the row count
//   (sec_scan_kernel)    } is read from n[branch] on the device and the grids are sized for a guess
//   cells_kernel         } (trx_cells.hpp)
//   lme_partial_kernel   first pass of the log-mean-exp and of the search for the smallest chi^2 in one pass; the block
//                        that finishes LAST folds the partials into the record: the evidence, the best draw (first of
//                        equals, NaN first: numpy's / torch's argmin), its columns, the masked count and the
//                        limb-darkening flag (scenario_final, trx_device.hpp), written straight into the caller's
//                        pinned record
// (with the bounded evaluation cells_kernel is up to five launches: pilot rows, pilot_stats_kernel, depth_screen_kernel,
// probe pass, the rows left alive -- trx_cells.hpp)
// 5 launches for a planet scenario (7 in round 3), 9 for a binary one (two branches; 10), no memset, no copy, NO
// sync: a caller can enqueue every lnZ_* call of a calc_probs on a few streams and wait once (trx_scenario_enqueue);
// trx_scenario_evidence is the same followed by one hipStreamSynchronize.  Every buffer lives in the stream's scratch
// (trx_internal.hpp), behind a small persistent block (the finished-block counter of the last stage, the draw
// kernel's flag) that the kernels leave at zero.  Results are bit for bit those of the torch-operator chain of
// fused.py (same arithmetic on the same rows in the same order).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "../../include/trx.h"
#include "../../include/trx_warp.h"
#include "trx_device.hpp"
#include "trx_internal.hpp"
#include "trx_knobs.hpp"
#include "trx_posterior.hpp"
#include "trx_warp.hpp"

namespace {

#define TRXS_HIP(call)                                   \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) return trx::fail_hip(e_);  \
    } while (0)

// bump allocator over one of the stream's scratch buffers (trx_internal.hpp): sizes first, then pointers
struct Arena {
    size_t used = 0;
    char* base = nullptr;
    size_t reserve(size_t bytes)
    {
        const size_t at = used;
        used += (bytes + 255) & ~(size_t)255;
        return at;
    }
    template <class T>
    T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

constexpr int kLmeParts = 2048;            // lme_blocks() never exceeds it

// ---------------------------------------------------------------------------------------------------------------
// The reference's table of the K best draws of a branch (marginal_likelihoods.py:152-171): the masked draws with the K
// smallest chi^2 (NaN last; exact ties: the earlier draw first), in that order, and the columns gathered at them.
// Not a hot path -- calc_probs keeps the best draw only, which the reduction's final stage already finds -- but what a
// caller of lnZ_* itself gets back, and until round 6 only the torch-operator chain could produce it (torch.topk).
// ONE workgroup streams the branch's chi^2 values through LDS, 2048 - 128 new ones at a time next to the 128 best so
// far, and sorts the 2048 (bitonic, (value, row) keys) whenever a new one can enter the best 128; then thread j
// gathers row j's columns -- or, past the masked count, the columns of draw j - count from the stand-in block
// compact_fill_kernel filled (the reference's table then holds draws of log-likelihood -inf in argsort's order of
// equals; the operator chain pads with draws 0, 1, 2 ...: so does this).
constexpr int kTableKeep = 128, kTableTile = 2048;
static_assert(TRX_TABLE_MAX_ROWS + 1 <= kTableKeep, "one more than the table's rows is kept (the caller's tie check)");
struct TableArgs {
    const double* h;          // chi^2/2 of the masked draws, in list order
    const long* n_dev;        // their number
    const double* cols;       // [ncol][N], dense (row r at position r; the twin branch: N - 1 - r)
    const double* cols_pad;   // [ncol][K]: draws 0 .. K - 1
    long N;
    int ncol, branch, K;
    double* table;            // this branch's TRX_TABLE_BRANCH(K) doubles
};

__device__ __forceinline__ bool table_before(double a, int ia, double b, int ib)
{
    const bool na = a != a, nb = b != b;
    if (na != nb) return nb;                 // NaN last (numpy's argsort, torch.topk(largest=False))
    if (!na && a != b) return a < b;
    return ia < ib;
}

__global__ __launch_bounds__(256) void table_kernel(TableArgs t)
{
    __shared__ double val[kTableTile];
    __shared__ int row[kTableTile];
    __shared__ int any_new;
    const long n = *t.n_dev;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < kTableKeep; i += 256) { val[i] = NAN; row[i] = 0x7fffffff; }      // (sorts behind every real entry)
    __syncthreads();
    for (long base = 0; base < n || base == 0; base += kTableTile - kTableKeep) {
        if (tid == 0) any_new = 0;
        __syncthreads();
        const double worst = val[kTableKeep - 1];
        const int wrow = row[kTableKeep - 1];
        bool mine = false;
        for (int i = kTableKeep + tid; i < kTableTile; i += 256) {
            const long r = base + (i - kTableKeep);
            const bool in = r < n;
            const double v = in ? t.h[r] : NAN;
            val[i] = v;
            row[i] = in ? (int)r : 0x7fffffff;
            mine = mine || (in && table_before(v, (int)r, worst, wrow));
        }
        if (mine) any_new = 1;
        __syncthreads();
        if (any_new) {
            for (int k = 2; k <= kTableTile; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < kTableTile; i += 256) {
                        const int p = i ^ j;
                        if (p > i) {
                            const bool up = (i & k) == 0;
                            const double a = val[i], b = val[p];
                            const int ia = row[i], ib = row[p];
                            if (table_before(b, ib, a, ia) == up) { val[i] = b; row[i] = ib; val[p] = a; row[p] = ia; }
                        }
                    }
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        if (n == 0) break;
    }
    const int K = t.K;
    if (tid <= K) {
        const bool real = row[tid] != 0x7fffffff;
        // the K + 1 smallest values (NaN where there is no such draw)
        t.table[14 * (K + 1) + tid] = real ? val[tid] : NAN;
        if (tid < K) {
            const long r = row[tid];
            const long pos = t.branch ? t.N - 1 - r : r;
            const long pad = ((long)tid - n) % (t.N > 0 ? t.N : 1);           // draw index of a spare row (tid >= n there)
            for (int c = 0; c < t.ncol; ++c)
                t.table[c * (K + 1) + tid] = real ? t.cols[(long)c * t.N + pos] : t.cols_pad[(long)c * K + (pad < K ? pad : 0)];
        }
    }
}

// doubles per branch record: TRX_SCENARIO_OUT, or TRX_SCENARIO_OUT_MOMENTS with TRX_FLAG_WEIGHT_MOMENTS
int record_stride(int flags) { return (flags & TRX_FLAG_WEIGHT_MOMENTS) ? TRX_SCENARIO_OUT_MOMENTS : TRX_SCENARIO_OUT; }

// ---------------------------------------------------------------------------------------------------------------
// ONE description of an lnZ_* call for both ways of enqueueing it -- enqueue(): the call alone; enqueue_chain(): up to 16
// calls in one launch chain -- so that a chained call IS a single call: its argument check (check_call), its buffers
// (CallLayout::reserve), a branch's ScenFinal / PostArgs / WarpHistArgs (branch_final / branch_post / branch_hist) and
// the copies back to the caller (copy_back) are written here, once.  What differs between the two is BranchPlace.

// The device's view of a caller's buffer, or null when the device cannot write there: the result then goes through the
// arena and a copy.  Pinned host memory (hipHostMalloc / torch pin_memory) is mapped into the device's address space.
enum class Dest { kPinnedHost, kHostOrDevice };
double* device_view(const void* p, Dest rule)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.devicePointer &&
        (attr.type == hipMemoryTypeHost || (rule == Dest::kHostOrDevice && attr.type == hipMemoryTypeDevice)))
        return static_cast<double*>(attr.devicePointer);
    (void)hipGetLastError();
    return nullptr;
}

// a table of the K best draws (include/trx.h): every masked draw evaluated to the end, K stand-in draws
int table_rows(const trx_scenario_args& s) { return s.table_rows > 1 ? s.table_rows : 0; }

int check_call(const trx_scenario_args& s)
{
    const long N = s.draw->N;
    if (N < 1 || N > 0x7fffffffL) return TRX_ERR_ARG;
    const int K = table_rows(s);
    if (K > TRX_TABLE_MAX_ROWS || (K && !s.table)) return TRX_ERR_ARG;
    // posterior rows (include/trx.h): M draws per branch in proportion to their weight, selected behind the evidence
    const int M = s.post_rows;
    if (M < 0 || M > TRX_POST_MAX_ROWS || (M && !s.post)) return TRX_ERR_ARG;
    // a weight histogram (include/trx.h): behind the evidence, like the posterior rows; the kernel's own uniforms only
    if (s.warp_hist && !s.draw->use_philox) return TRX_ERR_ARG;
    return TRX_OK;
}

struct Call;
// a call's buffers in an arena (offsets): 146 N bytes of draw-side buffers, the reductions' workspaces, and staging for
// the record, the posterior block and the table where the device cannot write the caller's
struct CallLayout {
    size_t cols, cols0, mask, mask2, prior, n, res, ws, pv, pi, idx[2], h[2], post, table;
    void reserve(Arena& A, const Call& c);
};

struct Call {
    const trx_scenario_args* s;
    double* out;                              // the caller's record
    long N;
    int planet, ncol, nbr, K, M, H, n_pad, want_prior, stride;
    double *rec_dev, *post_dev, *table_dev;   // the device's view of the caller's record / posterior block / table, or null
    CallLayout at;
    const Arena* A;                           // where `at` counts from (once the arena has its memory)

    Call(const trx_scenario_args& s_, double* out_) : s(&s_), out(out_), N(s_.draw->N), A(nullptr)
    {
        planet = s_.draw->planet != 0; ncol = planet ? 11 : 14; nbr = planet ? 1 : 2;
        K = table_rows(s_); M = s_.post_rows; H = s_.warp_hist != nullptr; n_pad = K ? K : 1;
        // a call with an importance map: its prior column carries ln J, whatever the scenario's prior
        want_prior = (s_.want_prior || s_.draw->warp) ? 1 : 0;
        stride = record_stride(s_.flags);         // (per call: a chain may mix calls with and without moments)
        rec_dev = device_view(out_, Dest::kPinnedHost);
        post_dev = M ? device_view(s_.post, Dest::kHostOrDevice) : nullptr;
        table_dev = K ? device_view(s_.table, Dest::kHostOrDevice) : nullptr;
    }
    Call() = default;

    double* cols() const { return A->at<double>(at.cols); }
    double* cols0() const { return A->at<double>(at.cols0); }
    double* lnprior() const { return want_prior ? A->at<double>(at.prior) : nullptr; }
    long* n_dev(int b) const { return A->at<long>(at.n) + b; }
    int* idx(int b) const { return (b && planet) ? nullptr : A->at<int>(at.idx[b]); }
    double* h(int b) const { return (b && planet) ? nullptr : A->at<double>(at.h[b]); }
    double* ws(int b) const { return A->at<double>(at.ws) + (size_t)b * trx::kLmePart * kLmeParts; }
    double* pv(int b) const { return A->at<double>(at.pv) + (size_t)b * kLmeParts; }
    long* pi(int b) const { return A->at<long>(at.pi) + (size_t)b * 2 * kLmeParts; }
    // where the device writes the record / a branch's posterior block / a branch's table: the caller's buffer if it can
    double* res() const { return rec_dev ? rec_dev : A->at<double>(at.res); }
    double* post(int b) const { return (post_dev ? post_dev : A->at<double>(at.post)) + (size_t)b * TRX_POST_BRANCH(M); }
    double* table(int b) const { return (table_dev ? table_dev : A->at<double>(at.table)) + (size_t)b * TRX_TABLE_BRANCH(K); }
    int model(int b) const { return planet ? TRX_MODEL_TP : (b ? TRX_MODEL_EB_TWIN : TRX_MODEL_EB); }

    // the caller's draw arguments with the outputs pointed at this call's buffers; state: the first branch's state word
    // (its word 1 is the draw kernel's flag -- zero between calls: the last branch's final stage clears it)
    trx_draw_args draw_args(unsigned* state) const
    {
        trx_draw_args d = *s->draw;
        d.cols = cols(); d.lnprior = lnprior(); d.dump = nullptr;
        d.mask = A->at<unsigned char>(at.mask);
        d.mask_twin = planet ? nullptr : A->at<unsigned char>(at.mask2);
        d.flag = reinterpret_cast<int*>(state + 1);
        return d;
    }
};

void CallLayout::reserve(Arena& A, const Call& c)
{
    const size_t N = (size_t)c.N, twin = c.planet ? 0 : N;
    cols = A.reserve(sizeof(double) * c.ncol * N);
    cols0 = A.reserve(sizeof(double) * 16 * c.n_pad);
    mask = A.reserve(N);
    mask2 = A.reserve(twin);
    prior = A.reserve(c.want_prior ? sizeof(double) * N : 0);
    n = A.reserve(2 * sizeof(long));
    res = A.reserve(sizeof(double) * (2 * TRX_SCENARIO_OUT_MOMENTS + 1));
    ws = A.reserve(sizeof(double) * 2 * trx::kLmePart * kLmeParts);
    pv = A.reserve(sizeof(double) * 2 * kLmeParts);
    pi = A.reserve(sizeof(long) * 2 * 2 * kLmeParts);
    idx[0] = A.reserve(sizeof(int) * N);
    idx[1] = A.reserve(sizeof(int) * twin);
    h[0] = A.reserve(sizeof(double) * N);              // (256-byte steps: lme_draws / lnl_lme_chain ask for 16)
    h[1] = A.reserve(sizeof(double) * twin);
    post = A.reserve((c.M && !c.post_dev) ? sizeof(double) * 2 * TRX_POST_BRANCH(c.M) : 0);
    table = A.reserve((c.K && !c.table_dev) ? sizeof(double) * 2 * TRX_TABLE_BRANCH(c.K) : 0);
}

// What the branches of an arena share out among themselves, in branch order: kPostWsBytes of tile sums for each branch
// with posterior rows, and for each branch with a weight histogram its block -- side by side: one memset -- and a place
// for X, the largest log-weight, which a branch with posterior rows keeps in its tile workspace instead
struct SharedLayout {
    size_t post_ws, hist, hist_x;
    static size_t hist_bytes(int n_hist) { return sizeof(unsigned long long) * TRX_WARP_BRANCH * (size_t)n_hist; }
    void reserve(Arena& A, int n_post, int n_hist)
    {
        post_ws = A.reserve(trx::kPostWsBytes * (size_t)n_post);
        hist = A.reserve(hist_bytes(n_hist));
        hist_x = A.reserve(sizeof(double) * (size_t)n_hist);
    }
};

// What differs between a branch of a single call and a branch in a chain
struct BranchPlace {
    unsigned* state;              // the branch's state word: the arena's zeroed head / the branch's kBranchHead slot
    int cols0_stride;             // of the stand-in columns: n_pad / 1
    char* post_ws;                // the branch's posterior workspace (SharedLayout), or null: no posterior rows
    double* hist_x;               // the branch's place for X without posterior rows, or null: no histogram
    unsigned long long* hist;     // the branch's histogram block, or null
    // the final stage leaves the branch's largest log-weight here, the posterior and histogram kernels read it
    double* post_x() const
    {
        return post_ws ? reinterpret_cast<double*>(post_ws + trx::kPostWsSums + trx::kPostWsCounts) : hist_x;
    }
};

BranchPlace branch_place(const Call& c, const Arena& A, const SharedLayout& sh, unsigned* state, int cols0_stride, int p_at,
                         int h_at)
{
    BranchPlace at{state, cols0_stride, nullptr, nullptr, nullptr};
    if (c.M) at.post_ws = A.at<char>(sh.post_ws) + trx::kPostWsBytes * (size_t)p_at;
    if (c.H) {
        at.hist_x = A.at<double>(sh.hist_x) + h_at;
        at.hist = A.at<unsigned long long>(sh.hist) + (size_t)h_at * TRX_WARP_BRANCH;
    }
    return at;
}

trx::ScenFinal branch_final(const Call& c, int b, const BranchPlace& at)
{
    trx::ScenFinal f{};
    f.idx = c.idx(b); f.cols = c.cols(); f.cols0 = c.cols0(); f.cols0_stride = at.cols0_stride; f.dense = 1;
    f.N = c.N; f.n_total = c.N; f.ncol = c.ncol; f.branch = b; f.last_branch = (b == c.nbr - 1) ? 1 : 0;
    f.stride = c.stride;
    f.res = c.res() + (size_t)b * c.stride;
    f.flag_out = (b == 0) ? c.res() + 2 * c.stride : nullptr;
    f.state = at.state;
    f.post_x = at.post_x();
    return f;
}

// the weights are the evidence's own (its largest log-weight is in the scratch: post_x); rows the bounded evaluation
// abandoned report a bound more than 90 below it and fall to the cut at -80.  The seed and the Philox counter are the
// call's own (post_seed, the branch WITHIN the call), so a block does not depend on the chain it was drawn in.
trx::PostArgs branch_post(const Call& c, int b, const BranchPlace& at)
{
    trx::PostArgs p{};
    p.h = c.h(b); p.lnprior = c.lnprior(); p.n_dev = c.n_dev(b); p.n = c.N; p.N = c.N; p.twin = b;
    p.c0 = trx::lnl_c0(c.s->lnsigma);
    p.M = c.M; p.branch = b; p.seed = c.s->post_seed;
    p.xmax = at.post_x();
    p.tile_q = reinterpret_cast<trx::u128*>(at.post_ws);
    p.tile_cnt = reinterpret_cast<long*>(at.post_ws + trx::kPostWsSums);
    p.cols = c.cols(); p.ncol = c.ncol;
    p.block = c.post(b);
    return p;
}

trx::WarpHistArgs branch_hist(const Call& c, int b, const BranchPlace& at)
{
    trx::WarpHistArgs w{};
    w.h = c.h(b); w.lnprior = c.lnprior(); w.n_dev = c.n_dev(b); w.idx = c.idx(b); w.N = c.N; w.twin = b;
    w.slots = trx::warp_consumed_slots(*c.s->draw);
    w.c0 = trx::lnl_c0(c.s->lnsigma);
    w.seed = c.s->draw->seed;
    w.xmax = at.post_x();
    w.out = at.hist;
    return w;
}

// behind the call's kernels: what the device could not write into the caller's memory; hist: the call's first block
int copy_back(const Call& c, const unsigned long long* hist, hipStream_t st)
{
    const trx_scenario_args& s = *c.s;
    if (c.H)
        TRXS_HIP(hipMemcpyAsync(s.warp_hist, hist, sizeof(unsigned long long) * (size_t)c.nbr * TRX_WARP_BRANCH, hipMemcpyDefault, st));
    if (c.M && !c.post_dev)
        TRXS_HIP(hipMemcpyAsync(s.post, c.post(0), sizeof(double) * (size_t)c.nbr * TRX_POST_BRANCH(c.M), hipMemcpyDefault, st));
    if (c.K && !c.table_dev)
        TRXS_HIP(hipMemcpyAsync(s.table, c.table(0), sizeof(double) * (size_t)c.nbr * TRX_TABLE_BRANCH(c.K), hipMemcpyDefault, st));
    if (!c.rec_dev)
        TRXS_HIP(hipMemcpyAsync(c.out, c.res(), sizeof(double) * (2 * c.stride + 1), hipMemcpyDeviceToHost, st));
    return TRX_OK;
}

int enqueue(const trx_scenario_args* s, double* out_host, hipStream_t st)
{
    if (int rc = check_call(*s)) return rc;
    trx::StreamLock turn(st);              // the whole call is enqueued back to back on the stream's scratch
    Call c(*s, out_host);
    const long N = c.N;
    const int flags = s->flags | (c.K ? TRX_FLAG_FULL_EVALUATION : 0);
    const int n_post = c.M ? c.nbr : 0, n_hist = c.H ? c.nbr : 0;

    Arena A;
    const size_t o_state = A.reserve(trx::kScratchZeroed);     // persistent: finished-block counter, the draw kernel's flag
    const size_t o_cnt = A.reserve(sizeof(int) * 2 * trx::kDrawMaxGroups);
    c.at.reserve(A, c);
    SharedLayout sh;
    sh.reserve(A, n_post, n_hist);
    TRXS_HIP(trx::stream_scratch(st, 1, A.used, reinterpret_cast<void**>(&A.base)));
    c.A = &A;
    unsigned* state = A.at<unsigned>(o_state);
    const trx_draw_args d = c.draw_args(state);
    long per = 0;
    int groups = 0;
    if (int rc = trx::draw_counted(d, A.at<int>(o_cnt), &per, &groups, st)) return rc;
    // from here on a failure leaves kernels enqueued that may have touched the persistent block: cleared on the way out
    auto bail = [&](int rc) {
        (void)hipMemsetAsync(state, 0, trx::kScratchZeroed, st);
        return rc;
    };
    if (int rc = trx::compact_fill(d, per, groups, A.at<int>(o_cnt), c.idx(0), c.idx(1), c.n_dev(0), c.cols0(), st, c.n_pad))
        return bail(rc);
    if (trx::knob_poison())          // tests: an unwritten row must show (include/trx_debug.h)
        for (int b = 0; b < c.nbr; ++b) TRXS_HIP(hipMemsetAsync(c.h(b), 0, sizeof(double) * (size_t)N, st));
    if (n_hist) TRXS_HIP(hipMemsetAsync(A.at<char>(sh.hist), 0, SharedLayout::hist_bytes(n_hist), st));
    for (int b = 0; b < c.nbr; ++b) {
        const BranchPlace at = branch_place(c, A, sh, state, c.n_pad, b, b);
        const double* bounds = nullptr;
        if (int rc = trx::lnl_draws(c.model(b), flags, s->time, s->flux, s->n_time, s->sigma, d.cols, N, c.n_dev(b), c.idx(b), N,
                                    b, s->exptime, s->nsupersample, c.h(b), d.lnprior, s->lnsigma, &bounds, st))
            return bail(rc);
        if (int rc = trx::lme_draws(c.h(b), d.lnprior, s->lnsigma, N, c.n_dev(b), c.idx(b), c.ws(b), c.pv(b), c.pi(b), bounds,
                                    branch_final(c, b, at), st))
            return bail(rc);
        if (c.K) {
            TableArgs t{};
            t.h = c.h(b); t.n_dev = c.n_dev(b); t.cols = d.cols; t.cols_pad = c.cols0(); t.N = N;
            t.ncol = c.ncol; t.branch = b; t.K = c.K;
            t.table = c.table(b);
            hipLaunchKernelGGL(table_kernel, dim3(1), dim3(256), 0, st, t);
            if (hipGetLastError() != hipSuccess) return bail(TRX_ERR_HIP);
        }
        if (c.M && trx::post_launch(branch_post(c, b, at), false, st) != TRX_OK) return bail(trx::fail_hip(hipErrorLaunchFailure));
        if (c.H && trx::warp_hist_launch(branch_hist(c, b, at), st) != TRX_OK) return bail(trx::fail_hip(hipErrorLaunchFailure));
    }
    return copy_back(c, A.at<unsigned long long>(sh.hist), st);
}

// ---------------------------------------------------------------------------------------------------------------
// One launch chain for several calls: draw_kernel, compact_fill_kernel, rowc_kernel, (sec_scan_kernel,) the passes of the
// bounded evaluation and lme_partial_kernel are launched ONCE each, with the call (draw side) or the branch (likelihood
// side) as a further grid dimension -- 11 launches and one small upload for up to 16 calls / 24 branches, where the calls
// one by one take 9 (planet) to 17 (binary) launches EACH.  Round 4 measured why that matters (profiles/
// r04/concurrency_levels.txt, r04/j_batch_kernel_stats.txt): the chip runs ~3 kernels at a time whatever the number of
// streams, a 64-target step was 10 183 launches, most of them 8-45 us long on a tenth of the machine, and the host spent
// 113 of the step's 155 ms enqueueing them.  The calls of a chain must share N, the time stamps, the exposure settings
// and the precision flag (the calls of one target do: triceratops.py:767-1428); flux and sigma may differ (a nearby
// star's light curve is the target's, renormalised).  Results are those of the calls one by one, bit for bit: the same
// kernels' bodies on the same rows in the same order, each call described by the same Call as in enqueue().
// Calls with posterior rows (post_rows > 0) join like any other: behind lnl_lme_chain the two posterior kernels run ONCE
// for the whole chain (post_launch_chain: the branch as the grid's second dimension, its PostArgs from a table that rides
// in the upload of the draw-argument table); the weight histograms likewise (warp_hist_launch_chain).
// Scratch: + 49 KB per branch with posterior rows, + 16 (8 + 16 M) bytes per call whose block the device cannot write
// directly (at most 1 MB, M = 4096) -- beside the call's 146 N bytes of draw-side buffers (14 columns, masks, prior, lists,
// chi^2) for which the Python side's stream cap books 360 N (sharding.stream_scratch_bytes): covered from N = 5000 draws
// on, and below that a whole chain is a few MB.
constexpr size_t kBranchHead = 64;       // bytes of the zeroed head per branch: [scan counter | finished blocks, flag]
static_assert(trx::kChainMaxBranchesHost * kBranchHead <= trx::kScratchZeroed, "zeroed head of the chain's arena");

int enqueue_chain(const trx_scenario_args* calls, const int* which, int n, double* const* out, hipStream_t st)
{
    if (n < 1 || n > trx::kChainMaxCalls) return TRX_ERR_ARG;
    const trx_scenario_args& s0 = calls[which[0]];
    const long N = s0.draw->N;
    trx::StreamLock turn(st);
    Call call[trx::kChainMaxCalls];
    int nbr_total = 0, n_post = 0, n_hist = 0;      // branches; those of them that want posterior rows / a weight histogram
    for (int i = 0; i < n; ++i) {
        const trx_scenario_args& s = calls[which[i]];
        if (int rc = check_call(s)) return rc;
        if (s.draw->N != N || s.n_time != s0.n_time || s.time != s0.time || s.nsupersample != s0.nsupersample ||
            s.exptime != s0.exptime || table_rows(s)) return TRX_ERR_ARG;        // (a table call goes alone: trx_star_enqueue)
        const Call& c = call[i] = Call(s, out[which[i]]);
        nbr_total += c.nbr;
        n_post += c.M ? c.nbr : 0;
        n_hist += c.H ? c.nbr : 0;
    }
    if (nbr_total > trx::kChainMaxBranchesHost) return TRX_ERR_ARG;
    const size_t branch_bytes = trx::chain_branch_scratch_bytes(N);

    Arena A;
    const size_t o_head = A.reserve(trx::kScratchZeroed);
    // the draw-argument table and, behind it, the PostArgs of the branches that want samples: one upload
    const size_t post_tab_at = (sizeof(trx_draw_args) * (size_t)n + 255) & ~(size_t)255;
    // ... and the WarpHistArgs of the branches that want a histogram
    const size_t hist_tab_at = (post_tab_at + sizeof(trx::PostArgs) * (size_t)n_post + 255) & ~(size_t)255;
    const size_t tab_bytes = hist_tab_at + sizeof(trx::WarpHistArgs) * (size_t)n_hist;
    const size_t o_tab = A.reserve(tab_bytes);
    const size_t o_cnt = A.reserve(sizeof(int) * 2 * trx::kDrawMaxGroups * (size_t)n);
    for (int i = 0; i < n; ++i) call[i].at.reserve(A, call[i]);
    SharedLayout sh;
    sh.reserve(A, n_post, n_hist);
    const size_t o_branch = A.reserve(branch_bytes * (size_t)nbr_total);
    TRXS_HIP(trx::stream_scratch(st, 2, A.used, reinterpret_cast<void**>(&A.base)));

    // the calls' argument blocks, output pointers set, staged in pinned memory and copied to the device table
    trx_draw_args* stage = nullptr;
    void* stage_ticket = nullptr;
    TRXS_HIP(trx::pinned_stage_begin(st, tab_bytes, reinterpret_cast<void**>(&stage), &stage_ticket));
    trx::PostArgs* post_stage = reinterpret_cast<trx::PostArgs*>(reinterpret_cast<char*>(stage) + post_tab_at);
    trx::WarpHistArgs* hist_stage = reinterpret_cast<trx::WarpHistArgs*>(reinterpret_cast<char*>(stage) + hist_tab_at);
    int hist_first[trx::kChainMaxCalls];       // a call's first histogram slot
    trx::ChainFill fills[trx::kChainMaxCalls];
    trx::ChainBranch br[trx::kChainMaxBranchesHost];
    trx::ScenFinal fin[trx::kChainMaxBranchesHost];
    int b_at = 0, p_at = 0, h_at = 0;
    for (int i = 0; i < n; ++i) {
        Call& c = call[i];
        const trx_scenario_args& s = *c.s;
        c.A = &A;
        // (the call's first branch: word 1 of its state is the call's flag)
        stage[i] = c.draw_args(reinterpret_cast<unsigned*>(A.base + o_head + (size_t)b_at * kBranchHead + 8));
        hist_first[i] = h_at;
        fills[i] = trx::ChainFill{c.idx(0), c.idx(1), c.n_dev(0), c.cols0()};
        for (int b = 0; b < c.nbr; ++b, ++b_at) {
            char* head = A.base + o_head + (size_t)b_at * kBranchHead;
            const BranchPlace at = branch_place(c, A, sh, reinterpret_cast<unsigned*>(head + 8), 1, p_at, h_at);
            trx::ChainBranch& cb = br[b_at];
            cb.model = c.model(b); cb.flags = s.flags; cb.twin = b;
            cb.flux = s.flux; cb.sigma = s.sigma; cb.lnsigma = s.lnsigma;
            cb.cols = c.cols(); cb.n_dev = c.n_dev(b); cb.src_idx = c.idx(b); cb.h = c.h(b); cb.lnprior = c.lnprior();
            cb.scratch = reinterpret_cast<double*>(A.base + o_branch + branch_bytes * (size_t)b_at);
            cb.scan_count = reinterpret_cast<unsigned long long*>(head);
            cb.ws = c.ws(b); cb.amin_pv = c.pv(b); cb.amin_pi = c.pi(b);
            fin[b_at] = branch_final(c, b, at);
            cb.fin = &fin[b_at];
            if (c.M) post_stage[p_at++] = branch_post(c, b, at);
            if (c.H) hist_stage[h_at++] = branch_hist(c, b, at);
        }
    }
    trx_draw_args* dev_tab = A.at<trx_draw_args>(o_tab);
    {
        const hipError_t e = hipMemcpyAsync(dev_tab, stage, tab_bytes, hipMemcpyHostToDevice, st);
        trx::pinned_stage_end(st, stage_ticket);
        if (e != hipSuccess) return trx::fail_hip(e);
    }
    auto bail = [&](int rc) {
        (void)hipMemsetAsync(A.base + o_head, 0, trx::kScratchZeroed, st);
        return rc;
    };
    long per = 0;
    int groups = 0;
    if (int rc = trx::draw_chain(stage, dev_tab, n, A.at<int>(o_cnt), fills, &per, &groups, st)) return bail(rc);
    if (trx::knob_poison())          // tests: an unwritten row must show (include/trx_debug.h)
        for (int b = 0; b < nbr_total; ++b) TRXS_HIP(hipMemsetAsync(br[b].h, 0, sizeof(double) * (size_t)N, st));
    if (int rc = trx::lnl_lme_chain(br, nbr_total, s0.time, s0.n_time, N, s0.exptime, s0.nsupersample, st)) {
        // (kChainNotApplicable cannot happen in the production library -- trx_star_enqueue asked lnl_chain_applicable with
        // the same arguments and nothing it depends on can change; in the testing library a switch of trx_debug.h was
        // flipped by another thread in between: the draw kernels are already enqueued, so this is an error, not a fall-back)
        if (rc == trx::kChainNotApplicable) rc = trx::fail_hip(hipErrorInvalidValue);
        return bail(rc);
    }
    if (n_post) {
        const trx::PostArgs* post_tab = reinterpret_cast<const trx::PostArgs*>(A.base + o_tab + post_tab_at);
        if (trx::post_launch_chain(post_tab, n_post, N, st) != TRX_OK) return bail(trx::fail_hip(hipErrorLaunchFailure));
    }
    if (n_hist) {
        TRXS_HIP(hipMemsetAsync(A.at<char>(sh.hist), 0, SharedLayout::hist_bytes(n_hist), st));
        const trx::WarpHistArgs* hist_tab = reinterpret_cast<const trx::WarpHistArgs*>(A.base + o_tab + hist_tab_at);
        if (trx::warp_hist_launch_chain(hist_tab, n_hist, st) != TRX_OK) return bail(trx::fail_hip(hipErrorLaunchFailure));
    }
    for (int i = 0; i < n; ++i)
        if (int rc = copy_back(call[i], A.at<unsigned long long>(sh.hist) + (size_t)hist_first[i] * TRX_WARP_BRANCH, st)) return rc;
    return TRX_OK;
}

bool chain_enabled() { return trx::knob_star_chain() != 0; }

#ifdef TRX_TESTING
// trx_debug_chain_counts (include/trx_debug.h): what trx_star_enqueue has put into launch chains so far
std::atomic<long> g_chains{0}, g_calls_in_chains{0}, g_posterior_calls_in_chains{0};
#endif

// may call j join a chain that starts with call i?  (same stream is the caller's business)
bool chain_compatible(const trx_scenario_args& a, const trx_scenario_args& b)
{
    return a.draw->N == b.draw->N && a.n_time == b.n_time && a.time == b.time && a.nsupersample == b.nsupersample &&
           a.exptime == b.exptime &&
           ((a.flags ^ b.flags) & trx::kChainSharedFlags) == 0 &&
           (a.draw->warp != nullptr) == (b.draw->warp != nullptr);     // mapped and unmapped draw kernels: the chain splits
}

}  // namespace

extern "C" int trx_scenario_enqueue(const trx_scenario_args* s, double* out, void* stream)
{
    if (!s || !s->draw || !out) return TRX_ERR_ARG;
    return enqueue(s, out, static_cast<hipStream_t>(stream));
}

extern "C" int trx_star_enqueue(const trx_scenario_args* calls, int n_calls, double* const* out, void* const* streams,
                                int* n_done)
{
    if (n_done) *n_done = 0;
    if (n_calls < 0 || (n_calls > 0 && (!calls || !out || !streams))) return TRX_ERR_ARG;
    for (int i = 0; i < n_calls; ++i)
        if (!calls[i].draw || !out[i]) return TRX_ERR_ARG;
    // Consecutive calls on one stream that share N, the time stamps, the exposure settings and the precision go into ONE
    // launch chain (enqueue_chain), up to kChainMaxCalls calls / kChainMaxBranchesHost branches at a time -- when the
    // bounded evaluation's passes apply to them and their scratch together stays below the budget (TRX_CHAIN_DRAWS,
    // default 2.5e7 draws' worth per chain: ~0.36 GB per 1e6 draws and call); everything else goes call by call.
    static const double draw_budget = trx::env_double("TRX_CHAIN_DRAWS", 2.5e7);
    int i = 0;
    while (i < n_calls) {
        hipStream_t st = static_cast<hipStream_t>(streams[i]);
        int which[trx::kChainMaxCalls];
        int n = 0, nbr = 0;
        if (chain_enabled() && calls[i].table_rows <= 1 &&
            trx::lnl_chain_applicable(calls[i].flags, calls[i].n_time, calls[i].draw->N, calls[i].nsupersample)) {
            for (int j = i; j < n_calls && n < trx::kChainMaxCalls; ++j) {
                if (streams[j] != streams[i] || calls[j].table_rows > 1 || !chain_compatible(calls[i], calls[j])) break;
                const int add = calls[j].draw->planet ? 1 : 2;
                if (nbr + add > trx::kChainMaxBranchesHost) break;
                if ((double)(n + 1) * (double)calls[i].draw->N > draw_budget && n > 0) break;
                which[n++] = j;
                nbr += add;
            }
        }
        if (n >= 2) {
            if (int rc = enqueue_chain(calls, which, n, out, st)) return rc;
#ifdef TRX_TESTING
            g_chains += 1;
            g_calls_in_chains += n;
            for (int k = 0; k < n; ++k) g_posterior_calls_in_chains += calls[which[k]].post_rows > 0 ? 1 : 0;
#endif
            i += n;
        } else {
            if (int rc = enqueue(&calls[i], out[i], st)) return rc;
            i += 1;
        }
        if (n_done) *n_done = i;
    }
    return TRX_OK;
}

#ifdef TRX_TESTING
extern "C" int trx_set_star_chain(int on)
{
    trx::g_knob_star_chain = on ? 1 : 0;
    return TRX_OK;
}

extern "C" int trx_debug_chain_counts(long* chains, long* calls_in_chains, long* posterior_calls_in_chains, int reset)
{
    if (chains) *chains = g_chains.load();
    if (calls_in_chains) *calls_in_chains = g_calls_in_chains.load();
    if (posterior_calls_in_chains) *posterior_calls_in_chains = g_posterior_calls_in_chains.load();
    if (reset) {
        g_chains = 0;
        g_calls_in_chains = 0;
        g_posterior_calls_in_chains = 0;
    }
    return TRX_OK;
}
#endif

extern "C" int trx_scenario_evidence(const trx_scenario_args* s, void* stream)
{
    if (!s || !s->draw || !s->out || !s->out_flag) return TRX_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    trx::StreamLock turn(st);              // the pinned staging record is the stream's, too
    double* pinned = nullptr;              // pinned, so that the copy is asynchronous
    TRXS_HIP(trx::stream_scratch(st, 3, sizeof(double) * (2 * TRX_SCENARIO_OUT_MOMENTS + 1), reinterpret_cast<void**>(&pinned)));
    if (int rc = enqueue(s, pinned, st)) return rc;
    TRXS_HIP(hipStreamSynchronize(st));
    const int nbr = s->draw->planet ? 1 : 2, stride = record_stride(s->flags);
    memcpy(s->out, pinned, (size_t)nbr * stride * sizeof(double));
    *s->out_flag = (int)pinned[2 * stride];
    return TRX_OK;
}

extern "C" size_t trx_scenario_args_size(void) { return sizeof(trx_scenario_args); }

extern "C" int trx_posterior_from_halfchi2(const double* halfchi2, const double* lnprior, long n, double lnsigma,
                                           int post_rows, unsigned long long post_seed, long* out_pos, double* out_hdr,
                                           void* workspace, size_t workspace_bytes, void* stream)
{
    static_assert(trx::kPostWsBytes <= 65536, "the reductions' workspace (trx_workspace_bytes) serves");
    if (n < 0 || n > 0x7fffffffL || (n > 0 && !halfchi2) || post_rows < 0 || post_rows > TRX_POST_MAX_ROWS || !out_hdr ||
        (post_rows > 0 && !out_pos))
        return TRX_ERR_ARG;
    if (!workspace || workspace_bytes < trx_workspace_bytes() || trx_workspace_bytes() < trx::kPostWsBytes)
        return TRX_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    trx::PostArgs p{};
    p.h = halfchi2; p.lnprior = lnprior; p.n = n; p.N = n;
    p.c0 = trx::lnl_c0(lnsigma);
    p.M = post_rows; p.seed = post_seed;
    p.tile_q = reinterpret_cast<trx::u128*>(ws);
    p.tile_cnt = reinterpret_cast<long*>(ws + trx::kPostWsSums);
    p.tile_max = reinterpret_cast<double*>(ws + trx::kPostWsSums);
    p.xmax = reinterpret_cast<double*>(ws + trx::kPostWsSums + trx::kPostWsCounts);
    p.out_pos = out_pos; p.out_hdr = out_hdr;
    if (trx::post_launch(p, true, static_cast<hipStream_t>(stream)) != TRX_OK) return trx::fail_hip(hipErrorLaunchFailure);
    return TRX_OK;
}

extern "C" int trxw_hist_from_halfchi2(const trx_draw_args* draw, const double* halfchi2, const double* lnprior,
                                       const long* idx, long n, double lnsigma, unsigned long long* out,
                                       void* workspace, size_t workspace_bytes, void* stream)
{
    if (!draw || !out || n < 0 || n > 0x7fffffffL || (n > 0 && (!halfchi2 || !idx)) || !draw->use_philox) return TRX_ERR_ARG;
    if (!workspace || workspace_bytes < trx_workspace_bytes() || trx_workspace_bytes() < trx::kPostWsBytes)
        return TRX_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    // X, the largest log-weight: there is no evidence pass to take it from (as in trx_posterior_from_halfchi2)
    trx::PostArgs p{};
    p.h = halfchi2; p.lnprior = lnprior; p.n = n; p.N = n;
    p.c0 = trx::lnl_c0(lnsigma);
    p.tile_max = reinterpret_cast<double*>(ws + trx::kPostWsSums);
    p.xmax = reinterpret_cast<double*>(ws + trx::kPostWsSums + trx::kPostWsCounts);
    int tiles, per_tile;
    trx::post_geometry(n, n, tiles, per_tile);
    hipLaunchKernelGGL(trx::post_max_kernel, dim3(tiles), dim3(256), 0, st, p);
    hipLaunchKernelGGL(trx::post_x_kernel, dim3(1), dim3(256), 0, st, p);
    if (hipGetLastError() != hipSuccess) return trx::fail_hip(hipErrorLaunchFailure);
    TRXS_HIP(hipMemsetAsync(out, 0, sizeof(unsigned long long) * TRX_WARP_BRANCH, st));
    trx::WarpHistArgs w{};
    w.h = halfchi2; w.lnprior = lnprior; w.n = n; w.idx64 = idx; w.N = n;
    w.slots = trx::warp_consumed_slots(*draw);
    w.c0 = p.c0;
    w.seed = draw->seed;
    w.xmax = p.xmax;
    w.out = out;
    if (trx::warp_hist_launch(w, st) != TRX_OK) return trx::fail_hip(hipErrorLaunchFailure);
    return TRX_OK;
}

#ifdef TRX_TESTING
extern "C" int trx_set_debug_poison(int on)
{
    trx::g_knob_poison = on ? 1 : 0;
    return TRX_OK;
}

// trx_debug_select_from_halfchi2 (include/trx_debug.h): what enqueue() runs for ONE branch behind its likelihood kernels
// -- lme_draws with the ScenFinal of branch_final, then table_kernel with enqueue()'s TableArgs -- on the caller's chi^2/2,
// prior and columns.  The scratch is the stream's scenario scratch (slot 1) behind its persistent block, as in enqueue().
extern "C" int trx_debug_select_from_halfchi2(const double* halfchi2, const double* lnprior, const double* cols,
                                              const double* cols_pad, long n, long N, long n_total, int ncol, int twin, int K,
                                              int moments, double lnsigma, double* out_record, double* out_post_x,
                                              double* out_table, void* stream)
{
    const int n_pad = K ? K : 1;
    if (!halfchi2 || ((uintptr_t)halfchi2 % 16) != 0 || !cols || !cols_pad || !out_record || !out_post_x) return TRX_ERR_ARG;
    if ((ncol != 11 && ncol != 14) || (twin != 0 && twin != 1) || (moments != 0 && moments != 1)) return TRX_ERR_ARG;
    if (K != 0 && (K < 2 || K > TRX_TABLE_MAX_ROWS || !out_table)) return TRX_ERR_ARG;
    if (n < 0 || N < 1 || N > 0x7fffffffL || n > N || N < n_pad || n_total < 1) return TRX_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    trx::StreamLock turn(st);
    const int stride = moments ? TRX_SCENARIO_OUT_MOMENTS : TRX_SCENARIO_OUT;
    const size_t rec_bytes = sizeof(double) * (2 * TRX_SCENARIO_OUT_MOMENTS + 1);
    const size_t table_bytes = K ? sizeof(double) * TRX_TABLE_BRANCH(K) : 0;

    Arena A;
    const size_t o_state = A.reserve(trx::kScratchZeroed);     // persistent, as in enqueue(): left at zero
    const size_t o_n = A.reserve(2 * sizeof(long));
    const size_t o_res = A.reserve(rec_bytes);
    const size_t o_ws = A.reserve(sizeof(double) * trx::kLmePart * kLmeParts);
    const size_t o_pv = A.reserve(sizeof(double) * kLmeParts);
    const size_t o_pi = A.reserve(sizeof(long) * 2 * kLmeParts);
    const size_t o_idx = A.reserve(sizeof(int) * (size_t)N);    // (dense columns: the list is handed on, never read)
    const size_t o_px = A.reserve(sizeof(double));
    const size_t o_table = A.reserve(table_bytes);
    TRXS_HIP(trx::stream_scratch(st, 1, A.used, reinterpret_cast<void**>(&A.base)));
    unsigned* state = A.at<unsigned>(o_state);
    long* n_dev = A.at<long>(o_n);
    double* res = A.at<double>(o_res);
    // the count goes to the device, where the kernels read it; what no kernel writes shows as 0x7f7f...: 1.38e306
    TRXS_HIP(hipMemsetAsync(n_dev, 0, 2 * sizeof(long), st));
    TRXS_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(n_dev), (int)n, 1, st));
    TRXS_HIP(hipMemsetAsync(A.at<int>(o_idx), 0, sizeof(int) * (size_t)N, st));
    TRXS_HIP(hipMemsetAsync(res, 0x7f, rec_bytes, st));
    TRXS_HIP(hipMemsetAsync(A.at<double>(o_px), 0x7f, sizeof(double), st));
    if (K) TRXS_HIP(hipMemsetAsync(A.at<double>(o_table), 0x7f, table_bytes, st));

    trx::ScenFinal f{};
    f.idx = A.at<int>(o_idx); f.cols = cols; f.cols0 = cols_pad; f.cols0_stride = n_pad; f.dense = 1;
    f.N = N; f.n_total = n_total; f.ncol = ncol; f.branch = twin; f.last_branch = 1;
    f.stride = stride;
    f.res = res + (size_t)twin * stride;
    f.flag_out = (twin == 0) ? res + 2 * stride : nullptr;
    f.state = state;
    f.post_x = A.at<double>(o_px);
    auto bail = [&](int rc) {
        (void)hipMemsetAsync(state, 0, trx::kScratchZeroed, st);
        return rc;
    };
    if (int rc = trx::lme_draws(halfchi2, lnprior, lnsigma, N, n_dev, f.idx, A.at<double>(o_ws), A.at<double>(o_pv),
                                A.at<long>(o_pi), nullptr, f, st))
        return bail(rc);
    if (K) {
        TableArgs t{};
        t.h = halfchi2; t.n_dev = n_dev; t.cols = cols; t.cols_pad = cols_pad; t.N = N;
        t.ncol = ncol; t.branch = twin; t.K = K;
        t.table = A.at<double>(o_table);
        hipLaunchKernelGGL(table_kernel, dim3(1), dim3(256), 0, st, t);
        if (hipGetLastError() != hipSuccess) return bail(TRX_ERR_HIP);
    }
    TRXS_HIP(hipMemcpyAsync(out_record, f.res, sizeof(double) * (size_t)stride, hipMemcpyDeviceToHost, st));
    TRXS_HIP(hipMemcpyAsync(out_post_x, f.post_x, sizeof(double), hipMemcpyDeviceToHost, st));
    if (K) TRXS_HIP(hipMemcpyAsync(out_table, A.at<double>(o_table), table_bytes, hipMemcpyDeviceToHost, st));
    TRXS_HIP(hipStreamSynchronize(st));
    return TRX_OK;
}
#endif
