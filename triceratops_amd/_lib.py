"""Loader and thin typed wrappers for libtrx.so (C ABI in include/trx.h).

The HIP library is the only compute backend of this package: if it is missing or fails to
load, importing the compute entry points raises -- there is no CPU fallback.
torch is used for device memory, streams and torch.distributed only.
"""
import ctypes
import os
import threading

import numpy as np
import torch  # noqa: F401  (imported first so libtrx binds to the HIP runtime torch loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
# The production library: no switches, no environment variables, no debug exports (include/trx.h).  TRX_LIB: A/B builds.
LIB_PATH = os.environ.get("TRX_LIB") or os.path.join(_HERE, "libtrx.so")
# The testing library (the same sources with -DTRX_TESTING): + include/trx_debug.h.  tests/ and profiles/ switch to it
# with use_testing_library() (or TRX_TESTING=1 in the environment, for old scripts); the product never does.
TESTING_LIB_PATH = os.environ.get("TRX_TESTING_LIB") or os.path.join(_HERE, "libtrx_testing.so")

MODEL_TP, MODEL_EB, MODEL_EB_TWIN, MODEL_RAW = 0, 1, 2, 3
FLAG_COMPANION_IS_HOST, FLAG_SCALAR_K, FLAG_FP32_MODEL, FLAG_EVALUATE_EXCLUDED = 1, 2, 4, 8
# result-neutral per-call choices (include/trx.h)
FLAG_ALL_SUBEXPOSURES, FLAG_NO_STENCIL, FLAG_COUNT_EVALUATIONS, FLAG_FULL_EVALUATION = 16, 32, 64, 128
# scenario records carry lnM2 and lnWmax of the evidence's weights (include/trx.h)
FLAG_WEIGHT_MOMENTS = 256
N_PARAM = {MODEL_TP: 10, MODEL_EB: 11, MODEL_EB_TWIN: 11, MODEL_RAW: 9}
ERR_NTOTAL = 4

# every symbol include/trx.h declares (tests check that libtrx.so exports all of them and nothing of trx_debug.h)
ABI_SYMBOLS = (
    "trx_lnl_batch", "trx_lnl_batch_weighted", "trx_flux_grid", "trx_chi2_grid", "trx_chi2_grid_weighted",
    "trx_chi2_grid_offset", "trx_chi2_grid_baseline", "trx_workspace_bytes",
    "trx_log_mean_exp", "trx_lnz_scenario", "trx_lnz_from_halfchi2", "trx_lnz_moments_from_halfchi2",
    "trx_posterior_from_halfchi2", "trx_grid_quantiles",
    "trx_lnl_batch_host", "trx_flux_grid_host",
    "trx_log_mean_exp_host", "trx_skipped_rows", "trx_pruned_rows",
    "trx_draw_scenario", "trx_draw_args_size", "trx_scenario_evidence", "trx_scenario_enqueue", "trx_star_enqueue",
    "trx_scenario_args_size", "trx_release_scratch", "trx_version", "trx_last_error", "trx_device_count",
)
# ... include/trx_warp.h (both libraries: the weight histogram on its own, prefix trxw_)
WARP_SYMBOLS = ("trxw_hist_from_halfchi2",)
# ... include/trx_noise.h (both libraries: the row reduction under correlated noise, prefix trxn_)
NOISE_SYMBOLS = ("trxn_chi2_grid_ou",)
# ... include/trx_mix.h (both libraries: the same over a grid of candidate noise models, prefix trxm_)
MIX_SYMBOLS = ("trxm_chi2_grid_ou_mix",)
# ... include/trx_shift.h (both libraries: the soft minimum over the nodes of a transit-time shift grid, prefix trxt_)
SHIFT_SYMBOLS = ("trxt_softmin_rows",)
# ... include/trx_robust.h (both libraries: the outlier-tolerant row reduction, prefix trxr_)
ROBUST_SYMBOLS = ("trxr_chi2_grid_robust",)
# ... include/trx_gls.h (both libraries: a linear baseline marginalised under correlated noise, prefix trxg_)
GLS_SYMBOLS = ("trxg_chi2_grid_ou_baseline",)
# ... include/trx_ss.h (both libraries: the row reduction under correlated noise with a two-dimensional state, prefix trxs_)
SS_SYMBOLS = ("trxs_chi2_grid_ss2",)
# ... include/trx_mix.h as well (both libraries: the weighted row reduction over a grid of candidate white-noise models,
# prefix trxv_)
WHITE_SYMBOLS = ("trxv_chi2_grid_white_mix",)
# ... include/trx_gls.h as well (both libraries: that reduction with baseline columns marginalised per candidate, prefix
# trxb_)
WLIN_SYMBOLS = ("trxb_chi2_grid_white_baseline",)
# ... include/trx_ss.h as well (both libraries: the two-state reduction with baseline columns marginalised under the same
# noise, prefix trxk_)
SSGLS_SYMBOLS = ("trxk_chi2_grid_ss2_baseline",)
# ... and include/trx_debug.h: the testing library only
DEBUG_SYMBOLS = (
    "trx_set_rows_per_wave", "trx_set_cell_packing_below", "trx_debug_batch_plan", "trx_set_supersample_tiers",
    "trx_set_stencil", "trx_set_skip_excluded", "trx_set_debug_node_counts", "trx_set_kepler_stepping",
    "trx_set_bounded_evaluation", "trx_set_debug_bounded_lnl", "trx_set_debug_poison", "trx_set_debug_bug",
    "trx_set_probe_rows", "trx_set_star_chain", "trx_debug_capture_buffers", "trx_debug_chain_counts",
    "trx_set_row_order", "trx_debug_row_order", "trx_set_whole_trips", "trx_debug_whole_trips", "trx_set_one_sweep",
    "trx_set_full_chunks", "trx_debug_cells_lds_one_row", "trx_debug_select_from_halfchi2", "trx_set_zone_loop",
    "trx_debug_zone_chunks",
)


class TrxError(RuntimeError):
    pass


# flags OR-ed into every likelihood launch of the lnZ_* / calc_probs layer: set_precision("fp32")
# puts TRX_FLAG_FP32_MODEL here (BASELINE config 5); the plain wrappers below take explicit flags
EXTRA_FLAGS = 0
# library default of trx_set_cell_packing_below (tests and A/B scripts restore it)
CELL_PACKING_BELOW = 320
# work counters of the scenario layer (bench.py reads them): rows and (row, time) cells that
# went through trx_lnz_scenario since the last reset
# native_calls: lnZ_* calls that went through the library's own chain (trx_scenario_enqueue / trx_star_enqueue)
STATS = {"rows": 0, "cells": 0, "launches": 0, "native_calls": 0}
_stats_lock = threading.Lock()


def count_launch(rows, n_time):
    """bench bookkeeping; the worker threads of sharding.threads update it side by side"""
    with _stats_lock:
        STATS["rows"] += rows
        STATS["cells"] += rows * n_time
        STATS["launches"] += 1
# measurement hook (bench.py --mode batch): a list that receives, per trx_lnz_scenario launch,
# (model, flags, n, n_time, start_event, end_event, first rows of the parameter block)
TRACE = None
TRACE_SAMPLE_ROWS = 128


def reset_stats():
    for k in STATS:
        STATS[k] = 0


def set_precision(mode):
    """'fp64' (default) or 'fp32': fp32 Mandel-Agol arithmetic with fp64 orbit, chi^2 and
    log-mean-exp (TRX_FLAG_FP32_MODEL) for every scenario evaluated through lnZ_* / calc_probs"""
    global EXTRA_FLAGS
    if mode not in ("fp64", "fp32"):
        raise ValueError("precision must be 'fp64' or 'fp32'")
    EXTRA_FLAGS = (EXTRA_FLAGS & ~FLAG_FP32_MODEL) | (FLAG_FP32_MODEL if mode == "fp32" else 0)


def set_full_evaluation(on):
    """True: every lnZ_* / calc_probs call evaluates every masked draw to the end (TRX_FLAG_FULL_EVALUATION on every
    scenario call) instead of the bounded evaluation; same lnZ to rounding, same best draws, slower"""
    global EXTRA_FLAGS
    EXTRA_FLAGS = (EXTRA_FLAGS | FLAG_FULL_EVALUATION) if on else (EXTRA_FLAGS & ~FLAG_FULL_EVALUATION)


_vp = ctypes.c_void_p
_lib = None                 # the library in use
_production = None
_testing = None


def lib():
    """The library in use: libtrx.so, loaded once (raises TrxError if the HIP extension was not built) -- or the
    testing library after use_testing_library()."""
    global _lib, _production
    if _lib is not None:
        return _lib
    if os.environ.get("TRX_TESTING") == "1":
        return use_testing_library(True)
    if _production is None:
        _production = _load(LIB_PATH, False)
    _lib = _production
    return _lib


def testing_lib():
    """libtrx_testing.so (include/trx_debug.h), loaded once; does not change the library in use"""
    global _testing
    if _testing is None:
        _testing = _load(TESTING_LIB_PATH, True)
    return _testing


def use_testing_library(on=True):
    """tests/ and profiles/ only: every wrapper of this module calls the testing library (its own scratch, its own
    switches, all at their defaults unless set) until use_testing_library(False).  Returns the library now in use."""
    global _lib, _production
    if on:
        _lib = testing_lib()
    else:
        if _production is None:
            _production = _load(LIB_PATH, False)
        _lib = _production
    return _lib


def _load(path, testing):
    if not os.path.exists(path):
        raise TrxError(
            "triceratops_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    L = ctypes.CDLL(path)
    c_int, c_long, c_double, c_size_t = ctypes.c_int, ctypes.c_long, ctypes.c_double, ctypes.c_size_t
    L.trx_lnl_batch.restype = c_int
    L.trx_lnl_batch.argtypes = [c_int, c_int, _vp, _vp, c_int, c_double, _vp, c_long, c_double,
                                c_int, _vp, _vp]
    L.trx_lnl_batch_weighted.restype = c_int
    L.trx_lnl_batch_weighted.argtypes = [c_int, c_int, _vp, _vp, _vp, c_int, _vp, c_long, c_double, c_int, c_double,
                                         c_int, _vp, _vp]
    L.trx_flux_grid.restype = c_int
    L.trx_flux_grid.argtypes = [c_int, c_int, _vp, c_int, _vp, c_long, c_double, c_int, _vp, _vp, _vp]
    L.trx_chi2_grid.restype = c_int
    L.trx_chi2_grid.argtypes = [_vp, _vp, c_int, c_long, c_double, _vp, _vp]
    L.trx_chi2_grid_weighted.restype = c_int
    L.trx_chi2_grid_weighted.argtypes = [_vp, _vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp]
    L.trx_chi2_grid_offset.restype = c_int
    L.trx_chi2_grid_offset.argtypes = [_vp, _vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, c_double, c_double, _vp,
                                       _vp]
    L.trx_chi2_grid_baseline.restype = c_int
    L.trx_chi2_grid_baseline.argtypes = [_vp, _vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, c_int, _vp, _vp,
                                         _vp]
    L.trx_workspace_bytes.restype = c_size_t
    L.trx_workspace_bytes.argtypes = []
    L.trx_log_mean_exp.restype = c_int
    L.trx_log_mean_exp.argtypes = [_vp, c_long, c_long, _vp, _vp, c_size_t, _vp]
    L.trx_lnz_scenario.restype = c_int
    L.trx_lnz_scenario.argtypes = [c_int, c_int, _vp, _vp, c_int, c_double, _vp, c_long, c_double,
                                   c_int, _vp, c_long, c_double, _vp, _vp, _vp, c_size_t, _vp]
    L.trx_lnz_from_halfchi2.restype = c_int
    L.trx_lnz_from_halfchi2.argtypes = [_vp, _vp, c_long, c_long, c_double, _vp, _vp, c_size_t, _vp]
    L.trx_lnz_moments_from_halfchi2.restype = c_int
    L.trx_lnz_moments_from_halfchi2.argtypes = [_vp, _vp, c_long, c_long, c_double, _vp, _vp, c_size_t, _vp]
    L.trx_posterior_from_halfchi2.restype = c_int
    L.trx_posterior_from_halfchi2.argtypes = [_vp, _vp, c_long, c_double, c_int, ctypes.c_ulonglong, _vp, _vp, _vp,
                                              c_size_t, _vp]
    L.trxw_hist_from_halfchi2.restype = c_int
    L.trxw_hist_from_halfchi2.argtypes = [_vp, _vp, _vp, _vp, c_long, c_double, _vp, _vp, c_size_t, _vp]
    L.trxn_chi2_grid_ou.restype = c_int
    L.trxn_chi2_grid_ou.argtypes = [_vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, _vp, _vp, _vp]
    L.trxm_chi2_grid_ou_mix.restype = c_int
    L.trxm_chi2_grid_ou_mix.argtypes = [_vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, _vp, _vp, c_int, _vp, _vp,
                                        _vp]
    L.trxv_chi2_grid_white_mix.restype = c_int
    L.trxv_chi2_grid_white_mix.argtypes = [_vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, c_int, _vp, _vp, _vp]
    L.trxb_chi2_grid_white_baseline.restype = c_int
    L.trxb_chi2_grid_white_baseline.argtypes = [_vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, _vp, c_int, c_int,
                                                _vp, _vp, _vp, _vp, _vp]
    L.trxt_softmin_rows.restype = c_int
    L.trxt_softmin_rows.argtypes = [_vp, c_long, c_long, c_int, _vp, c_int, _vp, _vp]
    L.trxr_chi2_grid_robust.restype = c_int
    L.trxr_chi2_grid_robust.argtypes = [_vp, _vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, c_double, c_double, c_double,
                                        _vp]
    L.trxg_chi2_grid_ou_baseline.restype = c_int
    L.trxg_chi2_grid_ou_baseline.argtypes = [_vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, _vp, _vp, _vp, c_int,
                                             _vp, _vp, _vp]
    L.trxs_chi2_grid_ss2.restype = c_int
    L.trxs_chi2_grid_ss2.argtypes = [_vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, _vp, _vp, _vp]
    L.trxk_chi2_grid_ss2_baseline.restype = c_int
    L.trxk_chi2_grid_ss2_baseline.argtypes = [_vp, _vp, c_int, c_long, _vp, c_double, c_int, _vp, _vp, _vp, _vp, _vp, c_int,
                                              _vp, _vp, _vp]
    L.trx_grid_quantiles.restype = c_int
    L.trx_grid_quantiles.argtypes = [_vp, c_long, c_int, _vp, _vp, c_long, _vp, c_int, _vp, _vp]
    L.trx_lnl_batch_host.restype = c_int
    L.trx_lnl_batch_host.argtypes = [c_int, c_int, _vp, _vp, c_int, c_double, _vp, c_long,
                                     c_double, c_int, _vp]
    L.trx_flux_grid_host.restype = c_int
    L.trx_flux_grid_host.argtypes = [c_int, c_int, _vp, c_int, _vp, c_long, c_double, c_int, _vp, _vp]
    L.trx_log_mean_exp_host.restype = c_int
    L.trx_log_mean_exp_host.argtypes = [_vp, c_long, c_long, _vp]
    L.trx_skipped_rows.restype = c_int
    L.trx_skipped_rows.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), c_int]
    L.trx_pruned_rows.restype = c_int
    L.trx_pruned_rows.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), c_int]
    L.trx_version.restype = ctypes.c_char_p
    L.trx_last_error.restype = ctypes.c_char_p
    L.trx_device_count.restype = c_int
    L.trx_testing = bool(testing)
    if testing:
        for name in ("trx_set_rows_per_wave", "trx_set_kepler_stepping", "trx_set_skip_excluded",
                     "trx_set_bounded_evaluation", "trx_set_debug_bounded_lnl", "trx_set_debug_poison",
                     "trx_set_debug_bug", "trx_set_star_chain", "trx_set_probe_rows", "trx_set_stencil",
                     "trx_set_supersample_tiers", "trx_set_debug_node_counts", "trx_set_cell_packing_below",
                     "trx_set_row_order", "trx_set_whole_trips", "trx_set_one_sweep", "trx_set_full_chunks",
                     "trx_set_zone_loop"):
            fn = getattr(L, name)
            fn.restype = c_int
            fn.argtypes = [c_int]
        L.trx_debug_cells_lds_one_row.restype = c_long
        L.trx_debug_cells_lds_one_row.argtypes = []
        L.trx_debug_capture_buffers.restype = c_int
        L.trx_debug_capture_buffers.argtypes = [ctypes.POINTER(c_long), ctypes.POINTER(c_long)]
        L.trx_debug_row_order.restype = c_int
        L.trx_debug_row_order.argtypes = [ctypes.POINTER(c_long), ctypes.POINTER(c_long), _vp, _vp, _vp]
        L.trx_debug_whole_trips.restype = c_int
        L.trx_debug_whole_trips.argtypes = [ctypes.POINTER(c_long), ctypes.POINTER(c_long), c_int]
        L.trx_debug_zone_chunks.restype = c_int
        L.trx_debug_zone_chunks.argtypes = [ctypes.POINTER(c_long), c_int]
        L.trx_debug_select_from_halfchi2.restype = c_int
        L.trx_debug_select_from_halfchi2.argtypes = [_vp, _vp, _vp, _vp, c_long, c_long, c_long, c_int, c_int, c_int, c_int,
                                                     c_double, _vp, _vp, _vp, _vp]
    return L


def check(rc):
    if rc:
        msg = lib().trx_last_error().decode()
        if rc == ERR_NTOTAL:
            raise ValueError(msg)
        raise TrxError("libtrx error %d: %s" % (rc, msg))


def version():
    return lib().trx_version().decode()


_gpu_seen = False


def require_gpu():
    """raises unless a GPU and the HIP library are there (checked until it has succeeded once:
    hipGetDeviceCount costs ~0.1 ms a call on this stack, a tenth of a small lnZ_* call)"""
    global _gpu_seen
    if _gpu_seen:
        return
    if not torch.cuda.is_available() or lib().trx_device_count() < 1:
        raise TrxError("triceratops_amd needs an AMD GPU (gfx950); none is visible and there is no "
                       "CPU fallback")
    _gpu_seen = True
    from . import hw_queues
    if hw_queues()["in_effect"] is False:
        import warnings
        warnings.warn("triceratops_amd was imported after the HIP runtime had been initialised: GPU_MAX_HW_QUEUES=16 "
                      "did not take effect (the runtime keeps its default of 4 hardware queues; calc_probs on more "
                      "than two streams runs ~10 % slower).  Import triceratops_amd before the first GPU call or "
                      "export GPU_MAX_HW_QUEUES=16.", RuntimeWarning, stacklevel=3)


def compute_device():
    """the current GPU as a torch.device (raises without one)"""
    require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


# ---------------------------------------------------------------------------------------
# device helpers
_upload_streams = {}
# events of uploads that may still be in flight: every stream about to read library inputs waits for them ON THE
# DEVICE (wait_uploads), the host never blocks
_pending_uploads = {}          # device index -> [(sequence number, event)], oldest first
_pending_lock = threading.Lock()
_upload_seq = {}               # device index -> sequence number of its newest upload
_stream_seen = {}              # (device index, stream handle) -> sequence number of the last upload it already waits for


def dev(x, device=None):
    """float64 contiguous device tensor from array-like / tensor.

    Host arrays go up asynchronously on a stream of their own, through a pinned staging block: a copy from
    pageable memory returns when it has COMPLETED, and with the GPU busy that was 0.5 ms per small table (a
    third of the host time of a 64-target batch step, profiles/r03/f_batch_host_profile.txt).  Nothing waits on
    the host: the upload leaves an event, the stream that is current here waits for it on the device, and so does
    every stream a library call is enqueued on while the event is pending (wait_uploads; cached tables are read
    by calls on other streams a few microseconds later).  A tensor from dev() is therefore ordered for the stream
    that was current at the upload and for every stream that passes through wait_uploads() / _stream() -- all library
    calls do; a torch operator launched on some OTHER stream right after must call wait_uploads(that stream) itself."""
    if isinstance(x, torch.Tensor):
        return x.to(device=device or "cuda", dtype=torch.float64).contiguous()
    a = np.ascontiguousarray(x, dtype=np.float64)
    d = torch.device(device or "cuda")
    if d.type != "cuda" or not torch.cuda.is_available():
        return torch.as_tensor(a).to(d).contiguous()
    if torch.cuda.is_current_stream_capturing():
        # (an upload is eager work on another stream: a captured call would not be ordered behind it, and its event may
        # neither be waited for nor queried while the capture lasts)
        raise TrxError("triceratops_amd: host data cannot be uploaded while the current stream is being captured into "
                       "a graph; stage the inputs with _lib.dev() before the capture begins")
    if d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    up = upload_stream(d).stream
    staged = torch.empty(a.shape, dtype=torch.float64, pin_memory=True)    # (torch caches pinned blocks)
    staged.numpy()[...] = a
    with torch.cuda.stream(up):
        t = staged.to(d, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(up)
    cur = torch.cuda.current_stream(d)
    t.record_stream(cur)      # the allocator must not hand the block out early
    with _pending_lock:
        seq = _upload_seq[d.index] = _upload_seq.get(d.index, 0) + 1
        _pending_uploads.setdefault(d.index, []).append((seq, ev))
    wait_uploads(cur)
    return t


def wait_uploads(stream):
    """`stream` waits (on the device) for every upload that has not completed yet -- each of them once: the uploads
    go up on ONE stream, in order, so waiting for the newest pending one covers all before it"""
    pend = _pending_uploads.get(stream.device.index)
    if not pend:
        return
    if torch.cuda.is_current_stream_capturing():
        # Nothing may be asked of an event while a capture lasts: hipEventQuery fails with "operation not permitted when
        # stream is capturing" AND invalidates the capture (found by profiles/r06/graph_stress.py: an upload still in
        # flight at the warm-up call leaves its event on the list, and the captured call that follows queried it --
        # one capture in ~2700).  A captured call is not executed now; torch.cuda.graph() synchronises the device before
        # it begins the capture, so every upload issued before it has landed, and dev() refuses uploads during one.
        return
    # (keyed per device: the default stream is handle 0 on every device, and sequence numbers are per device too)
    key = (stream.device.index, stream.cuda_stream)
    with _pending_lock:
        while pend and pend[0][1].query():
            pend.pop(0)                                 # (completed: nobody needs to wait any more)
        if not pend:
            # nothing in flight: forget who waited for what, so that a stream created later under a recycled handle
            # does not inherit the record of the one destroyed
            for k in [k for k in _stream_seen if k[0] == stream.device.index]:
                del _stream_seen[k]
            return
        seq, ev = pend[-1]
        if _stream_seen.get(key, 0) >= seq:
            return
        _stream_seen[key] = seq
    stream.wait_event(ev)


class upload_stream:
    """`with upload_stream(device):` -- torch work inside runs on the device's upload stream and has completed
    at exit: for small tables that several lnZ_* calls on different streams read afterwards"""

    def __init__(self, device):
        d = torch.device(device)
        self.stream = self.ctx = None
        if d.type != "cuda":                 # (the torch expression of the tests on CPU tensors)
            return
        if d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        self.stream = _upload_streams.get(d.index)
        if self.stream is None:
            self.stream = _upload_streams[d.index] = torch.cuda.Stream(d)
        self.ctx = torch.cuda.stream(self.stream)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()
        return self.stream

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
            self.stream.synchronize()
        return False


def _stream(t):
    """the stream a library call is enqueued on (behind the uploads still in flight)"""
    st = torch.cuda.current_stream(t.device)
    wait_uploads(st)
    return st.cuda_stream


_ws = {}


def workspace(device):
    """LME scratch, one per (device, stream): calls on different streams may overlap"""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    if key not in _ws:
        nbytes = lib().trx_workspace_bytes()
        _ws[key] = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)
    return _ws[key]


def pack_params(model, cols, n=None):
    """SoA [n_param][n] host block from per-sample columns (reference argument order)."""
    assert len(cols) == N_PARAM[model], (len(cols), N_PARAM[model])
    if n is None:
        n = max(int(np.size(c)) for c in cols)
    out = np.empty((len(cols), n), dtype=np.float64)
    for i, c in enumerate(cols):
        out[i] = c
    return out


def lnl_batch(model, flags, time_d, flux_d, sigma, params_d, exptime, nsamples, out=None):
    """chi^2/2 per row on the GPU.  All tensors are fp64 CUDA tensors; params_d is [n_param][n]."""
    require_gpu()
    n = params_d.shape[1]
    assert params_d.shape[0] == N_PARAM[model] and params_d.is_contiguous()
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=params_d.device)
    with torch.cuda.device(params_d.device):
        check(lib().trx_lnl_batch(model, flags, time_d.data_ptr(), flux_d.data_ptr(),
                                  time_d.numel(), float(sigma), params_d.data_ptr(), n,
                                  float(exptime), int(nsamples), out.data_ptr(), _stream(params_d)))
    return out


def debug_row_order():
    """Testing library only (trx_debug_row_order): the cost order that the last one-row likelihood launch of this thread
    built, as (counts [16 buckets][4 shards], lists: 64 arrays of row numbers, row_blocks [n][19])."""
    L = lib()
    assert L.trx_testing, "debug_row_order needs use_testing_library()"
    n, cap = ctypes.c_long(0), ctypes.c_long(0)
    check(L.trx_debug_row_order(ctypes.byref(n), ctypes.byref(cap), None, None, None))
    counts = np.zeros(64, dtype=np.int32)
    lists = np.zeros(64 * cap.value, dtype=np.int32)
    blocks = np.zeros((n.value, 19), dtype=np.float64)
    check(L.trx_debug_row_order(ctypes.byref(n), ctypes.byref(cap), counts.ctypes.data, lists.ctypes.data,
                                blocks.ctypes.data))
    lists = lists.reshape(64, cap.value)
    return counts.reshape(16, 4), [lists[s, :max(0, min(int(counts[s]), cap.value))].copy() for s in range(64)], blocks


def debug_whole_trips(reset=False):
    """Testing library only (trx_debug_whole_trips): the 64-cell trips of pass 1 that the stencil instantiation filed whole
    and those it walked cell by cell on the current device since the last reset, as (whole, walked)."""
    L = lib()
    assert L.trx_testing, "debug_whole_trips needs use_testing_library()"
    whole, walked = ctypes.c_long(0), ctypes.c_long(0)
    check(L.trx_debug_whole_trips(ctypes.byref(whole), ctypes.byref(walked), 1 if reset else 0))
    return whole.value, walked.value


def debug_zone_chunks(reset=False):
    """Testing library only (trx_debug_zone_chunks): the pass-2 chunks that the zone loop of the one-row stencil likelihood
    kernels took on the current device since the last reset."""
    L = lib()
    assert L.trx_testing, "debug_zone_chunks needs use_testing_library()"
    chunks = ctypes.c_long(0)
    check(L.trx_debug_zone_chunks(ctypes.byref(chunks), 1 if reset else 0))
    return chunks.value


def lnl_batch_weighted(model, flags, time_d, flux_d, inv_var_d, params_d, exptime, nsamples, sec_limit=float("inf"),
                       out=None):
    """0.5 * sum_t inv_var[t] (flux[t] - model_r(t))^2 per row, model and reduction in one kernel
    (trx_lnl_batch_weighted: no grid); +inf where model is MODEL_EB and the row's secondary depth >= sec_limit.  out: an
    [n] fp64 device tensor to ADD the rows' values to (the next light curve of an evidence over several); None: a fresh
    tensor.  All tensors are fp64 CUDA tensors; params_d is [n_param][n]."""
    require_gpu()
    n, nt = params_d.shape[1], time_d.numel()
    assert params_d.shape[0] == N_PARAM[model] and params_d.is_contiguous()
    assert flux_d.numel() == nt and inv_var_d.numel() == nt
    assert time_d.is_contiguous() and flux_d.is_contiguous() and inv_var_d.is_contiguous()
    accumulate = out is not None
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=params_d.device)
    assert out.shape == (n,) and out.dtype == torch.float64 and out.is_contiguous()
    if n == 0:
        return out                     # (an empty tensor has no address to pass)
    with torch.cuda.device(params_d.device):
        check(lib().trx_lnl_batch_weighted(model, flags, time_d.data_ptr(), flux_d.data_ptr(), inv_var_d.data_ptr(),
                                           nt, params_d.data_ptr(), n, float(exptime), int(nsamples),
                                           float(sec_limit), int(accumulate), out.data_ptr(), _stream(params_d)))
    return out


def flux_grid(model, flags, time_d, params_d, exptime, nsamples, want_secdepth=True, out=None):
    """out: an [n][n_time] contiguous fp64 device tensor to write into (e.g. a slice of rows of a larger grid)"""
    require_gpu()
    n = params_d.shape[1]
    assert params_d.shape[0] == N_PARAM[model] and params_d.is_contiguous()
    if out is None:
        out = torch.empty((n, time_d.numel()), dtype=torch.float64, device=params_d.device)
    assert out.shape == (n, time_d.numel()) and out.dtype == torch.float64 and out.is_contiguous()
    sec = torch.zeros(n, dtype=torch.float64, device=params_d.device) if want_secdepth else None
    with torch.cuda.device(params_d.device):
        check(lib().trx_flux_grid(model, flags, time_d.data_ptr(), time_d.numel(),
                                  params_d.data_ptr(), n, float(exptime), int(nsamples),
                                  out.data_ptr(), sec.data_ptr() if sec is not None else None,
                                  _stream(params_d)))
    return out, sec


def chi2_grid(flux_d, grid_d, sigma):
    require_gpu()
    n, nt = grid_d.shape
    assert grid_d.is_contiguous() and flux_d.numel() == nt
    out = torch.empty(n, dtype=torch.float64, device=grid_d.device)
    with torch.cuda.device(grid_d.device):
        check(lib().trx_chi2_grid(flux_d.data_ptr(), grid_d.data_ptr(), nt, n, float(sigma),
                                  out.data_ptr(), _stream(grid_d)))
    return out


def _chi2_rows(entry, curve, grid_d, secdepth_d, sec_limit, out, *extra):
    """What the row reductions of a materialised grid share: the checks of the grid, the light curve, the secondary depths
    and `out`, a fresh `out` unless one is given to add to, and the call of libtrx's `entry`.  curve: the [n_time] vectors
    of the light curve that `entry` takes in front of the grid, (flux, inv_var) or (flux,); `extra`: its arguments between
    out_halfchi2 and the stream."""
    require_gpu()
    n, nt = grid_d.shape
    assert grid_d.dtype == torch.float64 and grid_d.is_contiguous()
    assert all(v.numel() == nt and v.is_contiguous() for v in curve)
    assert secdepth_d is None or (secdepth_d.numel() == n and secdepth_d.is_contiguous())
    accumulate = out is not None
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=grid_d.device)
    assert out.shape == (n,) and out.dtype == torch.float64 and out.is_contiguous()
    if n == 0:
        return out                     # (an empty tensor has no address to pass)
    with torch.cuda.device(grid_d.device):
        check(getattr(lib(), entry)(*(v.data_ptr() for v in curve), grid_d.data_ptr(), nt, n,
                                    secdepth_d.data_ptr() if secdepth_d is not None else None, float(sec_limit),
                                    int(accumulate), out.data_ptr(), *extra, _stream(grid_d)))
    return out


def chi2_grid_weighted(flux_d, inv_var_d, grid_d, secdepth_d=None, sec_limit=float("inf"), out=None):
    """0.5 * sum_t inv_var[t] (flux[t] - grid[r][t])^2 per row of an [n][n_time] device grid (trx_chi2_grid_weighted);
    +inf where secdepth_d[r] >= sec_limit.  out: an [n] fp64 device tensor to ADD the rows' values to (the next light
    curve of an evidence over several); None: a fresh tensor.  Rows may start at any 8-byte boundary (a view's offset)."""
    return _chi2_rows("trx_chi2_grid_weighted", (flux_d, inv_var_d), grid_d, secdepth_d, sec_limit, out)


def chi2_grid_offset(flux_d, inv_var_d, grid_d, sum_w, prior_prec, secdepth_d=None, sec_limit=float("inf"), out=None,
                     offset_out=None):
    """chi2_grid_weighted with a constant offset c ~ N(0, 1 / prior_prec) of the light curve marginalised per row
    (trx_chi2_grid_offset): 0.5 * (S2 - S1^2 / (sum_w + prior_prec)), S1 and S2 the weighted sums of the residuals and of
    their squares.  sum_w: sum(inv_var), from the host; prior_prec: 0 = flat prior, +inf = no offset (chi2_grid_weighted's
    bits).  offset_out: an [n] fp64 device tensor that receives S1 / (sum_w + prior_prec), or None.  The other arguments are
    chi2_grid_weighted's."""
    assert offset_out is None or (offset_out.shape == (grid_d.shape[0],) and offset_out.dtype == torch.float64
                                  and offset_out.is_contiguous())
    return _chi2_rows("trx_chi2_grid_offset", (flux_d, inv_var_d), grid_d, secdepth_d, sec_limit, out, float(sum_w),
                      float(prior_prec), offset_out.data_ptr() if offset_out is not None else None)


def chi2_grid_baseline(flux_d, inv_var_d, grid_d, wbasis_d, minv, secdepth_d=None, sec_limit=float("inf"), out=None,
                       coef_out=None):
    """chi2_grid_weighted with a linear baseline sum_k c_k B_k[t] of the light curve marginalised per row
    (trx_chi2_grid_baseline): 0.5 * max(S2 - sum_ij M_ij b_i b_j, 0), b_k = sum_t wbasis[k][t] (flux[t] - grid[r][t]).
    wbasis_d: [K][n_time] fp64 device tensor, the columns w_t B_k[t] / sqrt(D_k); minv: the K (K + 1) / 2 entries of the
    upper triangle of M by rows, on the host (datasets.baseline_system); K = 1 .. 4.  coef_out: an [n][K] fp64 device
    tensor that receives the scaled posterior-mean coefficients M b, or None.  The other arguments are
    chi2_grid_weighted's."""
    n, nt = grid_d.shape
    assert wbasis_d.dim() == 2 and wbasis_d.shape[1] == nt and wbasis_d.dtype == torch.float64 and wbasis_d.is_contiguous()
    k = int(wbasis_d.shape[0])
    minv = np.ascontiguousarray(minv, dtype=np.float64).reshape(-1)
    assert minv.size == k * (k + 1) // 2, "minv: the packed upper triangle of a %d x %d matrix" % (k, k)
    assert coef_out is None or (coef_out.shape == (n, k) and coef_out.dtype == torch.float64
                                and coef_out.is_contiguous())
    return _chi2_rows("trx_chi2_grid_baseline", (flux_d, inv_var_d), grid_d, secdepth_d, sec_limit, out, wbasis_d.data_ptr(),
                      k, minv.ctypes.data, coef_out.data_ptr() if coef_out is not None else None)


def chi2_grid_robust(flux_d, inv_var_d, grid_d, c0, c1, k2, secdepth=None, sec_limit=float("inf"), out=None):
    """chi2_grid_weighted with every point a two-component mixture -- its stated error, or with probability eps a Gaussian
    kappa times wider --, the membership integrated out per point (trxr_chi2_grid_robust, include/trx_robust.h): per row
    sum_t (lo_t - log1p(exp(-|A_t - B_t|))), A_t = a_t + c0, B_t = a_t k2 + c1, lo_t = min(A_t, B_t),
    a_t = 0.5 inv_var[t] (flux[t] - grid[r][t])^2, clamped at 0 and not halved.  c0, c1, k2: datasets.robust_constants.  The
    other arguments are chi2_grid_weighted's."""
    return _chi2_rows("trxr_chi2_grid_robust", (flux_d, inv_var_d), grid_d, secdepth, sec_limit, out, float(c0), float(c1),
                      float(k2))


def chi2_grid_ou(flux_d, grid_d, alpha_d, beta_d, omega_d, secdepth=None, sec_limit=float("inf"), out=None):
    """chi2_grid_weighted for a light curve with white plus exponential (Ornstein-Uhlenbeck) noise (trxn_chi2_grid_ou,
    include/trx_noise.h): per row 0.5 sum_n omega[n] (y_n - g_n)^2, y = flux - grid[r], g_0 = 0,
    g_n = alpha[n] g_(n-1) + beta[n] y_(n-1).  alpha_d, beta_d, omega_d: [n_time] fp64 device tensors
    (datasets.ou_system).  The other arguments are chi2_grid_weighted's."""
    nt = grid_d.shape[1]
    for v in (flux_d, alpha_d, beta_d, omega_d):
        assert v.numel() == nt and v.dtype == torch.float64 and v.is_contiguous()
    return _chi2_rows("trxn_chi2_grid_ou", (flux_d,), grid_d, secdepth, sec_limit, out, alpha_d.data_ptr(),
                      beta_d.data_ptr(), omega_d.data_ptr())


def chi2_grid_ss2(flux_d, grid_d, A_d, g_d, omega_d, secdepth=None, sec_limit=float("inf"), out=None):
    """chi2_grid_ou for correlated noise whose Kalman filter carries two states -- a Matern-3/2 term, two exponential terms
    -- (trxs_chi2_grid_ss2, include/trx_ss.h): per row 0.5 sum_n omega[n] z_n^2, y = flux - grid[r], u_(-1) = 0,
    z_n = y_n - u_(n-1)[0], u_n = A[n] u_(n-1) + g[n] y_n.  A_d [n_time][2][2], g_d [n_time][2], omega_d [n_time]: fp64 device
    tensors (datasets.ss2_system).  The other arguments are chi2_grid_weighted's."""
    nt = grid_d.shape[1]
    for v, per in ((flux_d, 1), (A_d, 4), (g_d, 2), (omega_d, 1)):
        assert v.numel() == per * nt and v.dtype == torch.float64 and v.is_contiguous()
    return _chi2_rows("trxs_chi2_grid_ss2", (flux_d,), grid_d, secdepth, sec_limit, out, A_d.data_ptr(), g_d.data_ptr(),
                      omega_d.data_ptr())


def chi2_grid_ou_baseline(flux_d, grid_d, alpha_d, beta_d, omega_d, cols_d, minv, secdepth=None, sec_limit=float("inf"),
                          out=None, coef_out=None):
    """chi2_grid_ou with a linear baseline sum_k c_k B_k[t] of the light curve marginalised per row under the same noise
    (trxg_chi2_grid_ou_baseline, include/trx_gls.h): 0.5 * max(S2 - sum_ij M_ij b_i b_j, 0), S2 what chi2_grid_ou sums and
    b_k = sum_n cols[k][n] z_n over the same innovations z.  cols_d: [K][n_time] fp64 device tensor, the whitened scaled
    columns; minv: the K (K + 1) / 2 entries of the upper triangle of M by rows, on the host (datasets.ou_baseline_system);
    K = 1 .. 4.  coef_out: an [n][K] fp64 device tensor that receives the scaled posterior-mean coefficients M b, or None.
    The other arguments are chi2_grid_ou's."""
    n, nt = grid_d.shape
    for v in (flux_d, alpha_d, beta_d, omega_d):
        assert v.numel() == nt and v.dtype == torch.float64 and v.is_contiguous()
    assert cols_d.dim() == 2 and cols_d.shape[1] == nt and cols_d.dtype == torch.float64 and cols_d.is_contiguous()
    k = int(cols_d.shape[0])
    assert 1 <= k <= 4, "1 .. 4 columns (got %d)" % k
    minv = np.ascontiguousarray(minv, dtype=np.float64).reshape(-1)
    assert minv.size == k * (k + 1) // 2, "minv: the packed upper triangle of a %d x %d matrix" % (k, k)
    assert coef_out is None or (coef_out.shape == (n, k) and coef_out.dtype == torch.float64 and coef_out.is_contiguous())
    return _chi2_rows("trxg_chi2_grid_ou_baseline", (flux_d,), grid_d, secdepth, sec_limit, out, alpha_d.data_ptr(),
                      beta_d.data_ptr(), omega_d.data_ptr(), cols_d.data_ptr(), k, minv.ctypes.data,
                      coef_out.data_ptr() if coef_out is not None else None)


def chi2_grid_ss2_baseline(flux_d, grid_d, A_d, g_d, omega_d, cols_d, minv, secdepth=None, sec_limit=float("inf"),
                           out=None, coef_out=None):
    """chi2_grid_ss2 with a linear baseline sum_k c_k B_k[t] of the light curve marginalised per row under the same noise
    (trxk_chi2_grid_ss2_baseline, include/trx_ss.h): 0.5 * max(S2 - sum_ij M_ij b_i b_j, 0), S2 what chi2_grid_ss2 sums and
    b_k = sum_n cols[k][n] z_n over the same innovations z.  cols_d: [K][n_time] fp64 device tensor, the whitened scaled
    columns; minv: the K (K + 1) / 2 entries of the upper triangle of M by rows, on the host (datasets.ss2_baseline_system);
    K = 1 .. 4.  coef_out: an [n][K] fp64 device tensor that receives the scaled posterior-mean coefficients M b, or None.
    The other arguments are chi2_grid_ss2's."""
    n, nt = grid_d.shape
    for v, per in ((flux_d, 1), (A_d, 4), (g_d, 2), (omega_d, 1)):
        assert v.numel() == per * nt and v.dtype == torch.float64 and v.is_contiguous()
    assert cols_d.dim() == 2 and cols_d.shape[1] == nt and cols_d.dtype == torch.float64 and cols_d.is_contiguous()
    k = int(cols_d.shape[0])
    assert 1 <= k <= 4, "1 .. 4 columns (got %d)" % k
    minv = np.ascontiguousarray(minv, dtype=np.float64).reshape(-1)
    assert minv.size == k * (k + 1) // 2, "minv: the packed upper triangle of a %d x %d matrix" % (k, k)
    assert coef_out is None or (coef_out.shape == (n, k) and coef_out.dtype == torch.float64 and coef_out.is_contiguous())
    return _chi2_rows("trxk_chi2_grid_ss2_baseline", (flux_d,), grid_d, secdepth, sec_limit, out, A_d.data_ptr(),
                      g_d.data_ptr(), omega_d.data_ptr(), cols_d.data_ptr(), k, minv.ctypes.data,
                      coef_out.data_ptr() if coef_out is not None else None)


# blocks of 256 threads a CU of scan_rows_kernel<ONE, Ss2ColsFilter<K>>, [ONE][K - 1]: kSs2ColsBlocksPerCu of
# csrc/trx_ss2_cols.hpp (tests/test_build_resources_ss2_cols.py holds the two against each other and the code object)
SS2_COLS_BLOCKS_PER_CU = ((3, 3, 3, 3), (4, 3, 4, 3))


def ss2_baseline_blocks(n, n_time, K):
    """the blocks trxk_chi2_grid_ss2_baseline launches for n rows of n_time stamps and K columns (its launcher's cap, for
    the tests): 4 rows a block, on 256 CUs as many blocks a CU as the registers of the instantiation -- a single trip up to
    128 stamps, or trips -- leave resident"""
    return min((n + 3) // 4, 256 * SS2_COLS_BLOCKS_PER_CU[1 if n_time <= 128 else 0][K - 1])


def chi2_grid_ou_mix(flux_d, grid_d, alpha_d, beta_d, omega_d, lnc, secdepth=None, sec_limit=float("inf"), out=None,
                     cand_out=None):
    """chi2_grid_ou over J candidate noise models in one pass over the grid (trxm_chi2_grid_ou_mix, include/trx_mix.h): per
    row T = -ln sum_j exp(lnc[j] - h_j), h_j what chi2_grid_ou gives on row j of alpha_d, beta_d, omega_d ([J][n_time] fp64
    device tensors; datasets.ou_mix_system), clamped at 0.  lnc: [J] float64 on the host.  cand_out: an [n][J] fp64 device
    tensor that receives the h_j, or None.  The other arguments are chi2_grid_weighted's."""
    n, nt = grid_d.shape
    assert flux_d.dtype == torch.float64
    lnc = np.ascontiguousarray(lnc, dtype=np.float64)
    assert lnc.ndim == 1
    j = int(lnc.size)
    for v in (alpha_d, beta_d, omega_d):
        assert v.shape == (j, nt) and v.dtype == torch.float64 and v.is_contiguous()
    assert cand_out is None or (cand_out.shape == (n, j) and cand_out.dtype == torch.float64 and cand_out.is_contiguous())
    return _chi2_rows("trxm_chi2_grid_ou_mix", (flux_d,), grid_d, secdepth, sec_limit, out, alpha_d.data_ptr(),
                      beta_d.data_ptr(), omega_d.data_ptr(), j, lnc.ctypes.data,
                      cand_out.data_ptr() if cand_out is not None else None)


def chi2_grid_white_mix(flux_d, grid_d, w_d, lnc, secdepth=None, sec_limit=float("inf"), out=None, cand_out=None):
    """chi2_grid_weighted over J candidate white-noise models in one pass over the grid (trxv_chi2_grid_white_mix,
    include/trx_mix.h): per row T = -ln sum_j exp(lnc[j] - h_j), h_j what chi2_grid_weighted gives with inv_var = row j of w_d
    (a [J][n_time] fp64 device tensor; datasets.white_mix_system), clamped at 0.  lnc: [J] float64 on the host.  cand_out: an
    [n][J] fp64 device tensor that receives the h_j, or None.  The other arguments are chi2_grid_weighted's."""
    n, nt = grid_d.shape
    assert flux_d.dtype == torch.float64
    lnc = np.ascontiguousarray(lnc, dtype=np.float64)
    assert lnc.ndim == 1
    j = int(lnc.size)
    assert 1 <= j <= 8, "1 .. 8 candidates (got %d)" % j
    assert w_d.shape == (j, nt) and w_d.dtype == torch.float64 and w_d.is_contiguous()
    assert cand_out is None or (cand_out.shape == (n, j) and cand_out.dtype == torch.float64 and cand_out.is_contiguous())
    return _chi2_rows("trxv_chi2_grid_white_mix", (flux_d,), grid_d, secdepth, sec_limit, out, w_d.data_ptr(), j,
                      lnc.ctypes.data, cand_out.data_ptr() if cand_out is not None else None)


def white_mix_blocks(n, n_time, n_cand):
    """the blocks trxv_chi2_grid_white_mix launches for n rows of n_time stamps and n_cand candidates (its launcher's cap,
    for the tests): 4 rows a block, at most 8 blocks a CU -- fewer where the staged [1 + n_cand] vectors fill the 160 KB of
    LDS -- on 256 CUs; staged up to ((2 * 2048) // (1 + n_cand)) & ~1 stamps"""
    stage = n_time <= (((2 * 2048) // (1 + n_cand)) & ~1)
    lds = (1 + n_cand) * ((n_time + 1) & ~1) * 8 if stage else 0
    per_cu = min((160 * 1024) // lds, 8) if lds else 8
    return min((n + 3) // 4, 256 * per_cu)


def chi2_grid_white_baseline(flux_d, grid_d, w_d, basis_d, minv, lnc, secdepth=None, sec_limit=float("inf"), out=None,
                             cand_out=None, coef_out=None):
    """chi2_grid_white_mix with K baseline columns marginalised under every candidate (trxb_chi2_grid_white_baseline,
    include/trx_gls.h): per row T = -ln sum_j exp(lnc[j] - h_j), h_j = 0.5 max(S2_j - b_j . Ainv_j b_j, 0) with
    S2_j = sum_t w[j][t] d_t^2 and b_jk = sum_t w[j][t] basis[k][t] d_t, clamped at 0.  w_d: [J][n_time], basis_d: [K][n_time]
    fp64 device tensors; minv: [J][K (K + 1) / 2] and lnc: [J] float64 on the host (datasets.white_baseline_system).
    cand_out: an [n][J] fp64 device tensor that receives the h_j, coef_out: an [n][J][K] one that receives Ainv_j b_j, or
    None.  The other arguments are chi2_grid_weighted's."""
    n, nt = grid_d.shape
    assert flux_d.dtype == torch.float64
    lnc = np.ascontiguousarray(lnc, dtype=np.float64)
    assert lnc.ndim == 1
    j = int(lnc.size)
    assert 1 <= j <= 8, "1 .. 8 candidates (got %d)" % j
    assert w_d.shape == (j, nt) and w_d.dtype == torch.float64 and w_d.is_contiguous()
    assert basis_d.dim() == 2 and basis_d.shape[1] == nt and basis_d.dtype == torch.float64 and basis_d.is_contiguous()
    k = int(basis_d.shape[0])
    assert 1 <= k <= 4, "1 .. 4 columns (got %d)" % k
    minv = np.ascontiguousarray(minv, dtype=np.float64)
    assert minv.shape == (j, k * (k + 1) // 2), "minv: per candidate the packed upper triangle of a %d x %d matrix" % (k, k)
    assert cand_out is None or (cand_out.shape == (n, j) and cand_out.dtype == torch.float64 and cand_out.is_contiguous())
    assert coef_out is None or (coef_out.shape == (n, j, k) and coef_out.dtype == torch.float64
                                and coef_out.is_contiguous())
    return _chi2_rows("trxb_chi2_grid_white_baseline", (flux_d,), grid_d, secdepth, sec_limit, out, w_d.data_ptr(),
                      basis_d.data_ptr(), j, k, minv.ctypes.data, lnc.ctypes.data,
                      cand_out.data_ptr() if cand_out is not None else None,
                      coef_out.data_ptr() if coef_out is not None else None)


def white_lin_blocks(n, n_time, n_cand, n_terms):
    """the blocks trxb_chi2_grid_white_baseline launches for n rows of n_time stamps, n_cand candidates and n_terms columns
    (its launcher's cap, for the tests): 4 rows a block; a CU holds 4 blocks up to 24 sums a row
    (n_cand * (1 + n_terms) <= 24: at most 128 VGPRs), 3 up to 35 (at most 168) and 2 at 40 (at most 256) -- fewer where
    the LDS of a block, the candidates' packed inverses and the staged [1 + n_cand + n_terms] vectors, fills the 160 KB -- on
    256 CUs; staged up to ((2 * 2048) // (1 + n_cand + n_terms)) & ~1 stamps"""
    vectors = 1 + n_cand + n_terms
    sums = n_cand * (1 + n_terms)
    stage = n_time <= (((2 * 2048) // vectors) & ~1)
    lds = 8 * (((n_cand * (n_terms * (n_terms + 1) // 2) + 1) & ~1) + (vectors * ((n_time + 1) & ~1) if stage else 0))
    by_regs = 4 if sums <= 24 else 3 if sums <= 35 else 2
    return min((n + 3) // 4, 256 * min((160 * 1024) // lds, by_regs))


def softmin_rows(cand_d, lnc, out=None):
    """The soft minimum over the J rows of cand_d (trxt_softmin_rows, include/trx_shift.h): per column r
    T = -ln sum_j exp(lnc[j] - cand_d[j][r]), clamped at 0.  cand_d: a [J][n] fp64 device tensor whose rows are contiguous
    (any row stride >= n); lnc: [J] float64 on the host.  out: an [n] fp64 device tensor that T is added to; None: a new
    tensor that receives T."""
    require_gpu()
    assert cand_d.dim() == 2 and cand_d.dtype == torch.float64
    j, n = (int(v) for v in cand_d.shape)
    stride = int(cand_d.stride(0)) if j > 1 else n       # (a single row has no next row to reach)
    assert n <= 1 or cand_d.stride(1) == 1
    assert n == 0 or stride >= n
    lnc = np.ascontiguousarray(lnc, dtype=np.float64)
    assert lnc.shape == (j,)
    accumulate = out is not None
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=cand_d.device)
    assert out.shape == (n,) and out.dtype == torch.float64 and out.is_contiguous()
    if n == 0:
        return out                     # (an empty tensor has no address to pass)
    with torch.cuda.device(cand_d.device):
        check(lib().trxt_softmin_rows(cand_d.data_ptr(), stride, n, j, lnc.ctypes.data, int(accumulate), out.data_ptr(),
                                      _stream(cand_d)))
    return out


def log_mean_exp(logw_d, n_total):
    """Device log-mean-exp; returns a 1-element device tensor (no sync)."""
    require_gpu()
    ws = workspace(logw_d.device)
    out = torch.empty(1, dtype=torch.float64, device=logw_d.device)
    with torch.cuda.device(logw_d.device):
        check(lib().trx_log_mean_exp(logw_d.data_ptr(), logw_d.numel(), int(n_total),
                                     out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                     _stream(logw_d)))
    return out


def lnz_scenario(model, flags, time_d, flux_d, sigma, params_d, exptime, nsamples, lnprior_d,
                 n_total, lnsigma):
    """Fused chi^2/2 -> log-mean-exp.  Returns (halfchi2[n], lnz[1]) device tensors."""
    require_gpu()
    n = params_d.shape[1]
    device = params_d.device
    flags |= EXTRA_FLAGS
    count_launch(n, time_d.numel())
    h = torch.empty(max(n, 1), dtype=torch.float64, device=device)
    out = torch.empty(1, dtype=torch.float64, device=device)
    ws = workspace(device)
    ev = None
    if TRACE is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    with torch.cuda.device(device):
        check(lib().trx_lnz_scenario(model, flags, time_d.data_ptr(), flux_d.data_ptr(),
                                     time_d.numel(), float(sigma), params_d.data_ptr(), n,
                                     float(exptime), int(nsamples),
                                     lnprior_d.data_ptr() if lnprior_d is not None else None,
                                     int(n_total), float(lnsigma), h.data_ptr(), out.data_ptr(),
                                     ws.data_ptr(), ws.numel() * 8, _stream(params_d)))
    if ev is not None:
        ev[1].record()
        keep = params_d[:, :TRACE_SAMPLE_ROWS].clone() if len(TRACE) < 64 else None
        TRACE.append((model, flags, n, time_d.numel(), ev[0], ev[1], keep))
    return h[:n], out


def lnz_from_halfchi2(h_d, lnprior_d, n_total, lnsigma):
    """lnZ (1-element device tensor) from device chi^2/2 values of the masked draws."""
    require_gpu()
    device = h_d.device
    out = torch.empty(1, dtype=torch.float64, device=device)
    ws = workspace(device)
    with torch.cuda.device(device):
        check(lib().trx_lnz_from_halfchi2(h_d.data_ptr() if h_d.numel() else None,
                                          lnprior_d.data_ptr() if lnprior_d is not None else None,
                                          h_d.numel(), int(n_total), float(lnsigma),
                                          out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                          _stream(h_d)))
    return out


def lnz_moments_from_halfchi2(h_d, lnprior_d, n_total, lnsigma):
    """(lnZ, lnM2, lnWmax) as a 3-element device tensor from device chi^2/2 values of the masked draws
    (trx_lnz_moments_from_halfchi2: lnZ is lnz_from_halfchi2's value bit for bit)."""
    require_gpu()
    device = h_d.device
    out = torch.empty(3, dtype=torch.float64, device=device)
    ws = workspace(device)
    with torch.cuda.device(device):
        check(lib().trx_lnz_moments_from_halfchi2(h_d.data_ptr() if h_d.numel() else None,
                                                  lnprior_d.data_ptr() if lnprior_d is not None else None,
                                                  h_d.numel(), int(n_total), float(lnsigma),
                                                  out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                  _stream(h_d)))
    return out


POST_MAX_ROWS = 4096       # TRX_POST_MAX_ROWS (include/trx.h)
QUANTILES_MAX = 16         # quantile levels of one trx_grid_quantiles call


def grid_quantiles(grid_d, q, rows_d=None, scale_d=None):
    """Column quantiles of a row-major device grid (trx_grid_quantiles): np.quantile(v, q, axis=0) as an [n_q][n_cols]
    device tensor (no sync), v the rows of grid_d -- or, with rows_d (int64 device tensor, repeats allowed), the rows
    grid_d[rows_d] -- and, with scale_d (one fp64 per row of v), 1 - scale[:, None] * (1 - v)."""
    require_gpu()
    assert grid_d.dim() == 2 and grid_d.dtype == torch.float64 and grid_d.is_contiguous()
    n_grid_rows, n_cols = grid_d.shape
    n_rows = n_grid_rows
    if rows_d is not None:
        assert rows_d.dtype == torch.int64 and rows_d.is_contiguous() and rows_d.device == grid_d.device
        n_rows = rows_d.numel()
    if scale_d is not None:
        assert scale_d.dtype == torch.float64 and scale_d.is_contiguous() and scale_d.numel() == n_rows
    qa = np.ascontiguousarray(q, dtype=np.float64).ravel()
    out = torch.empty((qa.size, n_cols), dtype=torch.float64, device=grid_d.device)
    with torch.cuda.device(grid_d.device):
        check(lib().trx_grid_quantiles(grid_d.data_ptr(), n_grid_rows, n_cols,
                                       rows_d.data_ptr() if rows_d is not None else None,
                                       scale_d.data_ptr() if scale_d is not None else None, n_rows,
                                       qa.ctypes.data, qa.size, out.data_ptr(), _stream(grid_d)))
    return out
WARP_DIMS, WARP_BINS = 7, 64                  # TRX_WARP_DIMS, TRX_WARP_BINS: the importance map of trx_draw_args.warp
WARP_BRANCH = 8 + WARP_DIMS * WARP_BINS       # TRX_WARP_BRANCH: 64-bit words of one branch's weight histogram


def posterior_from_halfchi2(h_d, lnprior_d, lnsigma, rows, seed):
    """Systematic resampling of the weights exp(-ln sigma - 0.5 ln 2 pi - h [+ lnprior]) on the device
    (trx_posterior_from_halfchi2): (positions, header) as device tensors -- `rows` list positions (int64, non-decreasing;
    -1 where no row carries weight) and the header (u, X, ln S, rows with positive weight)."""
    require_gpu()
    device = h_d.device
    pos = torch.empty(int(rows), dtype=torch.int64, device=device)
    hdr = torch.empty(4, dtype=torch.float64, device=device)
    ws = workspace(device)
    with torch.cuda.device(device):
        check(lib().trx_posterior_from_halfchi2(h_d.data_ptr() if h_d.numel() else None,
                                                lnprior_d.data_ptr() if lnprior_d is not None else None,
                                                h_d.numel(), float(lnsigma), int(rows), int(seed),
                                                pos.data_ptr() if rows else None, hdr.data_ptr(),
                                                ws.data_ptr(), ws.numel() * 8, _stream(h_d)))
    return pos, hdr


def warp_hist_from_halfchi2(draw_args, h_d, lnprior_d, idx_d, lnsigma):
    """The weight histogram of one branch from device chi^2/2 values (trxw_hist_from_halfchi2, include/trx_warp.h): a device
    int64[WARP_BRANCH] -- word 0 X's bits, word 1 the rows with weight, words 8.. the [WARP_DIMS][WARP_BINS] sums of
    floor(w 2^32) over the bins of the draws' pre-map uniforms.  draw_args: the ctypes trx_draw_args the draws were made
    with (host; its seed and consumed slots); idx_d: the rows' draw indices (int64).  No sync."""
    require_gpu()
    device = h_d.device
    assert idx_d.dtype == torch.int64 and idx_d.is_contiguous() and idx_d.numel() == h_d.numel()
    assert h_d.dtype == torch.float64 and h_d.is_contiguous()
    out = torch.empty(WARP_BRANCH, dtype=torch.int64, device=device)
    ws = workspace(device)
    with torch.cuda.device(device):
        check(lib().trxw_hist_from_halfchi2(ctypes.addressof(draw_args), h_d.data_ptr() if h_d.numel() else None,
                                                lnprior_d.data_ptr() if lnprior_d is not None else None,
                                                idx_d.data_ptr() if idx_d.numel() else None, h_d.numel(), float(lnsigma),
                                                out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(h_d)))
    return out


# The Monte-Carlo moments (lnM2, lnWmax) of the branches a lnZ_* call evaluates, on their way to sharding.run_units
# without entering the call's result dicts: run_units opens a sink on each thread that evaluates its units (when
# fused.MOMENTS is on), the evidence paths that are not the library's deferred records (the numpy mode, the operator
# chain, a call resolved at once) append one pair per branch, in branch order, and run_units takes a unit's pairs as
# the part of the list its call appended (moments_mark / moments_since).  An open sink is also what makes a native call
# ask the library for the moments.  Thread-local: the worker threads of run_units each have their own.
_moments_tls = threading.local()


def moments_swap(sink):
    """opens ([]) or closes (None) this thread's sink; returns the one it replaces"""
    old = getattr(_moments_tls, "sink", None)
    _moments_tls.sink = sink
    return old


def moments_mark():
    sink = getattr(_moments_tls, "sink", None)
    return None if sink is None else len(sink)


def moments_since(mark):
    """the pairs appended since moments_mark() returned `mark`"""
    sink = getattr(_moments_tls, "sink", None)
    return [] if sink is None or mark is None else sink[mark:]


def moments_wanted():
    return getattr(_moments_tls, "sink", None) is not None


def moments_emit(lnm2, lnwmax):
    sink = getattr(_moments_tls, "sink", None)
    if sink is not None:
        sink.append((float(lnm2), float(lnwmax)))
