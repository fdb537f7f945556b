"""The ten lnZ_* of calc_probs on the fused per-draw kernel (trx_draw_scenario, include/trx.h).

tests/torch_pipeline.py (round 1's device path) expresses a scenario as ~350 elementwise torch launches (samplers, splines,
priors, masks); here the whole draw -> derive -> mask -> prior chain of a scenario is ONE HIP
kernel over the N draws, fed with staged random numbers in the reference's draw order (the RNG
classes of device_pipeline: torch's device generator, or numpy's global stream), followed by the
compaction (nonzero + one index_select), the likelihood / log-mean-exp kernels and the best-fit
table.  About 15 launches per scenario branch instead of ~360.

Host work per call: the constants of the broken power laws (priors.py:16-383), the Moe &
Di Stefano rate constants (priors.py:601-660) and table pointers -- nothing per draw.
"""
import contextlib
import ctypes
import math
import os
import threading
from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, funcs
from .datasets import (Datasets, baseline_system, ou_baseline_system, ou_mix_system, ou_system, robust_constants, white_mix_system,
                       ss2_baseline_system, ss2_system, white_baseline_system)
from . import device_pipeline as dp
from . import marginal_likelihoods as ml
from ._lib import FLAG_COMPANION_IS_HOST, FLAG_SCALAR_K, MODEL_EB, MODEL_EB_TWIN, MODEL_TP
from .constants import G, Msun, Rsun, pi

F64 = torch.float64
N_BEST = ml.N_BEST
# rows of the best-fit table a call returns.  The reference's lnZ_* return the 100 best draws but
# calc_probs reads only the best one (triceratops.py:809-823); run_units asks for 1 row while it
# evaluates the units of a calc_probs with the device generator, which turns the top-101 selection
# (a device sort, ~15 launches per branch) into one argmin.  Direct lnZ_* calls keep 100.
TABLE_ROWS = N_BEST
TABLE_MAX_ROWS = 127       # TRX_TABLE_MAX_ROWS (include/trx.h)
# True: with the device generator (set_sampling("device")) the random numbers are made inside the
# draw kernel (Philox4x32-10 keyed by one 62-bit seed per call taken from torch's CPU generator, so
# torch.manual_seed reproduces a run); False: torch's device generator fills staged arrays
PHILOX = True
_tls = threading.local()


def set_thread_seed(seed):
    """key of the calls this thread makes next (sharding.run_units: one seed per work unit, so a
    unit's draws do not depend on which rank or thread evaluates it); None = take the key from
    torch's CPU generator"""
    _tls.seed, _tls.count = seed, 0


def threadable():
    """True when lnZ_* calls may run side by side on several host threads: device sampling with
    the kernel's own random numbers (no global generator is consumed)"""
    return ml._sampling["mode"] == "device" and PHILOX and isinstance(dp.RNG, dp.TorchRng)


def staged_native():
    """True when lnZ_* calls under calc_probs go to the library's chain with STAGED random numbers: numpy's global
    stream consumed on the calling thread in the reference's order (set_sampling("numpy-device")).  One host thread
    only; the calls can still be deferred and dealt to streams like the device generator's."""
    return ml._sampling["mode"] == "numpy-device" and NATIVE and isinstance(dp.RNG, dp.NumpyStreamRng)


def _mix(seed, count):
    """splitmix64 of (seed, count): a 62-bit Philox key"""
    z = (seed * 0x9E3779B97F4A7C15 + count * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return (z ^ (z >> 31)) >> 2


DUMP = None        # tests: a list that receives the [9][N] tensor of random numbers every call used
HOST_TARGET, HOST_COMPANION, HOST_FIELD = 0, 1, 2
COMP_NONE, COMP_BOUND, COMP_FIELD = 0, 1, 2
PRIOR_NONE, PRIOR_BOUND_TP, PRIOR_BOUND_EB, PRIOR_FIELD = 0, 1, 2, 3
MAX_KNOTS, N_SPLINES, MAX_CC, MAX_LUT = 16, 6, 256, 160
SPLINE_DOUBLES = 1 + 5 * MAX_KNOTS

_d3 = ctypes.c_double * 3
_vp = ctypes.c_void_p


class PowerLaw(ctypes.Structure):
    _fields_ = [("nseg", ctypes.c_int), ("ones", ctypes.c_int), ("norm", ctypes.c_double),
                ("hi", _d3), ("lo", _d3), ("cum", _d3), ("p1", _d3), ("amp", _d3), ("base", _d3),
                ("ip", _d3)]


class DrawArgs(ctypes.Structure):
    _fields_ = ([("N", ctypes.c_long)]
                + [(k, ctypes.c_int) for k in ("planet", "host", "comp", "prior", "parallel", "flat",
                                               "use_cc", "n_cc", "n_lut")]
                + [(k, ctypes.c_double) for k in ("P_lo", "P_hi", "M_s", "R_s", "Teff", "u1", "u2",
                                                  "ecc_pow", "teff_cap", "f0_tess", "f0_band",
                                                  "dist_pc", "kepler_c", "f1", "f2", "f3", "t2", "t3",
                                                  "t4", "t5", "bg_const", "bg_amp")]
                + [(k, PowerLaw) for k in ("law_rp_hi", "law_rp_lo", "law_q", "law_qc")]
                + [(k, _vp) for k in ("splines", "cc_seps", "cc_cons", "lut", "f_mass", "f_radius",
                                      "f_teff", "f_logg", "f_fr", "f_delta", "f_frband", "f_u1", "f_u2",
                                      "uP", "uQc", "uRp", "uInc", "uQ", "uEcc", "uW", "ecc_in", "qc_in",
                                      "idx", "cols", "mask", "mask_twin", "lnprior", "flag")]
                + [("use_philox", ctypes.c_int), ("range_P", ctypes.c_int), ("n_field_draw", ctypes.c_long),
                   ("pretest", ctypes.c_int), ("seed", ctypes.c_ulonglong), ("dump", _vp),
                   ("sep_in", _vp), ("dm_out", _vp), ("warp", _vp)])


class ScenarioArgs(ctypes.Structure):
    """trx_scenario_args (include/trx.h)"""
    _fields_ = [("draw", ctypes.POINTER(DrawArgs)), ("time", _vp), ("flux", _vp),
                ("n_time", ctypes.c_int), ("nsupersample", ctypes.c_int),
                ("sigma", ctypes.c_double), ("lnsigma", ctypes.c_double), ("exptime", ctypes.c_double),
                ("flags", ctypes.c_int), ("want_prior", ctypes.c_int),
                ("out", ctypes.POINTER(ctypes.c_double)), ("out_flag", ctypes.POINTER(ctypes.c_int)),
                ("table_rows", ctypes.c_int), ("table", _vp), ("warp_hist", _vp),
                ("post_rows", ctypes.c_int), ("post", _vp), ("post_seed", ctypes.c_ulonglong)]


def _post_branch(M):
    """TRX_POST_BRANCH(M): doubles of one branch's posterior block (include/trx.h)"""
    return 8 + 16 * M


def _table_branch(K):
    """TRX_TABLE_BRANCH(K): doubles of one branch's table (include/trx.h)"""
    return 15 * (K + 1)


SCENARIO_OUT = 18      # TRX_SCENARIO_OUT
SCEN_TIES, SCEN_STATUS = 16, 17      # record slots: rows holding the smallest chi^2; 1 = a row was never written
SCENARIO_OUT_MOMENTS = 20            # TRX_SCENARIO_OUT_MOMENTS: a record of TRX_FLAG_WEIGHT_MOMENTS ...
SCEN_LNM2, SCEN_LNWMAX = 18, 19      # ... + the log mean squared weight and the largest weight's share
# True: a lnZ_* call that only has to return its best draw (calc_probs: TABLE_ROWS == 1, device
# generator) is ONE library call, trx_scenario_evidence; False: the chain of torch operators around
# trx_draw_scenario / trx_lnz_scenario below (the path of the 100-row table; kept as cross-check)
NATIVE = os.environ.get("TRX_NATIVE", "1") != "0"      # TRX_NATIVE=0: A/B runs of whole programs
# the draw kernel's fp32 pre-test of the geometry (csrc/trx_draw.hip, may_transit): the fp64 mask is evaluated
# only for the draws it lets through.  Same masks; TRX_PRETEST=0 / PRETEST = False evaluates every draw (tests)
PRETEST = os.environ.get("TRX_PRETEST", "1") != "0"
# the native calls of calc_probs / calc_probs_many (sharding.run_units: a moments sink is open, _lib.moments_begin) ask
# the library for the Monte-Carlo moments of every evidence as well (TRX_FLAG_WEIGHT_MOMENTS: records of
# SCENARIO_OUT_MOMENTS doubles; lnZ and the best draw are the same bits either way).  False: records as before, and
# the target's error attributes are NaN (tests)
MOMENTS = True
# Posterior samples per scenario: M > 0 makes a native lnZ_* call ask the library for M draws of
# each branch in proportion to their weight in the evidence (trx_scenario_args.post_rows: systematic resampling on the
# device); every result dict gains "posterior" -- a dict of [M] arrays under the dict's own keys plus "lnw" (the sampled
# draws' log-weights) and "row" (their positions in the branch's list of masked draws), or None where no draw carries
# weight.  The operator chain produces the same key through trx_posterior_from_halfchi2.  Every other key: same bits.
POSTERIOR_ROWS = 0
POST_MAX_ROWS = _lib.POST_MAX_ROWS
# The columns of a branch, once.  *_COLS: as the library writes them (trx_draw_args.cols, include/trx.h) -- the first
# slots of a branch record, the rows of a table and of a posterior block ("a": the orbit's semi-major axis in cm,
# "a_twin": at 2 P_orb).  RECORD_COLS: the reference's names (marginal_likelihoods.py:152-171) in the order of a row of
# sharding.run_units' table; _physical below takes the one to the other.
PLANET_COLS = ("R_p", "P_orb", "inc", "a", "R_s", "u1", "u2", "ecc", "argp", "fluxratio_comp", "M_s")
BINARY_COLS = ("R_EB", "fluxratio_EB", "P_orb", "inc", "a", "R_s", "u1", "u2", "ecc", "argp", "fluxratio_comp", "a_twin",
               "M_EB", "M_s")
RECORD_COLS = ("M_s", "R_s", "u1", "u2", "P_orb", "inc", "b", "R_p", "ecc", "argp", "M_EB", "R_EB", "fluxratio_EB",
               "fluxratio_comp", "lnZ")
POSTERIOR_PARAMS = RECORD_COLS[:14]      # the physical columns
POSTERIOR_KEYS = POSTERIOR_PARAMS + ("lnw", "row")
_POST_SALT = 0x706F7374       # post_seed = _mix(the call's draw seed, this): no generator is advanced
# calc_posteriors_many(keep="summary"): a tuple of quantile levels q.  The rank that evaluated a unit then reduces every
# scenario row's samples to len(q) quantiles of the 14 physical columns BEFORE the table is gathered
# (sharding.RowLayout.summarise: quantile columns instead of sample columns).  None: the rows carry their samples.
POSTERIOR_SUMMARY = None


def _physical(t, planet, twin):
    """a branch's columns in the library's order ([11] planet / [14] binary, any trailing shape: [K] draws of a table
    or posterior block, [calls] of a pass) -> the 14 physical columns in RECORD_COLS order.  The twin branch is the
    binary at 2 P_orb on the orbit of 2 P_orb."""
    c = dict(zip(PLANET_COLS if planet else BINARY_COLS, t))
    P, sm, Rh, ecc, w, inc = c["P_orb"], c["a"], c["R_s"], c["ecc"], c["argp"], c["inc"]
    if twin:
        P, sm = 2 * P, c["a_twin"]
    c["P_orb"] = P
    c["b"] = sm * (1 - ecc ** 2) / (1 + ecc * np.sin(w * pi / 180)) * np.cos(inc * pi / 180) / (Rh * Rsun)
    return [c[k] if k in c else np.zeros(np.shape(P)) for k in POSTERIOR_PARAMS]


def record_row(d):
    """a result dict's best draw and lnZ, in RECORD_COLS order"""
    return [d[c] if c == "lnZ" else d[c][0] for c in RECORD_COLS]


def posterior_to_flat(post, M):
    """a "posterior" dict as the sample columns of a row of sharding.run_units' table, NaN for None"""
    if post is None:
        return np.full(len(POSTERIOR_KEYS) * M, np.nan)
    return np.concatenate([np.asarray(post[k], dtype=np.float64) for k in POSTERIOR_KEYS])


def posterior_from_flat(flat, M):
    """the sample columns of a row of sharding.run_units' table (sharding.RowLayout: len(POSTERIOR_KEYS) * M doubles,
    POSTERIOR_KEYS order) as a "posterior" dict; None for a row of NaN ("lnw" is the defining slot)"""
    flat = np.asarray(flat, dtype=np.float64)
    if flat.size != len(POSTERIOR_KEYS) * M or M == 0 or np.isnan(flat[POSTERIOR_KEYS.index("lnw") * M]):
        return None
    post = {k: flat[i * M:(i + 1) * M].copy() for i, k in enumerate(POSTERIOR_KEYS)}
    post["row"] = post["row"].astype(np.int64)
    return post


# Adaptive importance sampling (target.calc_probs_refined sets both for the length of a pass):
# WARP_GRIDS = {unit: [7][65] edges}: the native lnZ_* call of work unit `unit` (sharding.run_units names the unit it is
# evaluating: set_thread_unit) draws its uniforms through that importance map (trx_draw_args.warp); a unit without an
# entry draws as ever.  WARP_HIST = True: every native call also returns the histogram of its evidence's weight over the
# bins of its uniforms (trx_scenario_args.warp_hist) -- WARP_BRANCH more columns per scenario row in run_units' table:
# X, the number of rows with weight, six zeros, then the [7][64] sums as doubles.  Needs the kernel's own random numbers.
WARP_GRIDS = None
WARP_HIST = False
WARP_BRANCH = _lib.WARP_BRANCH


# Several light curves with per-point errors: a lnZ_* call whose `time` is a datasets.Datasets
# object evaluates every masked draw in full on every dataset -- trx_flux_grid writes the model curves of a chunk of rows,
# trx_chi2_grid_weighted adds their weighted chi^2/2 -- through run_operator_chain: no bounded evaluation, no launch
# chain.  DATASET_GRID_BYTES bounds the grid of one chunk; the results are the same bits for any value.
# DATASET_EVALUATION = "fused": one trx_lnl_batch_weighted per dataset over all rows of a branch instead -- model and
# weighted chi^2 in one kernel, no grid, no chunks; the same evidences to rounding (target.calc_probs_datasets sets it
# for the length of a call).
# A dataset with an `offset_sigma` (datasets.py) has its constant baseline offset marginalised per draw: its reduction is
# trx_chi2_grid_offset in place of trx_chi2_grid_weighted (grid evaluation only).  DATASET_OFFSETS = {}: every such call
# also leaves {work unit: [per branch, an [L] array]} there -- the posterior-mean offset of the branch's best draw per
# dataset, in the call's (its star's) normalisation, NaN for a dataset without an offset (target.dataset_offsets).
# A dataset with a `baseline` has the coefficients of its baseline columns -- and its offset, if it has offset_sigma, as
# term 0 of the same system (datasets.baseline_system) -- marginalised per draw by trx_chi2_grid_baseline.
# DATASET_BASELINES = {}: every such call leaves {work unit: [per branch, a list per dataset: None or the [K_b] posterior-
# mean coefficients of the branch's best draw]} there, in the call's normalisation (target.dataset_baselines).
# A dataset with `red_sigma` / `red_timescale` has correlated (Ornstein-Uhlenbeck) noise next to its white errors: its
# reduction is trxn_chi2_grid_ou on the alpha, beta, omega of datasets.ou_system (grid evaluation only).
# With `red_kernel` = "matern32" or "ou2" next to them the noise is a Matern-3/2 term or two exponential terms: a process with
# a two-dimensional state, reduced by trxs_chi2_grid_ss2 on the A, g, omega of datasets.ss2_system (grid evaluation only).
# A dataset with a `red_grid` has that noise's amplitude and time scale marginalised over its candidates per draw: its
# reduction is trxm_chi2_grid_ou_mix on the tables and log-weights of datasets.ou_mix_system (grid evaluation only).
# DATASET_RED_NOISE = {}: every such call leaves {work unit: [per branch, a list per dataset: None or the [J] posterior
# weights of the candidates at the branch's best draw, softmax_j(lnc_j - h_j)]} there (target.dataset_red_noise).
# A dataset with a `t0_grid` (Datasets.t0_grids) has a transit-time shift marginalised over its nodes per draw: its model grid
# and its reduction -- whichever of the above -- run once per node on the stamps time + shift_j, and trxt_softmin_rows folds
# the nodes' terms into one (grid evaluation only).  DATASET_T0 = {}: every such call leaves {work unit: [per branch, a list
# per dataset: None or the [J] posterior weights of the nodes at the branch's best draw, softmax_j(ln pi_j - h_j)]} there
# (target.dataset_t0); the offsets, baselines and red-noise weights of such a dataset are those of its heaviest node.
# A dataset with `outlier_frac` / `outlier_scale` (Datasets.outliers) has every point's membership in a kappa times wider
# outlier component integrated out per draw: its reduction is trxr_chi2_grid_robust on the constants of
# datasets.robust_constants (grid evaluation only).  DATASET_OUTLIERS = {}: every such call leaves {work unit: [per branch, a
# list per dataset: None or the [T] posterior outlier probabilities of the points at the branch's best draw
# (_numerics.robust_responsibility; with a t0_grid on its heaviest node)]} there (target.dataset_outliers).
# A dataset with `red_baseline` (Datasets.red_baselines) has the columns' coefficients marginalised per draw under its
# red_sigma / red_timescale noise: its reduction is trxg_chi2_grid_ou_baseline on the tables of datasets.ou_baseline_system
# (grid evaluation only).  DATASET_RED_BASELINES = {}: every such call leaves {work unit: [per branch, a list per dataset:
# None or the [K_b] posterior-mean coefficients at the branch's best draw, in the call's normalisation (with a t0_grid on
# its heaviest node)]} there (target.dataset_red_baselines).
# A dataset with a `white_grid` (Datasets.white_grids) has the size of its white noise -- an error scale and a jitter --
# marginalised over its candidates per draw: its reduction is trxv_chi2_grid_white_mix on the weights and log-weights of
# datasets.white_mix_system (grid evaluation only).  DATASET_WHITE_NOISE = {}: every such call leaves {work unit: [per branch, a
# list per dataset: None or the [J] posterior weights of the candidates at the branch's best draw, softmax_j(lnc_j - h_j)
# (with a t0_grid on its heaviest node)]} there (target.dataset_white_noise).
# A dataset with `white_baseline` columns next to its white_grid (Datasets.white_baselines) has them marginalised under every
# candidate: its reduction is trxb_chi2_grid_white_baseline on the tables of datasets.white_baseline_system (grid evaluation
# only).  DATASET_WHITE_BASELINES = {}: every such call leaves {work unit: [per branch, a list per dataset: None or
# {"coef": the [J][K] posterior-mean coefficients under each candidate at the branch's best draw, in the call's
# normalisation, "mean": [K] their average under the candidates' posterior weights} (with a t0_grid on its heaviest
# node)]} there (target.dataset_white_baselines).
# A dataset with `red_kernel_baseline` columns (Datasets.red_kernel_baselines) has their coefficients marginalised per draw
# under its Matern-3/2 or two-term noise: its reduction is trxk_chi2_grid_ss2_baseline on the tables of
# datasets.ss2_baseline_system (grid evaluation only).  DATASET_RED_KERNEL_BASELINES = {}: every such call leaves {work unit:
# [per branch, a list per dataset: None or the [K_b] posterior-mean coefficients at the branch's best draw, in the call's
# normalisation (with a t0_grid on its heaviest node)]} there (target.dataset_red_kernel_baselines).
DATASET_GRID_BYTES = 512 << 20
DATASET_EVALUATIONS = ("grid", "fused")
DATASET_EVALUATION = "grid"
DATASET_OFFSETS = None
DATASET_BASELINES = None
DATASET_RED_NOISE = None
DATASET_T0 = None
DATASET_OUTLIERS = None
DATASET_RED_BASELINES = None
DATASET_WHITE_NOISE = None
DATASET_WHITE_BASELINES = None
DATASET_RED_KERNEL_BASELINES = None
# An importance map (WARP_GRIDS) applies to a datasets call as to any other: its draws are trx_draw_scenario's.  The weight
# histogram of the library's own chain (WARP_HIST) does not exist here -- chi^2/2 is computed outside that chain -- so
# DATASET_WARP_HIST = {}: every datasets call leaves {work unit: [branches][WARP_BRANCH] uint64 words} there, one
# trxw_hist_from_halfchi2 per branch on the numbers its evidence is formed from (target.calc_probs_datasets_refined
# opens it for the length of an adaptation pass).  The row layout of sharding.run_units does not change.
DATASET_WARP_HIST = None


@contextlib.contextmanager
def switches(**values):
    """POSTERIOR_ROWS, POSTERIOR_SUMMARY, WARP_GRIDS, WARP_HIST, DATASET_GRID_BYTES, DATASET_EVALUATION, DATASET_OFFSETS, DATASET_BASELINES, DATASET_RED_NOISE, DATASET_T0, DATASET_OUTLIERS, DATASET_RED_BASELINES, DATASET_WHITE_NOISE, DATASET_WHITE_BASELINES, DATASET_RED_KERNEL_BASELINES, DATASET_WARP_HIST = ... for the length of a `with` block: what they were
    before -- a user's own setting included -- comes back on exit, also on an error"""
    saved = {name: globals()[name] for name in values}
    globals().update(values)
    try:
        yield
    finally:
        globals().update(saved)


def warp_identity():
    from ._numerics import warp_identity as ident
    return ident()


def set_thread_unit(unit):
    """the work unit whose lnZ_* call this thread makes next (sharding.run_units), or None"""
    _tls.unit = unit


def warp_hist_to_flat(words):
    """a branch's TRX_WARP_BRANCH words (int64 / uint64) as doubles: word 0 is X's bits, the others are counts"""
    words = np.ascontiguousarray(words).astype(np.uint64)
    flat = words.astype(np.float64)
    flat[0] = words[:1].view(np.float64)[0]
    return flat


def _fn_scenario():
    L = _lib.lib()
    if not getattr(L, "trx_bound_scenario", False):          # (per library: tests switch to the testing build and back)
        _fn()
        L.trx_scenario_evidence.restype = ctypes.c_int
        L.trx_scenario_evidence.argtypes = [ctypes.POINTER(ScenarioArgs), _vp]
        L.trx_scenario_enqueue.restype = ctypes.c_int
        L.trx_scenario_enqueue.argtypes = [ctypes.POINTER(ScenarioArgs), _vp, _vp]
        L.trx_star_enqueue.restype = ctypes.c_int
        L.trx_star_enqueue.argtypes = [ctypes.POINTER(ScenarioArgs), ctypes.c_int, ctypes.POINTER(_vp),
                                       ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_int)]
        L.trx_scenario_args_size.restype = ctypes.c_size_t
        if L.trx_scenario_args_size() != ctypes.sizeof(ScenarioArgs):
            raise _lib.TrxError("trx_scenario_args layout mismatch: library %d bytes, binding %d"
                                % (L.trx_scenario_args_size(), ctypes.sizeof(ScenarioArgs)))
        L.trx_bound_scenario = True
    return L.trx_scenario_enqueue


# ---------------------------------------------------------------------------------------
# Calls in flight.  trx_scenario_enqueue never waits for the device, so the lnZ_* calls of a
# calc_probs can all be enqueued (on a few streams, from one host thread) before anything is read
# back: between begin_deferred() and end_deferred() a native call returns a Pending instead of its
# result dicts, and sharding.run_units resolves them after one synchronisation per stream.
RECORD = 2 * SCENARIO_OUT + 1      # doubles per call: two branch records + the limb-darkening flag
RECORD_MOMENTS = 2 * SCENARIO_OUT_MOMENTS + 1      # ... of a call with TRX_FLAG_WEIGHT_MOMENTS (the slots' size)


class Pending:
    """one trx_scenario_enqueue call whose record has not been read yet"""

    def __init__(self, scen, out, stream, keep, ncol, n_time, *, is_host=False, stride=SCENARIO_OUT, table=None,
                 table_rows=0, post=None, post_rows=0, hist=None):
        self.scen = scen                  # the _Scenario: its draw arguments, and the operator chain of a replay
        self.out = out                    # pinned record: two branch records of `stride` doubles + the limb-darkening flag
        self.stream = stream
        self.keep = keep                  # tensors the call reads: alive until its record has been read
        self.ncol = ncol                  # 11 planet / 14 binary
        self.n_time = n_time
        self.is_host = is_host
        self.stride = stride              # SCENARIO_OUT[_MOMENTS]
        self.table, self.table_rows = table, table_rows        # pinned [2][15][K + 1] block of a call with a table
        self.post, self.post_rows = post, post_rows            # pinned [2][8 + 16 M] block of a call with posterior rows
        self.hist = hist                  # pinned [2][WARP_BRANCH] words of a call with a weight histogram

    def result(self):
        """the call's result dict(s); the stream must have been synchronised.  The one-call case of records_to_rows:
        the same rows, handed out as the dicts of a direct lnZ_* call"""
        try:
            (rows,) = _decode([self])
        except ValueError:
            self.keep = None
            raise
        if rows is None:
            return self.scen.run_operator_chain(self.is_host, self.ncol)
        self.keep = None
        K, res = self.table_rows, []
        for b, row in enumerate(rows):
            lnZ, lnm2, lnwmax = row[len(POSTERIOR_PARAMS):]
            if self.stride == SCENARIO_OUT_MOMENTS:
                _lib.moments_emit(lnm2, lnwmax)
            if K > 1:
                blk = self.table.numpy()[b].reshape(15, K + 1)
                res.append(self.scen._table(blk[:self.ncol, :K].copy(), float(lnZ), b == 1))
            else:
                res.append(dict({c: row[j:j + 1] for j, c in enumerate(POSTERIOR_PARAMS)}, lnZ=float(lnZ)))
            if self.post_rows:
                res[-1]["posterior"] = self.posterior(b)
        return res[0] if len(res) == 1 else (res[0], res[1])

    def posterior(self, b):
        """branch b's "posterior" dict from the library's block (None: no draw carries weight)"""
        return self.scen._posterior(self.post.numpy()[b], self.ncol, b == 1)

    def replay_for_ties(self, rec):
        """The seeded numpy modes promise the reference's OWN best draw, and the reference takes it from an argsort
        that orders exact ties its own way (marginal_likelihoods.py:152: introsort, not stable); the library reports
        the first of equals and how many rows tie (record slot 16).  With a tie at the minimum the call is evaluated
        again by the operator chain, on the same staged numbers (still alive in self.keep), whose best-draw search
        reproduces numpy's order.  (Exact ties at the minimum are what flat models give: a scenario none of whose
        draws touches the data.)"""
        if not isinstance(dp.RNG, dp.NumpyStreamRng) or self.scen.philox:
            return False
        nbr = 1 if self.scen.a.planet else 2
        K = self.table_rows
        W = self.stride
        if K > 1:
            # a table of the K best draws: the reference's order needs the K + 1 smallest chi^2 to be finite and
            # strictly increasing, and more than K masked draws (the operator chain's own rule, _best below: anything
            # else goes through numpy's argsort on the host)
            for b in range(nbr):
                n = int(rec[b * W + self.ncol + 1])
                hv = self.table.numpy()[b].reshape(15, K + 1)[14]
                if n <= K or not (np.isfinite(hv[-1]) and np.all(hv[1:] > hv[:-1])):
                    return True
            return False
        return any(rec[b * W + SCEN_TIES] > 1.0 for b in range(nbr))


def _check_status(recs, planet, stride=SCENARIO_OUT):
    """raises when a record says that a masked draw's chi^2 was never written (an internal error of the passes of the
    bounded evaluation: round 4 shipped two such bugs, and a stale value read as a result gave FPP = 1)"""
    for b in range(2):
        bad = recs[:, b * stride + SCEN_STATUS] != 0.0
        if b == 1:
            bad = bad & ~np.asarray(planet, dtype=bool)
        if np.any(bad):
            raise _lib.TrxError("libtrx: %d lnZ_* call(s) of this pass report rows of their likelihood that no kernel "
                                "wrote (branch %d; record status 1) -- an internal error, the results are not usable; "
                                "triceratops_amd.set_full_evaluation(True) (TRX_FLAG_FULL_EVALUATION) evaluates every "
                                "row in one pass" % (int(bad.sum()), b))


_stats_lock = threading.Lock()


def _widen(rec, stride):
    """a call's record in the layout of TRX_FLAG_WEIGHT_MOMENTS (moments NaN where the call did not ask for them)"""
    if stride == SCENARIO_OUT_MOMENTS:
        return rec[:RECORD_MOMENTS]
    W = SCENARIO_OUT_MOMENTS
    out = np.full(RECORD_MOMENTS, np.nan)
    out[:SCENARIO_OUT] = rec[:SCENARIO_OUT]
    out[W:W + SCENARIO_OUT] = rec[SCENARIO_OUT:2 * SCENARIO_OUT]
    out[2 * W] = rec[2 * SCENARIO_OUT]
    return out


def _decode(calls):
    """The one reader of the records the library writes (include/trx.h, TRX_SCENARIO_OUT): the Pendings of a pass,
    their streams synchronised -> per call its (branches, 17) rows -- RECORD_COLS, then lnM2 and lnWmax (NaN where the
    call did not ask for them) -- or None for a call that the operator chain has to evaluate again
    (Pending.replay_for_ties).  Raises what a call by call reading raises; books the calls in _lib.STATS."""
    W = SCENARIO_OUT_MOMENTS
    recs = np.stack([_widen(p.out.numpy(), p.stride) for p in calls])      # [calls][41]
    if np.any(recs[:, 2 * W] != 0.0):
        # (a draw needs a limb-darkening cell the grid lacks: the reference fails there, with this text)
        raise ValueError("can only convert an array of size 1 to a Python scalar")
    planet = np.array([bool(p.scen.a.planet) for p in calls])
    _check_status(recs, planet, W)
    # (on the record as the library wrote it: replay_for_ties reads it at the call's own stride)
    live = np.array([not p.replay_for_ties(p.out.numpy()) for p in calls])
    n_time = np.array([p.n_time for p in calls])
    rows = [None] * len(calls)
    n_rows = n_cells = launches = 0
    for is_planet, ncol in ((True, len(PLANET_COLS)), (False, len(BINARY_COLS))):
        sel = live & (planet == is_planet)
        if not sel.any():
            continue
        blocks = []
        for b in range(1 if is_planet else 2):
            q = recs[sel, b * W:(b + 1) * W]
            lnz, n = q[:, ncol], q[:, ncol + 1]                            # (n: the draws that passed the mask)
            blocks.append(np.stack(_physical(q[:, :ncol].T, is_planet, b == 1) + [lnz, q[:, SCEN_LNM2], q[:, SCEN_LNWMAX]],
                                   axis=1))
            n_rows += int(n.sum())
            n_cells += int((n * n_time[sel]).sum())
            launches += q.shape[0]
        for i, r in zip(np.flatnonzero(sel), np.stack(blocks, axis=1)):    # [calls][branches][17]
            rows[i] = r
    with _stats_lock:
        _lib.STATS["rows"] += n_rows
        _lib.STATS["cells"] += n_cells
        _lib.STATS["launches"] += launches
        _lib.STATS["native_calls"] += len(calls)
    return rows


def _replay_rows(p):
    """the rows of a call with a tie at its minimum, from the operator chain on the same staged numbers (seeded numpy
    modes only: the reference's own order among exactly tied best draws, see Pending.replay_for_ties)"""
    p.scen.want_moments = p.stride == SCENARIO_OUT_MOMENTS
    with torch.cuda.stream(p.stream):
        res = p.scen.run_operator_chain(p.is_host, p.ncol)
    p.stream.synchronize()
    dicts = res if isinstance(res, tuple) else (res,)
    mom = p.scen.moments or [(np.nan, np.nan)] * len(dicts)
    return np.array([record_row(d) + list(m)
                     + (list(posterior_to_flat(d.get("posterior"), p.post_rows)) if p.post_rows else [])
                     for d, m in zip(dicts, mom)])


def records_to_rows(pending):
    """The calls of a pass in one go: [(unit, Pending)] -> {unit: (branches, 17) array in RECORD_COLS order
    (M_s R_s u1 u2 P_orb inc b R_p ecc argp M_EB R_EB fluxratio_EB fluxratio_comp lnZ), then sharding.MOMENT_COLS
    (lnM2 lnWmax: NaN where the call did not ask for them)}, what Pending.result() + sharding._record give call by call
    (768 calls of a 64-target step: 12 ms of dict building; here a few array expressions), then the columns of
    sharding.RowLayout that the call carries: its posterior rows, its weight histogram.  The streams must have been
    synchronised."""
    if not pending:
        return {}
    out = {}
    for (k, p), rows in zip(pending, _decode([p for _, p in pending])):
        if rows is None:
            out[k] = _replay_rows(p)
            continue
        nbr = rows.shape[0]
        if p.post_rows:
            flat = [posterior_to_flat(p.posterior(b), p.post_rows) for b in range(nbr)]
            rows = np.concatenate([rows, np.stack(flat)], axis=1)
        if p.hist is not None:
            # (a pass with WARP_HIST: WARP_BRANCH more columns per branch)
            rows = np.concatenate([rows, np.stack([warp_hist_to_flat(w) for w in p.hist.numpy()[:nbr]])], axis=1)
        out[k] = rows
    for _, p in pending:
        p.keep = None
    return out


def begin_deferred(n_calls):
    """this thread's native lnZ_* calls return Pending objects until end_deferred(); n_calls bounds
    their number (one pinned block holds all their records).  The calls are not handed to the library one by
    one: they collect in a list that flush() passes on in ONE call (trx_star_enqueue) -- sharding.run_units
    flushes at the end of every star's units."""
    _tls.records = torch.empty((max(int(n_calls), 1), RECORD_MOMENTS), dtype=F64, pin_memory=True)
    _tls.next_record = 0
    _tls.batch = []
    # (a pass with WARP_HIST: the calls' histogram blocks, one pinned allocation like the records)
    _tls.hists = torch.empty((max(int(n_calls), 1), 2, WARP_BRANCH), dtype=torch.int64, pin_memory=True) if WARP_HIST else None


def flush():
    """hand the calls collected since the last flush to the library: one trx_star_enqueue"""
    batch = getattr(_tls, "batch", None)
    if not batch:
        return
    _tls.batch = []
    n = len(batch)
    calls = (ScenarioArgs * n)()
    outs, sts = (_vp * n)(), (_vp * n)()
    waited = set()
    for i, (sa, out, stream, dev) in enumerate(batch):
        calls[i] = sa
        outs[i], sts[i] = out.data_ptr(), stream.cuda_stream
        if stream.cuda_stream not in waited:
            waited.add(stream.cuda_stream)
            _lib.wait_uploads(stream)
    done = ctypes.c_int(0)
    _fn_scenario()
    with torch.cuda.device(batch[0][3]):
        rc = _lib.lib().trx_star_enqueue(calls, n, outs, sts, ctypes.byref(done))
    if rc:
        raise _lib.TrxError("trx_star_enqueue failed at call %d of %d with status %d: %s"
                            % (done.value, n, rc, _lib.lib().trx_last_error().decode()))


def end_deferred():
    _tls.records = None
    _tls.batch = None
    _tls.hists = None


def _record_slot():
    """(pinned record of the next call, deferred?)"""
    recs = getattr(_tls, "records", None)
    if recs is not None and _tls.next_record < recs.shape[0]:
        _tls.next_record += 1
        return recs[_tls.next_record - 1], True
    one = getattr(_tls, "one_record", None)
    if one is None:
        one = _tls.one_record = torch.empty(RECORD_MOMENTS, dtype=F64).pin_memory()
    return one, False


def _fn():
    L = _lib.lib()
    if not getattr(L, "trx_bound_draw", False):
        L.trx_draw_scenario.restype = ctypes.c_int
        L.trx_draw_scenario.argtypes = [ctypes.POINTER(DrawArgs), _vp]
        L.trx_draw_args_size.restype = ctypes.c_size_t
        if L.trx_draw_args_size() != ctypes.sizeof(DrawArgs):
            raise _lib.TrxError("trx_draw_args layout mismatch: library %d bytes, binding %d"
                                % (L.trx_draw_args_size(), ctypes.sizeof(DrawArgs)))
        L.trx_bound_draw = True
    return L.trx_draw_scenario


# ---------------------------------------------------------------------------------------
# host constants
def _law(edges, powers, amps_int, amps_inv):
    """constants of tests/torch_pipeline._invert, same Python-float arithmetic"""
    law = PowerLaw()
    ints = []
    for j, p in enumerate(powers):
        span = edges[j + 1] ** (p + 1) - edges[j] ** (p + 1)
        ints.append(span / (p + 1) if amps_int[j] is None else amps_int[j] * span / (p + 1))
    norm = 1 / sum(ints)
    law.nseg, law.ones, law.norm = len(powers), 0, norm
    cum = 0.0
    for j, p in enumerate(powers):
        upper = cum + ints[j]
        law.lo[j], law.hi[j], law.cum[j] = norm * cum, norm * upper, cum
        law.p1[j] = p + 1
        law.amp[j] = 0.0 if amps_inv[j] is None else amps_inv[j]
        law.base[j] = edges[j] ** (p + 1)
        law.ip[j] = 1 / (p + 1)
        cum = upper
    return law


def _rp_laws():
    edges = (0.5, 3.0, 6.0, 20.0)
    out = []
    for powers in ((0.0, -4.0, -0.5), (0.0, -7.0, -0.5)):
        p1, p2, p3 = powers
        A1 = edges[1] ** p1 / edges[1] ** p2
        A2 = edges[2] ** p2 / edges[2] ** p3
        out.append(_law(edges, powers, (None, A1, A2 * A1), (None, A1, A1 * A2)))
    return out


def _cached(cache, key, limit, build):
    """cache[key], from build() on a miss.  The caches below hold what the ~10 lnZ_* calls of one star share, so a
    few entries are live at a time: one that holds more than `limit` is emptied, not trimmed.
    (Where that happens depends on everything the process has cached before.  Emptying _lc_cache between two calls of one
    star gives the later call a second device copy of the light curve, and trx_star_enqueue chains calls by the address
    of their time stamps: that star's chain splits there -- the same results, one launch chain more.  Tests that count
    chains therefore depend on what ran before them; tests/test_gpu_draw_columns.py hands the caches back as it found them.)"""
    v = cache.get(key)
    if v is None:
        if len(cache) > limit:
            cache.clear()
        v = cache[key] = build()
    return v


_q_law_cache = {}


def _q_law(M_s, p_hi, F_twin):
    """tests/torch_pipeline._mass_ratio (priors.py:168-383); constants of a star's calls are built once"""
    return _cached(_q_law_cache, (float(M_s), p_hi, F_twin), 256, lambda: _q_law_build(M_s, p_hi, F_twin))


def _q_law_build(M_s, p_hi, F_twin):
    if M_s <= 0.1:
        law = PowerLaw()
        law.ones = 1
        return law
    p1, p2 = 0.3, p_hi

    def twin_amp(lo):
        return (1 + F_twin / (1 - F_twin) * ((1.0 - lo ** (p2 + 1)) / (p2 + 1))
                / ((1.0 - 0.95 ** (p2 + 1)) / (p2 + 1)))

    if M_s >= 0.3:
        q_min = 0.1 if M_s >= 1.0 else 0.1 / M_s
        A1 = (0.3 ** p1) / (0.3 ** p2)
        A2 = twin_amp(0.3)
        return _law((q_min, 0.3, 0.95, 1.0), (p1, p2, p2), (None, A1, A2 * A1), (None, A1, A1 * A2))
    q_min = 0.1 / M_s
    A2 = twin_amp(q_min)
    return _law((q_min, 0.95, 1.0), (p2, p2), (None, A2), (None, A2))


_RP = None
_tab_cache = {}
_ldc_star_cache = {}


def _spline_table(device, band):
    """the six piecewise cubics the kernel stages in LDS, [6][1 + 5 * 16] doubles"""
    key = (device.type, device.index, band)
    if key not in _tab_cache:
        from scipy.interpolate import PPoly
        tab = np.zeros((N_SPLINES, SPLINE_DOUBLES))
        fb = funcs._flux_spl[band if band in funcs._flux_spl else "TESS"]
        for i, spl in enumerate((funcs._spl["R_hot"], funcs._spl["T_hot"], funcs._spl["R_cool"],
                                 funcs._spl["T_cool"], funcs._flux_spl["TESS"], fb)):
            pp = PPoly.from_spline(spl._eval_args)
            keep = np.diff(pp.x) > 0
            x, c = pp.x[:-1][keep], pp.c[:, keep]
            m = x.size
            assert m <= MAX_KNOTS
            tab[i, 0] = m
            tab[i, 1:1 + m] = x
            for r in range(4):
                tab[i, 1 + MAX_KNOTS * (r + 1):1 + MAX_KNOTS * (r + 1) + m] = c[r]
        _tab_cache[key] = _lib.dev(tab.ravel(), device)
    return _tab_cache[key]


_flux0_cache = {}


def _flux0(M_s, band):
    """flux_relation(M_s) as tests/torch_pipeline._flux_share forms it (the ten calls of a star ask for the
    same two or three values: kept)"""
    return _cached(_flux0_cache, (float(M_s), band), 256,
                   lambda: float(10 ** funcs._flux_spl[band](np.array([M_s]))[0]))


_cc_cache = {}
# Experiments only (profiles/anchor_sensitivity.py): a callable(args, kind) applied to the Moe & Di Stefano constants of a
# bound-companion prior after they are set, and the angular separation that stands in for a contrast curve
# (marginal_likelihoods.py:479-487: 2.2 arcsec)
BOUND_HOOK = None
NO_CC_SEPARATION = 2.2


def _contrast_curve(cc_file, device):
    key = (cc_file, device.type, device.index, NO_CC_SEPARATION if cc_file is None else None)
    if key not in _cc_cache:
        if cc_file is None:
            seps, cons = np.array([float(NO_CC_SEPARATION)]), np.array([1.0])
        else:
            seps, cons = funcs.file_to_contrast_curve(cc_file)
        if cons.size > MAX_CC:
            raise ValueError("contrast curve has more than %d points" % MAX_CC)
        # (the host copies and whether the contrasts are monotonic: _Scenario._replay_interp)
        _cc_cache[key] = (_lib.dev(seps, device), _lib.dev(cons, device), int(cons.size), seps, cons,
                          bool(cons.size > 1 and np.any(np.diff(cons) <= 0)))
    return _cc_cache[key]


_lut_cache = {}
_field_cache = {}      # TRILEGAL populations on the device, by (file, target magnitudes, mission, device)


def _companion_lut(mission, Z, teff_cap, device):
    key = (mission, float(Z), teff_cap, device.type, device.index)
    if key not in _lut_cache:
        tab = ml._ldc(mission)
        atZ = tab.Zs == tab.Zs[np.abs(tab.Zs - Z).argmin()]
        nT = int((teff_cap - 3500) // 250) + 1
        lut = np.full((2, nT * 4), np.nan)
        for tz, gz, a1, a2 in zip(tab.Teffs[atZ], tab.loggs[atZ], tab.u1s[atZ], tab.u2s[atZ]):
            it, ig = (tz - 3500) / 250, (gz - 3.5) / 0.5
            if 0 <= it < nT and it == int(it) and 0 <= ig < 4 and ig == int(ig):
                lut[:, int(it) * 4 + int(ig)] = (a1, a2)
        assert nT * 4 <= MAX_LUT
        _lut_cache[key] = (_lib.dev(lut.ravel(), device), nT * 4)
    return _lut_cache[key]


def _bound_constants(a, M_s, plx):
    """constants of tests/torch_pipeline._bound_rate (priors.py:601-660)"""
    if np.isnan(plx):
        plx = 0.1
    M_ref = M_s if M_s >= 1.0 else 1.0
    lm = np.log10(M_ref)
    f1 = 0.020 + 0.04 * lm + 0.07 * lm ** 2
    f2 = 0.039 + 0.07 * lm + 0.01 * lm ** 2
    f3 = 0.078 - 0.05 * lm + 0.04 * lm ** 2
    alpha, dlogP = 0.018, 0.7
    k = f2 - f1 - alpha * dlogP
    k4 = f3 - f2 - alpha * dlogP
    a.dist_pc = 1000 / plx
    a.kepler_c = (4 * pi ** 2) / (G * M_ref * Msun)
    a.f1, a.f2, a.f3 = f1, f2, f3
    a.t2 = 0.5 * (2.0 * f1 + k)
    a.t3 = 0.5 * alpha * (3.4 ** 2 - 5.4 * 3.4 + 6.8) + f2 * (3.4 - 2.0)
    a.t4 = alpha * dlogP * (5.5 - 3.4) + f2 * (5.5 - 3.4) + k4 * (0.238095 * 5.5 ** 2 - 0.952381 * 5.5 + 0.485714)
    a.t5 = f3 * (3.33333 - 17.3566 * np.exp(-0.3 * 8.0))


def _ptr(t):
    return None if t is None else t.data_ptr()


_lc_cache = {}


def _on_device(a, device):
    """device copy of a light-curve array; the ~10 lnZ_* calls of one star pass the same arrays, so
    the last few are kept (keyed by content: 100-2000 doubles hash in microseconds)"""
    if isinstance(a, torch.Tensor):
        return _lib.dev(a, device)
    a = np.ascontiguousarray(a, dtype=np.float64)
    return _cached(_lc_cache, (a.shape, hash(a.tobytes()), device.index), 32, lambda: _lib.dev(a, device))


# What a dataset's reduction marginalises is one `term` record on its _Dataset -- one type per kind, below -- and, next to
# any of them, the nodes of a transit-time shift (`shift`, a _Shift).  A record holds its kind's tables and answers what
# the callers ask (the defaults are _Term's):
#   reduce(d, grid, ...)   the one _lib.chi2_grid_* call of its kind (_Dataset.halfchi2)
#   coef_shape, lnc        the per-node shape of its coef_out buffer, and the host log-weights of its candidates
#                          (cand_out is [J] per node), or None (_Scenario._best_offsets)
#   refusal                its place in, and its sentence of, the fused evaluation's refusals (_Scenario._datasets_halfchi2)
#   reports, entry(...)    the DATASET_* switches it feeds, by name, and what it leaves in each for the best draw of a
#                          branch, NaN-filled without one (_Scenario._leave_best_terms)
# The kinds with tables that take a loop or an eigenproblem to form keep them in a cache of their own, by content, for the
# lnZ_* calls of a star (not in _lc_cache: its entries decide where a star's launch chain splits).
class _Best(NamedTuple):
    """what evaluating a branch's best draw again leaves for one dataset (on the heaviest node of a t0_grid): the [1] +
    coef_shape coefficients, the [1][J] per-candidate chi^2/2, the [J] per-node terms, the [1][T] model row -- each None
    where nobody asked, all None without a draw.  Device tensors from _best_offsets; a term's entry() reads host copies"""
    coef: Optional[torch.Tensor] = None
    cand: Optional[torch.Tensor] = None
    nodes: Optional[torch.Tensor] = None
    row: Optional[torch.Tensor] = None


def _weights(lnc, h):
    """softmax_j(lnc_j - h_j): the posterior weights of candidates (or nodes) of log-weights lnc at a draw whose
    per-candidate chi^2/2 is h; NaN without a draw"""
    if h is None:
        return np.full(lnc.size, np.nan)
    x = lnc - h.reshape(-1)
    w = np.exp(x - np.max(x))
    return w / w.sum()


def _unscaled(coef, sqrt_d):
    """c_k = c~_k / sqrt(D_k): a draw's scaled coefficients in the call's normalisation; NaN without a
    draw"""
    return np.full(sqrt_d.size, np.nan) if coef is None else coef.reshape(-1) / sqrt_d


def _refusal(rank, what, why):
    return rank, "evaluation='fused' with %s dataset is not built: %s; use evaluation='grid'" % (what, why)


_NO_RECURRENCE = "the fused kernel carries no recurrence along the row"


def _noise_terms(d):
    return tuple(tuple(np.ravel(np.asarray(v, dtype=np.float64)).tolist()) for v in (d.red_sigma, d.red_timescale))


def _hashes(*arrays):
    return tuple(hash(np.ascontiguousarray(a).tobytes()) for a in arrays)


class _Term:
    """the answers of a kind that has nothing to give back"""
    always = False           # the best row is evaluated again whichever switch is open
    coef_shape = None
    coef_switch = None       # the switch under which coef_out is read (`always`: under any)
    lnc = None
    wants_row = False        # entry() reads the best draw's model row
    reports = ()

    def entry(self, switch, d, off, best):
        raise NotImplementedError(switch)


class _Offset(namedtuple("_Offset", "sum_w inv_s2"), _Term):
    """offset_sigma: the sum of the weights and 1 / s^2.  DATASET_OFFSETS: the posterior-mean offset S1 / (S0 + 1 / s^2)"""
    always = True
    refusal = _refusal(0, "an offset_sigma", "the fused kernel carries no sum of w * residual")
    reports = ("DATASET_OFFSETS",)

    @classmethod
    def on_device(cls, d, inv_var):
        # (sum_w is the correctly rounded sum of the weights the device holds)
        return cls(math.fsum(inv_var.tolist()), 0.0 if math.isinf(d.offset_sigma) else 1.0 / (d.offset_sigma * d.offset_sigma))

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_offset(d.flux, d.inv_var, grid, *self, secdepth, sec_limit, out=out, offset_out=offset_out)

    def entry(self, switch, d, off, best):
        return off


class _Baseline(namedtuple("_Baseline", "g minv sqrt_d has_offset"), _Term):
    """baseline (datasets.baseline_system): the scaled columns [K][T] on the device, M's packed upper triangle, sqrt(D),
    and whether term 0 is the dataset's offset.  DATASET_BASELINES: the coefficients c_k = c~_k / sqrt(D_k) of the columns;
    DATASET_OFFSETS: term 0, if it is the offset"""
    always = True
    refusal = _refusal(1, "a baseline", "the fused kernel carries no sums of basis * residual")
    reports = ("DATASET_BASELINES", "DATASET_OFFSETS")

    @classmethod
    def on_device(cls, d, device):
        system = baseline_system(d)
        return cls(_on_device(system.g, device), system.minv, np.sqrt(system.D), d.offset_sigma is not None)

    @property
    def coef_shape(self):
        return (int(self.g.shape[0]),)

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_baseline(d.flux, d.inv_var, grid, self.g, self.minv, secdepth, sec_limit, out=out,
                                       coef_out=coef_out)

    def entry(self, switch, d, off, best):
        ck = _unscaled(best.coef, self.sqrt_d)
        if switch == "DATASET_OFFSETS":
            return ck[0] if self.has_offset else off
        return ck[1:] if self.has_offset else ck


class _Ou(namedtuple("_Ou", "alpha beta omega"), _Term):
    """red_sigma / red_timescale (datasets.ou_system): the three [T] tables on the device"""
    refusal = _refusal(4, "a red_sigma", _NO_RECURRENCE)

    @classmethod
    def on_device(cls, d, device):
        return cls(*(_on_device(v, device) for v in ou_system(d)))

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_ou(d.flux, grid, *self, secdepth, sec_limit, out=out)


_mix_cache = {}


class _OuMix(namedtuple("_OuMix", "alpha beta omega lnc"), _Term):
    """red_grid (datasets.ou_mix_system): alpha, beta, omega [J][T] on the device and lnc [J] on the host, formed once per
    content of stamps, errors and candidates -- J * T steps of a Python loop.  DATASET_RED_NOISE: the candidates' weights"""
    refusal = _refusal(6, "a red_grid", _NO_RECURRENCE)
    reports = ("DATASET_RED_NOISE",)

    @classmethod
    def on_device(cls, d, device):
        key = (tuple(hash(a.tobytes()) for a in (d.time, d.flux_err, d.red_grid)), d.red_grid.shape, device.index)

        def build():
            alpha, beta, omega, lnc = ou_mix_system(d)
            return cls(_lib.dev(alpha, device), _lib.dev(beta, device), _lib.dev(omega, device), lnc)
        return _cached(_mix_cache, key, 32, build)

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_ou_mix(d.flux, grid, *self, secdepth, sec_limit, out=out, cand_out=cand_out)

    def entry(self, switch, d, off, best):
        return _weights(self.lnc, best.cand)


_gls_cache = {}


class _OuLin(namedtuple("_OuLin", "ou c minv sqrt_d"), _Term):
    """red_baseline (datasets.ou_baseline_system): (alpha, beta, omega) and the whitened scaled columns [K][T] on the device,
    M's packed upper triangle, sqrt(D) -- formed once per content of stamps, errors, noise keys, columns and prior sigmas:
    (1 + K) * T steps of a Python loop and a K x K eigenproblem.  DATASET_RED_BASELINES: c_k = c~_k / sqrt(D_k)"""
    refusal = _refusal(2, "a red_baseline", _NO_RECURRENCE)
    reports = ("DATASET_RED_BASELINES",)
    coef_switch = "DATASET_RED_BASELINES"

    @classmethod
    def on_device(cls, d, pair, device):
        B, sigmas = pair
        key = (_hashes(d.time, d.flux_err, B, sigmas), B.shape, float(d.red_sigma), float(d.red_timescale), device.index)

        def build():
            system = ou_baseline_system(d, B, sigmas)
            return cls(tuple(_lib.dev(v, device) for v in (system.alpha, system.beta, system.omega)),
                       _lib.dev(system.c, device), system.minv, np.sqrt(system.D))
        return _cached(_gls_cache, key, 32, build)

    @property
    def coef_shape(self):
        return (int(self.c.shape[0]),)

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_ou_baseline(d.flux, grid, *self.ou, self.c, self.minv, secdepth, sec_limit, out=out,
                                          coef_out=coef_out)

    def entry(self, switch, d, off, best):
        return _unscaled(best.coef, self.sqrt_d)


_ss2_cache = {}


class _Ss2(namedtuple("_Ss2", "A g omega"), _Term):
    """red_kernel "matern32" or "ou2" (datasets.ss2_system): A [T][2][2], g [T][2], omega [T] on the device, formed once per
    content of stamps, errors and noise keys -- T steps of a Python loop"""
    refusal = _refusal(5, "a red_kernel", _NO_RECURRENCE)

    @classmethod
    def on_device(cls, d, device):
        key = (tuple(hash(a.tobytes()) for a in (d.time, d.flux_err)), d.time.shape, d.red_kernel, _noise_terms(d), device.index)
        return _cached(_ss2_cache, key, 32, lambda: cls(*(_lib.dev(np.ascontiguousarray(v), device) for v in ss2_system(d))))

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_ss2(d.flux, grid, *self, secdepth, sec_limit, out=out)


_ss2gls_cache = {}


class _Ss2Lin(namedtuple("_Ss2Lin", "tables c minv sqrt_d"), _Term):
    """red_kernel_baseline (datasets.ss2_baseline_system): (A, g, omega) and the whitened scaled columns [K][T] on the
    device, M's packed upper triangle, sqrt(D) -- formed once per content of stamps, errors, noise keys, columns and prior
    sigmas, as _OuLin's.  DATASET_RED_KERNEL_BASELINES: c_k = c~_k / sqrt(D_k)"""
    refusal = _refusal(3, "a red_kernel_baseline", _NO_RECURRENCE)
    reports = ("DATASET_RED_KERNEL_BASELINES",)
    coef_switch = "DATASET_RED_KERNEL_BASELINES"

    @classmethod
    def on_device(cls, d, pair, device):
        B, sigmas = pair
        key = (_hashes(d.time, d.flux_err, B, sigmas), B.shape, d.red_kernel, _noise_terms(d), device.index)

        def build():
            system = ss2_baseline_system(d, B, sigmas)
            return cls(tuple(_lib.dev(np.ascontiguousarray(v), device) for v in (system.A, system.g, system.omega)),
                       _lib.dev(system.c, device), system.minv, np.sqrt(system.D))
        return _cached(_ss2gls_cache, key, 32, build)

    coef_shape = _OuLin.coef_shape
    entry = _OuLin.entry

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_ss2_baseline(d.flux, grid, *self.tables, self.c, self.minv, secdepth, sec_limit, out=out,
                                           coef_out=coef_out)


class _Robust(namedtuple("_Robust", "c0 c1 k2"), _Term):
    """outlier_frac / outlier_scale (datasets.robust_constants).  DATASET_OUTLIERS: the [T] posterior outlier probabilities
    of the points, _numerics.robust_responsibility on the draw's model row, formed on the host"""
    refusal = _refusal(9, "an outlier_frac", "the fused kernel carries no exp and log1p per point")
    reports = ("DATASET_OUTLIERS",)
    wants_row = True

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_robust(d.flux, d.inv_var, grid, *self, secdepth, sec_limit, out=out)

    def entry(self, switch, d, off, best):
        from ._numerics import robust_responsibility
        if best.row is None:
            return np.full(int(d.flux.numel()), np.nan)
        resid = d.flux.cpu().numpy() - best.row.reshape(-1)
        return robust_responsibility(resid, d.inv_var.cpu().numpy(), *self)


_white_cache = {}


class _WhiteMix(namedtuple("_WhiteMix", "w lnc"), _Term):
    """white_grid [J][3] (datasets.white_mix_system): the candidates' weights [J][T] on the device and lnc [J] on the host,
    formed once per content of errors and candidates.  DATASET_WHITE_NOISE: the candidates' weights"""
    refusal = _refusal(7, "a white_grid", "the fused kernel carries one sum per row, not one per candidate")
    reports = ("DATASET_WHITE_NOISE",)

    @classmethod
    def on_device(cls, d, grid, device):
        key = (hash(d.flux_err.tobytes()), hash(grid.tobytes()), d.flux_err.shape, grid.shape, device.index)

        def build():
            w, lnc = white_mix_system(d, grid)
            return cls(_lib.dev(w, device), lnc)
        return _cached(_white_cache, key, 32, build)

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_white_mix(d.flux, grid, *self, secdepth, sec_limit, out=out, cand_out=cand_out)

    def entry(self, switch, d, off, best):
        return _weights(self.lnc, best.cand)


_white_lin_cache = {}


class _WhiteLin(namedtuple("_WhiteLin", "w lnc basis minv"), _Term):
    """white_baseline columns next to a white_grid (datasets.white_baseline_system): w and lnc as _WhiteMix's (lnc with the
    determinants of the candidates' systems), the columns [K][T] as given on the device, and A_j^-1 [J][K (K + 1) / 2],
    packed upper triangles, on the host -- formed once per content of errors, candidates, columns and prior sigmas: J
    eigenproblems of K x K.  DATASET_WHITE_NOISE: the candidates' weights; DATASET_WHITE_BASELINES: {"coef": the [J][K]
    coefficients under each candidate, "mean": [K] their average under those weights}"""
    refusal = _WhiteMix.refusal
    reports = ("DATASET_WHITE_NOISE", "DATASET_WHITE_BASELINES")
    coef_switch = "DATASET_WHITE_BASELINES"

    @classmethod
    def on_device(cls, d, grid, pair, device):
        B, sigmas = pair
        key = (_hashes(d.flux_err, grid, B, sigmas), d.flux_err.shape, grid.shape, B.shape, device.index)

        def build():
            system = white_baseline_system(d, grid, B, sigmas)
            return cls(_lib.dev(system.w, device), system.lnc, _lib.dev(system.B, device), system.minv)
        return _cached(_white_lin_cache, key, 32, build)

    @property
    def coef_shape(self):
        return int(self.lnc.size), int(self.basis.shape[0])

    def reduce(self, d, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out):
        return _lib.chi2_grid_white_baseline(d.flux, grid, self.w, self.basis, self.minv, self.lnc, secdepth, sec_limit,
                                             out=out, cand_out=cand_out, coef_out=coef_out)

    def entry(self, switch, d, off, best):
        w = _weights(self.lnc, best.cand)
        if switch == "DATASET_WHITE_NOISE":
            return w
        J, K = self.coef_shape
        if best.coef is None or best.cand is None:
            return {"coef": np.full((J, K), np.nan), "mean": np.full(K, np.nan)}
        coef = best.coef.reshape(J, K)
        # (a candidate of weight 0 -- switched off, or far below -- does not enter, whatever its coefficients)
        return {"coef": coef, "mean": np.sum(np.where(w[:, None] > 0, w[:, None] * coef, 0.0), axis=0)}


_shift_cache = {}


class _Shift(namedtuple("_Shift", "stamps lnpi lnpi_dev"), _Term):
    """t0_grid [J][2]: the J device tensors time + shift_j, ln pi [J] on the host and the same on the device.  The sums are
    float64, formed once on the host per content of the stamps and the grid.  The device copy of ln pi serves the best
    draw's choice of a node: an upload per branch would make the host wait for the device there.  DATASET_T0: the nodes'
    weights softmax_j(ln pi_j - h_j)"""
    refusal = _refusal(8, "a t0_grid", "the nodes' terms are folded from the grid reductions")
    reports = ("DATASET_T0",)

    @classmethod
    def on_device(cls, d, grid, device):
        key = (hash(d.time.tobytes()), hash(grid.tobytes()), d.time.shape, grid.shape, device.index)

        def build():
            lnpi = np.log(grid[:, 1])
            return cls([_lib.dev(np.ascontiguousarray(d.time + shift), device) for shift in grid[:, 0]], lnpi,
                       _lib.dev(lnpi, device))
        return _cached(_shift_cache, key, 32, build)

    def entry(self, switch, d, off, best):
        return _weights(self.lnpi, best.nodes)


# (DATASET_OFFSETS is an [L] array per branch, NaN where the others hold None)
_TERM_SWITCHES = ("DATASET_OFFSETS", "DATASET_BASELINES", "DATASET_RED_NOISE", "DATASET_T0", "DATASET_OUTLIERS",
                  "DATASET_RED_BASELINES", "DATASET_WHITE_NOISE", "DATASET_WHITE_BASELINES", "DATASET_RED_KERNEL_BASELINES")


def _open(switch):
    return switch is not None and globals()[switch] is not None


class _Dataset(NamedTuple):
    """one light curve of a Datasets call on the device; what its reduction marginalises (`term`: None for nothing, else
    one of the records above); and, next to any term, the nodes of a transit-time shift (`shift`: the reduction then runs
    once per node)"""
    time: torch.Tensor
    flux: torch.Tensor
    inv_var: torch.Tensor
    exptime: float
    nsamples: int
    term: Optional[_Term] = None
    shift: Optional[_Shift] = None

    @classmethod
    def upload(cls, d, dev, t0_grid=None, outliers=None, red_baseline=None, white_grid=None, white_baseline=None,
               red_kernel_baseline=None):
        """the record of a validated dataset: the one place that picks its term from its keys"""
        inv_var = 1.0 / (d.flux_err * d.flux_err)
        rec = cls(_on_device(d.time, dev), _on_device(d.flux, dev), _on_device(inv_var, dev), d.exptime, d.nsamples)
        if t0_grid is not None:
            # (next to whatever else the dataset marginalises: a shift leaves all of that as it is)
            rec = rec._replace(shift=_Shift.on_device(d, t0_grid, dev))
        term = None
        if outliers is not None:
            # (validate refuses anything but a t0_grid next to it)
            term = _Robust(*robust_constants(*outliers))
        elif white_grid is not None:
            # (validate refuses anything but a t0_grid, or these columns, next to it)
            term = (_WhiteMix.on_device(d, white_grid, dev) if white_baseline is None
                    else _WhiteLin.on_device(d, white_grid, white_baseline, dev))
        elif d.red_grid is not None:
            # (validate refuses anything else next to it)
            term = _OuMix.on_device(d, dev)
        elif red_baseline is not None:
            # (validate wants red_sigma / red_timescale next to it and refuses an offset, a baseline or a red_grid)
            term = _OuLin.on_device(d, red_baseline, dev)
        elif red_kernel_baseline is not None:
            # (validate wants red_kernel matern32 / ou2 next to it and refuses anything else but a t0_grid)
            term = _Ss2Lin.on_device(d, red_kernel_baseline, dev)
        elif d.red_kernel is not None:
            # (validate refuses anything but a t0_grid or those columns next to it)
            term = _Ss2.on_device(d, dev)
        elif d.red_sigma is not None:
            # (validate refuses an offset or a baseline next to it)
            term = _Ou.on_device(d, dev)
        elif d.baseline is not None:
            # (its offset, if it has offset_sigma, is term 0 of the same system)
            term = _Baseline.on_device(d, dev)
        elif d.offset_sigma is not None:
            term = _Offset.on_device(d, inv_var)
        return rec._replace(term=term)

    def halfchi2(self, grid, secdepth=None, sec_limit=float("inf"), out=None, offset_out=None, coef_out=None,
                 cand_out=None):
        """this dataset's weighted chi^2/2 of every row of a model grid [n][T], written or added to `out`; +inf where
        secdepth >= sec_limit: its term's reduction (offset_out: the rows' offsets; coef_out: the rows' scaled
        coefficients; cand_out: the rows' per-candidate chi^2/2 -- each for the kinds that have them), else
        trx_chi2_grid_weighted"""
        if self.term is not None:
            return self.term.reduce(self, grid, secdepth, sec_limit, out, offset_out, coef_out, cand_out)
        return _lib.chi2_grid_weighted(self.flux, self.inv_var, grid, secdepth, sec_limit, out=out)



# ---------------------------------------------------------------------------------------
class _Scenario:
    """one lnZ_* call: draws, the fused kernel, the branch evidences and tables"""

    def __init__(self, time, flux, sigma, N, parallel, exptime, nsamples, mission, flatpriors):
        self.dev = _lib.compute_device()
        self.datasets = None
        if isinstance(time, Datasets):
            # (several light curves: sigma is their sigma_bar; exptime / nsamples are each dataset's own)
            self.datasets = [_Dataset.upload(d, self.dev, g, o, b, w, wb, kb)
                             for d, g, o, b, w, wb, kb in zip(time.sets, time.t0_grids, time.outliers, time.red_baselines,
                                                              time.white_grids, time.white_baselines,
                                                              time.red_kernel_baselines)]
            sigma = time.sigma_ref
            self.time, self.flux = self.datasets[0].time, self.datasets[0].flux
        else:
            self.time, self.flux = _on_device(time, self.dev), _on_device(flux, self.dev)
        self.sigma, self.N = float(sigma), int(N)
        self.parallel, self.exptime, self.nsamples = bool(parallel), exptime, nsamples
        self.mission, self.flat = mission, bool(flatpriors)
        self.keep = []                       # tensors the kernel reads: alive until it has run
        a = self.a = DrawArgs()
        a.N, a.parallel, a.flat = self.N, int(self.parallel), int(self.flat)
        self.philox = PHILOX and isinstance(dp.RNG, dp.TorchRng)
        grids = WARP_GRIDS
        self.warp = None if grids is None else grids.get(getattr(_tls, "unit", None))
        self.want_hist = bool(WARP_HIST)
        if self.philox:
            a.use_philox = 1
            ts = getattr(_tls, "seed", None)
            if ts is None:
                a.seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
            else:
                a.seed = _mix(int(ts), _tls.count)
                _tls.count += 1
        global _RP
        if _RP is None:
            _RP = _rp_laws()
        a.law_rp_hi, a.law_rp_lo = _RP

    def u(self):
        """pointer to one staged array of N uniforms -- or None: the kernel draws them itself"""
        if self.philox:
            return None
        t = dp.RNG.uniform(self.N, self.dev).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def period(self, P_orb):
        a = self.a
        if type(P_orb) not in [float, int]:
            a.P_lo, a.P_hi = float(P_orb[0]), float(P_orb[-1])
            a.range_P = 1
            if self.philox:
                return 0.5 * (a.P_lo + a.P_hi)          # the expectation of the mean below
            t = dp.RNG.uniform(self.N, self.dev).contiguous()
            self.keep.append(t)
            a.uP = t.data_ptr()
            # sample_ecc is handed np.mean(P_orb) of the drawn periods (e.g. marginal_likelihoods.py:103)
            return float((a.P_lo + (a.P_hi - a.P_lo) * t).mean())
        a.P_lo = a.P_hi = float(P_orb)
        return float(P_orb)

    def target(self, M_s, R_s, Teff, Z):
        a = self.a
        a.M_s, a.R_s, a.Teff = float(M_s), float(R_s), float(Teff)
        if Z is not None:
            a.u1, a.u2 = _cached(_ldc_star_cache, (self.mission, float(Z), float(Teff), float(M_s), float(R_s)), 256,
                                 lambda: ml._ldc(self.mission).star(Z, Teff, ml._logg(M_s, R_s)))
        a.f0_tess = _flux0(M_s, "TESS")
        a.law_q = _q_law(M_s, -0.5, 0.30)

    def planet_draws(self, P_mean):
        a = self.a
        a.planet = 1
        a.uRp, a.uInc = self.u(), self.u()
        if not self.philox:
            dp.RNG.discard(self.N)
            # a sampler may return a strided view (torch's Beta does): the kernel reads [N] doubles
            e = dp.RNG.beta(self.N, 0.867, 3.030, self.dev).to(F64).contiguous()
            self.keep.append(e)
            a.ecc_in = e.data_ptr()
        a.uW = self.u()

    def binary_draws(self, P_mean):
        a = self.a
        a.planet = 0
        a.uInc, a.uQ = self.u(), self.u()
        dp.RNG.discard(self.N)
        a.uEcc = self.u()
        a.ecc_pow = 1.0 / (0.2 if P_mean <= 10 else 0.6)
        a.uW = self.u()

    def bound_companion(self, M_s, molusc_file):
        a = self.a
        a.comp = COMP_BOUND
        a.law_qc = _q_law(M_s, -0.95, 0.05)
        if molusc_file is None:
            a.uQc = self.u()
        else:
            q = _lib.dev(ml._bound_companions(M_s, self.N, molusc_file), self.dev).contiguous()
            self.keep.append(q)
            a.qc_in = q.data_ptr()

    def bound_prior(self, kind, M_s, plx, cc_file, filt, molusc_file):
        a = self.a
        if molusc_file is not None:
            a.prior = PRIOR_NONE
            self.want_prior = True          # lnprior = zeros
            return
        a.prior = kind
        self.want_prior = True
        _bound_constants(a, M_s, plx)
        if BOUND_HOOK is not None:
            BOUND_HOOK(a, kind)
        self._cc(cc_file, filt, M_s)

    def _cc(self, cc_file, filt, M_s):
        a = self.a
        seps, cons, n, self.cc_host_seps, self.cc_host_cons, self.cc_nonmono = _contrast_curve(cc_file, self.dev)
        a.cc_seps, a.cc_cons, a.n_cc = seps.data_ptr(), cons.data_ptr(), n
        a.use_cc = int(cc_file is not None)
        self.band = filt if (cc_file is not None and filt in ("J", "H", "K")) else "TESS"
        a.f0_band = _flux0(M_s, self.band)

    def field(self, trilegal_fname, mags, need_ldc, cc_file, filt, M_s, hi_offset):
        """TRILEGAL population + the index draw; hi_offset = -1 for the D scenarios (sic)"""
        a = self.a
        # the D and B calls of one star share the population (the last few stars' are kept)
        # (limit 7: the cache never holds more than eight populations)
        f = _cached(_field_cache, (trilegal_fname, tuple(float(m) for m in mags), self.mission, self.dev.index), 7,
                    lambda: dp._Field({"device": self.dev}, trilegal_fname, *mags, self.mission, False))
        if need_ldc:
            f.need_ldc()
        self.keep.append(f)
        a.comp = COMP_FIELD
        a.f_mass, a.f_radius, a.f_teff, a.f_logg = (f.masses.data_ptr(), f.radii.data_ptr(),
                                                    f.Teffs.data_ptr(), f.loggs.data_ptr())
        a.f_fr = f.fluxratios.data_ptr()
        if need_ldc:
            a.f_u1, a.f_u2 = f.u1.data_ptr(), f.u2.data_ptr()
        self._cc(cc_file, filt, M_s)
        band = filt if cc_file is not None else "T"
        delta = f.band_delta(band).contiguous()
        frband = f.band_fluxratio(band).contiguous()
        self.keep += [delta, frband]
        a.f_delta, a.f_frband = delta.data_ptr(), frband.data_ptr()
        a.prior = PRIOR_FIELD
        self.want_prior = True
        a.bg_amp = (f.N_comp / 0.1) * (1 / 3600) ** 2
        a.bg_const = float(np.log(a.bg_amp * 2.2 ** 2))
        self.n_field, self.hi_offset = f.N_comp, hi_offset

    def field_index(self):
        self.a.n_field_draw = self.n_field + self.hi_offset
        if self.philox:
            return
        idx = dp.RNG.randint(self.n_field + self.hi_offset, self.N, self.dev).to(torch.int64).contiguous()
        self.keep.append(idx)
        self.a.idx = idx.data_ptr()

    want_prior = False
    band = "TESS"
    cc_nonmono = False
    want_moments = False
    moments = None

    def _replay_interp(self, ncol):
        """The reference interpolates the contrast curve with np.interp (funcs.py:222-238), and on a curve whose contrasts
        are not monotonic -- TOI-465.01's measured curve wiggles beyond 9 mag -- np.interp returns the interval its search
        ends in, a search numpy starts from the PREVIOUS draw's interval: the reference's prior of a draw on such a
        plateau depends on the draw before it.  The draw kernel bisects.  In the seeded validation mode
        ("numpy-device": the reference's draws) the reference's own values are replayed: one pass of the draw kernel
        gives every draw's contrast (trx_draw_args.dm_out), np.interp runs over them HERE, in draw order -- numpy's search
        with numpy's memory -- and the separations go back in (sep_in).  Until round 6 this was a documented deviation
        (|d lnZ| <= 8.5e-8 on TOI-465.01's D and B scenarios, tolerance 1e-6 there); now those rows meet the 1e-8 of
        all the others.  One host synchronisation, in a mode that spends its time drawing 3e8 numpy uniforms anyway."""
        a = self.a
        a.sep_in = None
        o = self._draw(ncol, dm_out=True)
        x = o["dm_out"].abs().cpu().numpy()
        self.sep = _lib.dev(np.interp(x, self.cc_host_cons, self.cc_host_seps), self.dev)
        self.keep.append(self.sep)
        a.dm_out, a.sep_in = None, self.sep.data_ptr()
        a.cols = a.mask = a.mask_twin = a.flag = None

    def _draw(self, ncol, lnprior=False, dm_out=False, dump=False):
        """trx_draw_scenario on the current stream, every draw in full: its outputs as a dict of device tensors under
        the names of trx_draw_args (None for those not asked for, and for a planet's mask_twin)"""
        a, N, dev = self.a, self.N, self.dev
        o = {"cols": torch.empty((ncol, N), dtype=F64, device=dev),
             "mask": torch.empty(N, dtype=torch.uint8, device=dev),
             "mask_twin": torch.empty(N, dtype=torch.uint8, device=dev) if not a.planet else None,
             "lnprior": torch.empty(N, dtype=F64, device=dev) if lnprior else None,
             "flag": torch.zeros(1, dtype=torch.int32, device=dev),
             "dm_out": torch.empty(N, dtype=F64, device=dev) if dm_out else None,
             "dump": torch.zeros((9, N), dtype=F64, device=dev) if dump else None}
        for name, t in o.items():
            setattr(a, name, _ptr(t))
        with torch.cuda.device(dev):
            _lib.wait_uploads(torch.cuda.current_stream(dev))
            rc = _fn()(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            raise _lib.TrxError("trx_draw_scenario failed with status %d" % rc)
        return o

    def _upload_warp(self):
        """the call's importance map (WARP_GRIDS) on the device, alive until the kernel has read it"""
        grid = _lib.dev(np.ascontiguousarray(self.warp, dtype=np.float64).reshape(-1), self.dev)
        self.keep.append(grid)
        self.a.warp = grid.data_ptr()

    def _flags(self, is_host):
        """the call's TRX_FLAG_* word, less the library-wide _lib.EXTRA_FLAGS"""
        return (FLAG_COMPANION_IS_HOST if is_host else 0) | (0 if self.parallel else FLAG_SCALAR_K)

    # -----------------------------------------------------------------------------------
    def run(self, is_host):
        a, N, dev = self.a, self.N, self.dev
        tab = _spline_table(dev, self.band)
        a.splines = tab.data_ptr()
        ncol = 11 if a.planet else 14
        if (self.cc_nonmono and a.use_cc and not self.philox and isinstance(dp.RNG, dp.NumpyStreamRng)
                and a.prior in (PRIOR_BOUND_TP, PRIOR_BOUND_EB, PRIOR_FIELD)):
            self._replay_interp(ncol)
        # calc_probs (TABLE_ROWS == 1) takes the library's own chain in BOTH device modes: with numpy's stream the staged
        # uniforms go in through trx_draw_args.uP ... uW (use_philox = 0), so a seeded "numpy-device" run is the
        # production chain -- trx_star_enqueue, bounded evaluation -- on the reference's draws
        # (tests/test_gpu_production_pin.py).  The best draw is the FIRST of equal minima (numpy's argmin); the
        # reference's argsort may order exact ties differently (the operator chain below reproduces that too).
        # A direct lnZ_* call (TABLE_ROWS = 100, marginal_likelihoods.py:152-171) takes the library's chain too, since
        # round 6: the table of the K best draws is selected and gathered on the device (trx_scenario_args.table_rows;
        # every masked draw evaluated to the end).  The operator chain below remains as the cross-check, the path of the
        # dump / trace hooks, and the replay of exact ties in the seeded numpy modes.
        if self.datasets is not None:
            # (an importance map goes through the operator chain's draw; the histogram of ITS weights is DATASET_WARP_HIST)
            if self.want_hist:
                raise NotImplementedError("WARP_HIST together with datasets is not built: the histogram of the library's "
                                          "own chain; the datasets path leaves its histograms in DATASET_WARP_HIST")
            return self.run_operator_chain(is_host, ncol)
        if NATIVE and DUMP is None and _lib.TRACE is None and TABLE_ROWS <= TABLE_MAX_ROWS:
            return self._run_native(is_host, ncol)
        if self.want_hist:
            raise NotImplementedError("a weight histogram needs the library's own chain")
        return self.run_operator_chain(is_host, ncol)

    def run_operator_chain(self, is_host, ncol):
        """trx_draw_scenario (every draw in full) + torch operators for the compaction and the best-draw table +
        trx_lnz_scenario per branch: the path of the 100-row tables of direct lnZ_* calls, and the cross-check of
        the library's own chain"""
        a, N = self.a, self.N
        if self.warp is not None:
            # (the dump / cross-check path of a mapped call: ln J rides in the prior column, whatever the scenario's prior)
            if not self.philox:
                raise NotImplementedError("an importance map needs set_sampling('device'): a staged uniform is never mapped")
            self._upload_warp()
            self.want_prior = True
        o = self._draw(ncol, lnprior=self.want_prior, dump=DUMP is not None)
        cols, mask, mask2, lnprior, flag = o["cols"], o["mask"], o["mask_twin"], o["lnprior"], o["flag"]
        if DUMP is not None:
            DUMP.append({k: o[k] for k in ("dump", "cols", "mask", "mask_twin", "lnprior")})
        self.keep = []
        out = []
        # the Monte-Carlo moments of each branch's evidence (calc_probs: _lib.moments_wanted; a replay of a record that
        # carried them: want_moments), from the chi^2/2 values already on the device
        moments = MOMENTS and (_lib.moments_wanted() or self.want_moments)
        self.moments = [] if moments else None
        flags = self._flags(is_host)
        # (the DATASET_* switches of the terms: per branch the best draw's offsets and what else its datasets' terms give
        # back, still on the device -- wanted where an open switch is fed by a dataset of the call)
        offsets, bests = [], []
        want_terms = self.datasets is not None and any(_open(s) for d in self.datasets for t in (d.term, d.shift)
                                                       if t is not None for s in t.reports)
        hists = None       # (DATASET_WARP_HIST: per branch the weight histogram of its evidence, likewise)
        if self.datasets is not None and DATASET_WARP_HIST is not None:
            if not self.philox:
                raise NotImplementedError("a weight histogram needs set_sampling('device'): the pre-map uniforms are "
                                          "recomputed from the kernel's own generator")
            hists = []
        branches = ((MODEL_TP, mask, False),) if a.planet else ((MODEL_EB, mask, False), (MODEL_EB_TWIN, mask2, True))
        for model, m, twin in branches:
            idx = torch.nonzero(m, as_tuple=False).flatten()
            n = int(idx.numel())
            nblk = 10 if a.planet else 11
            block = cols[:nblk].index_select(1, idx)
            if twin:
                block[2] *= 2.0                                  # 2 P_orb
                block[4] = cols[11].index_select(0, idx)         # a at 2 P_orb
            lp = None if lnprior is None else lnprior.index_select(0, idx)
            if self.datasets is not None:
                h = self._datasets_halfchi2(model, flags, block)
                lnz = _lib.lnz_from_halfchi2(h, lp, N, float(np.log(self.sigma)))
                if hists is not None:
                    hists.append(_lib.warp_hist_from_halfchi2(a, h, lp, idx, float(np.log(self.sigma))))
            else:
                h, lnz = _lib.lnz_scenario(model, flags, self.time, self.flux, self.sigma, block, self.exptime,
                                           self.nsamples, lp, N, float(np.log(self.sigma)))
            if moments:
                mom = _lib.lnz_moments_from_halfchi2(h, lp, N, float(np.log(self.sigma))).cpu().numpy()
                self.moments.append((float(mom[1]), float(mom[2])))
                _lib.moments_emit(mom[1], mom[2])
            best = self._best(h, idx, n)
            if want_terms:
                o, b = self._best_offsets(model,flags, cols, best, twin, nblk) if n else (None, None)
                offsets.append(o)
                bests.append(b)
            post = None
            if POSTERIOR_ROWS:
                # the same selection on this chain's chi^2/2 values (trx_posterior_from_halfchi2; the twin branch draws
                # its uniform from a key of its own: the export has no branch counter)
                M = int(POSTERIOR_ROWS)
                pos, hdr = _lib.posterior_from_halfchi2(h, lp, float(np.log(self.sigma)), M,
                                                        _mix(self.post_seed(), 1) if twin else self.post_seed())
                if float(hdr[3]) > 0:
                    x = (-0.5 * np.log(2 * pi) - float(np.log(self.sigma))) - h.index_select(0, pos)
                    if lp is not None:
                        x = x + lp.index_select(0, pos)
                    post = torch.cat([cols.index_select(1, idx.index_select(0, pos)), pos.to(F64)[None, :], x[None, :]])
            out.append((best, lnz, twin, post))
        # one device -> host copy per branch: the N_BEST x ncol table, lnZ and (once) the flag
        res = []
        for best, lnz, twin, post in out:
            tabl = torch.cat([cols.index_select(1, best).reshape(-1), lnz, flag.to(F64)]).cpu().numpy()
            if tabl[-1] != 0.0:
                raise ValueError("can only convert an array of size 1 to a Python scalar")
            res.append(self._table(tabl[:-2].reshape(ncol, -1), float(tabl[-2]), twin))
            if POSTERIOR_ROWS:
                res[-1]["posterior"] = None if post is None else self._posterior_dict(post.cpu().numpy(), ncol, twin)
        if offsets:
            self._leave_best_terms(offsets, bests)
        if hists is not None:
            DATASET_WARP_HIST[getattr(_tls, "unit", None)] = torch.stack(hists).cpu().numpy().view(np.uint64)
        return res[0] if a.planet else (res[0], res[1])

    def _leave_best_terms(self, offsets, bests):
        """what the branches' best draws give back, from the device to every open DATASET_* switch of the terms under this
        thread's work unit: per branch a list per dataset -- None, or the entry of the dataset's term (of its shift, for
        DATASET_T0) if that feeds the switch; NaN-filled for a branch without a draw -- and for DATASET_OFFSETS an [L]
        array, NaN in place of None"""
        unit = getattr(_tls, "unit", None)
        offsets = [np.full(len(self.datasets), np.nan) if o is None else o.cpu().numpy() for o in offsets]
        # (one copy to the host of what a dataset's best draw left, whichever switches read it)
        bests = [per if per is None else [_Best(*(v if v is None else v.cpu().numpy() for v in b)) for b in per]
                 for per in bests]
        for switch in _TERM_SWITCHES:
            if not _open(switch):
                continue
            rows = []
            for o, per in zip(offsets, bests):
                row = [None] * len(self.datasets)
                for l, d in enumerate(self.datasets):
                    for t in (d.term, d.shift):
                        if t is not None and switch in t.reports:
                            row[l] = t.entry(switch, d, o[l], _Best() if per is None else per[l])
                rows.append(row)
            if switch == "DATASET_OFFSETS":
                rows = [np.array([np.nan if v is None else v for v in row]) for row in rows]
            globals()[switch][unit] = rows

    @staticmethod
    def _fed(t):
        """whether a best draw is evaluated again for this term (or shift) of a dataset"""
        return t is not None and (t.always or any(_open(s) for s in t.reports))

    def _best_offsets(self, model, flags, cols, best, twin, nblk):
        """([L] device tensor, a _Best per dataset) of the branch's best draw: per dataset the posterior-mean baseline offset
        S1 / (S0 + 1 / s^2), NaN for a dataset without an offset of its own; and what its term writes through coef_out and
        cand_out -- the coefficients only where they are read: always for a term that is always evaluated, else under the
        term's coef_switch.  The one row is evaluated again -- trx_flux_grid on one row, then the dataset's reduction
        (_Dataset.halfchi2) -- so nothing of size n x L is kept: always for an offset or a baseline, else where the term or the
        shift feeds an open switch.  A t0_grid dataset has the row evaluated on every node: `nodes` holds its per-node terms
        h_j, and its offset, coefficients and candidates are those of the node of largest ln pi_j - h_j (on a tie the first),
        picked on the device.  `row` holds the draw's model row (on that node) where the term's entry reads it."""
        out = torch.full((len(self.datasets),), float("nan"), dtype=F64, device=self.dev)
        bests = [_Best()] * len(self.datasets)
        row = cols[:nblk].index_select(1, best[:1]).contiguous()
        if twin:
            row[2] *= 2.0
            row[4] = cols[11].index_select(0, best[:1])
        flags |= _lib.EXTRA_FLAGS & _lib.FLAG_FP32_MODEL
        for l, d in enumerate(self.datasets):
            term, shift = d.term, d.shift
            if not (self._fed(term) or self._fed(shift)):
                continue
            keep = self._fed(term) and term.wants_row
            grids = []
            stamps = [d.time] if shift is None else shift.stamps
            J = len(stamps)
            off = out[l:l + 1] if shift is None else torch.full((J,), float("nan"), dtype=F64, device=self.dev)
            coefs = cands = nodes = kept = None
            if term is not None and term.coef_shape is not None and (term.always or _open(term.coef_switch)):
                coefs = torch.empty((J,) + tuple(term.coef_shape), dtype=F64, device=self.dev)
            if term is not None and term.lnc is not None:
                cands = torch.empty((J, int(term.lnc.size)), dtype=F64, device=self.dev)
            hs = []
            for j, t in enumerate(stamps):
                grid, _ = _lib.flux_grid(model, flags, t, row, d.exptime, d.nsamples, want_secdepth=False)
                if keep:
                    grids.append(grid)
                hs.append(d.halfchi2(grid, offset_out=off[j:j + 1], coef_out=None if coefs is None else coefs[j:j + 1],
                                     cand_out=None if cands is None else cands[j:j + 1]))
            if shift is not None:
                nodes = torch.cat(hs)
                top = torch.argmax(shift.lnpi_dev - nodes).reshape(1)   # (the first of equal maxima)
                out[l:l + 1] = off.index_select(0, top)
                coefs = None if coefs is None else coefs.index_select(0, top)
                cands = None if cands is None else cands.index_select(0, top)
                if keep:
                    kept = torch.cat(grids).index_select(0, top)
            elif keep:
                kept = grids[0]
            bests[l] = _Best(coefs, cands, nodes, kept)
        return out, bests

    def _datasets_halfchi2(self, model, flags, block):
        """sum over the datasets of the weighted chi^2/2 of every row of `block` ([n_param][n], the masked draws of one
        branch): per chunk of rows and per dataset one trx_flux_grid and the dataset's accumulating reduction
        (_Dataset.halfchi2: trx_chi2_grid_weighted, or its term's); for a dataset
        with a t0_grid, J of each on the stamps time + shift_j into a zeroed [J][rows] buffer, then one trxt_softmin_rows that
        adds -ln sum_j pi_j exp(-h_j).  The EB
        branch's secondary-eclipse rule (secdepth >= 1.5 sigma_bar -> +inf) rides in the first dataset's reduction: the
        depth does not depend on the time stamps (asked for once; with a t0_grid on the first dataset it rides every node's
        reduction: all nodes +inf give +inf).  A row's value does not depend on the chunk it falls in.
        DATASET_EVALUATION = "fused": one trx_lnl_batch_weighted per dataset over the whole block instead -- no grid, no
        chunks; the rule rides in the first dataset's call as its sec_limit.  It has no form for any term, nor for a shift: each
        is refused with its own sentence."""
        if DATASET_EVALUATION not in DATASET_EVALUATIONS:
            raise ValueError("fused.DATASET_EVALUATION must be one of %s (got %r)" % (DATASET_EVALUATIONS, DATASET_EVALUATION))
        refused = [t.refusal for d in self.datasets for t in (d.term, d.shift) if t is not None]
        if DATASET_EVALUATION == "fused" and refused:
            # (every term is a grid reduction; of several kinds in a list, the sentence of the first in the terms' ranking)
            raise NotImplementedError(min(refused)[1])
        n = int(block.shape[1])
        h = torch.zeros(n, dtype=F64, device=self.dev)         # (0 + x = x: every reduction accumulates)
        if n == 0:
            return h
        flags |= _lib.EXTRA_FLAGS & _lib.FLAG_FP32_MODEL         # (set_precision; the evaluation is full either way)
        chunks = 1         # (launches per dataset)
        if DATASET_EVALUATION == "fused":
            for l, d in enumerate(self.datasets):
                limit = 1.5 * self.sigma if (model == MODEL_EB and l == 0) else float("inf")
                _lib.lnl_batch_weighted(model, flags, d.time, d.flux, d.inv_var, block, d.exptime, d.nsamples, limit, out=h)
        else:
            t_max = max(int(d.time.numel()) for d in self.datasets)
            rows = max(1, int(DATASET_GRID_BYTES) // (8 * t_max))
            chunks = -(-n // rows)
            buf = torch.empty(min(rows, n) * t_max, dtype=F64, device=self.dev)
            eb = model == MODEL_EB
            for r0 in range(0, n, rows):
                r1 = min(r0 + rows, n)
                blk = block if (r0 == 0 and r1 == n) else block[:, r0:r1].contiguous()
                for l, d in enumerate(self.datasets):
                    nt = int(d.time.numel())
                    if d.shift is not None:
                        stamps, lnpi = d.shift.stamps, d.shift.lnpi
                        cand = torch.zeros((len(stamps), r1 - r0), dtype=F64, device=self.dev)
                        sec = None
                        for j, t in enumerate(stamps):
                            grid, s = _lib.flux_grid(model, flags, t, blk, d.exptime, d.nsamples,
                                                     want_secdepth=eb and l == 0 and j == 0,
                                                     out=buf[:(r1 - r0) * nt].view(r1 - r0, nt))
                            sec = s if j == 0 else sec
                            d.halfchi2(grid, sec, 1.5 * self.sigma, out=cand[j])
                        _lib.softmin_rows(cand, lnpi, out=h[r0:r1])
                        continue
                    grid, sec = _lib.flux_grid(model, flags, d.time, blk, d.exptime, d.nsamples, want_secdepth=eb and l == 0,
                                               out=buf[:(r1 - r0) * nt].view(r1 - r0, nt))
                    d.halfchi2(grid, sec, 1.5 * self.sigma, out=h[r0:r1])
        with _stats_lock:
            # (the masked draws once, every (draw, time stamp) cell of every dataset)
            _lib.STATS["rows"] += n
            nodes = [1 if d.shift is None else len(d.shift.stamps) for d in self.datasets]
            _lib.STATS["cells"] += n * sum(j * int(d.time.numel()) for j, d in zip(nodes, self.datasets))
            _lib.STATS["launches"] += sum(nodes) * chunks
        return h

    def _run_native(self, is_host, ncol):
        """the whole call in the library: draws, masks, compaction, likelihood, evidence, best draw --
        enqueued without a host synchronisation (trx_scenario_enqueue)"""
        a, dev = self.a, self.dev
        a.pretest = int(PRETEST)
        sa = ScenarioArgs()
        sa.draw = ctypes.pointer(a)
        sa.time, sa.flux = self.time.data_ptr(), self.flux.data_ptr()
        sa.n_time, sa.nsupersample = int(self.time.numel()), int(self.nsamples)
        sa.sigma, sa.lnsigma, sa.exptime = float(self.sigma), float(np.log(self.sigma)), float(self.exptime)
        sa.flags = self._flags(is_host) | _lib.EXTRA_FLAGS
        # (calc_probs / calc_probs_many: records with the moments of the evidence; a direct lnZ_* call keeps today's)
        stride = SCENARIO_OUT
        if MOMENTS and _lib.moments_wanted():
            sa.flags |= _lib.FLAG_WEIGHT_MOMENTS
            stride = SCENARIO_OUT_MOMENTS
        sa.want_prior = int(self.want_prior)
        out, deferred = _record_slot()
        stream = torch.cuda.current_stream(dev)
        table, K = None, int(TABLE_ROWS)
        if K > 1:
            table = torch.empty((2, _table_branch(K)), dtype=F64).pin_memory()
            sa.table_rows, sa.table = K, table.data_ptr()
        post, M = None, int(POSTERIOR_ROWS)
        if M < 0 or M > POST_MAX_ROWS:
            raise ValueError("fused.POSTERIOR_ROWS must lie in [0, %d]" % POST_MAX_ROWS)
        if M:
            post = torch.empty((2, _post_branch(M)), dtype=F64).pin_memory()
            sa.post_rows, sa.post, sa.post_seed = M, post.data_ptr(), self.post_seed()
        hist = None
        if self.warp is not None or self.want_hist:
            if not self.philox:
                raise NotImplementedError("an importance map / weight histogram needs set_sampling('device'): the numpy "
                                          "modes stage their uniforms, and a staged uniform is never mapped")
            if self.want_hist and M:
                raise NotImplementedError("a weight histogram and posterior rows in one pass are not built")
        if self.warp is not None:
            self._upload_warp()
        if self.want_hist:
            block = getattr(_tls, "hists", None)
            hist = (block[_tls.next_record - 1] if deferred and block is not None and _tls.next_record <= block.shape[0]
                    else torch.empty((2, WARP_BRANCH), dtype=torch.int64).pin_memory())
            sa.warp_hist = hist.data_ptr()
        pend = Pending(self, out, stream, self.keep + [self.time, self.flux], ncol, sa.n_time, is_host=is_host, stride=stride,
                       table=table, table_rows=K if K > 1 else 0, post=post, post_rows=M, hist=hist)
        self.keep = []
        if deferred and getattr(_tls, "batch", None) is not None:
            _tls.batch.append((sa, out, stream, dev))      # (sa.draw points at self.a: alive in the Pending)
            return pend
        fn = _fn_scenario()
        _lib.wait_uploads(stream)
        with torch.cuda.device(dev):
            rc = fn(ctypes.byref(sa), out.data_ptr(), stream.cuda_stream)
        if rc:
            raise _lib.TrxError("trx_scenario_enqueue failed with status %d: %s"
                                % (rc, _lib.lib().trx_last_error().decode()))
        if deferred:
            return pend
        stream.synchronize()
        return pend.result()

    def _best(self, h, idx, n):
        """indices of the N_BEST best draws (see tests/torch_pipeline._evidence for the tie rules)"""
        dev, N = self.dev, self.N
        if not isinstance(dp.RNG, dp.NumpyStreamRng):
            rows = TABLE_ROWS
            if rows == 1 and n > 0:
                return idx[torch.argmin(h).reshape(1)]
            k = min(rows, n)
            best = idx[torch.topk(h, k, largest=False, sorted=True).indices] if k else idx
            if k < rows:
                best = torch.cat([best, torch.arange(rows - k, device=dev) % max(N, 1)])
            return best
        best = None
        if n > N_BEST:
            hv, hi = torch.topk(h, N_BEST + 1, largest=False, sorted=True)
            if bool(torch.isfinite(hv[-1]) & (hv[1:] > hv[:-1]).all()):
                best = idx[hi[:N_BEST]]
        if best is None:
            lnL = np.full(N, -np.inf)
            lnL[idx.cpu().numpy()] = -0.5 * np.log(2 * pi) - np.log(self.sigma) - h.cpu().numpy()
            best = torch.as_tensor((-lnL).argsort()[:N_BEST]).to(dev)
        return best

    def post_seed(self):
        """key of the resampler's uniform: from the call's draw seed, no generator is advanced"""
        return _mix(int(self.a.seed), _POST_SALT)

    def _posterior(self, block, ncol, twin):
        """a branch's TRX_POST_BRANCH(M) block (include/trx.h) -> its "posterior" dict, or None without weight"""
        M = (block.size - 8) // 16
        if block[3] == 0.0:
            return None
        rows = block[8:].reshape(16, M)
        return self._posterior_dict(np.concatenate([rows[:ncol], rows[14:16]]), ncol, twin)

    def _posterior_dict(self, t, ncol, twin):
        """[ncol + 2][M]: the sampled draws' columns, their list positions and log-weights"""
        d = self._table(t[:ncol].copy(), 0.0, twin)
        del d["lnZ"]
        d["lnw"], d["row"] = t[ncol + 1].copy(), t[ncol].astype(np.int64)
        return d

    def _table(self, t, lnZ, twin):
        """the reference's result dict from the gathered columns (marginal_likelihoods.py:152-171)"""
        return dict(zip(RECORD_COLS, _physical(t, bool(self.a.planet), twin) + [lnZ]))


# ---------------------------------------------------------------------------------------
# the ten scenarios: random numbers are drawn in the reference's order (App. B of SURVEY.md)
def _start(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N, parallel, mission, flatpriors, exptime, nsamples):
    s = _Scenario(time, flux, sigma, N, parallel, exptime, nsamples, mission, flatpriors)
    P_mean = s.period(P_orb)
    s.target(M_s, R_s, Teff, Z)
    return s, P_mean


def lnZ_TTP(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N=1000000, parallel=False, mission="TESS",
            flatpriors=False, exptime=0.00139, nsamples=20):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N, parallel, mission, flatpriors, exptime, nsamples)
    s.planet_draws(Pm)
    return s.run(False)


def lnZ_TEB(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N=1000000, parallel=False, mission="TESS",
            flatpriors=False, exptime=0.00139, nsamples=20):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N, parallel, mission, flatpriors, exptime, nsamples)
    s.binary_draws(Pm)
    return s.run(False)


def lnZ_PTP(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, plx, contrast_curve_file=None, filt="TESS",
            N=1000000, parallel=False, mission="TESS", flatpriors=False, exptime=0.00139,
            nsamples=20, molusc_file=None):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N, parallel, mission, flatpriors, exptime, nsamples)
    s.bound_companion(M_s, molusc_file)
    s.bound_prior(PRIOR_BOUND_TP, M_s, plx, contrast_curve_file, filt, molusc_file)
    s.planet_draws(Pm)
    return s.run(False)


def lnZ_PEB(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, plx, contrast_curve_file=None, filt="TESS",
            N=1000000, parallel=False, mission="TESS", flatpriors=False, exptime=0.00139,
            nsamples=20, molusc_file=None):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N, parallel, mission, flatpriors, exptime, nsamples)
    s.binary_draws(Pm)
    s.bound_companion(M_s, molusc_file)
    s.bound_prior(PRIOR_BOUND_EB, M_s, plx, contrast_curve_file, filt, molusc_file)
    return s.run(False)


def _companion_host(s, Z, teff_cap):
    a = s.a
    a.host = HOST_COMPANION
    lut, n = _companion_lut(s.mission, Z, teff_cap, s.dev)
    a.lut, a.n_lut, a.teff_cap = lut.data_ptr(), n, float(teff_cap)


def lnZ_STP(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, plx, contrast_curve_file=None, filt="TESS",
            N=1000000, parallel=False, mission="TESS", flatpriors=False, exptime=0.00139,
            nsamples=20, molusc_file=None):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, None, N, parallel, mission, flatpriors, exptime, nsamples)
    s.bound_companion(M_s, molusc_file)
    _companion_host(s, Z, 10000)
    s.bound_prior(PRIOR_BOUND_TP, M_s, plx, contrast_curve_file, filt, molusc_file)
    s.planet_draws(Pm)
    return s.run(True)


def lnZ_SEB(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, plx, contrast_curve_file=None, filt="TESS",
            N=1000000, parallel=False, mission="TESS", flatpriors=False, exptime=0.00139,
            nsamples=20, molusc_file=None):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, None, N, parallel, mission, flatpriors, exptime, nsamples)
    s.binary_draws(Pm)
    s.bound_companion(M_s, molusc_file)
    _companion_host(s, Z, 13000)
    s.bound_prior(PRIOR_BOUND_EB, M_s, plx, contrast_curve_file, filt, molusc_file)
    return s.run(True)


def lnZ_DTP(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, Tmag, Jmag, Hmag, Kmag, trilegal_fname,
            contrast_curve_file=None, filt="TESS", N=1000000, parallel=False, mission="TESS",
            flatpriors=False, exptime=0.00139, nsamples=20):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N, parallel, mission, flatpriors, exptime, nsamples)
    s.field(trilegal_fname, (Tmag, Jmag, Hmag, Kmag), False, contrast_curve_file, filt, M_s, -1)
    s.field_index()
    s.planet_draws(Pm)
    return s.run(False)


def lnZ_DEB(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, Tmag, Jmag, Hmag, Kmag, trilegal_fname,
            contrast_curve_file=None, filt="TESS", N=1000000, parallel=False, mission="TESS",
            flatpriors=False, exptime=0.00139, nsamples=20):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, Z, N, parallel, mission, flatpriors, exptime, nsamples)
    s.binary_draws(Pm)
    s.field(trilegal_fname, (Tmag, Jmag, Hmag, Kmag), False, contrast_curve_file, filt, M_s, -1)
    s.field_index()
    return s.run(False)


def lnZ_BTP(time, flux, sigma, P_orb, M_s, R_s, Teff, Tmag, Jmag, Hmag, Kmag, trilegal_fname,
            contrast_curve_file=None, filt="TESS", N=1000000, parallel=False, mission="TESS",
            flatpriors=False, exptime=0.00139, nsamples=20):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, None, N, parallel, mission, flatpriors, exptime, nsamples)
    s.field(trilegal_fname, (Tmag, Jmag, Hmag, Kmag), True, contrast_curve_file, filt, M_s, 0)
    s.a.host = HOST_FIELD
    s.field_index()
    s.planet_draws(Pm)
    return s.run(True)


def lnZ_BEB(time, flux, sigma, P_orb, M_s, R_s, Teff, Tmag, Jmag, Hmag, Kmag, trilegal_fname,
            contrast_curve_file=None, filt="TESS", N=1000000, parallel=False, mission="TESS",
            flatpriors=False, exptime=0.00139, nsamples=20):
    s, Pm = _start(time, flux, sigma, P_orb, M_s, R_s, Teff, None, N, parallel, mission, flatpriors, exptime, nsamples)
    a = s.a
    a.planet = 0
    a.uInc, a.uQ = s.u(), s.u()
    dp.RNG.discard(s.N)                 # companion mass ratios: drawn and unused (:2089)
    dp.RNG.discard(s.N)                 # sample_ecc's own uniforms
    a.uEcc = s.u()
    a.ecc_pow = 1.0 / (0.2 if Pm <= 10 else 0.6)
    a.uW = s.u()
    s.field(trilegal_fname, (Tmag, Jmag, Hmag, Kmag), True, contrast_curve_file, filt, M_s, 0)
    a.host = HOST_FIELD
    s.field_index()
    return s.run(True)
