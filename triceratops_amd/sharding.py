"""Scenario-level sharding of calc_probs over the GPUs of one node.

The reference runs its (star, lnZ_* call) units strictly one after the other in one Python
thread (triceratops.py:736-1428).  The units are independent given the light curve, so here
they are dealt to the ranks of a torch.distributed job (one process per GPU; backend "nccl" is
RCCL over xGMI) with a longest-processing-time-first schedule, every rank evaluates its own
units on its own GPU, and ONE all_gather of a small fp64 record table (15 numbers per
scenario: the best-fit row + lnZ) assembles the result on every rank.  No other collective is
on the data path; the message is a few KB, i.e. latency-bound, so a single direct all_gather
is the right primitive (no ring, no bucketing).

Random numbers.  world == 1: the generator of the sampling mode is consumed unit after unit (numpy modes:
identical to the reference under the same np.random.seed), unless per_unit_seed is set.  world > 1: each
unit draws from its own seed, derived from (base of the rank that owns it, unit index).  base is one draw of
the sampling mode's host generator -- torch's CPU generator in "device" mode (torch.manual_seed governs every
path of that mode), numpy's global stream in the numpy modes -- taken on EVERY rank.  Ranks seeded alike
(the way to a reproducible run) draw the same base, and the result then depends neither on the partition nor
on the world size (per_unit_seed = True gives the same numbers on one GPU).  Ranks that were not seeded -- the
reference's normal usage -- draw different bases: each unit is still an independent draw, the run is just
not reproducible, which is what "unseeded" means.  No seed broadcast: the all_gather is the only collective
of a calc_probs; every rank's base rides in its chunk's header row and is kept in `last_seed_bases` (all
equal = the run can be repeated from the seed).
"""
import os
from typing import NamedTuple

import numpy as np

from . import _lib
from . import fused as _fused

RECORD_COLS = _fused.RECORD_COLS      # the best draw's 14 physical columns + lnZ (defined beside the library's own order)
# run_units' table carries the Monte-Carlo moments of every evidence behind RECORD_COLS (NaN where a path gave none):
# lnM2 = log of the mean squared weight, lnWmax = log of the largest weight's share (include/trx.h,
# trx_lnz_moments_from_halfchi2).  They never enter a result dict; target._finish reads them from the rows.
MOMENT_COLS = ("lnM2", "lnWmax")
per_unit_seed = False
# Host threads that evaluate this rank's units side by side, each on its own HIP stream
# (set_sampling("device") with the kernel's own random numbers only).  A lnZ_* call is ~25 small
# launches and two host syncs around one or two large kernels; a second and third call in flight
# fill the GPU while the first waits for Python.  Implies per-unit seeding (the numbers a unit draws
# depend on its seed only, so the result does not depend on the number of threads).
threads = 1
# HIP streams ONE host thread deals the lnZ_* calls of a calc_probs to (set_sampling("device")): a call
# is enqueued without any host synchronisation (trx_scenario_enqueue), so the thread enqueues every
# unit, the streams overlap the small kernels of one call with the large ones of another, and the
# results are read after one wait.  The library keeps ~0.3 GB of scratch per stream at N = 1e6.
# Four: a call is a chain of dependent launches, most of them small, so a stream keeps the chip busy only while its
# likelihood kernel runs, and the other streams fill those gaps.  64 TOIs x 18 scenarios, the stream counts visited in
# turn over seven rounds (profiles/batch_timing.py, profiles/r04/hw_queues.txt): 0.35 s a step on one stream, 0.225 on
# two, 0.19 on three, 0.175 on four, 0.18-0.19 on six and on eight -- with one hardware queue per stream
# (GPU_MAX_HW_QUEUES = 16 since round 6 -- 8 until then --, set by the package: with the runtime's default of 4, streams share queues and three streams
# run slower than two).
streams = int(os.environ.get("TRX_STREAMS", "4"))
# host seconds of the last single-thread pass: enqueueing every call, then waiting for the streams
# (+ the collective, and -- calc_probs_many -- the unit lists and the result tables of all targets)
timing = {"enqueue_s": 0.0, "wait_s": 0.0, "gather_s": 0.0, "prepare_s": 0.0, "finish_s": 0.0, "build_s": 0.0,
          "library_s": 0.0}
# seed bases of the ranks of the last multi-rank run_units (from the all_gather's header rows)
last_seed_bases = None
# what the schedule of the last run_units gave every rank: lnZ_* calls, distinct (job, star)s and distinct jobs
last_share = {"calls": [0], "stars": [0], "jobs": [0]}
last_own_jobs = set()
last_layout = None              # the RowLayout of the last run_units pass: what its rows' columns are
_warned_bases = False
# Opt-in (advisor, round 5): True makes the first device pass call gc.freeze() once -- every object alive then moves to
# the collector's permanent generation, so that the full collection which follows a held-off pass looks at the pass's own
# objects only (a 64-target step lost 75 ms to one every fourth step, profiles/r05/gc_pause.txt).  freeze() is for good:
# cyclic garbage that forms LATER among the frozen objects is never reclaimed until release() (gc.unfreeze()), which a
# long-lived service may not want decided for it -- so the default leaves the collector's generations alone (bench.py
# and TRX_FREEZE_GC=1 switch it on).  Either way the collector is held off (gc.disable(), process-wide: it affects the
# caller's other threads too) only while a pass enqueues and waits, and is switched back on afterwards.
freeze_gc = os.environ.get("TRX_FREEZE_GC", "0") == "1"
_gc_frozen = False
# Device scratch of one stream of a pass (include/trx.h): a launch chain of c calls holds c x (~0.36 GB of draw-side
# buffers + ~0.16 GB of likelihood scratch per branch, 1.5 branches a call on average) per 1e6 draws -- c = chain_calls
# (12), or fewer when TRX_CHAIN_DRAWS (2.5e7 draws' worth) bounds the chain: ~7 GB per stream at N = 1e6, ~15 GB at
# N = 2-3e6 (advisor, round 5: the round-4 figure of 0.36 GB per stream predates the chains).  The streams of a pass
# are capped so that their scratch together stays near this many bytes: 6 streams at N = 1e6, 3 at 3e6, 2 from ~5e6 on.
# A sixth of an MI355X's 288 GB by default; several ranks sharing one device should divide it (TRX_SCRATCH_GB).
scratch_budget_bytes = float(os.environ.get("TRX_SCRATCH_GB", "48")) * 1e9


def stream_scratch_bytes(n_draws):
    """estimate of the library's scratch per stream for calls of n_draws draws (see scratch_budget_bytes)"""
    # (posterior rows in a chain add 49 KB per branch and at most 1 MB per call -- csrc/trx_scenario.hip, enqueue_chain --
    # to draw-side buffers of 146 bytes per draw for which 360 are booked here: the margin covers them from N = 5000 on,
    # and the cap below only binds from N ~ 1e6)
    per_call = (0.36e9 + 1.5 * 0.16e9) * n_draws / 1e6
    calls = max(1.0, min(float(chain_calls), 2.5e7 / max(n_draws, 1)))
    return calls * per_call


def release():
    """gives back what a pass with freeze_gc kept: the collector's permanent generation is thawed (gc.unfreeze()) and
    the next device pass freezes afresh if freeze_gc is still set"""
    import gc
    global _gc_frozen
    if _gc_frozen:
        gc.unfreeze()
        _gc_frozen = False

# relative cost of a unit by its drop key: EB calls evaluate two branches plus the 25-point
# secondary-eclipse scan; companion/background hosts add per-draw stellar relations
_COST = {"TP": 1.0, "PTP": 1.1, "STP": 1.2, "DTP": 1.1, "BTP": 1.2, "NTP": 1.0,
         "EB": 1.7, "PEB": 1.8, "SEB": 1.9, "DEB": 1.8, "BEB": 1.9, "NEB": 1.7}


def _draw_base():
    """one 31-bit seed base from the host generator that governs the current sampling mode"""
    if _fused.threadable():
        import torch
        return int(torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64).item())
    return int(np.random.randint(0, 2 ** 31 - 1))


# True: a process group of ONE rank takes the multi-rank path too -- schedule, per-unit seeds, the record table through
# the group's all_gather_into_tensor (RCCL on the "nccl" backend: device tensors, header rows, padding) -- so that the
# collective branch can be executed and timed on a single GPU (tests/test_gpu_rccl_world1.py; bench.py's `batch` object
# reports its gather_s).  False (default): one rank has nothing to gather and skips it.
collective_at_world_one = os.environ.get("TRX_COLLECTIVE_WORLD1", "0") == "1"


def _dist():
    try:
        import torch.distributed as dist
    except Exception:  # pragma: no cover
        return None
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or collective_at_world_one):
        return dist
    return None


def _lpt(items, cost, load, calls, n_calls):
    """longest-processing-time-first: the dearest item first, each to the rank with the least load so far (ties:
    fewest calls, then rank index)"""
    out = {}
    for it in sorted(items, key=lambda it: (-cost[it], it)):
        r = min(range(len(load)), key=lambda i: (load[i], calls[i], i))
        out[it] = r
        load[r] += cost[it]
        calls[r] += n_calls[it]
    return out


def schedule(costs, world, groups=None):
    """Owner of every unit; every rank computes the same table.

    groups[k] = (job, star) of unit k (calc_probs_many: the TOI and the star of the lnZ_* call).  A rank pays for
    every star it touches on the HOST as well -- the renormalised light curve, the star's constants and tables,
    one trx_star_enqueue per star -- so units are dealt as whole TOIs, then as whole stars, and only what is left
    as single calls (round 4 dealt single calls: 64 like-sized TOIs on 8 ranks gave every rank 16 TOIs x 6 calls
    instead of 8 x 12, and the host path of a rank shrank to a quarter, not an eighth).  At each level the groups
    are dealt longest-first while there are at least two per rank; a group dearer than 3/4 of a rank's fair share
    (the target star of a single crowded field), and the len mod world cheapest ones, go on to the next level,
    where they fill in what the whole groups left uneven.  groups = None: single units (one calc_probs)."""
    n = len(costs)
    load, calls = [0.0] * world, [0] * world
    owner = [0] * n
    if world <= 1 or n == 0:
        return owner
    fair = 0.75 * sum(costs) / world
    todo = list(range(n))
    levels = [] if groups is None else [lambda k: groups[k][0], lambda k: groups[k]]
    for level in levels:
        members = {}
        for k in todo:
            members.setdefault(level(k), []).append(k)
        cost = {g: sum(costs[k] for k in ks) for g, ks in members.items()}
        whole = sorted((g for g in members if cost[g] <= fair), key=lambda g: (-cost[g], members[g][0]))
        if len(whole) < 2 * world:
            continue
        whole = whole[:len(whole) - len(whole) % world]
        dealt = _lpt(whole, cost, load, calls, {g: len(members[g]) for g in whole})
        for g, r in dealt.items():
            for k in members[g]:
                owner[k] = r
        todo = [k for k in todo if level(k) not in dealt]
    dealt = _lpt(todo, {k: costs[k] for k in todo}, load, calls, {k: 1 for k in todo})
    for k, r in dealt.items():
        owner[k] = r
    return owner


class Unit(NamedTuple):
    """One (star, lnZ_* call) work unit of run_units.  A plain tuple underneath: units built by hand with the first six
    fields (the tests') are coerced with Unit(*u), and a unit pickles and unpacks like the tuple it is."""
    first_row: int          # of the unit's scenario rows in its target's table
    names: tuple            # the scenarios of those rows: one per branch of the call
    star_num: int
    ID: object
    thunk: object           # () -> result dict(s) or fused.Pending; None: a dropped scenario
    key: str                # the drop key, and the call's relative cost (_COST)
    weight: float = 1.0     # scales that cost in the schedule (calc_probs_many: jobs of different sizes)
    draws: int = None       # N of the lnZ_* call (stream scratch, the error attributes); None: the unit does not say
    group: tuple = None     # (job, star): the schedule deals whole jobs and whole stars first


def as_units(units):
    return [u if type(u) is Unit else Unit(*u) for u in units]


def unit_cost(u):
    return _COST.get(u.key, 1.0) * u.weight


def _star_of(u):
    """(job, star) of a unit when the caller gave it (target._units), else its star's ID"""
    return u.ID if u.group is None else u.group


def _job_of(u):
    return 0 if u.group is None else u.group[0]


class RowLayout:
    """The one place that knows the columns of a row of run_units' table: RECORD_COLS, MOMENT_COLS, the row's posterior
    (post_rows samples of each of fused.POSTERIOR_KEYS or, with summary_q, len(summary_q) quantiles of each of
    fused.POSTERIOR_PARAMS), then with hist (calc_probs_refined) its fused.WARP_BRANCH histogram words.  `record`, `moments`,
    `extra`, `hist`: the column slices (empty where the pass carries none); `lnZ`: a column; `width`: the row's length."""

    def __init__(self, post_rows=0, summary_q=None, hist=False):
        post_rows, summary_q = int(post_rows), summary_q if post_rows else None
        n, m = len(RECORD_COLS), len(RECORD_COLS) + len(MOMENT_COLS)
        e = m + (len(_fused.POSTERIOR_KEYS) * post_rows if summary_q is None else len(_fused.POSTERIOR_PARAMS) * len(summary_q))
        h = e + (_fused.WARP_BRANCH if hist else 0)
        key = None if not post_rows else "posterior" if summary_q is None else "posterior_quantiles"
        self.__dict__.update(post_rows=post_rows, summary_q=summary_q, record=slice(0, n), lnZ=n - 1, moments=slice(n, m),
                             extra=slice(m, e), hist=slice(e, h), width=h, extra_key=key)

    def __setattr__(self, name, value):
        raise AttributeError("RowLayout is immutable")

    def encode(self, post):
        """a "posterior" dict (or None) as the row's extra columns, one key after the other: the samples, or
        np.quantile(samples, summary_q); NaN where absent"""
        if self.summary_q is None:
            return _fused.posterior_to_flat(post, self.post_rows)
        if post is None:
            return np.full(self.extra.stop - self.extra.start, np.nan)
        return np.concatenate([np.quantile(post[c], self.summary_q) for c in _fused.POSTERIOR_PARAMS])

    def decode(self, row):
        """the inverse, from a whole row: what a result dict holds under extra_key (None for NaN in the defining slot)"""
        flat = np.asarray(row[self.extra], dtype=np.float64)
        if self.summary_q is None:
            return _fused.posterior_from_flat(flat, self.post_rows)
        n_q = len(self.summary_q)
        if n_q == 0 or flat.size != self.extra.stop - self.extra.start or np.isnan(flat[0]):
            return None
        return {c: flat[i * n_q:(i + 1) * n_q].copy() for i, c in enumerate(_fused.POSTERIOR_PARAMS)}

    def summarise(self, rec):
        """the owner-side reduction of a summary pass: a unit's rows as its owner has them -- the samples still in place
        of the quantiles -- with every row's samples reduced to quantiles (of the dict target.posterior would hold)"""
        samples = RowLayout(self.post_rows)
        out = np.full((rec.shape[0], self.width), np.nan)
        have = min(self.moments.stop, rec.shape[1])
        out[:, :have] = rec[:, :have]
        if rec.shape[1] >= samples.width:
            for i in range(rec.shape[0]):
                out[i, self.extra] = self.encode(samples.decode(rec[i]))
        return out


def _record(res):
    """(res,) or (res, res_twin) -> (n, 15) array of the best row + lnZ of each dict"""
    dicts = res if isinstance(res, tuple) else (res,)
    return np.array([_fused.record_row(d) for d in dicts], dtype=np.float64)


def _as_dicts(rec, layout):
    out = tuple({c: rec[i, j] for j, c in enumerate(RECORD_COLS)} for i in range(rec.shape[0]))
    if layout.extra_key:
        for i, d in enumerate(out):
            d[layout.extra_key] = layout.decode(rec[i])
    return out


def run_units(units, verbose=0, as_rows=False, job_done=None):
    """Evaluate the work units of one calc_probs.

    units: list of Unit, or of plain tuples with a Unit's first six fields or more (coerced here, once).
    Returns, per unit, None (dropped scenario) or a tuple of per-scenario dicts
    {column: best value, 'lnZ': float} -- with as_rows, the unit's (branches, width) rows of the pass's table instead
    (what target._finish reads: building a dict per scenario and taking it apart again cost 4 ms of a 64-target step,
    on every rank); their columns are `last_layout`'s, the RowLayout this pass builds from fused's switches at its start.
    job_done(job, results_of_its_units): called as soon as every unit of a job (the first element of a unit's
    group) has its records -- while the GPU still works on later jobs -- on one rank with the calls enqueued
    from one host thread; elsewhere never (the caller finishes what is left)."""
    units = as_units(units)
    dist = _dist()
    world, rank = (dist.get_world_size(), dist.get_rank()) if dist else (1, 0)
    live = [k for k, u in enumerate(units) if u.thunk is not None]
    owner, base = {k: 0 for k in live}, None
    if dist:
        base = _draw_base()         # ranks seeded alike draw the same one (module docstring)
        groups = [units[k].group for k in live]
        own = schedule([unit_cost(units[k]) for k in live], world, None if None in groups else groups)
        owner = {k: own[i] for i, k in enumerate(live)}
    global last_share, last_own_jobs
    calls, stars, jobs = [0] * world, [set() for _ in range(world)], [set() for _ in range(world)]
    for k in live:                          # (one pass over the units: this runs on every rank for ALL units)
        r = owner[k]
        calls[r] += 1
        stars[r].add(_star_of(units[k]))
        jobs[r].add(_job_of(units[k]))
    last_share = {"calls": calls, "stars": [len(x) for x in stars], "jobs": [len(x) for x in jobs]}
    last_own_jobs = jobs[rank]              # (calc_probs_many: the targets whose tables this rank fills at once)
    # calc_probs keeps the best draw of every scenario only: with the device generator the fused
    # path then selects it with one argmin instead of a top-100 sort (fused.TABLE_ROWS)
    if not dist and (per_unit_seed or (threads > 1 and _fused.threadable())):
        # (threads only apply to the device generator: the numpy modes keep consuming the caller's stream)
        base = _draw_base()
    _fused.TABLE_ROWS = 1
    # (this thread's moments sink for the pass: the evidences report lnM2 / lnWmax, see _lib.moments_swap)
    prev_sink = _lib.moments_swap([] if _fused.MOMENTS else None)
    try:
        return _run_units(units, live, owner, base, dist, world, rank, verbose, as_rows, job_done if not dist else None)
    finally:
        _lib.moments_swap(prev_sink)
        _fused.TABLE_ROWS = _fused.N_BEST


_streams = {}


def _worker_streams(device, n):
    """the worker threads' HIP streams, kept from call to call: the library keeps its scratch per
    stream (include/trx.h), so fresh streams every calc_probs would keep growing new buffers"""
    import torch
    have = _streams.setdefault(device, [])
    while len(have) < n:
        have.append(torch.cuda.Stream(device))
    return have[:n]


# lnZ_* calls per launch chain the dealing aims at (the library takes up to 16 calls / 24 branches per chain)
chain_calls = int(os.environ.get("TRX_CHAIN_CALLS", "12"))


def _pieces(units, mine_k, n_streams):
    """this rank's units as contiguous runs of one target's calls: whole targets when there are at least as many as
    streams, else a target's calls in enough runs to keep the streams busy (a 75-scenario calc_probs: 50 calls in
    five runs of ten)"""
    units = as_units(units)
    jobs = []
    for k in mine_k:
        j = _job_of(units[k])
        if jobs and jobs[-1][0] == j:
            jobs[-1][1].append(k)
        else:
            jobs.append((j, [k]))
    out = []
    for _, ks in jobs:
        n = len(ks)
        want = -(-n // max(chain_calls, 1))
        if len(jobs) < n_streams:
            want = max(want, min(n_streams // len(jobs), n // 5))
        want = max(1, min(want, n))
        cost = [_COST.get(units[k].key, 1.0) for k in ks]
        total, acc, at = sum(cost), 0.0, 0
        for p in range(want):
            # contiguous, balanced by cost: piece p ends where the running cost passes (p + 1) / want of the total
            end = at
            while end < n and (p == want - 1 or acc + cost[end] <= total * (p + 1) / want + 1e-9 or end == at):
                acc += cost[end]
                end += 1
            if end > at:
                out.append(ks[at:end])
            at = end
    return out


class _Pass:
    """What the execution modes of one run_units pass share: the record table of all live units (after the gather every
    rank holds all of it), where each unit's rows lie in it, this rank's units and its calls still in flight."""

    def __init__(self, units, live, owner, base, dist, rank, verbose, layout):
        self.units, self.live, self.owner, self.base = units, live, owner, base
        self.dist, self.rank, self.verbose, self.layout = dist, rank, verbose, layout
        self.rows = {k: len(units[k].names) for k in live}
        self.at, total = {}, 0                        # unit -> its rows of the table
        for k in live:
            self.at[k] = slice(total, total + self.rows[k])
            total += self.rows[k]
        self.table = np.full((total, layout.width), np.nan)        # (what a path does not give -- moments, samples -- stays NaN)
        self.mine_k = [k for k in live if owner[k] == rank]
        self.pending = []                             # (unit, fused.Pending): calls in flight
        self.n_threads = 1

    def result(self, k, as_rows):
        return self.table[self.at[k]] if as_rows else _as_dicts(self.table[self.at[k]], self.layout)

    def put(self, k, rec):
        if self.layout.summary_q is not None:
            rec = self.layout.summarise(rec)         # (by the unit's owner, as its records come in: before the gather)
        self.table[self.at[k], :rec.shape[1]] = rec

    def resolve(self, pending):
        """the rows of calls whose streams have been synchronised -> the table; returns their units"""
        got = _fused.records_to_rows(pending)
        for k, rec in got.items():
            self.put(k, rec)
        return got

    def one(self, k):
        u, base, layout = self.units[k], self.base, self.layout
        if self.verbose == 1:
            print("Calculating " + ", ".join(u.names) + " scenario probabilit"
                  + ("y" if len(u.names) == 1 else "ies") + " for " + str(u.ID)
                  + (" [rank %d]" % self.rank if self.dist else "") + ".")
        if base is not None:
            unit_seed = (base + 7919 * (k + 1)) % (2 ** 32)
            _fused.set_thread_seed(unit_seed)        # the draw kernel's Philox key (thread-local)
            if self.n_threads == 1 and not _fused.threadable():
                np.random.seed(unit_seed)            # the numpy sampling modes
                import torch
                torch.manual_seed(unit_seed)         # staged draws from torch's generator
        mark = _lib.moments_mark()                   # (the moments this unit's evidences report: fused / ml)
        _fused.set_thread_unit(k)                    # (calc_probs_refined keeps an importance grid per unit)
        try:
            res = u.thunk()
        finally:
            _fused.set_thread_seed(None)
            _fused.set_thread_unit(None)
        mom = _lib.moments_since(mark)
        if isinstance(res, _fused.Pending):
            self.pending.append((k, res))            # list.append is atomic: worker threads share it
        else:
            blk = self.table[self.at[k]]
            blk[:, layout.record] = _record(res)
            if len(mom) == self.rows[k]:
                blk[:, layout.moments] = mom
            if layout.post_rows:
                for i, d in enumerate(res if isinstance(res, tuple) else (res,)):
                    blk[i, layout.extra] = layout.encode(d.get("posterior"))


def _run_units(units, live, owner, base, dist, world, rank, verbose, as_rows=False, job_done=None):
    # (the switches are read HERE, once a pass: whatever rides beside the records rides in the ONE all_gather below)
    global last_layout
    last_layout = RowLayout(_fused.POSTERIOR_ROWS, _fused.POSTERIOR_SUMMARY, _fused.WARP_HIST)
    p = _Pass(units, live, owner, base, dist, rank, verbose, last_layout)
    on_device = _fused.threadable() or _fused.staged_native()
    if on_device:
        import torch
        on_device = torch.cuda.is_available()          # (without a GPU the thunks fail loudly themselves)
    # (numpy's stream is consumed on this thread, call after call, in the reference's order: one host thread)
    if base is not None and on_device and _fused.threadable():
        p.n_threads = min(threads, len(p.mine_k))
    if p.n_threads <= 1 and not (on_device and p.mine_k):
        for k in p.mine_k:
            p.one(k)
    elif p.n_threads <= 1:
        _run_streams(p, as_rows, job_done)
    else:
        _run_threads(p)
    if dist:
        _gather(p, world)
    return [None if u.thunk is None else p.result(k, as_rows) for k, u in enumerate(units)]


def _run_streams(p, as_rows, job_done):
    """one host thread, a few streams: every call is enqueued, then one wait per stream"""
    import torch
    units, mine_k, pending = p.units, p.mine_k, p.pending
    device = torch.cuda.current_device()
    n_draws = max([units[k].draws for k in mine_k if units[k].draws is not None] + [1])
    cap = max(2, int(scratch_budget_bytes // stream_scratch_bytes(n_draws)))
    pool = _worker_streams(device, max(1, min(streams, cap, len(mine_k))))
    torch.cuda.current_stream().synchronize()    # inputs staged on the caller's stream
    _fused.begin_deferred(len(mine_k))
    drained = False
    # The cyclic garbage collector is held off while the calls are enqueued and awaited (freeze_gc above, DESIGN.md
    # section 4.5): the pass's few thousand small objects -- no reference cycles among them -- now and then tipped it into
    # a FULL collection, 75 ms inside a 140 ms step.  Reference counting frees them as before.
    import gc
    global _gc_frozen
    if freeze_gc and not _gc_frozen:
        gc.collect()                 # (once: what is alive now moves to the collector's permanent generation)
        gc.freeze()
        _gc_frozen = True
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        import time
        t0 = time.perf_counter()
        # The library turns consecutive calls on ONE stream that share a light curve's time stamps and N into one launch
        # chain (trx_star_enqueue, include/trx.h).  So the calls go to the streams in PIECES (_pieces), each to the stream
        # with the least work queued so far (by the schedule's cost weights); one library call per piece.
        load = [0.0] * len(pool)
        done_marks = []                # (event behind a piece, number of pending calls up to and including it)
        t_build = t_lib = 0.0          # of enqueue_s: Python building the argument blocks / inside trx_star_enqueue
        for piece in _pieces(units, mine_k, len(pool)):
            j = min(range(len(pool)), key=lambda i: (load[i], i))
            load[j] += sum(unit_cost(units[k]) for k in piece)
            t_a = time.perf_counter()
            with torch.cuda.stream(pool[j]):
                for k in piece:
                    p.one(k)
            t_b = time.perf_counter()
            _fused.flush()
            t_build += t_b - t_a
            t_lib += time.perf_counter() - t_b
            ev = torch.cuda.Event()
            ev.record(pool[j])
            done_marks.append((ev, len(pending)))
        timing["build_s"], timing["library_s"] = t_build, t_lib
        timing["enqueue_s"] = time.perf_counter() - t0
        # The records are turned into table rows piece by piece, as the pieces finish, while the GPU works on the later
        # ones (3-5 ms of every step that the host would else spend after the wait).  Pieces on one stream finish in
        # order; across streams the order of enqueueing is a good guess and a wrong one only waits a little longer.
        at = 0
        t_wait = 0.0
        # (a job whose units all have their rows is handed to the caller at once: run_units' docstring)
        left, members = {}, {}
        if job_done is not None:
            for k, u in enumerate(units):
                members.setdefault(_job_of(u), []).append(k)
            for k in mine_k:
                left[_job_of(units[k])] = left.get(_job_of(units[k]), 0) + 1
            for k in set(mine_k) - {k for k, _ in pending}:         # (calls that returned their records at once)
                left[_job_of(units[k])] -= 1
        for ev, upto in done_marks:
            t_w = time.perf_counter()
            ev.synchronize()
            t_wait += time.perf_counter() - t_w
            if upto > at:
                got = p.resolve(pending[at:upto])
                at = upto
                if job_done is not None:
                    for k in got:
                        j = _job_of(units[k])
                        left[j] -= 1
                        if left[j] == 0:
                            job_done(j, [None if units[m].thunk is None else p.result(m, as_rows) for m in members[j]])
        for st in pool:
            st.synchronize()
        drained = True
        timing["wait_s"] = t_wait
        if at < len(pending):
            p.resolve(pending[at:])
    finally:
        if not drained:
            # a call failed after others were enqueued: their kernels and record copies still use the
            # pinned block and the cached tables -- wait for them before anything is released
            for st in pool:
                st.synchronize()
        pending.clear()
        _fused.end_deferred()
        if gc_was_on:
            gc.enable()


def _run_threads(p):
    """worker threads, each on its own stream, take this rank's units from one queue, the dearest first"""
    import queue
    import threading
    import torch
    mine_k, n_threads = p.mine_k, p.n_threads
    device = torch.cuda.current_device()
    todo = queue.SimpleQueue()
    cost = {k: unit_cost(p.units[k]) for k in mine_k}
    for k in sorted(mine_k, key=lambda k: (-cost[k], k)):
        todo.put(k)
    errors = []
    pool_streams = _worker_streams(device, n_threads)

    def worker(stream):
        _lib.moments_swap([] if _fused.MOMENTS else None)
        try:
            torch.cuda.set_device(device)        # the current device is thread-local
            _fused.begin_deferred(len(mine_k))
            with torch.cuda.stream(stream):
                while True:
                    try:
                        k = todo.get_nowait()
                    except queue.Empty:
                        break
                    p.one(k)
                    _fused.flush()
        except BaseException as exc:              # re-raised in the caller's thread
            errors.append(exc)
        finally:
            stream.synchronize()                  # (also after an error: calls enqueued before it are in flight)
            _fused.end_deferred()
            _lib.moments_swap(None)

    torch.cuda.current_stream().synchronize()    # inputs staged on the caller's stream
    pool = [threading.Thread(target=worker, args=(pool_streams[i],)) for i in range(n_threads)]
    for t in pool:
        t.start()
    for t in pool:
        t.join()
    if errors:
        p.pending.clear()
        raise errors[0]
    p.resolve(p.pending)


def _gather(p, world):
    """ONE collective: every rank contributes the records of its own units (in unit order, padded to the largest share)
    behind one header row that carries its seed base -- a table row per scenario (RowLayout; 17 doubles without posterior
    columns), a few KB per rank, latency-bound: a direct all_gather, no ring, no bucketing"""
    import time
    import torch
    dist, table, rows, live, owner = p.dist, p.table, p.rows, p.live, p.owner
    t_g = time.perf_counter()
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    share = [sum(rows[k] for k in live if owner[k] == r) for r in range(world)]
    chunk = np.full((1 + max(share + [0]), p.layout.width), np.nan)
    chunk[0, 0] = float(p.base)
    at = 1
    for k in p.mine_k:
        chunk[at:at + rows[k]] = table[p.at[k]]
        at += rows[k]
    mine = torch.as_tensor(chunk).to(dev).reshape(-1)
    gathered = torch.empty(world * mine.numel(), dtype=mine.dtype, device=dev)
    dist.all_gather_into_tensor(gathered, mine)          # the single collective
    g = gathered.cpu().numpy().reshape((world,) + chunk.shape)
    global last_seed_bases, _warned_bases
    last_seed_bases = [int(b) for b in g[:, 0, 0]]
    if len(set(last_seed_bases)) > 1 and not _warned_bases:
        # (unseeded ranks just run; who seeded only some, or only numpy in "device" mode, should hear of it)
        import warnings
        warnings.warn("calc_probs on %d ranks: the ranks drew different seed bases %s, so this run is not reproducible "
                      "and its numbers depend on the partition.  Seed every rank alike (torch.manual_seed in 'device' "
                      "mode, np.random.seed in the numpy modes) for a repeatable, partition-independent run."
                      % (world, last_seed_bases[:4]), RuntimeWarning, stacklevel=5)
        _warned_bases = True
    at = [1] * world
    for k in live:
        r = owner[k]
        table[p.at[k]] = g[r, at[r]:at[r] + rows[k]]
        at[r] += rows[k]
    timing["gather_s"] = time.perf_counter() - t_g
