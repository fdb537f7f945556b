"""Posterior rows inside launch chains (trx_star_enqueue, csrc/trx_scenario.hip enqueue_chain) and
calc_posteriors_many.  The yardstick for every number is the same call enqueued on its own (trx_set_star_chain(0), or
target.calc_posteriors): records and posterior blocks must agree bit for bit, because the chain's posterior kernels run
the single-call kernels' bodies with the call's own key and counter."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import GOLD
from test_gpu_posterior import N_DRAWS, SEED, _device_mode, _gold, _target

pytestmark = pytest.mark.gpu

TRI = os.path.join(GOLD, "trilegal_synth.csv")
CC = os.path.join(GOLD, "toi465_cc.csv")
ROWS = (1000, 0, 1, 257, 4096, 0, 1000, 257, 0, 1, 4096, 1000)       # post_rows of the twelve calls


def _calls():
    """a target's twelve calls: the ten scenarios of the target star (planet and binary kinds, with and without a
    companion prior) and the two of a nearby star"""
    G = _gold()
    s = lambda k: float(G["real_stars_%s" % k][0])
    lc = (G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0]))
    star = (s("mass"), s("rad"), s("Teff"))
    mags = (s("Tmag"), s("Jmag"), s("Hmag"), s("Kmag"))
    kw = dict(N=N_DRAWS, parallel=True)
    plain = lc + star + (0.0,)
    bound = plain + (s("plx"), CC, "TESS")
    field = plain + mags + (TRI, CC, "TESS")
    back = lc + star + mags + (TRI, CC, "TESS")
    return [("lnZ_TTP", plain, kw), ("lnZ_TEB", plain, kw), ("lnZ_PTP", bound, kw), ("lnZ_PEB", bound, kw),
            ("lnZ_STP", bound, kw), ("lnZ_SEB", bound, kw), ("lnZ_DTP", field, kw), ("lnZ_DEB", field, kw),
            ("lnZ_BTP", back, kw), ("lnZ_BEB", back, kw), ("lnZ_TTP", plain, kw), ("lnZ_TEB", plain, kw)]


def _slots(pend):
    """the record slots a call defines (tests/test_gpu_posterior.py::test_record_is_unchanged_by_posterior_rows)"""
    W = pend.stride
    nbr, ncol = (1, 11) if pend.scen.a.planet else (2, 14)
    return [b * W + i for b in range(nbr) for i in list(range(ncol + 2)) + list(range(16, W))] + [2 * W]


def _star(rows, chain, extra_flags=0, table_at=None, calls=None, counts=None):
    """ONE trx_star_enqueue of the calls on one stream: per call (defined record slots, posterior block [nbr][8 + 16 M]
    or None, the Pending); every second call asks for TRX_FLAG_WEIGHT_MOMENTS.  counts: a list that receives
    trx_debug_chain_counts of this enqueue."""
    from triceratops_amd import _lib, fused
    L = _lib.lib()
    calls = _calls() if calls is None else calls
    old = (fused.POSTERIOR_ROWS, fused.TABLE_ROWS, _lib.EXTRA_FLAGS)
    sink = _lib.moments_swap(None)
    pends = []
    with _device_mode():
        try:
            L.trx_set_star_chain(1 if chain else 0)
            _lib.EXTRA_FLAGS = extra_flags
            fused.set_thread_seed(SEED)
            fused.begin_deferred(len(calls))
            for i, (name, args, kw) in enumerate(calls):
                fused.POSTERIOR_ROWS = rows[i]
                fused.TABLE_ROWS = 100 if i == table_at else 1
                _lib.moments_swap([] if i % 2 else None)
                pend = getattr(fused, name)(*args, **kw)
                assert isinstance(pend, fused.Pending)
                pends.append(pend)
            c = [ctypes.c_long(0) for _ in range(3)]
            L.trx_debug_chain_counts(None, None, None, 1)
            fused.flush()
            L.trx_debug_chain_counts(ctypes.byref(c[0]), ctypes.byref(c[1]), ctypes.byref(c[2]), 0)
            if counts is not None:
                counts.append(tuple(int(x.value) for x in c))
            torch.cuda.synchronize()
            out = []
            for p in pends:
                nbr = 1 if p.scen.a.planet else 2
                rec = p.out.numpy().copy()
                out.append((rec[_slots(p)], None if p.post is None else p.post.numpy()[:nbr].copy(), p))
        finally:
            fused.end_deferred()
            _lib.moments_swap(sink)
            L.trx_set_star_chain(1)
            fused.POSTERIOR_ROWS, fused.TABLE_ROWS, _lib.EXTRA_FLAGS = old
    return out


def _equal(a, b):
    for i, ((ra, pa, _), (rb, pb, _)) in enumerate(zip(a, b)):
        assert ra.tobytes() == rb.tobytes(), "record of call %d" % i
        assert (pa is None) == (pb is None)
        if pa is not None:
            assert pa.shape == pb.shape and pa.tobytes() == pb.tobytes(), "posterior block of call %d" % i


@pytest.mark.parametrize("full", [False, True])
def test_chain_equals_the_calls_one_by_one_and_they_really_chained(full):
    """1 and 2: twelve calls with post_rows 0, 1, 257, 1000, 4096 mixed, with and without moments, in one chain.
    With TRX_FLAG_FULL_EVALUATION the equality is asserted all the same, but no chain forms: a launch chain is built
    from the passes of the bounded evaluation (lnl_chain_applicable, as before posterior rows), so such calls go one by
    one with chains switched on, too."""
    from triceratops_amd import _lib
    _lib.require_gpu()
    flags = _lib.FLAG_FULL_EVALUATION if full else 0
    counts = []
    chained = _star(ROWS, True, flags, counts=counts)
    single = _star(ROWS, False, flags, counts=counts)
    assert counts[0] == ((0, 0, 0) if full else (1, 12, sum(1 for m in ROWS if m > 0))), counts
    assert counts[1] == (0, 0, 0), counts
    _equal(chained, single)
    for (rec, post, pend), M in zip(chained, ROWS):
        assert (post is None) == (M == 0)
        if M:
            assert post.shape[1] == 8 + 16 * M and np.all(post[:, 3] > 0) and np.all(np.isfinite(post))
            pos = post[:, 8 + 14 * M:8 + 15 * M]
            assert np.all(np.diff(pos, axis=1) >= 0)
    # the key is the call's own: calls 0 and 10 are the same scenario with different seeds, and differ
    assert chained[0][1][0, 0] != chained[10][1][0, 0]


def test_a_table_call_goes_alone_and_splits_the_chain():
    from triceratops_amd import _lib
    _lib.require_gpu()
    counts = []
    chained = _star(ROWS, True, table_at=5, counts=counts)
    single = _star(ROWS, False, table_at=5, counts=counts)
    # calls 0 .. 4 and 6 .. 11 chain, call 5 goes alone (it has no posterior rows: ROWS[5] = 0)
    assert counts[0] == (2, 11, sum(1 for m in ROWS if m > 0)) and counts[1] == (0, 0, 0), counts
    _equal(chained, single)
    rows = list(ROWS)
    rows[5] = 257                                            # a table AND posterior rows: still alone
    both = _star(rows, True, table_at=5, counts=counts)
    assert counts[2] == (2, 11, sum(1 for m in ROWS if m > 0)), counts
    _equal(both, _star(rows, False, table_at=5))


def test_records_of_neighbours_are_untouched():
    """3: only ONE call of the chain has post_rows > 0: the other records are those of the all-zero chain"""
    from triceratops_amd import _lib
    _lib.require_gpu()
    counts = []
    none = _star([0] * 12, True, counts=counts)
    one = _star([0, 0, 0, 1000] + [0] * 8, True, counts=counts)
    assert counts == [(1, 12, 0), (1, 12, 1)]
    for i, ((ra, pa, _), (rb, pb, _)) in enumerate(zip(none, one)):
        assert ra.tobytes() == rb.tobytes(), i
        assert pa is None and (pb is None) == (i != 3)
    assert np.all(one[3][1][:, 3] > 0)


def test_degenerate_branches_inside_a_chain():
    """4: a call none of whose draws passes the geometry mask (a period of 1e9 days) and a call whose evidence is -inf
    (sigma = 1e-170: every chi^2 overflows) beside ordinary ones: header [3] = 0, sixteen rows NaN, neighbours as in
    the chain without the two"""
    from triceratops_amd import _lib
    _lib.require_gpu()
    calls = _calls()[:6]
    name, args, kw = calls[1]
    calls[1] = (name, args[:3] + (1e9,) + args[4:], kw)                  # binary, no masked draw
    name, args, kw = calls[2]
    calls[2] = (name, args[:2] + (1e-170,) + args[3:], kw)               # planet with a prior, evidence -inf
    rows = [1000, 257, 1000, 4096, 1, 1000]
    counts = []
    chained = _star(rows, True, calls=calls, counts=counts)
    single = _star(rows, False, calls=calls)
    assert counts[0] == (1, 6, 6)
    _equal(chained, single)
    rec, post, pend = chained[1]
    W = pend.stride
    assert rec[14 + 1] == 0 and rec[14 + 2 + (W - 16) + 14 + 1] == 0     # masked counts of both branches
    assert np.all(post[:, 3] == 0) and np.all(np.isnan(post[:, 8:]))
    rec, post, pend = chained[2]
    assert rec[11] == -np.inf and rec[12] > 0                            # lnZ = -inf with masked draws
    assert post[0, 3] == 0 and np.all(np.isnan(post[0, 8:]))
    for i in (0, 3, 4, 5):
        assert np.all(chained[i][1][:, 3] > 0) and np.all(np.isfinite(chained[i][1]))
    # the ordinary calls do not notice their neighbours: the same chain with ordinary calls in places 1 and 2
    plain = _star(rows, True, calls=_calls()[:6])
    for i in (0, 3, 4, 5):
        assert chained[i][0].tobytes() == plain[i][0].tobytes() and chained[i][1].tobytes() == plain[i][1].tobytes(), i


# ---------------------------------------------------------------------------------------------------------------------
M_ROWS = 1000


def _jobs():
    """TOI-465.01 with its full light curve and, a second target, with every second point (another N too: two chains'
    worth of different shapes)"""
    G = _gold()
    kw = dict(contrast_curve_file=CC, parallel=True)
    a = dict(time=G["time"], flux_0=G["flux"], flux_err_0=float(G["sigma"][0]), P_orb=float(G["P_orb"][0]), N=N_DRAWS, **kw)
    b = dict(time=G["time"][::2].copy(), flux_0=G["flux"][::2].copy(), flux_err_0=float(G["sigma"][0]),
             P_orb=float(G["P_orb"][0]), N=60000, **kw)
    return [(_target(), a), (_target(), b)]


def _with_base(monkeypatch, base, fn):
    """fn() with per-unit seeding from a GIVEN base: unit k of the pass draws from base + 7919 (k + 1)"""
    from triceratops_amd import sharding
    monkeypatch.setattr(sharding, "_draw_base", lambda: base)
    monkeypatch.setattr(sharding, "per_unit_seed", True)
    try:
        return fn()
    finally:
        monkeypatch.undo()


def test_calc_posteriors_many_equals_the_loop(monkeypatch):
    """5: tables and error attributes equal calc_probs_many's from the same seed bit for bit; every .posterior[j] equals
    what calc_posteriors on that target alone gives for the same unit seeds.  Per-unit seeds are base + 7919 (k + 1) with
    k the unit's index in the PASS, so the loop's pass over the second target starts from base + 7919 x (the units of
    the first): sharding._draw_base is replaced by a constant for that (no generator decides the base then)."""
    import triceratops_amd
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    BASE = 465001
    triceratops_amd.set_sampling("device")
    try:
        probs = _jobs()
        _with_base(monkeypatch, BASE, lambda: triceratops_amd.calc_probs_many(probs))
        many = _jobs()
        _with_base(monkeypatch, BASE, lambda: triceratops_amd.calc_posteriors_many(many, n_samples=M_ROWS))
        assert fused.POSTERIOR_ROWS == 0
        loop = _jobs()
        n_first = len(loop[0][0]._prepare(**loop[0][1])[0])
        for (tg, kw), base in zip(loop, (BASE, BASE + 7919 * n_first)):
            kw = dict(kw)
            call = [kw.pop(k) for k in ("time", "flux_0", "flux_err_0", "P_orb")]
            _with_base(monkeypatch, base, lambda: tg.calc_posteriors(*call, n_samples=M_ROWS, verbose=0, **kw))
    finally:
        triceratops_amd.set_sampling("numpy")
    for (p, _), (m, _), (l, _) in zip(probs, many, loop):
        for name in ("lnZ", "ess", "lnZ_err"):
            assert np.asarray(getattr(p, name)).tobytes() == np.asarray(getattr(m, name)).tobytes(), name
        assert p.probs.equals(m.probs)
        assert p.FPP == m.FPP and p.NFPP == m.NFPP and p.FPP_err == m.FPP_err and p.NFPP_err == m.NFPP_err
        assert all(x is None for x in p.posterior)
        assert np.asarray(l.lnZ).tobytes() == np.asarray(m.lnZ).tobytes()
        assert len(m.posterior) == len(l.posterior) == 15
        n_with = 0
        for j, (x, y) in enumerate(zip(m.posterior, l.posterior)):
            assert (x is None) == (y is None) == (not np.isfinite(m.lnZ[j])), j
            if x is not None:
                n_with += 1
                assert set(x) == set(y) == set(fused.POSTERIOR_KEYS)
                for key in x:
                    assert x[key].shape == (M_ROWS,) and np.array_equal(x[key], y[key]), (j, key)
        assert n_with >= 8
        assert m.posterior_summary().equals(l.posterior_summary())
        assert len(m.posterior_samples(50, rng=np.random.default_rng(1))) == 50


def test_keep_summary_is_np_quantile_of_keep_samples(monkeypatch):
    """6: from the same seed, keep="summary" holds exactly np.quantile of what keep="samples" holds"""
    import triceratops_amd
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    q = (0.16, 0.5, 0.84)
    triceratops_amd.set_sampling("device")
    try:
        a, b = _jobs(), _jobs()
        torch.manual_seed(77)
        triceratops_amd.calc_posteriors_many(a, n_samples=M_ROWS)
        torch.manual_seed(77)
        triceratops_amd.calc_posteriors_many(b, n_samples=M_ROWS, keep="summary", q=q)
    finally:
        triceratops_amd.set_sampling("numpy")
    for (x, _), (y, _) in zip(a, b):
        assert np.asarray(x.lnZ).tobytes() == np.asarray(y.lnZ).tobytes() and x.FPP == y.FPP
        assert y.posterior is None and x.posterior_quantiles is None
        for j, (p, s) in enumerate(zip(x.posterior, y.posterior_quantiles)):
            assert (p is None) == (s is None), j
            if p is not None:
                for c in fused.POSTERIOR_KEYS[:14]:
                    assert np.array_equal(np.quantile(p[c], q), s[c]), (j, c)
        assert x.posterior_summary(q).equals(y.posterior_summary(q)) and len(x.posterior_summary(q)) >= 8
        with pytest.raises(ValueError):
            y.posterior_summary((0.5,))


# ---------------------------------------------------------------------------------------------------------------------
# 7: the summary-width table through the device-tensor branch of the collective (a one-rank "nccl" group, as
# tests/test_gpu_rccl_world1.py runs calc_probs_many; that file's child is an inline script, so this one has its own)
_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import triceratops_amd
import torch, torch.distributed as dist
from triceratops_amd import fused, sharding, synth
torch.cuda.set_device(0)
store = "/tmp/trx_test_pg_post_%%d" %% os.getpid()
dist.init_process_group("nccl", init_method="file://" + store, rank=0, world_size=1, device_id=torch.device("cuda", 0))
triceratops_amd.set_sampling("device")
gold = os.path.join(%(root)r, "tests", "golden")
Q = (0.16, 0.5, 0.84)
sent = []
real = dist.all_gather_into_tensor
def spy(out, mine, *a, **k):
    sent.append((int(mine.numel()), mine.device.type))
    return real(out, mine, *a, **k)
dist.all_gather_into_tensor = spy
def batch(collective):
    jobs = synth.toi_jobs(4, n_time=200, N=50000, seed=synth.SEED, trilegal_fname=os.path.join(gold, "trilegal_synth.csv"),
                          contrast_curve_file=os.path.join(gold, "contrast_curve_synth.csv"))
    torch.manual_seed(9)
    sharding.collective_at_world_one = collective
    sharding.per_unit_seed = not collective        # (the multi-rank path seeds per unit: same numbers either way)
    try:
        return triceratops_amd.calc_posteriors_many(jobs, n_samples=500, keep="summary", q=Q)
    finally:
        sharding.collective_at_world_one = False
        sharding.per_unit_seed = False
plain = batch(False)
sharding.timing["gather_s"] = 0.0
coll = batch(True)
equal, rows_with = True, 0
for a, b in zip(plain, coll):
    equal = equal and np.array_equal(a.lnZ, b.lnZ, equal_nan=True) and a.FPP == b.FPP and b.posterior is None
    for x, y in zip(a.posterior_quantiles, b.posterior_quantiles):
        equal = equal and (x is None) == (y is None)
        if x is not None:
            rows_with += 1
            equal = equal and all(np.array_equal(x[c], y[c]) for c in fused.POSTERIOR_PARAMS)
    equal = equal and a.posterior_summary(Q).equals(b.posterior_summary(Q))
rows = sum(len(t.lnZ) for t in coll)
out = {"backend": dist.get_backend(), "equal": bool(equal), "rows_with": rows_with, "sent": sent, "rows": rows,
       "gather_s": float(sharding.timing["gather_s"]), "switches": [int(fused.POSTERIOR_ROWS), fused.POSTERIOR_SUMMARY]}
dist.barrier()
dist.destroy_process_group()
print("RESULT " + json.dumps(out))
"""


def test_summary_mode_through_a_one_rank_rccl_group():
    import json
    import subprocess
    import sys
    from triceratops_amd import sharding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    p = subprocess.run([sys.executable, "-c", _CHILD % {"root": root}], capture_output=True, text=True, timeout=600,
                       cwd=root, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    print(d)
    assert d["backend"] == "nccl" and d["equal"] and d["rows_with"] >= 20 and d["gather_s"] > 0.0
    width = len(sharding.RECORD_COLS) + len(sharding.MOMENT_COLS) + 14 * 3
    # ONE collective, a device tensor: the header row and this rank's rows (every live row of the batch), summary wide
    assert len(d["sent"]) == 1 and d["sent"][0][1] == "cuda"
    assert d["sent"][0][0] % width == 0 and 1 < d["sent"][0][0] // width <= 1 + d["rows"]
    assert d["switches"] == [0, None]
