"""The importance map of the draw kernels (trx_draw_args.warp) and the weight histogram (trx_scenario_args.warp_hist):
DESIGN.md section 12.  Exact checks: the identity grid is no grid, bit for bit; the kernel's map is _numerics.warp_apply
and its Jacobian is in the prior column; the fp32 pre-test, the mask pass and the fill pass see the same mapped numbers;
the histogram is the one numpy forms from the draws' uniforms and weights, and repeats bit for bit, alone or in a chain."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import staged as _staged
from test_gpu_posterior import SEED, _device_mode
from test_gpu_posterior_chain import _calls, _slots

pytestmark = pytest.mark.gpu

KINDS = {"TTP": 0, "PTP": 2, "TEB": 1, "BEB": 9}          # places in test_gpu_posterior_chain._calls()
# the slots each scenario takes from the kernel's own generator (P is fixed in these calls; 7, the field star, is never mapped)
CONSUMED = {"TTP": (2, 3, 5, 6), "PTP": (1, 2, 3, 5, 6), "TEB": (3, 4, 5, 6), "BEB": (3, 4, 5, 6)}


def _four():
    c = _calls()
    return [c[i] for i in KINDS.values()]


def _grid(seed=3):
    """a fixed non-trivial grid: two refinements on random, strongly peaked histograms (density floor 0.1)"""
    from triceratops_amd import _numerics as nm
    rng = np.random.default_rng(seed)
    e = nm.warp_identity()
    for _ in range(2):
        e = nm.warp_refine(e, rng.random((nm.WARP_DIMS, nm.WARP_BINS)) ** 10 * 1e9)
    assert np.all(np.diff(e, axis=1) > 0) and not np.array_equal(e, nm.warp_identity())
    return e


def _star(calls, chain, grids=None, hist=False, rows=0, extra_flags=0, counts=None):
    """ONE trx_star_enqueue of the calls on one stream; call i is work unit i (grids: {unit: edges}).  Per call: (the
    record's defined slots, posterior block or None, histogram [nbr][WARP_BRANCH] or None, the whole record)."""
    from triceratops_amd import _lib, fused
    L = _lib.lib()
    old = (fused.POSTERIOR_ROWS, fused.TABLE_ROWS, _lib.EXTRA_FLAGS, fused.WARP_GRIDS, fused.WARP_HIST)
    sink = _lib.moments_swap([])
    pends = []
    with _device_mode():
        try:
            L.trx_set_star_chain(1 if chain else 0)
            _lib.EXTRA_FLAGS = extra_flags
            fused.POSTERIOR_ROWS, fused.TABLE_ROWS, fused.WARP_GRIDS, fused.WARP_HIST = rows, 1, grids, hist
            fused.set_thread_seed(SEED)
            fused.begin_deferred(len(calls))
            for i, (name, args, kw) in enumerate(calls):
                fused.set_thread_unit(i)
                pends.append(getattr(fused, name)(*args, **kw))
                assert isinstance(pends[-1], fused.Pending)
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
                out.append((rec[_slots(p)], None if p.post is None else p.post.numpy()[:nbr].copy(),
                            None if p.hist is None else p.hist.numpy()[:nbr].copy().view(np.uint64), rec))
        finally:
            fused.set_thread_unit(None)
            fused.end_deferred()
            _lib.moments_swap(sink)
            L.trx_set_star_chain(1)
            fused.POSTERIOR_ROWS, fused.TABLE_ROWS, _lib.EXTRA_FLAGS, fused.WARP_GRIDS, fused.WARP_HIST = old
    return out


def _operator(call, grid, monkeypatch):
    """the call through trx_draw_scenario with `dump` (the operator chain, every draw in full) on the same seed:
    {"dump" [9][N], "cols", "mask", "mask_twin", "lnprior", "h": chi^2/2 per branch, "scen": the _Scenario}"""
    from triceratops_amd import _lib, fused
    name, args, kw = call
    dump, hs, scen = [], [], []
    real, real_chain = _lib.lnz_scenario, fused._Scenario.run_operator_chain

    def spy(model, flags, time_d, flux_d, sigma, block, *rest):
        h, lnz = real(model, flags, time_d, flux_d, sigma, block, *rest)
        hs.append(h[:block.shape[1]].cpu().numpy())
        return h, lnz

    def keep_scen(self, *a):
        scen.append(self)
        return real_chain(self, *a)

    monkeypatch.setattr(_lib, "lnz_scenario", spy)
    monkeypatch.setattr(fused._Scenario, "run_operator_chain", keep_scen)
    monkeypatch.setattr(fused, "DUMP", dump)
    monkeypatch.setattr(fused, "TABLE_ROWS", 1)
    monkeypatch.setattr(fused, "WARP_GRIDS", None if grid is None else {0: grid})
    with _device_mode():
        fused.set_thread_seed(SEED)
        fused.set_thread_unit(0)
        try:
            getattr(fused, name)(*args, **kw)
        finally:
            fused.set_thread_unit(None)
        torch.cuda.synchronize()
    monkeypatch.undo()
    d = {k: (None if v is None else v.cpu().numpy()) for k, v in dump[0].items()}
    d["h"], d["scen"] = hs, scen[0]
    return d


# ---- 1. identity grid = no grid ------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("chain", [False, True])
def test_identity_grid_is_no_grid_bit_for_bit(chain, full):
    from triceratops_amd import _lib, _numerics as nm
    _lib.require_gpu()
    flags = _lib.FLAG_FULL_EVALUATION if full else 0
    counts = []
    plain = _star(_four(), chain, None, rows=257, extra_flags=flags, counts=counts)
    ident = _star(_four(), chain, {i: nm.warp_identity() for i in range(4)}, rows=257, extra_flags=flags, counts=counts)
    if chain and not full:
        assert counts[0][:2] == (1, 4) and counts[1][:2] == (1, 4), counts        # both really chained
    for i, (a, b) in enumerate(zip(plain, ident)):
        assert a[0].tobytes() == b[0].tobytes(), "record (with moments) of call %d" % i
        assert a[1].tobytes() == b[1].tobytes(), "posterior block of call %d" % i
        assert np.all(np.isfinite(a[1][:, 3])) and np.all(a[1][:, 3] > 0)


@pytest.mark.parametrize("kind", list(KINDS))
def test_identity_grid_leaves_the_dump_alone(kind, monkeypatch):
    from triceratops_amd import _lib, _numerics as nm
    _lib.require_gpu()
    call = _calls()[KINDS[kind]]
    a, b = _operator(call, None, monkeypatch), _operator(call, nm.warp_identity(), monkeypatch)
    for k in ("dump", "cols", "mask", "mask_twin"):
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert a[k].tobytes() == b[k].tobytes(), k
    if a["lnprior"] is None:
        assert np.all(b["lnprior"] == 0.0)            # (a scenario without a prior: the forced column holds ln J = 0)
    else:
        assert a["lnprior"].tobytes() == b["lnprior"].tobytes()
    for ha, hb in zip(a["h"], b["h"]):
        assert ha.tobytes() == hb.tobytes()


# ---- 2. the map ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_kernel_maps_as_warp_apply_and_every_phase_sees_it(kind, monkeypatch):
    from triceratops_amd import _lib, fused, _numerics as nm
    _lib.require_gpu()
    call = _calls()[KINDS[kind]]
    grid = _grid()
    ident = _operator(call, nm.warp_identity(), monkeypatch)
    warped = _operator(call, grid, monkeypatch)
    y, u = ident["dump"], warped["dump"]
    used = CONSUMED[kind]
    lnj = np.zeros(y.shape[1])
    for d in range(7):
        if d in used:
            err = np.max(np.abs(u[d] - nm.warp_apply(grid[d], y[d])))
            print("%s slot %d: max |u - warp_apply| = %.3g" % (kind, d, err))
            assert err <= 2e-16
            assert not np.array_equal(u[d], y[d])
            lnj += nm.warp_lnj(grid[d], y[d])
        else:
            assert u[d].tobytes() == y[d].tobytes() and np.all(u[d] == 0.0)       # never drawn
    assert u[7].tobytes() == y[7].tobytes()                                       # the field-star index is never mapped
    if kind in ("TTP", "TEB"):
        # no prior of the scenario's own: the mapped run's column less the identity run's is ln J itself
        both = np.isfinite(ident["lnprior"]) & np.isfinite(warped["lnprior"])
        assert both.all() and np.max(np.abs((warped["lnprior"] - ident["lnprior"]) - lnj)) <= 1e-13
    # (PTP, BEB: the prior itself is a function of mapped uniforms -- q_companion, q -- so the yardstick is the prior of
    # the SAME physical draws: the staged run below, fed the mapped numbers, no map, no ln J)
    staged = _staged(warped, fused)
    assert staged["mask"].tobytes() == warped["mask"].tobytes()
    if warped["mask_twin"] is not None:
        assert staged["mask_twin"].tobytes() == warped["mask_twin"].tobytes()
    assert staged["cols"].tobytes() == warped["cols"].tobytes()
    # ln J: the mapped run's prior column less the prior of the SAME physical draws (the staged run: no map, no ln J)
    prior0 = staged["lnprior"] if staged["lnprior"] is not None else np.zeros(y.shape[1])
    fin = np.isfinite(prior0) & np.isfinite(warped["lnprior"])
    assert fin.any()
    err = np.max(np.abs((warped["lnprior"][fin] - prior0[fin]) - lnj[fin]))
    print("%s: max |ln J - sum log(64 width)| = %.3g over %d rows" % (kind, err, int(fin.sum())))
    assert err <= 1e-13
    # the library's own chain (fp32 pre-test, mask pass, fill pass) on the mapped numbers: the same masked counts
    rec = _star([call], False, {0: grid})[0][3]
    W, ncol = fused.SCENARIO_OUT_MOMENTS, (11 if staged["mask_twin"] is None else 14)
    assert rec[ncol + 1] == staged["mask"].sum()
    if staged["mask_twin"] is not None:
        assert rec[W + ncol + 1] == staged["mask_twin"].sum()


# ---- 3. the histogram ------------------------------------------------------------------------------------------------
def _expected_hist(run, y, used, X_dev):
    """numpy's histogram per branch from the run's masks, chi^2/2, prior column and the PRE-MAP uniforms y"""
    out = []
    masks = [run["mask"]] + ([] if run["mask_twin"] is None else [run["mask_twin"]])
    for b, (m, h) in enumerate(zip(masks, run["h"])):
        idx = np.flatnonzero(m)
        assert idx.size == h.size
        sigma = run["scen"].sigma
        x = (-0.5 * np.log(2 * np.pi) - np.log(sigma)) - h
        if run["lnprior"] is not None:
            x = x + run["lnprior"][idx]
        X = X_dev[b]
        assert abs(X - np.nanmax(x)) < 1e-9
        d = x - X
        keep = d > -80.0
        q = np.floor(np.minimum(np.exp(d[keep]), 1.0) * 2.0 ** 32)
        bins = np.zeros((7, 64))
        rows = np.zeros((7, 64))
        for s in used:
            k = np.minimum((y[s][idx][keep] * 64).astype(int), 63)
            np.add.at(bins[s], k, q)
            np.add.at(rows[s], k, 1.0)
        out.append((int(keep.sum()), bins, rows))
    return out


@pytest.mark.parametrize("kind", ["TTP", "PTP", "TEB", "BEB"])
@pytest.mark.parametrize("mapped", [False, True])
def test_histogram_is_numpys(kind, mapped, monkeypatch):
    from triceratops_amd import _lib, _numerics as nm
    _lib.require_gpu()
    call = _calls()[KINDS[kind]]
    grid = _grid() if mapped else None
    y = _operator(call, None, monkeypatch)["dump"]                       # the pre-map uniforms of this seed
    run = _operator(call, grid, monkeypatch) if mapped else _operator(call, nm.warp_identity(), monkeypatch)
    got = _star([call], False, None if grid is None else {0: grid}, hist=True)[0][2]
    X = np.ascontiguousarray(got[:, 0]).view(np.float64)
    for b, (n_rows, bins, rows) in enumerate(_expected_hist(run, y, CONSUMED[kind], X)):
        assert got[b, 1] == n_rows and np.all(got[b, 2:8] == 0)
        dev = got[b, 8:].astype(np.float64).reshape(7, 64)
        worst = np.max(np.abs(dev - bins) - rows)
        print("%s branch %d: %d rows with weight, worst |device - numpy| - rows in bin = %g" % (kind, b, n_rows, worst))
        assert np.all(np.abs(dev - bins) <= rows)
        for s in range(7):
            if s not in CONSUMED[kind]:
                assert np.all(dev[s] == 0)
        assert dev.sum() > 0


def test_histogram_repeats_in_and_out_of_a_chain_and_leaves_the_records_alone():
    from triceratops_amd import _lib
    _lib.require_gpu()
    grids = {i: _grid(10 + i) for i in range(4)}
    counts = []
    chained = _star(_four(), True, grids, hist=True, counts=counts)
    single = _star(_four(), False, grids, hist=True, counts=counts)
    again = _star(_four(), True, grids, hist=True)
    without = _star(_four(), True, grids, hist=False, counts=counts)
    assert counts[0][:2] == (1, 4) and counts[1][:2] == (0, 0) and counts[2][:2] == (1, 4), counts       # a chain stays a chain
    for i in range(4):
        assert chained[i][2].tobytes() == single[i][2].tobytes() == again[i][2].tobytes(), i
        assert chained[i][0].tobytes() == single[i][0].tobytes() == without[i][0].tobytes(), i
        assert chained[i][2][:, 1].min() > 0
    # a mapped call and an unmapped one do not share a chain: the chain splits there (include/trx.h)
    counts = []
    mixed = _star(_four(), True, {0: grids[0], 1: grids[1]}, hist=True, counts=counts)
    assert counts[0][:2] == (2, 4), counts
    for i in (0, 1):
        assert mixed[i][2].tobytes() == chained[i][2].tobytes() and mixed[i][0].tobytes() == chained[i][0].tobytes()


def test_branches_without_weight_get_zeros():
    """a call none of whose draws passes the geometry (a period of 1e9 days) and one whose evidence is -inf (sigma =
    1e-170: every chi^2 overflows), beside an ordinary one"""
    from triceratops_amd import _lib
    _lib.require_gpu()
    calls = _calls()[:3]
    name, args, kw = calls[1]
    calls[1] = (name, args[:3] + (1e9,) + args[4:], kw)
    name, args, kw = calls[2]
    calls[2] = (name, args[:2] + (1e-170,) + args[3:], kw)
    for chain in (True, False):
        out = _star(calls, chain, None, hist=True)
        assert out[0][2][0, 1] > 0 and out[0][2][0, 8:].sum() > 0
        assert not out[1][2].any() and not out[2][2].any()
