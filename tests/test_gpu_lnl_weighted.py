"""trx_lnl_batch_weighted on the GPU: the light-curve model and its chi^2 with one weight per
time stamp in one kernel -- cells_kernel<..., WT> -- against the CPU oracle, against the grid route on the device
(trx_flux_grid + trx_chi2_grid_weighted), its accumulation / secondary-eclipse / argument rules, and
target.calc_probs_datasets(evaluation="fused") against evaluation="grid".

Tolerances, none of them chosen here:
  RTOL_H = 1e-9    chi^2/2 of the device model against the oracle's: tests/test_gpu_kernels.py (RTOL_H, _cmp_h);
  1e-12 relative   the fused kernel against the grid route: the two evaluate the same model value in every cell (one
                   template, two output modes) and differ in the order of a sum of n_time terms -- the bar
                   tests/test_gpu_kernels.py::test_chi2_grid_matches_fused_and_oracle holds the unweighted pair to;
  end to end       |d lnZ| <= 1e-12 x (largest chi^2/2 among the row's draws within 80 of its best log-weight) + 1e-12,
                   from the 1e-12 relative agreement of the two chi^2 pipelines (tests/test_gpu_datasets.py).

Shapes: the smallest that reach each path of the kernel -- 64 / 65 stamps (rows batched per wave, even and odd length),
320 (the first one-row-per-wave length, uniform grid: centre-value stencil and window trips), 1100 (several 64-cell
trips skipped, more than one stencil chunk), 333 sorted random stamps (one row per wave, no stencil); 300 rows (more
than one workgroup of batches, a tapered tail), and 1 and 5 rows (a batch that is not full).
"""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

from helpers import GOLD, gold
from oracle import oracle as O
from triceratops_amd import _lib, synth
from triceratops_amd.datasets import sigma_bar

pytestmark = pytest.mark.gpu

RTOL_H = 1e-9
RTOL_ROUTES = 1e-12
INF = float("inf")
MODELS = ((O.MODEL_TP, False), (O.MODEL_EB, False), (O.MODEL_EB_TWIN, True))
# (n_time, irregular stamps, rows)
SHAPES = ((64, False, 300), (65, False, 300), (65, False, 1), (65, False, 5), (320, False, 300), (1100, False, 300),
          (333, True, 300))
_IDS = ["%d%s-n%d" % (nt, "irr" if irr else "", n) for nt, irr, n in SHAPES]

_cases = {}


def _case(model, twin, n_time, irregular, n):
    """the light curve of tests/test_gpu_datasets.py::_lnl_case with sigma_t = U(0.5, 2) x synth.SIGMA, n rows of the
    model, the oracle's curves and secondary depths, and everything on the device -- made once per shape and model"""
    key = (model, n_time, irregular, n)
    if key not in _cases:
        rng = np.random.default_rng(synth.SEED + n_time)
        t = synth.time_grid(n_time)
        if irregular:
            t = np.sort(rng.uniform(t[0], t[-1], n_time))
        curve = O.flux_grid(O.MODEL_TP, t, synth.reference_tp_row())[0][0]
        flux = synth.noisy_light_curve(rng, curve)
        sig = rng.uniform(0.5, 2.0, n_time) * synth.SIGMA
        rows = synth.tp_rows(rng, n) if model == O.MODEL_TP else synth.eb_rows(rng, n, twin=twin)
        grid, sec = O.flux_grid(model, t, rows)
        c = dict(t=t, flux=flux, sig=sig, w=1.0 / sig ** 2, rows=rows, grid=grid, sec=sec,
                 limit=1.5 * sigma_bar([sig]) if model == O.MODEL_EB else INF)
        c.update(t_d=_lib.dev(t), f_d=_lib.dev(flux), w_d=_lib.dev(c["w"]), rows_d=_lib.dev(rows))
        _cases[key] = c
    return _cases[key]


def _fused(c, model, flags=0, limit=None, out=None, w_d=None):
    return _lib.lnl_batch_weighted(model, flags, c["t_d"], c["f_d"], c["w_d"] if w_d is None else w_d, c["rows_d"],
                                   synth.EXPTIME, synth.NSAMPLES, c["limit"] if limit is None else limit, out=out)


def _grid_route(c, model, flags=0, limit=None, w_d=None):
    grid, sec = _lib.flux_grid(model, flags, c["t_d"], c["rows_d"], synth.EXPTIME, synth.NSAMPLES)
    return _lib.chi2_grid_weighted(c["f_d"], c["w_d"] if w_d is None else w_d, grid, sec if model == O.MODEL_EB else None,
                                   c["limit"] if limit is None else limit)


def _rel(got, want):
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


# ---------------------------------------------------------------------------------------
# 1. against the CPU oracle
@pytest.mark.parametrize("model,twin", MODELS, ids=["TP", "EB", "EB_TWIN"])
@pytest.mark.parametrize("n_time,irregular,n", SHAPES, ids=_IDS)
def test_weighted_likelihood_against_the_oracle(model, twin, n_time, irregular, n):
    c = _case(model, twin, n_time, irregular, n)
    got = _fused(c, model).cpu().numpy()
    want = 0.5 * np.sum((c["flux"] - c["grid"]) ** 2 / c["sig"] ** 2, axis=1)
    if model == O.MODEL_EB:
        want[c["sec"] >= c["limit"]] = np.inf
        if n == 300:
            assert 0 < np.isposinf(want).sum() < n          # excluded and kept rows
    assert not np.isnan(got).any()
    assert np.array_equal(np.isposinf(want), np.isposinf(got))
    rel = _rel(got, want)
    print("model %d n_time %d n %d: max relative error against the oracle %.3g" % (model, n_time, n, rel))
    assert rel < RTOL_H


# ---------------------------------------------------------------------------------------
# 2. against the grid route on the device
@pytest.mark.parametrize("model,twin", MODELS, ids=["TP", "EB", "EB_TWIN"])
@pytest.mark.parametrize("n_time,irregular,n", SHAPES, ids=_IDS)
def test_weighted_likelihood_against_the_grid_route(model, twin, n_time, irregular, n):
    c = _case(model, twin, n_time, irregular, n)
    got = _fused(c, model).cpu().numpy()
    want = _grid_route(c, model).cpu().numpy()
    assert np.array_equal(np.isposinf(want), np.isposinf(got)) and np.array_equal(np.isnan(want), np.isnan(got))
    rel = _rel(got, want)
    print("model %d n_time %d n %d: max relative difference to the grid route %.3g" % (model, n_time, n, rel))
    assert rel < RTOL_ROUTES


@pytest.mark.parametrize("n_time,irregular", [(65, False), (320, False), (333, True)], ids=["65", "320", "333irr"])
def test_fp32_model_flag_reaches_the_weighted_kernel(n_time, irregular):
    """TRX_FLAG_FP32_MODEL: both routes then carry the fp32 flux model, cell for cell the same value -- the bar between
    the routes stays 1e-12 --, and the result moves against the fp64 one (the flag is not ignored) by no more than the
    fp32 model's error allows: |d h| <= sum_t w_t |r_t| eps + n_time eps^2 w_max / 2 with eps = 2e-6, the bound
    tests/test_gpu_batch.py holds the fp32 model to"""
    c = _case(O.MODEL_TP, False, n_time, irregular, 300)
    got = _fused(c, _lib.MODEL_TP, _lib.FLAG_FP32_MODEL).cpu().numpy()
    want = _grid_route(c, _lib.MODEL_TP, _lib.FLAG_FP32_MODEL).cpu().numpy()
    rel = _rel(got, want)
    print("fp32 n_time %d: max relative difference to the grid route %.3g" % (n_time, rel))
    assert rel < RTOL_ROUTES
    fp64 = _fused(c, _lib.MODEL_TP).cpu().numpy()
    eps = 2e-6
    slack = np.sum(c["w"] * np.abs(c["flux"] - c["grid"]), axis=1) * eps + 0.5 * n_time * eps ** 2 * c["w"].max()
    assert not np.array_equal(got, fp64)
    assert (np.abs(got - fp64) <= slack).all()


# ---------------------------------------------------------------------------------------
# 3. semantics
def test_accumulation_over_two_light_curves():
    for model, twin in MODELS:
        ca, cb = _case(model, twin, 65, False, 300), _case(model, twin, 333, True, 300)
        # (one parameter block for both light curves)
        cb = dict(cb, rows_d=ca["rows_d"])
        a, b = _fused(ca, model, limit=INF), _fused(cb, model, limit=INF)
        ab = _fused(cb, model, limit=INF, out=a.clone())
        ba = _fused(ca, model, limit=INF, out=b.clone())
        assert torch.isfinite(ab).all()
        assert torch.equal(ab, a + b) and torch.equal(ba, b + a)          # two datasets = the sum of two plain calls
        x, y = ab.cpu().numpy(), ba.cpu().numpy()
        assert (np.abs(x - y) <= 1e-12 * x).all()
        assert ab.data_ptr() != a.data_ptr() and not torch.equal(ab, a)


def test_secondary_rule_and_accumulation():
    c = _case(O.MODEL_EB, False, 65, False, 300)
    first = _fused(c, _lib.MODEL_EB)
    excluded = c["sec"] >= c["limit"]
    assert 0 < excluded.sum() < 300
    assert np.array_equal(np.isposinf(first.cpu().numpy()), excluded)
    # +inf survives a second light curve, with a rule of its own and without one; no NaN appears
    c2 = dict(_case(O.MODEL_EB, False, 64, False, 300), rows_d=c["rows_d"])
    for limit in (INF, c["limit"]):
        more = _fused(c2, _lib.MODEL_EB, limit=limit, out=first.clone()).cpu().numpy()
        assert np.array_equal(np.isposinf(more), excluded) and not np.isnan(more).any()
        plain = _fused(c2, _lib.MODEL_EB, limit=INF).cpu().numpy()
        assert np.array_equal(more[~excluded], first.cpu().numpy()[~excluded] + plain[~excluded])
    # sec_limit = +inf: the rule is off
    off = _fused(c, _lib.MODEL_EB, limit=INF).cpu().numpy()
    assert np.isfinite(off).all()
    assert np.array_equal(off[~excluded], first.cpu().numpy()[~excluded])
    # the limit is taken as given: equality excludes, the next double above does not
    dev_sec = _lib.flux_grid(_lib.MODEL_EB, 0, c["t_d"], c["rows_d"], synth.EXPTIME, synth.NSAMPLES)[1].cpu().numpy()
    k = int(np.argsort(dev_sec)[150])
    at = _fused(c, _lib.MODEL_EB, limit=float(dev_sec[k])).cpu().numpy()
    above = _fused(c, _lib.MODEL_EB, limit=float(np.nextafter(dev_sec[k], np.inf))).cpu().numpy()
    assert np.isposinf(at[k]) and np.isfinite(above[k])
    assert np.array_equal(np.isposinf(at), dev_sec >= dev_sec[k])


def test_nan_secondary_depth_excludes_nothing():
    """a companion flux ratio of 1 makes the dilution of the secondary depth inf / inf: the depth is NaN, the weighted
    rule (depth >= limit) keeps the row -- its chi^2 is NaN like its model -- where trx_lnl_batch's !(depth < limit)
    gives +inf"""
    c = _case(O.MODEL_EB, False, 65, False, 300)
    rows = c["rows"].copy()
    bad = np.arange(0, 300, 37)
    rows[10, bad] = 1.0
    cn = dict(c, rows_d=_lib.dev(rows))
    dev_sec = _lib.flux_grid(_lib.MODEL_EB, 0, cn["t_d"], cn["rows_d"], synth.EXPTIME, synth.NSAMPLES)[1].cpu().numpy()
    if not np.isnan(dev_sec[bad]).all():
        pytest.skip("synth has no parameter block with a NaN secondary depth")
    got = _fused(cn, _lib.MODEL_EB).cpu().numpy()
    want = _grid_route(cn, _lib.MODEL_EB).cpu().numpy()
    assert not np.isposinf(got[bad]).any() and np.isnan(got[bad]).all()
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isnan(got), np.isnan(want))
    scalar = _lib.lnl_batch(_lib.MODEL_EB, 0, cn["t_d"], cn["f_d"], synth.SIGMA, cn["rows_d"], synth.EXPTIME,
                            synth.NSAMPLES).cpu().numpy()
    assert np.isposinf(scalar[bad]).all()


@pytest.mark.parametrize("model,twin", MODELS, ids=["TP", "EB", "EB_TWIN"])
def test_zero_weights_drop_points(model, twin):
    rng = np.random.default_rng(synth.SEED + 7)
    # irregular stamps, one row per wave in both calls: the same model value in every kept cell, another order of the sum
    c = _case(model, twin, 333, True, 300)
    drop = np.zeros(333, dtype=bool)
    drop[rng.choice(333, 10, replace=False)] = True
    assert 333 - drop.sum() >= _lib.CELL_PACKING_BELOW
    w0 = np.where(drop, 0.0, c["w"])
    got = _fused(c, model, w_d=_lib.dev(w0)).cpu().numpy()
    kept = dict(c, t_d=_lib.dev(c["t"][~drop]), f_d=_lib.dev(c["flux"][~drop]), w_d=_lib.dev(c["w"][~drop]))
    want = _fused(kept, model).cpu().numpy()
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isnan(got).any()
    assert _rel(got, want) < RTOL_ROUTES
    # batched rows on a uniform grid (dropping stamps would leave another kind of grid): against the oracle
    c = _case(model, twin, 65, False, 300)
    drop = np.zeros(65, dtype=bool)
    drop[rng.choice(65, 9, replace=False)] = True
    got = _fused(c, model, w_d=_lib.dev(np.where(drop, 0.0, c["w"]))).cpu().numpy()
    want = 0.5 * np.sum(((c["flux"] - c["grid"]) ** 2 / c["sig"] ** 2)[:, ~drop], axis=1)
    if model == O.MODEL_EB:
        want[c["sec"] >= c["limit"]] = np.inf
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isnan(got).any()
    assert _rel(got, want) < RTOL_H


@pytest.mark.parametrize("n_time,irregular", [(65, False), (320, False), (333, True)], ids=["65", "320", "333irr"])
def test_equal_weights_are_the_scalar_sigma_kernel(n_time, irregular):
    for model, twin in MODELS:
        c = _case(model, twin, n_time, irregular, 300)
        w_d = _lib.dev(np.full(n_time, 1.0 / synth.SIGMA ** 2))
        got = _fused(c, model, limit=1.5 * synth.SIGMA if model == O.MODEL_EB else INF, w_d=w_d).cpu().numpy()
        want = _lib.lnl_batch(model, _lib.FLAG_FULL_EVALUATION, c["t_d"], c["f_d"], synth.SIGMA, c["rows_d"],
                              synth.EXPTIME, synth.NSAMPLES).cpu().numpy()
        assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isnan(got).any()
        rel = _rel(got, want)
        print("model %d n_time %d: max relative difference to trx_lnl_batch %.3g" % (model, n_time, rel))
        assert rel < RTOL_ROUTES


def test_argument_errors_enqueue_nothing():
    c = _case(O.MODEL_TP, False, 65, False, 5)
    L = _lib.lib()
    out = torch.full((5,), -7.0, dtype=torch.float64, device=c["rows_d"].device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t, f, w, p, o = (c["t_d"].data_ptr(), c["f_d"].data_ptr(), c["w_d"].data_ptr(), c["rows_d"].data_ptr(), out.data_ptr())

    def call(model=_lib.MODEL_TP, time=t, flux=f, inv_var=w, n_time=65, params=p, n=5, out_ptr=o):
        return L.trx_lnl_batch_weighted(model, 0, time, flux, inv_var, n_time, params, n, synth.EXPTIME, synth.NSAMPLES,
                                        INF, 0, out_ptr, st)

    assert call(n=0) == 0                                                   # n == 0: nothing runs
    for kw in (dict(model=_lib.MODEL_RAW), dict(model=17), dict(time=None), dict(flux=None), dict(inv_var=None),
               dict(params=None), dict(out_ptr=None), dict(n=-1), dict(n_time=0), dict(n_time=-3)):
        assert call(**kw) == 1, kw                                          # TRX_ERR_ARG
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                              # nothing was enqueued
    assert _lib.lnl_batch_weighted(_lib.MODEL_TP, 0, c["t_d"], c["f_d"], c["w_d"], c["rows_d"][:, :0].contiguous(),
                                   synth.EXPTIME, synth.NSAMPLES).shape == (0,)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and (out > 0).all()


# ---------------------------------------------------------------------------------------
# 4. end to end: calc_probs_datasets(evaluation="fused") against evaluation="grid"
G = gold("toi465_calc_probs.npz")
CC = os.path.join(GOLD, "toi465_cc.csv")
STAR_COLS = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
SEED = 465
LC = dict(time=G["time"], flux=G["flux"], sigma=float(G["sigma"][0]), P_orb=float(G["P_orb"][0]))
KW = dict(contrast_curve_file=CC, N=20000, parallel=True, verbose=0)
N_POST = 50


def _target():
    from triceratops_amd.triceratops import target
    st = pd.DataFrame({c: G["real_stars_%s" % c] for c in STAR_COLS})
    st["ID"] = st["ID"].astype(np.int64)
    return target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))


def _two_cadences():
    """TOI-465.01's 100 points as two cadences with per-point errors (tests/test_gpu_datasets.py::_two_cadences)"""
    sigma = LC["sigma"]
    ia, ib = np.arange(0, 100, 2), np.arange(2, 100, 4)[:21]
    ea = sigma * np.linspace(0.6, 1.8, 50)
    a = {"time": LC["time"][ia], "flux": LC["flux"][ia], "flux_err": ea, "exptime": 0.00139, "nsamples": 20}
    b = {"time": LC["time"][ib], "flux": LC["flux"][ib], "flux_err": 1.4 * sigma, "exptime": 0.0208, "nsamples": 5}
    assert a["time"].size == 50 and b["time"].size == 21
    return [a, b]


@pytest.fixture
def device_mode():
    import triceratops_amd as ta
    mode = ta.get_sampling()
    ta.set_sampling("device")
    yield
    ta.set_sampling(mode)


def _pass(monkeypatch, evaluation, datasets=None):
    """one calc_probs_datasets pass from the seed (datasets: _two_cadences() unless given): the target's results, per
    evidence the largest chi^2/2 among the draws within 80 of the best log-weight, the calls of _lib.flux_grid and the
    peak of the allocator above its level at the start"""
    hmax, grids = [], []
    real_lnz, real_grid = _lib.lnz_from_halfchi2, _lib.flux_grid

    def lnz_spy(h_d, lp_d, n_total, lnsigma):
        h = h_d.cpu().numpy()
        x = -h if lp_d is None else lp_d.cpu().numpy() - h
        ok = np.isfinite(x)
        hmax.append(float(h[ok][x[ok] >= x[ok].max() - 80.0].max()) if ok.any() else 0.0)
        return real_lnz(h_d, lp_d, n_total, lnsigma)

    def grid_spy(*args, **kwargs):
        grids.append(args[3].shape[1])
        return real_grid(*args, **kwargs)

    monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz_spy)
    monkeypatch.setattr(_lib, "flux_grid", grid_spy)
    tg = _target()
    torch.manual_seed(SEED)
    _lib.reset_stats()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    level = torch.cuda.memory_allocated()
    tg.calc_probs_datasets(_two_cadences() if datasets is None else datasets, LC["P_orb"], n_samples=N_POST, evaluation=evaluation, **KW)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - level
    monkeypatch.undo()
    cols = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB")
    return dict(lnZ=tg.lnZ.copy(), prob=tg.probs.prob.values.copy(), best=np.stack([tg.probs[c].values for c in cols]),
                u1=tg.u1.copy(), frc=tg.fluxratio_comp.copy(), FPP=float(tg.FPP), NFPP=float(tg.NFPP),
                posterior=tg.posterior, sigma_ref=tg.sigma_ref, stats=dict(_lib.STATS), hmax=np.array(hmax),
                grids=grids, peak=peak)


def test_calc_probs_datasets_fused_is_the_grid_evaluation(device_mode, monkeypatch):
    grid = _pass(monkeypatch, "grid")
    fused = _pass(monkeypatch, "fused")
    # the same masked draws, counted the same way; one launch per dataset and evidence
    assert fused["stats"]["rows"] == grid["stats"]["rows"] > 0 and fused["stats"]["cells"] == grid["stats"]["cells"]
    # (one chunk at this N: the grid route launches once per dataset and evidence, too; an evidence without a masked
    # draw launches nothing)
    assert 0 < fused["stats"]["launches"] == grid["stats"]["launches"] <= 2 * fused["hmax"].size
    assert fused["stats"]["launches"] % 2 == 0
    # the same best draws
    assert np.array_equal(fused["best"], grid["best"]) and np.array_equal(fused["u1"], grid["u1"])
    assert np.array_equal(fused["frc"], grid["frc"]) and fused["sigma_ref"] == grid["sigma_ref"]
    # the same evidences
    fin = np.isfinite(grid["lnZ"])
    assert np.array_equal(fin, np.isfinite(fused["lnZ"])) and fin.sum() >= 10
    assert grid["hmax"].size == fin.size == fused["hmax"].size
    d = np.abs(fused["lnZ"][fin] - grid["lnZ"][fin])
    bound = 1e-12 * grid["hmax"][fin] + 1e-12
    print("fused against grid: max |d lnZ| %.3g, max of |d lnZ| / bound %.3g, max |d prob| %.3g, |d FPP| %.3g, |d NFPP| %.3g"
          % (d.max(), (d / bound).max(), np.abs(fused["prob"] - grid["prob"]).max(), abs(fused["FPP"] - grid["FPP"]),
             abs(fused["NFPP"] - grid["NFPP"])))
    assert (d <= bound).all(), (d, bound)
    assert abs(fused["FPP"] - grid["FPP"]) <= 1e-12 and abs(fused["NFPP"] - grid["NFPP"]) <= 1e-12
    # the same posterior rows
    assert len(fused["posterior"]) == len(grid["posterior"]) == fin.size
    for j, (p, q) in enumerate(zip(fused["posterior"], grid["posterior"])):
        assert (p is None) == (q is None)
        if p is None:
            continue
        assert p["row"].shape == (N_POST,) and np.array_equal(p["row"], q["row"])
        assert all(np.array_equal(p[k], q[k]) for k in q if k != "lnw")
        assert (np.abs(p["lnw"] - q["lnw"]) <= 1e-12 * grid["hmax"][j] + 1e-12).all()
    # no grid: trx_flux_grid is never called, and the allocator's peak stays below the grid route's
    assert fused["grids"] == [] and len(grid["grids"]) == grid["stats"]["launches"]
    print("allocator peak above the level at the start: grid %d B, fused %d B" % (grid["peak"], fused["peak"]))
    assert fused["peak"] < grid["peak"]
