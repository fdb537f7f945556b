"""Several light curves with per-point errors on the GPU: chi2_rows_kernel<STAGE, Chi2Plain>, the array
path of lnL_*_p, and target.calc_probs_datasets against calc_probs (one dataset, one sigma) and against the CPU oracle
(two cadences, errors that differ from point to point).

Tolerances, none of them chosen here:
  1e-12 relative   the weighted reduction against numpy on the downloaded grid -- the bar of
                   tests/test_gpu_kernels.py::test_chi2_grid_matches_fused_and_oracle for the unweighted kernel;
  RTOL_H = 1e-9    chi^2/2 of the device model against the oracle's: tests/test_gpu_kernels.py (RTOL_H, _cmp_h);
  LNZ_TOL = 1e-9   lnZ against the oracle, absolute: tests/test_gpu_golden.py ("lnZ absolute 1e-9") and the 1e-9 of
                   tests/test_gpu_fused.py::_same;
  one dataset against calc_probs: |d lnZ| <= 1e-12 x (largest chi^2/2 among the row's draws within 80 of its best
                   log-weight) + 1e-12, from the 1e-12 relative agreement of the two chi^2 pipelines.
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

pytestmark = pytest.mark.gpu

RTOL_H = 1e-9
LNZ_TOL = 1e-9
G = gold("toi465_calc_probs.npz")
CC = os.path.join(GOLD, "toi465_cc.csv")
STAR_COLS = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
SEED = 465
TARGET_SHARE = float(G["real_stars_fluxratio"][G["real_stars_tdepth"] > 0][0])      # the first star that can host the signal


# ---------------------------------------------------------------------------------------
# 1. the kernel
def _want(f, w, g):
    return 0.5 * np.sum(w * (f - g) ** 2, axis=1)


_kernel_cache = {}


def _kernel_case(n_time, n):
    """EB rows, their device grid and secondary depths, a light curve and per-point errors (made once per shape)"""
    key = (n_time, n)
    if key not in _kernel_cache:
        rng = np.random.default_rng(synth.SEED + 1000 * n_time + n)
        t = synth.time_grid(n_time)
        rows = synth.eb_rows(rng, n)
        grid, sec = _lib.flux_grid(_lib.MODEL_EB, 0, _lib.dev(t), _lib.dev(rows), synth.EXPTIME, synth.NSAMPLES)
        flux = 1.0 + rng.normal(0.0, synth.SIGMA, n_time)
        sig = rng.uniform(0.5, 2.0, n_time) * synth.SIGMA
        _kernel_cache[key] = (grid, sec, flux, 1.0 / sig ** 2, grid.cpu().numpy(), sec.cpu().numpy())
    return _kernel_cache[key]


@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("n_time", [1, 2, 33, 64, 65, 399])
def test_weighted_reduction_matches_numpy(n_time, n):
    grid, _, flux, w, g, _ = _kernel_case(n_time, n)
    f_d, w_d = _lib.dev(flux), _lib.dev(w)
    got = _lib.chi2_grid_weighted(f_d, w_d, grid)
    want = _want(flux, w, g)
    rel = np.abs(got.cpu().numpy() - want) / want
    print("n_time %d n %d: max relative error %.3g" % (n_time, n, rel.max()))
    assert rel.max() < 1e-12
    # two identical calls: identical bits
    again = _lib.chi2_grid_weighted(f_d, w_d, grid)
    assert torch.equal(got, again)
    # every operand one double off its 16-byte boundary: the same bits (the 8-byte loads feed the same arithmetic)
    pad = torch.empty(grid.numel() + 1, dtype=torch.float64, device=grid.device)
    pad[1:] = grid.reshape(-1)
    f_off = torch.cat([f_d[:1], f_d])[1:]
    w_off = torch.cat([w_d[:1], w_d])[1:]
    g_off = pad[1:].view(n, n_time)
    assert g_off.data_ptr() % 16 == 8 and f_off.data_ptr() % 16 == 8 and f_off.is_contiguous()
    off = _lib.chi2_grid_weighted(f_off, w_off, g_off)
    assert torch.equal(off, got)
    # ... and a row's value does not depend on where the grid starts (the chunks of fused._datasets_halfchi2)
    if n > 2:
        tail = _lib.chi2_grid_weighted(f_d, w_d, grid[1:])
        assert torch.equal(tail, got[1:])


def test_weighted_reduction_accumulates():
    (ga, _, fa, wa, _, _), (gb, _, fb, wb, _, _) = _kernel_case(65, 257), _kernel_case(33, 257)
    a = _lib.chi2_grid_weighted(_lib.dev(fa), _lib.dev(wa), ga)
    b = _lib.chi2_grid_weighted(_lib.dev(fb), _lib.dev(wb), gb)
    ab = _lib.chi2_grid_weighted(_lib.dev(fb), _lib.dev(wb), gb, out=a.clone())
    ba = _lib.chi2_grid_weighted(_lib.dev(fa), _lib.dev(wa), ga, out=b.clone())
    assert torch.equal(ab, a + b)                                  # two datasets = the sum of two single calls
    assert torch.equal(ab, ba)
    assert (np.abs(ab.cpu().numpy() - ba.cpu().numpy()) <= 1e-12 * ab.cpu().numpy()).all()
    assert ab.data_ptr() != a.data_ptr() and not torch.equal(ab, a)


def test_weighted_reduction_secondary_rule():
    grid, sec_d, flux, w, g, sec = _kernel_case(64, 257)
    limit = float(np.median(sec))
    sec_nan = sec.copy()
    sec_nan[:7] = np.nan
    sec_nan[7] = limit                                             # equality excludes
    got = _lib.chi2_grid_weighted(_lib.dev(flux), _lib.dev(w), grid, _lib.dev(sec_nan), limit).cpu().numpy()
    excluded = sec_nan >= limit                                    # (false for NaN)
    assert excluded[7] and not excluded[:7].any() and 0 < excluded.sum() < excluded.size
    assert np.array_equal(np.isposinf(got), excluded)
    want = _want(flux, w, g)
    assert np.array_equal(got[~excluded], _lib.chi2_grid_weighted(_lib.dev(flux), _lib.dev(w), grid).cpu().numpy()[~excluded])
    assert (np.abs(got[~excluded] - want[~excluded]) < 1e-12 * want[~excluded]).all()
    # +inf survives a second dataset, with and without a rule of its own
    more = _lib.chi2_grid_weighted(_lib.dev(flux), _lib.dev(w), grid, out=_lib.dev(got))
    assert np.array_equal(np.isposinf(more.cpu().numpy()), excluded) and not np.isnan(more.cpu().numpy()).any()
    assert np.array_equal(more.cpu().numpy()[~excluded], 2 * got[~excluded])


def test_weighted_reduction_arguments():
    grid, _, flux, w, _, _ = _kernel_case(33, 5)
    f_d, w_d = _lib.dev(flux), _lib.dev(w)
    empty = _lib.chi2_grid_weighted(f_d, w_d, grid[:0])
    assert empty.shape == (0,)
    L, out = _lib.lib(), torch.full((5,), -7.0, dtype=torch.float64, device=grid.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    inf = float("inf")
    ptrs = (f_d.data_ptr(), w_d.data_ptr(), grid.data_ptr())
    assert L.trx_chi2_grid_weighted(*ptrs, 33, 0, None, inf, 0, out.data_ptr(), st) == 0          # n == 0: nothing runs
    for args in ((None, ptrs[1], ptrs[2], 33, 5, None, inf, 0, out.data_ptr()),
                 (ptrs[0], None, ptrs[2], 33, 5, None, inf, 0, out.data_ptr()),
                 (ptrs[0], ptrs[1], None, 33, 5, None, inf, 0, out.data_ptr()),
                 (*ptrs, 33, 5, None, inf, 0, None),
                 (*ptrs, 33, -1, None, inf, 0, out.data_ptr()),
                 (*ptrs, 0, 5, None, inf, 0, out.data_ptr())):
        assert L.trx_chi2_grid_weighted(*args, st) == 1                                            # TRX_ERR_ARG
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                                                     # nothing was enqueued


# ---------------------------------------------------------------------------------------
# 2. and 3. the array path of lnL_*_p
_LNL = (("lnL_TP_p", O.MODEL_TP, False), ("lnL_EB_p", O.MODEL_EB, False), ("lnL_EB_twin_p", O.MODEL_EB_TWIN, True))


def _lnl_case(n_time, n=300):
    rng = np.random.default_rng(synth.SEED + n_time)
    t = synth.time_grid(n_time)
    curve = O.flux_grid(O.MODEL_TP, t, synth.reference_tp_row())[0][0]
    return rng, t, synth.noisy_light_curve(rng, curve)


@pytest.mark.parametrize("n_time", [64, 65])
def test_array_sigma_equals_scalar_sigma(n_time):
    from triceratops_amd import likelihoods as lk
    rng, t, flux = _lnl_case(n_time)
    for name, model, twin in _LNL:
        rows = synth.tp_rows(rng, 300) if model == O.MODEL_TP else synth.eb_rows(rng, 300, twin=twin)
        scalar = getattr(lk, name)(t, flux, synth.SIGMA, *rows)
        array = getattr(lk, name)(t, flux, np.full(n_time, synth.SIGMA), *rows)
        assert np.array_equal(np.isposinf(scalar), np.isposinf(array)) and not np.isnan(array).any()
        if model == O.MODEL_EB:
            assert 0 < np.isposinf(scalar).sum() < 300
        fin = np.isfinite(scalar)
        rel = np.abs(array[fin] - scalar[fin]) / scalar[fin]
        print("%s n_time %d: max relative difference %.3g" % (name, n_time, rel.max()))
        assert rel.max() < 1e-12


@pytest.mark.parametrize("n_time", [64, 65])
def test_per_point_sigma_against_the_oracle(n_time):
    from triceratops_amd import likelihoods as lk
    from triceratops_amd.datasets import sigma_bar
    rng, t, flux = _lnl_case(n_time)
    sig = rng.uniform(0.5, 2.0, n_time) * synth.SIGMA
    for name, model, twin in _LNL:
        rows = synth.tp_rows(rng, 300) if model == O.MODEL_TP else synth.eb_rows(rng, 300, twin=twin)
        got = getattr(lk, name)(t, flux, sig, *rows)
        grid, sec = O.flux_grid(model, t, rows)
        want = 0.5 * np.sum((flux - grid) ** 2 / sig ** 2, axis=1)
        if model == O.MODEL_EB:
            want[sec >= 1.5 * sigma_bar([sig])] = np.inf
            assert 0 < np.isposinf(want).sum() < 300
        assert np.array_equal(np.isposinf(want), np.isposinf(got)) and not np.isnan(got).any()
        fin = np.isfinite(want)
        rel = np.abs(got[fin] - want[fin]) / want[fin]
        print("%s n_time %d: max relative error against the oracle %.3g" % (name, n_time, rel.max()))
        assert rel.max() < RTOL_H


# ---------------------------------------------------------------------------------------
# 4. - 8. calc_probs_datasets
def _target():
    from triceratops_amd.triceratops import target
    st = pd.DataFrame({c: G["real_stars_%s" % c] for c in STAR_COLS})
    st["ID"] = st["ID"].astype(np.int64)
    return target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))


@pytest.fixture
def device_mode():
    import triceratops_amd as ta
    mode = ta.get_sampling()
    ta.set_sampling("device")
    yield
    ta.set_sampling(mode)


LC = dict(time=G["time"], flux=G["flux"], sigma=float(G["sigma"][0]), P_orb=float(G["P_orb"][0]))
KW = dict(contrast_curve_file=CC, N=20000, parallel=True, verbose=0)
_runs = {}


def _weights_spy(monkeypatch):
    """per evidence of a pass, in order: the largest chi^2/2 among the draws within 80 of the best log-weight"""
    seen = []
    real = _lib.lnz_from_halfchi2

    def spy(h_d, lp_d, n_total, lnsigma):
        h = h_d.cpu().numpy()
        x = -h if lp_d is None else lp_d.cpu().numpy() - h
        ok = np.isfinite(x)
        seen.append(float(h[ok][x[ok] >= x[ok].max() - 80.0].max()) if ok.any() else 0.0)
        return real(h_d, lp_d, n_total, lnsigma)

    monkeypatch.setattr(_lib, "lnz_from_halfchi2", spy)
    return seen


def _snapshot(tg):
    cols = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB")
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": _lib.STATS["rows"],
            "best": np.stack([tg.probs[c].values for c in cols]), "u1": tg.u1.copy(), "frc": tg.fluxratio_comp.copy()}


def _one_dataset_runs(monkeypatch):
    """calc_probs, calc_probs_datasets([the same light curve, scalar sigma]) and the even / odd split, from one seed"""
    if not _runs:
        tg = _target()
        torch.manual_seed(SEED)
        _lib.reset_stats()
        tg.calc_probs(LC["time"], LC["flux"], LC["sigma"], LC["P_orb"], **KW)
        _runs["calc_probs"] = _snapshot(tg)
        one = [{"time": LC["time"], "flux": LC["flux"], "flux_err": LC["sigma"]}]
        hmax = _weights_spy(monkeypatch)
        torch.manual_seed(SEED)
        _lib.reset_stats()
        tg.calc_probs_datasets(one, LC["P_orb"], **KW)
        _runs["one"] = _snapshot(tg)
        _runs["hmax"] = np.array(hmax)
        _runs["sigma_ref"] = tg.sigma_ref
        two = [{"time": LC["time"][k::2], "flux": LC["flux"][k::2], "flux_err": LC["sigma"]} for k in (0, 1)]
        torch.manual_seed(SEED)
        _lib.reset_stats()
        tg.calc_probs_datasets(two, LC["P_orb"], **KW)
        _runs["two"] = _snapshot(tg)
        monkeypatch.undo()
    return _runs


def _check_same_evidence(a, b, hmax, what):
    assert a["rows"] == b["rows"] > 0, "masked counts differ"
    assert np.array_equal(a["best"], b["best"]) and np.array_equal(a["u1"], b["u1"]) and np.array_equal(a["frc"], b["frc"])
    fin = np.isfinite(b["lnZ"])
    assert np.array_equal(fin, np.isfinite(a["lnZ"])) and fin.sum() >= 10 and hmax.size == fin.size
    d = np.abs(a["lnZ"][fin] - b["lnZ"][fin])
    bound = 1e-12 * hmax[fin] + 1e-12
    print("%s: max |d lnZ| %.3g, max of |d lnZ| / bound %.3g, max |d prob| %.3g"
          % (what, d.max(), (d / bound).max(), np.abs(a["prob"] - b["prob"]).max()))
    assert (d <= bound).all(), (d, bound)
    assert np.abs(a["prob"] - b["prob"]).max() <= 2 * d.max()


def test_one_dataset_is_calc_probs(device_mode, monkeypatch):
    r = _one_dataset_runs(monkeypatch)
    assert r["sigma_ref"] == LC["sigma"] / float(TARGET_SHARE)
    _check_same_evidence(r["one"], r["calc_probs"], r["hmax"], "one dataset against calc_probs")


def test_split_light_curve_is_the_same_evidence(device_mode, monkeypatch):
    r = _one_dataset_runs(monkeypatch)
    _check_same_evidence(r["two"], r["one"], r["hmax"], "even / odd split against one dataset")


# -- two cadences, per-point errors
DROP = ["STP", "SEB", "DTP", "DEB", "BTP", "BEB"]
KW2 = dict(contrast_curve_file=CC, N=4000, parallel=True, verbose=0, drop_scenario=DROP)
N_SCEN = 6          # TP, EB, EBx2P, PTP, PEB, PEBx2P


def _two_cadences(mean_errors=False):
    sigma = LC["sigma"]
    ia, ib = np.arange(0, 100, 2), np.arange(2, 100, 4)[:21]
    ea = sigma * np.linspace(0.6, 1.8, 50)                       # varying 3x
    if mean_errors:
        ea = np.full(50, ea.mean())
    a = {"time": LC["time"][ia], "flux": LC["flux"][ia], "flux_err": ea, "exptime": 0.00139, "nsamples": 20}
    b = {"time": LC["time"][ib], "flux": LC["flux"][ib], "flux_err": 1.4 * sigma, "exptime": 0.0208, "nsamples": 5}
    assert a["time"].size == 50 and b["time"].size == 21
    return [a, b]


_het = {}


def _het_runs(monkeypatch):
    """the pass on the two-cadence input (with 200 posterior samples), its draws (fused.DUMP on the same seed: the
    draws do not depend on the light curve) and the pass with dataset A's errors replaced by their mean"""
    from triceratops_amd import fused
    if not _het:
        tg = _target()
        dump = []
        monkeypatch.setattr(fused, "DUMP", dump)
        torch.manual_seed(SEED)
        tg.calc_probs_datasets(_two_cadences(), LC["P_orb"], n_samples=200, **KW2)
        monkeypatch.undo()
        _het["lnZ"], _het["posterior"], _het["sigma_ref"] = tg.lnZ.copy(), tg.posterior, tg.sigma_ref
        _het["best"] = tg.probs.copy()
        _het["draws"] = [{k: (None if v is None else v.cpu().numpy()) for k, v in d.items() if k != "dump"} for d in dump]
        torch.manual_seed(SEED)
        tg.calc_probs_datasets(_two_cadences(mean_errors=True), LC["P_orb"], **KW2)
        _het["lnZ_mean"] = tg.lnZ.copy()
        _het["oracle"] = _oracle_evidences(_het["draws"], tg)
    return _het


def _oracle_evidences(draws, tg):
    """per scenario row (x of every masked draw, lnZ): h from the oracle's model curves and numpy weights, the EB rule
    on the host, log-mean-exp from the oracle"""
    from triceratops_amd.datasets import Datasets, validate
    ds = Datasets(validate(_two_cadences())).renorm(float(TARGET_SHARE))
    assert len(draws) == 4
    out = []
    for d in draws:
        cols, planet = d["cols"], d["mask_twin"] is None
        branches = ((O.MODEL_TP, d["mask"], False),) if planet else ((O.MODEL_EB, d["mask"], False),
                                                                     (O.MODEL_EB_TWIN, d["mask_twin"], True))
        for model, mask, twin in branches:
            idx = np.flatnonzero(mask)
            block = cols[:10 if planet else 11][:, idx].copy()
            if twin:
                block[2] *= 2.0
                block[4] = cols[11][idx]
            h = np.zeros(idx.size)
            for l, s in enumerate(ds.sets):
                grid, sec = O.flux_grid(model, s.time, block, exptime=s.exptime, nsamples=s.nsamples)
                h += 0.5 * np.sum((s.flux - grid) ** 2 / s.flux_err ** 2, axis=1)
                if l == 0 and model == O.MODEL_EB:
                    h[sec >= 1.5 * ds.sigma_ref] = np.inf
            x = -0.5 * np.log(2 * np.pi) - np.log(ds.sigma_ref) - h
            if d["lnprior"] is not None:
                x = x + d["lnprior"][idx]
            full = np.full(mask.size, -np.inf)
            full[idx] = x
            out.append((x, O.log_mean_exp(full, mask.size)))
    return out


def test_two_cadences_per_point_errors_against_the_oracle(device_mode, monkeypatch):
    r = _het_runs(monkeypatch)
    want = np.array([z for _, z in r["oracle"]])
    got = r["lnZ"][:N_SCEN]
    assert np.isfinite(want).sum() >= 4 and np.array_equal(np.isfinite(want), np.isfinite(got))
    assert np.all(np.isneginf(r["lnZ"][N_SCEN:]))                  # the dropped scenarios
    fin = np.isfinite(want)
    print("max |lnZ - oracle| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() < LNZ_TOL
    # the per-point path must not collapse to one error per dataset
    moved = np.abs(got[fin] - r["lnZ_mean"][:N_SCEN][fin])
    print("lnZ moves by %s with dataset A's errors replaced by their mean" % moved)
    assert moved.max() > 100 * LNZ_TOL


def test_chunked_grids_give_the_same_bits(device_mode, monkeypatch):
    from triceratops_amd import fused
    r = _het_runs(monkeypatch)
    n_min = min(x.size for x, _ in r["oracle"])
    assert n_min >= 3
    tg = _target()
    # (a chunk of n_min // 3 rows of the longer dataset: every branch takes at least 3 chunks)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        torch.manual_seed(SEED)
        tg.calc_probs_datasets(_two_cadences(), LC["P_orb"], n_samples=200, **KW2)
    assert tg.lnZ.tobytes() == r["lnZ"].tobytes()
    assert tg.probs.equals(r["best"])
    for p, q in zip(tg.posterior, r["posterior"]):
        assert (p is None) == (q is None)
        if p is not None:
            assert all(np.array_equal(p[k], q[k]) for k in q)


def test_posterior_rows_of_the_datasets_path(device_mode, monkeypatch):
    r = _het_runs(monkeypatch)
    post = r["posterior"]
    assert len(post) == r["lnZ"].size
    for j, (x, lnz) in enumerate(r["oracle"]):
        if not np.isfinite(lnz):
            assert post[j] is None
            continue
        p = post[j]
        assert p is not None and p["lnw"].shape == (200,) and p["row"].shape == (200,)
        assert np.all(np.diff(p["row"]) >= 0) and p["row"].min() >= 0 and p["row"].max() < x.size
        assert np.abs(p["lnw"] - x[p["row"]]).max() < 1e-9
    assert all(p is None for p in post[N_SCEN:])


def test_maps_and_histograms_are_refused(device_mode):
    from triceratops_amd import fused
    tg = _target()
    with fused.switches(WARP_HIST=True):
        with pytest.raises(NotImplementedError):
            tg.calc_probs_datasets(_two_cadences(), LC["P_orb"], **KW2)
