"""target.calc_probs_datasets with per-dataset linear baseline models marginalised (`baseline`, `baseline_sigma`; DESIGN.md
section 14), end to end on the fixtures of tests/test_gpu_datasets_offset.py: TOI-465.01, two cadences, N = 20 000,
set_sampling("device"), one seed for every pass.

Bars, none of them chosen from results (K = 2 terms on dataset 1: a flat offset and one slope column; lambda_min the
smallest eigenvalue of its scaled system):
  no keys / None: the same bits;
  a trend a + b u of rms 3 sigma added to dataset 1: |d lnZ| <= 1e-12 x chi^2/2 x (1 + 4 sqrt(2 / lambda_min)) + 1e-12,
        chi^2/2 the unprofiled one of the pass's best draw -- the kernel's bound on one draw's h
        (tests/test_gpu_chi2_baseline.py); the best draw is the same wherever the row's two smallest h differ by more;
  dataset_baselines / dataset_offsets: with trend - without = b / a to 1e-9 relative where the best draw is the same;
  an explicit ones column against offset_sigma = inf: the first bar;
  tight prior s = 1e-6 sigma_bar: |d lnZ| <= 1e-6, from |d h| <= |D^(1/2) s|^2 x 0.5 S2 (computed per draw in the test);
  against the CPU oracle: |d lnZ| <= 1e-9, the bar of tests/test_gpu_lnl_weighted.py."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets_offset import (COLS, KW, KW2, LC, SEED, SIGMA_BAR, TARGET_SHARE, _target, _two_cadences,  # noqa: F401
                                      device_mode)
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import Datasets, baseline_system, validate
from triceratops_amd.lightcurve import polynomial_baseline

pytestmark = pytest.mark.gpu

INF = float("inf")
_B = _two_cadences()[1]
U = polynomial_baseline(_B["time"], 1)[0]
SIGMA_1 = float(np.mean(np.broadcast_to(_B["flux_err"], U.shape)))          # dataset 1 has one error for all points
# a + b u of rms 3 sigma_1, half of the mean square in each term
A_TREND = 3.0 * SIGMA_1 / math.sqrt(2.0)
B_TREND = 3.0 * SIGMA_1 / math.sqrt(2.0 * float(np.mean(U * U)))
TREND = A_TREND + B_TREND * U
LAMBDA_MIN = baseline_system(validate([dict(_B, offset_sigma=INF, baseline=U)])[0]).lambda_min
AMPLIFY = 1.0 + 4.0 * math.sqrt(2.0 / LAMBDA_MIN)


def _inputs(trend=False, **keys):
    a, b = _two_cadences()
    if trend:
        b = dict(b, flux=b["flux"] + TREND)
    return [a, dict(b, **keys)]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it, h with nothing marginalised (the same rows evaluated again
    with offsets and baselines switched off), the draws' priors; and the number of trx_chi2_grid_baseline calls"""

    def __init__(self, monkeypatch):
        self.h, self.plain, self.lp, self.calls = [], [], [], 0
        real_h, real_z, real_b = fused._Scenario._datasets_halfchi2, _lib.lnz_from_halfchi2, _lib.chi2_grid_baseline
        spy = self

        def halfchi2(scen, model, flags, block):
            h = real_h(scen, model, flags, block)
            kept, scen.datasets = scen.datasets, [d._replace(term=None) for d in scen.datasets]
            try:
                spy.plain.append(real_h(scen, model, flags, block).cpu().numpy())
            finally:
                scen.datasets = kept
            return h

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            spy.lp.append(None if lp_d is None else lp_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def baseline(*a, **k):
            spy.calls += 1
            return real_b(*a, **k)

        monkeypatch.setattr(fused._Scenario, "_datasets_halfchi2", halfchi2)
        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "chi2_grid_baseline", baseline)


def _run(monkeypatch, datasets, spy=False, **kw):
    tg = _target()
    s = _Spy(monkeypatch) if spy else None
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(KW, **kw))
    monkeypatch.undo()
    out = {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "best": np.stack([tg.probs[c].values for c in COLS]),
           "offsets": tg.dataset_offsets, "baselines": tg.dataset_baselines, "target": tg, "sigma_ref": tg.sigma_ref}
    if spy:
        out.update(h=s.h, plain=s.plain, lp=s.lp, calls=s.calls)
        assert len(s.h) == len(s.plain) > 0
    return out


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["none_trend"] = _run(monkeypatch, _inputs(trend=True))
        _runs["slope"] = _run(monkeypatch, _inputs(offset_sigma=INF, baseline=U), spy=True)
        _runs["slope_trend"] = _run(monkeypatch, _inputs(trend=True, offset_sigma=INF, baseline=U), spy=True)
    return _runs


def _bars(run):
    """per scenario row: the bar on lnZ from the unprofiled chi^2/2 of the pass's best draw, and whether the row's two
    smallest h are further apart than it"""
    bars, sep = np.full(run["lnZ"].size, np.nan), np.zeros(run["lnZ"].size, dtype=bool)
    for j in np.flatnonzero(np.isfinite(run["lnZ"])):
        h = run["h"][j]
        bars[j] = 1e-12 * run["plain"][j][int(np.argmin(h))] * AMPLIFY + 1e-12
        two = np.partition(h, 1)[:2] if h.size > 1 else np.array([h[0], np.inf])
        sep[j] = two[1] - two[0] > bars[j]
    return bars, sep


def test_without_the_keys_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(baseline=None, baseline_sigma=None), spy=True)
    assert a["baselines"] is None and b["baselines"] is None and a["offsets"] is None and b["offsets"] is None
    assert np.isfinite(a["lnZ"]).sum() >= 10 and b["calls"] == 0
    assert a["lnZ"].tobytes() == b["lnZ"].tobytes() and a["prob"].tobytes() == b["prob"].tobytes()
    assert a["best"].tobytes() == b["best"].tobytes()


def test_an_offset_only_dataset_keeps_its_path(device_mode, monkeypatch):
    r = _run(monkeypatch, _inputs(offset_sigma=INF), spy=True, **{k: v for k, v in KW2.items() if k != "verbose"})
    assert r["calls"] == 0 and r["baselines"] is None and r["offsets"] is not None
    assert np.isfinite(r["lnZ"]).sum() >= 4


def test_flat_slope_and_offset_absorb_a_trend(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    u, s, plain, plain_s = r["slope"], r["slope_trend"], r["none"], r["none_trend"]
    assert u["calls"] > 0 and len(s["h"]) == len(u["h"]) == s["lnZ"].size
    fin = np.isfinite(u["lnZ"])
    assert np.array_equal(fin, np.isfinite(s["lnZ"])) and fin.sum() >= 10
    bars, sep = _bars(s)
    d = np.abs(u["lnZ"][fin] - s["lnZ"][fin])
    same = np.array([np.array_equal(u["best"][:, j], s["best"][:, j]) for j in range(fin.size)])
    print("flat offset + slope, trend of rms 3 sigma (lambda_min %.3g): max |d lnZ| / bar %.3g over %d finite rows; two "
          "smallest h further apart than the bar in %d rows, the same best draw in %d"
          % (LAMBDA_MIN, (d / bars[fin]).max(), fin.sum(), sep.sum(), (same & fin).sum()))
    assert (d <= bars[fin]).all()
    assert sep.sum() >= 0.9 * fin.sum()
    assert same[sep].all()
    # without the keys the same trend moves the evidence of the best-fitting row by more than 1: the point of the feature
    top = int(np.nanargmax(np.where(np.isfinite(plain["lnZ"]), plain["lnZ"], -np.inf)))
    moved = abs(plain["lnZ"][top] - plain_s["lnZ"][top])
    print("no baseline keys: lnZ of row %d moves by %.4g under the same trend" % (top, moved))
    assert moved > 1.0


def test_coefficients_recover_the_trend(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    u, s = r["slope"], r["slope_trend"]
    n_scen = u["lnZ"].size
    assert r["none"]["baselines"] is None
    assert len(u["baselines"]) == len(s["baselines"]) == n_scen and u["offsets"].shape == (n_scen, 2)
    fin = np.isfinite(u["lnZ"])
    for run in (u, s):
        assert all(row[0] is None and row[1].shape == (1,) for row in run["baselines"])
        slope = np.array([row[1][0] for row in run["baselines"]])
        assert np.array_equal(np.isfinite(slope), fin) and np.array_equal(np.isfinite(run["offsets"][:, 1]), fin)
        assert np.isnan(run["offsets"][:, 0]).all()
    same = fin & np.array([np.array_equal(u["best"][:, j], s["best"][:, j]) for j in range(n_scen)])
    assert same.sum() >= 0.9 * fin.sum()
    d_b = np.array([s["baselines"][j][1][0] - u["baselines"][j][1][0] for j in np.flatnonzero(same)])
    d_a = s["offsets"][same, 1] - u["offsets"][same, 1]
    rel_b, rel_a = np.abs(d_b - B_TREND) / B_TREND, np.abs(d_a - A_TREND) / A_TREND
    print("dataset_baselines / dataset_offsets: with trend - without against b, a: max relative error %.3g, %.3g over %d rows"
          % (rel_b.max(), rel_a.max(), same.sum()))
    assert rel_b.max() <= 1e-9 and rel_a.max() <= 1e-9


def test_an_explicit_ones_column_is_offset_sigma(device_mode, monkeypatch):
    r = _passes(monkeypatch)["slope_trend"]
    e = _run(monkeypatch, _inputs(trend=True, baseline=np.stack([np.ones_like(U), U])), spy=True)
    fin = np.isfinite(r["lnZ"])
    assert np.array_equal(fin, np.isfinite(e["lnZ"])) and e["offsets"] is None
    bars, _ = _bars(r)
    d = np.abs(r["lnZ"][fin] - e["lnZ"][fin])
    print("ones column against offset_sigma = inf: max |d lnZ| / bar %.3g" % (d / bars[fin]).max())
    assert (d <= bars[fin]).all()
    # ... and its coefficients are the offset and the slope
    same = fin & np.array([np.array_equal(r["best"][:, j], e["best"][:, j]) for j in range(fin.size)])
    assert same.sum() >= 0.9 * fin.sum()
    for j in np.flatnonzero(same):
        got = e["baselines"][j][1]
        want = np.array([r["offsets"][j, 1], r["baselines"][j][1][0]])
        assert got.shape == (2,) and (np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-12 * SIGMA_1).all()


def test_tight_prior_is_no_baseline(device_mode, monkeypatch):
    plain = _passes(monkeypatch)["none"]
    s_in = 1e-6 * SIGMA_BAR
    t = _run(monkeypatch, _inputs(baseline=U, baseline_sigma=s_in), spy=True)
    fin = np.isfinite(plain["lnZ"])
    assert np.array_equal(fin, np.isfinite(t["lnZ"])) and len(t["h"]) == t["lnZ"].size
    # b^T A^-1 b <= sum_k s_k^2 b_k^2 (A >= diag(1 / s^2)) and b_k^2 <= D_k S2 (Cauchy-Schwarz): |d h| <= |D^(1/2) s|^2 x
    # 0.5 S2 <= s^2 D x (the draw's h without baselines); s^2 D is the same in every star's normalisation.  Only draws
    # within 80 of the row's best log-weight enter lnZ.
    d1 = validate(_inputs(baseline=U, baseline_sigma=s_in))[1]
    s2D = float(d1.baseline_sigma[0] ** 2 * np.sum(U * U / d1.flux_err ** 2))
    worst_bound = worst = 0.0
    for j in np.flatnonzero(fin):
        h, p, lp = t["h"][j], t["plain"][j], t["lp"][j]
        x = -p if lp is None else lp - p
        live = np.isfinite(x) & (x >= np.nanmax(np.where(np.isfinite(x), x, -np.inf)) - 80.0)
        assert live.any()
        bound = s2D * p[live] + 1e-12 * p[live] * 5.0          # (+ the reductions' rounding: K = 1, lambda_min >= 1)
        assert (np.abs(h[live] - p[live]) <= bound).all()
        worst_bound, worst = max(worst_bound, float(bound.max())), max(worst, float(np.abs(h[live] - p[live]).max()))
    d = np.abs(t["lnZ"][fin] - plain["lnZ"][fin]).max()
    print("tight prior: s^2 D = %.3g, computed bound on |d h| of the draws with weight %.3g, measured %.3g, max |d lnZ| %.3g"
          % (s2D, worst_bound, worst, d))
    assert worst_bound <= 1e-6 and d <= 1e-6
    assert np.array_equal(t["best"], plain["best"])


def test_fused_evaluation_is_refused_and_posteriors_follow_h(device_mode, monkeypatch):
    tg = _target()
    with pytest.raises(NotImplementedError):
        tg.calc_probs_datasets(_inputs(baseline=U), LC["P_orb"], evaluation="fused", **KW2)
    p = _run(monkeypatch, _inputs(trend=True, offset_sigma=INF, baseline=U), spy=True, n_samples=50,
             **{k: v for k, v in KW2.items() if k != "verbose"})
    post = p["target"].posterior
    lnsig = float(np.log(p["sigma_ref"]))
    checked = 0
    assert len(p["h"]) == 6                                       # TP, EB, EBx2P, PTP, PEB, PEBx2P: rows 0 .. 5
    for j, lnz in enumerate(p["lnZ"][:6]):
        if not np.isfinite(lnz):
            assert post[j] is None
            continue
        q = post[j]
        assert q is not None and q["lnw"].shape == (50,) and q["row"].min() >= 0 and q["row"].max() < p["h"][j].size
        x = -0.5 * np.log(2 * np.pi) - lnsig - p["h"][j][q["row"]]
        if p["lp"][j] is not None:
            x = x + p["lp"][j][q["row"]]
        assert np.abs(q["lnw"] - x).max() <= 1e-12 * np.abs(x).max() + 1e-12
        # the rows were weighted with the marginalised h, not the plain one
        assert np.abs(p["plain"][j][q["row"]] - p["h"][j][q["row"]]).max() > 0.0
        checked += 1
    assert checked >= 4


def test_baseline_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences: a Gaussian offset and a flat slope on dataset 0, a flat offset
    and two columns (one with a prior) on dataset 1, which carries the trend: the model curves from the oracle, the sums
    and the evidence in numpy (_numerics.baseline_halfchi2)."""
    data = _inputs(trend=True, offset_sigma=INF, baseline=np.stack([U, U * U]), baseline_sigma=[INF, 2.0 * SIGMA_BAR])
    u0 = polynomial_baseline(data[0]["time"], 1)
    data[0] = dict(data[0], offset_sigma=2.0 * SIGMA_BAR, baseline=u0)
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    ds = Datasets(validate(data)).renorm(float(TARGET_SHARE))
    want = []
    for d in dump:
        cols = d["cols"].cpu().numpy()
        mask, mask2 = d["mask"].cpu().numpy(), None if d["mask_twin"] is None else d["mask_twin"].cpu().numpy()
        lnprior = None if d["lnprior"] is None else d["lnprior"].cpu().numpy()
        planet = mask2 is None
        branches = ((O.MODEL_TP, mask, False),) if planet else ((O.MODEL_EB, mask, False), (O.MODEL_EB_TWIN, mask2, True))
        for model, m, twin in branches:
            idx = np.flatnonzero(m)
            block = cols[:10 if planet else 11][:, idx].copy()
            if twin:
                block[2] *= 2.0
                block[4] = cols[11][idx]
            h = np.zeros(idx.size)
            for l, s in enumerate(ds.sets):
                grid, sec = O.flux_grid(model, s.time, block, exptime=s.exptime, nsamples=s.nsamples)
                basis = np.vstack([np.ones((1, s.time.size)), s.baseline])
                h += _numerics.baseline_halfchi2(s.flux - grid, 1.0 / s.flux_err ** 2, basis,
                                                 np.concatenate([[s.offset_sigma], s.baseline_sigma]))
                if l == 0 and model == O.MODEL_EB:
                    h[sec >= 1.5 * ds.sigma_ref] = np.inf
            x = -0.5 * np.log(2 * np.pi) - np.log(ds.sigma_ref) - h
            if lnprior is not None:
                x = x + lnprior[idx]
            full = np.full(m.size, -np.inf)
            full[idx] = x
            want.append(O.log_mean_exp(full, m.size))
    want = np.array(want)
    got = tg.lnZ[:3]
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and np.isfinite(want).sum() >= 2
    fin = np.isfinite(want)
    print("baseline datasets against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
    assert all(row[0].shape == (1,) and row[1].shape == (2,) for row in tg.dataset_baselines)
    assert np.isfinite(tg.dataset_offsets[:3][fin]).all()
