"""target.calc_probs_datasets with baseline columns marginalised next to a grid of white-noise candidates (`white_baseline` /
`white_baseline_sigma` next to `white_grid`), end to end on the fixtures of tests/test_gpu_datasets.py:
TOI-465.01, two cadences, N = 20 000, set_sampling("device"), one seed for every pass.

Bars, none of them chosen from results:
  no keys / keys = None: the same bits, and _lib.chi2_grid_white_baseline is never called;
  one candidate (1, 0, 1) with the columns (ones, u) and the sigmas (inf, s) against the same dataset with offset_sigma = inf,
        baseline = u, baseline_sigma = s: the same statement (lnc = 0, the same dropped determinant), two kernels:
        |d lnZ| <= 1e-9, the datasets path's oracle bar;
  linearity: exp(-T) = sum_j c_j exp(-h_j) per draw and the masks depend on sigma_bar alone, so from one seed
        lnZ{A, B} = logsumexp(lnc_A + lnZ_A, lnc_B + lnZ_B) per scenario row, lnc from white_baseline_system of the input;
        |d| <= 8 eps (1 + the largest finite h among the row's draws) + 1e-12, tests/test_gpu_datasets_white_grid.py's;
  against the CPU oracle's model grid reduced with _numerics.white_baseline_halfchi2: |d lnZ| <= 1e-9;
  .dataset_white_baselines: "mean" = sum_j weight_j coef_j with `.dataset_white_noise`'s weights to 16 eps max|coef|; on data
        with 0.003 u added and errors understated twofold the candidate k = 2 of [1, 2, 4] carries the largest weight at
        every scenario's best draw and mean[1] lies within three posterior sigmas (sqrt of (A_2^-1)_11, k = 2) of 0.003;
  three chunks of the grid, calc_probs_datasets_refined(n_adapt = 0) and a one-node t0_grid (0, 1): the same bits.
"""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from test_gpu_datasets_baseline import U
from test_gpu_datasets_red_noise import COLS, SIGMA_1, _same_bits
from test_gpu_datasets_white_grid import NOISE, _noisy_inputs
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import (Datasets, validate, white_baseline_system, white_baselines, white_grids,
                                      white_mix_system)
from triceratops_amd.lightcurve import white_noise_grid

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
INF = float("inf")
A = (1.5, 0.0)
B = (1.0, 2.0 * SIGMA_1)
AB = [A + (0.3,), B + (0.7,)]
BASIS = np.stack([np.ones(U.size), U])
S_SLOPE = 5.0 * SIGMA_1
LIN = dict(white_baseline=BASIS, white_baseline_sigma=[INF, S_SLOPE])


def _inputs(**keys):
    a, b = _two_cadences()
    return [a, dict(b, **keys)]


def _system(data, share=1.0):
    sets = validate(data)
    ds = Datasets(sets, white_grids=white_grids(data, sets), white_baselines=white_baselines(data, sets)).renorm(share)
    return white_baseline_system(ds.sets[1], ds.white_grids[1], *ds.white_baselines[1])


def _run(monkeypatch, datasets, refined=None, **kw):
    """one pass; per evidence h as the evidence saw it, the calls of the two white reductions, the best draws' rows"""
    tg = _target()
    seen = {"h": [], "lin": 0, "mix": 0, "best": []}
    real_z, real_lin, real_mix, real_half = (_lib.lnz_from_halfchi2, _lib.chi2_grid_white_baseline,
                                             _lib.chi2_grid_white_mix, fused._Dataset.halfchi2)

    def lnz(h_d, lp_d, n_total, lnsigma):
        seen["h"].append(h_d.cpu().numpy())
        return real_z(h_d, lp_d, n_total, lnsigma)

    def lin(*a, **k):
        seen["lin"] += 1
        return real_lin(*a, **k)

    def mix(*a, **k):
        seen["mix"] += 1
        return real_mix(*a, **k)

    def halfchi2(d, grid, *a, **k):
        if k.get("cand_out") is not None:
            seen["best"].append((len(seen["h"]) - 1, d, grid.clone()))
        return real_half(d, grid, *a, **k)

    monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
    monkeypatch.setattr(_lib, "chi2_grid_white_baseline", lin)
    monkeypatch.setattr(_lib, "chi2_grid_white_mix", mix)
    monkeypatch.setattr(fused._Dataset, "halfchi2", halfchi2)
    torch.manual_seed(SEED)
    _lib.reset_stats()
    if refined is not None:
        tg.calc_probs_datasets_refined(datasets, LC["P_orb"], n_adapt=refined, **dict(KW, **kw))
    else:
        tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(KW, **kw))
    rows = _lib.STATS["rows"]
    monkeypatch.undo()
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows,
            "best": np.stack([tg.probs[c].values for c in COLS]), "target": tg, "h": seen["h"], "lin_calls": seen["lin"],
            "mix_calls": seen["mix"], "best_rows": seen["best"]}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["mix"] = _run(monkeypatch, _inputs(white_grid=AB))
        _runs["A"] = _run(monkeypatch, _inputs(white_grid=[A + (1.0,)], **LIN))
        _runs["B"] = _run(monkeypatch, _inputs(white_grid=[B + (5.0,)], **LIN))
        _runs["AB"] = _run(monkeypatch, _inputs(white_grid=AB, **LIN))
    return _runs


def test_without_the_keys_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["mix"]
    b = _run(monkeypatch, _inputs(white_grid=AB, white_baseline=None, white_baseline_sigma=None))
    assert np.isfinite(a["lnZ"]).sum() >= 10 and _same_bits(a, b)
    assert a["lin_calls"] == b["lin_calls"] == 0 and a["mix_calls"] == b["mix_calls"] > 0
    assert a["target"].dataset_white_baselines is None and b["target"].dataset_white_baselines is None
    assert len(a["h"]) == len(b["h"]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["h"], b["h"]))
    m = _passes(monkeypatch)["AB"]
    assert m["lin_calls"] > 0 and m["mix_calls"] == 0
    fin = np.isfinite(m["lnZ"])
    assert np.abs(m["lnZ"][fin] - a["lnZ"][fin]).max() > 1e-3            # (a marginalised trend changes the evidence)


def test_the_unit_candidate_is_the_plain_baseline(device_mode, monkeypatch):
    g = _run(monkeypatch, _inputs(white_grid=[(1.0, 0.0, 1.0)], **LIN))
    p = _run(monkeypatch, _inputs(offset_sigma=INF, baseline=U, baseline_sigma=S_SLOPE))
    assert g["lin_calls"] > 0 and p["lin_calls"] == 0
    fin = np.isfinite(p["lnZ"])
    assert np.array_equal(fin, np.isfinite(g["lnZ"])) and fin.sum() >= 10 and g["rows"] == p["rows"]
    d = np.abs(g["lnZ"][fin] - p["lnZ"][fin]).max()
    print("unit candidate with (ones, u) against offset_sigma + baseline: max |d lnZ| %.3g" % d)
    assert d <= 1e-9
    # ... and the coefficients are that path's offset and slope
    tg, tp = g["target"], p["target"]
    for j in np.flatnonzero(fin):
        row = tg.dataset_white_baselines[j]
        assert row[0] is None and row[1]["coef"].shape == (1, 2) and row[1]["mean"].shape == (2,)
        assert np.array_equal(row[1]["coef"][0], row[1]["mean"])
        if np.array_equal(g["best"][:, j], p["best"][:, j]):             # (the same best draw)
            want = np.array([tp.dataset_offsets[j][1], tp.dataset_baselines[j][1][0]])
            assert np.abs(row[1]["mean"] - want).max() <= 1e-9 * (1.0 + np.abs(want).max())
    for j in np.flatnonzero(~np.isfinite(g["lnZ"])):
        assert np.isnan(tg.dataset_white_baselines[j][1]["coef"]).all()


def test_the_evidence_is_linear_in_the_candidates(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    a, b, m = r["A"], r["B"], r["AB"]
    lnc = _system(_inputs(white_grid=AB, **LIN)).lnc
    assert lnc.shape == (2,) and np.isfinite(lnc).all()
    # the determinants of the candidates' systems are part of the weights
    lnc_mix = white_mix_system(validate(_inputs())[1], np.array(AB))[1]
    assert np.abs(lnc - lnc_mix).max() > 1e-3
    assert a["rows"] == b["rows"] == m["rows"] == r["mix"]["rows"] > 0, "masked counts differ"
    assert len(a["h"]) == len(b["h"]) == len(m["h"]) == m["lnZ"].size
    fin = np.isfinite(m["lnZ"])
    assert np.array_equal(fin, np.isfinite(a["lnZ"])) and np.array_equal(fin, np.isfinite(b["lnZ"])) and fin.sum() >= 10
    worst = 0.0
    for j in np.flatnonzero(fin):
        top = max(float(h[np.isfinite(h)].max()) for h in (a["h"][j], b["h"][j], m["h"][j]))
        bar = 8 * EPS * (1.0 + top) + 1e-12
        x, y = lnc[0] + a["lnZ"][j], lnc[1] + b["lnZ"][j]
        want = max(x, y) + math.log(math.fsum((math.exp(x - max(x, y)), math.exp(y - max(x, y)))))
        d = abs(m["lnZ"][j] - want)
        worst = max(worst, d / bar)
        print("row %d: lnZ_A %.6f lnZ_B %.6f lnZ_AB %.6f, |d| %.3g, bar %.3g (largest finite h %.4g)"
              % (j, a["lnZ"][j], b["lnZ"][j], m["lnZ"][j], d, bar, top))
        assert d <= bar, (j, d, bar)
    print("linearity: lnc %s, max |d lnZ| / bar %.3g over %d finite rows" % (lnc, worst, fin.sum()))
    assert np.abs(a["lnZ"][fin] - b["lnZ"][fin]).max() > 1e-3


def _check_report(m, data):
    """.dataset_white_baselines and .dataset_white_noise of a pass: shapes, NaN without an evidence, and the mean under the
    candidates' weights; returns ([finite][J] weights, [finite][K] means)"""
    tg = m["target"]
    J = white_grids(data, validate(data))[1].shape[0]
    table, noise = tg.dataset_white_baselines, tg.dataset_white_noise
    assert isinstance(table, list) and len(table) == m["lnZ"].size == len(noise)
    ws, means = [], []
    for row, nrow, lnz in zip(table, noise, m["lnZ"]):
        assert len(row) == 2 and row[0] is None and sorted(row[1]) == ["coef", "mean"]
        coef, mean, w = row[1]["coef"], row[1]["mean"], nrow[1]["weight"]
        assert coef.shape == (J, 2) and mean.shape == (2,) and w.shape == (J,)
        if not np.isfinite(lnz):
            assert np.isnan(coef).all() and np.isnan(mean).all()
            continue
        assert np.isfinite(coef).all()
        assert (np.abs(mean - w @ coef) <= 16 * EPS * np.abs(coef).max()).all()
        ws.append(w)
        means.append(mean)
    assert len(ws) == np.isfinite(m["lnZ"]).sum() >= 10
    return np.array(ws), np.array(means)


def test_coefficients_at_the_best_draw(device_mode, monkeypatch):
    m = _passes(monkeypatch)["AB"]
    _check_report(m, _inputs(white_grid=AB, **LIN))
    # the coefficients are those of the statement on the best draw's model row, in the units of the given flux
    tg = m["target"]
    best = {k: (d, grid) for k, d, grid in m["best_rows"]}
    assert len(best) == len(m["best_rows"]), "one re-evaluation per evidence"
    checked = 0
    for j, (d, grid) in best.items():
        if not np.isfinite(m["lnZ"][j]):
            continue
        y = (d.flux - grid[0]).cpu().numpy()
        system = _system(_inputs(white_grid=AB, **LIN))._replace(w=d.term.w.cpu().numpy(), minv=d.term.minv, lnc=d.term.lnc)
        _, _, coef = _numerics.white_baseline_halfchi2(y, system, return_candidates=True, return_coef=True)
        got = tg.dataset_white_baselines[j][1]["coef"]
        share = got[0, 0] / coef[0, 0]
        assert 0.0 < share <= 1.0 + 1e-12
        assert np.abs(got - coef * share).max() <= 1e-9 * np.abs(got).max()
        checked += 1
    assert checked >= 10
    assert _passes(monkeypatch)["mix"]["target"].dataset_white_baselines is None


def test_understated_errors_and_a_trend(device_mode, monkeypatch):
    keys = dict(white_grid=white_noise_grid([1.0, 2.0, 4.0]), white_baseline=BASIS, white_baseline_sigma=[INF, INF])
    data = _noisy_inputs(**keys)
    data[1] = dict(data[1], flux=data[1]["flux"] + 0.003 * U)
    m = _run(monkeypatch, data)
    w, means = _check_report(m, data)
    print("posterior weights of k = 1, 2, 4 at the best draws:\n%s\nmean coefficients:\n%s" % (w, means))
    assert (np.argmax(w, axis=1) == 1).all()
    e = NOISE * LC["sigma"]
    Ainv = np.linalg.inv((BASIS / (2.0 * e) ** 2) @ BASIS.T)
    sd = math.sqrt(Ainv[1, 1])
    print("slope: posterior sigma under k = 2 %.3g, largest |mean[1] - 0.003| %.3g" % (sd, np.abs(means[:, 1] - 0.003).max()))
    assert (np.abs(means[:, 1] - 0.003) <= 3.0 * sd).all()


def test_chunks_refined_passes_a_single_node_and_the_fused_refusal(device_mode, monkeypatch):
    data = _inputs(white_grid=AB, **LIN)
    whole = _passes(monkeypatch)["AB"]
    assert whole["lin_calls"] > 0 and np.isfinite(whole["lnZ"]).sum() >= 10
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["lin_calls"] - len(chunked["best_rows"]) >= 3 * sum(h.size >= 3 for h in whole["h"])
    assert _same_bits(whole, chunked)
    refined = _run(monkeypatch, data, refined=0)
    node = _run(monkeypatch, _inputs(white_grid=AB, t0_grid=[(0.0, 1.0)], **LIN))
    for other in (chunked, refined, node):
        assert _same_bits(whole, other)
        for x, y in zip(whole["target"].dataset_white_baselines, other["target"].dataset_white_baselines):
            assert np.array_equal(x[1]["coef"], y[1]["coef"], equal_nan=True)
            assert np.array_equal(x[1]["mean"], y[1]["mean"], equal_nan=True)
    assert node["target"].dataset_t0 is not None and whole["target"].dataset_t0 is None
    tg = _target()
    with pytest.raises(NotImplementedError, match="white"):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, dataset 1 with errors understated twofold, a trend of 0.003 u,
    six candidates and the columns (ones, u) with a flat constant and a finite slope prior: the model curves from the
    oracle, the sums, the quadratic forms, the soft minimum and the evidence in numpy."""
    keys = dict(white_grid=white_noise_grid([1.0, 2.0, 3.0], [0.0, NOISE * LC["sigma"]], [[1.0, 2.0], [3.0, 2.0], [1.0, 1.0]]),
                white_baseline=BASIS, white_baseline_sigma=[INF, 0.01])
    data = _noisy_inputs(**keys)
    data[1] = dict(data[1], flux=data[1]["flux"] + 0.003 * U)
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    sets = validate(data)
    ds = Datasets(sets, white_grids=white_grids(data, sets),
                  white_baselines=white_baselines(data, sets)).renorm(float(TARGET_SHARE))
    assert ds.white_baselines[0] is None and ds.white_baselines[1][1][1] == 0.01 / float(TARGET_SHARE)
    system = white_baseline_system(ds.sets[1], ds.white_grids[1], *ds.white_baselines[1])
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
                r = s.flux - grid
                if l == 0:
                    h += 0.5 * np.sum(r * r / s.flux_err ** 2, axis=1)
                else:
                    h += _numerics.white_baseline_halfchi2(r, system)
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
    print("white_baseline dataset against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
