"""target.calc_probs_datasets with a transit-time shift grid per dataset (`t0_grid`), end to end on the
fixtures of tests/test_gpu_datasets.py: TOI-465.01, two cadences, N = 20 000, set_sampling("device"), one seed for every pass.

Bars, none of them chosen from results:
  no key / key = None: the same bits, and _lib.softmin_rows is never called;
  a grid of one node (d, 1) on dataset 1 against dataset 1 with time + d and no key, d = 4 cadences of that dataset: the same
        lnZ, prob and best-draw bits (ln 1 = 0, and the kernel's T is then h_1 bit for bit) -- plain, and with offset_sigma,
        a baseline column and red_sigma / red_timescale on that dataset;
  linearity: exp(-T) = sum_j pi_j exp(-h_j) per draw and the masks depend on sigma_bar alone, so from one seed
        lnZ{A, B} = logsumexp(ln 0.3 + lnZ_A, ln 0.7 + lnZ_B) per scenario row;
        |d| <= 8 eps (1 + the largest finite h among the row's draws) + 1e-12, the bar of tests/test_gpu_datasets_red_grid.py:
        the h_j are the same bits in the three passes, so only the kernel's exp / log and the three log-mean-exp folds differ;
  a five-node grid of lightcurve.t0_shift_grid on dataset 1 (and two nodes on dataset 0, where the secondary-eclipse rule
        rides every node), against the CPU oracle's model grids on the shifted stamps reduced with
        _numerics.t0_mix_halfchi2: |d lnZ| <= 1e-9, the bar of the other oracle checks of the datasets path;
  three chunks of the grid, and calc_probs_datasets_refined(n_adapt = 0): the same bits;
  .dataset_t0: weights >= 0, their sum 1 to 8 eps J, and equal to softmax_j(ln pi_j - h_j) with the h_j of
        _lib.chi2_grid_weighted on the best draw's J model rows, to 16 eps (1 + max_j h_j);
  recovery: dataset 1 with time - d; the grid {-d, 0, +d} at equal weights against the single node {+d}: by linearity every
        finite row has lnZ_grid >= lnZ_single - ln 3, less the bar of the linearity test.  The weight of node +d at the best
        draw of the most probable scenario is printed and not gated: no d was confirmed with the CPU oracle beforehand.
"""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from test_gpu_datasets_red_noise import CADENCE_1, COLS, SIGMA_1, _same_bits
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import Datasets, t0_grids, validate
from triceratops_amd.lightcurve import t0_shift_grid

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DELTA = 4.0 * CADENCE_1
A = DELTA
B = -1.5 * CADENCE_1
AB = [(A, 0.3), (B, 0.7)]
CADENCE_0 = float(np.median(np.diff(_two_cadences()[0]["time"])))


def _inputs(shift=0.0, **keys):
    a, b = _two_cadences()
    return [a, dict(b, time=b["time"] + shift, **keys)]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it; the calls of _lib.softmin_rows; and per evidence that had a
    draw, the best draw's re-evaluations (one model row, no `out`): the evidence's index, the dataset's device record, the
    row"""

    def __init__(self, monkeypatch):
        self.h, self.softmin_calls, self.best = [], 0, []
        real_z, real_soft, real_half = _lib.lnz_from_halfchi2, _lib.softmin_rows, fused._Dataset.halfchi2
        spy = self

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def soft(*a, **k):
            spy.softmin_calls += 1
            return real_soft(*a, **k)

        def halfchi2(d, grid, *a, **k):
            if k.get("out") is None:
                spy.best.append((len(spy.h) - 1, d, grid.clone()))
            return real_half(d, grid, *a, **k)

        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "softmin_rows", soft)
        monkeypatch.setattr(fused._Dataset, "halfchi2", halfchi2)


def _run(monkeypatch, datasets, refined=False, **kw):
    tg = _target()
    s = _Spy(monkeypatch)
    torch.manual_seed(SEED)
    _lib.reset_stats()
    if refined:
        tg.calc_probs_datasets_refined(datasets, LC["P_orb"], n_adapt=0, **dict(KW, **kw))
    else:
        tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(KW, **kw))
    rows, cells, launches = _lib.STATS["rows"], _lib.STATS["cells"], _lib.STATS["launches"]
    monkeypatch.undo()
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows, "cells": cells, "launches": launches,
            "best": np.stack([tg.probs[c].values for c in COLS]), "target": tg, "h": s.h, "softmin_calls": s.softmin_calls,
            "best_rows": s.best}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["A"] = _run(monkeypatch, _inputs(t0_grid=[(A, 1.0)]))
        _runs["B"] = _run(monkeypatch, _inputs(t0_grid=[(B, 5.0)]))
        _runs["AB"] = _run(monkeypatch, _inputs(t0_grid=AB))
    return _runs


def test_without_the_key_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(t0_grid=None))
    assert np.isfinite(a["lnZ"]).sum() >= 10 and _same_bits(a, b)
    assert a["softmin_calls"] == b["softmin_calls"] == 0
    assert a["cells"] == b["cells"] and a["launches"] == b["launches"]
    assert a["target"].dataset_t0 is None and b["target"].dataset_t0 is None
    m = _passes(monkeypatch)["AB"]
    assert m["softmin_calls"] > 0
    # J x T cells and J launches per chunk for the dataset with the key: 50 + 21 points, two nodes on the 21
    assert a["rows"] == m["rows"] and a["cells"] == a["rows"] * 71 and m["cells"] == m["rows"] * (50 + 2 * 21)
    assert 2 * m["launches"] == 3 * a["launches"]


EXTRAS = {"plain": {}, "offset": {"offset_sigma": 2.0 * SIGMA_1},
          "baseline": {"baseline": np.linspace(-1.0, 1.0, 21), "baseline_sigma": 3.0 * SIGMA_1},
          "red": {"red_sigma": 2.0 * SIGMA_1, "red_timescale": 20.0 * CADENCE_1}}


@pytest.mark.parametrize("extra", sorted(EXTRAS))
def test_one_node_is_the_shifted_stamps_in_bits(device_mode, monkeypatch, extra):
    keys = EXTRAS[extra]
    g = _passes(monkeypatch)["A"] if extra == "plain" else _run(monkeypatch, _inputs(t0_grid=[(DELTA, 1.0)], **keys))
    p = _run(monkeypatch, _inputs(shift=DELTA, **keys))
    assert g["softmin_calls"] > 0 and p["softmin_calls"] == 0
    assert np.isfinite(g["lnZ"]).sum() >= 10 and _same_bits(g, p)
    assert len(g["h"]) == len(p["h"]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(g["h"], p["h"]))
    assert g["cells"] == p["cells"] and g["launches"] == p["launches"]
    # the shift changes the evidence: the point of the feature
    fin = np.isfinite(g["lnZ"])
    if extra == "plain":
        assert np.abs(g["lnZ"][fin] - _passes(monkeypatch)["none"]["lnZ"][fin]).max() > 1e-3
    # what the best draw reports is what the shifted stamps report
    tg, tp = g["target"], p["target"]
    for name in ("dataset_offsets", "dataset_baselines"):
        x, y = getattr(tg, name), getattr(tp, name)
        assert (x is None) == (y is None)
        if name == "dataset_offsets" and x is not None:
            assert np.array_equal(x, y, equal_nan=True)
        elif x is not None:
            assert all(np.array_equal(u[1], v[1], equal_nan=True) for u, v in zip(x, y))
    # one node: its weight is 1 wherever there is a best draw, and the mean is the shift
    assert tp.dataset_t0 is None
    for row, lnz in zip(tg.dataset_t0, g["lnZ"]):
        assert row[0] is None and row[1]["shift"].tolist() == [DELTA] and row[1]["weight"].shape == (1,)
        if np.isfinite(lnz):
            assert row[1]["weight"][0] == 1.0 and row[1]["mean"] == DELTA
        else:
            assert np.isnan(row[1]["weight"][0]) and np.isnan(row[1]["mean"])


def _bar(*hs):
    top = max(float(h[np.isfinite(h)].max()) for h in hs)
    return 8 * EPS * (1.0 + top) + 1e-12, top


def test_the_evidence_is_linear_in_the_nodes(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    a, b, m = r["A"], r["B"], r["AB"]
    data = _inputs(t0_grid=AB)
    lnpi = np.log(t0_grids(data, validate(data))[1][:, 1])
    assert lnpi.shape == (2,) and np.allclose(np.exp(lnpi), [0.3, 0.7], rtol=4 * EPS)
    assert a["rows"] == b["rows"] == m["rows"] == r["none"]["rows"] > 0, "masked counts differ"
    assert len(a["h"]) == len(b["h"]) == len(m["h"]) == m["lnZ"].size
    fin = np.isfinite(m["lnZ"])
    assert np.array_equal(fin, np.isfinite(a["lnZ"])) and np.array_equal(fin, np.isfinite(b["lnZ"])) and fin.sum() >= 10
    worst = 0.0
    for j in np.flatnonzero(fin):
        assert a["h"][j].shape == b["h"][j].shape == m["h"][j].shape
        bar, top = _bar(a["h"][j], b["h"][j], m["h"][j])
        x, y = lnpi[0] + a["lnZ"][j], lnpi[1] + b["lnZ"][j]
        want = max(x, y) + math.log(math.fsum((math.exp(x - max(x, y)), math.exp(y - max(x, y)))))
        d = abs(m["lnZ"][j] - want)
        worst = max(worst, d / bar)
        print("row %d: lnZ_A %.6f lnZ_B %.6f lnZ_AB %.6f, |d| %.3g, bar %.3g (largest finite h %.4g)"
              % (j, a["lnZ"][j], b["lnZ"][j], m["lnZ"][j], d, bar, top))
        assert d <= bar, (j, d, bar)
        # per draw as well: T = -ln(0.3 exp(-h_A) + 0.7 exp(-h_B)), to the kernel's own rounding
        ha, hb, t = a["h"][j], b["h"][j], m["h"][j]
        ok = np.isfinite(ha) & np.isfinite(hb)
        assert np.array_equal(ok, np.isfinite(t))
        ref = -np.logaddexp(lnpi[0] - ha[ok], lnpi[1] - hb[ok])
        assert (np.abs(t[ok] - np.maximum(ref, 0.0)) <= 8 * EPS * (1.0 + np.abs(t[ok]) + np.abs(lnpi).max()) + 1e-12).all()
    print("linearity: ln pi %s, max |d lnZ| / bar %.3g over %d finite rows" % (lnpi, worst, fin.sum()))
    # the two nodes give different evidences
    assert np.abs(a["lnZ"][fin] - b["lnZ"][fin]).max() > 1e-3


def test_node_weights_at_the_best_draw(device_mode, monkeypatch):
    m = _passes(monkeypatch)["AB"]
    tg = m["target"]
    table = tg.dataset_t0
    data = _inputs(t0_grid=AB)
    given = t0_grids(data, validate(data))[1]
    assert isinstance(table, list) and len(table) == m["lnZ"].size
    best = {}
    for k, d, grid in m["best_rows"]:
        best.setdefault(k, []).append((d, grid))
    checked, worst = 0, 0.0
    for j, (row, lnz) in enumerate(zip(table, m["lnZ"])):
        assert len(row) == 2 and row[0] is None
        assert np.array_equal(row[1]["shift"], given[:, 0])
        w = row[1]["weight"]
        assert w.shape == (2,) and w.dtype == np.float64
        if not np.isfinite(lnz):
            assert np.isnan(w).all() and np.isnan(row[1]["mean"])
            continue
        assert (w >= 0).all() and abs(math.fsum(w) - 1.0) <= 8 * EPS * 2
        assert abs(row[1]["mean"] - float(np.sum(w * given[:, 0]))) <= 4 * EPS * np.abs(given[:, 0]).max()
        assert len(best[j]) == 2, "one re-evaluation per node"
        h = np.array([float(_lib.chi2_grid_weighted(d.flux, d.inv_var, grid).cpu()[0]) for d, grid in best[j]])
        x = np.log(given[:, 1]) - h
        want = np.exp(x - x.max())
        want = want / want.sum()
        bar = 16 * EPS * (1.0 + h.max())
        worst = max(worst, float(np.abs(w - want).max() / bar))
        print("row %d: h %s, weights %s" % (j, h, w))
        assert (np.abs(w - want) <= bar).all()
        checked += 1
    print("node weights: max |d w| / bar %.3g" % worst)
    assert checked == np.isfinite(m["lnZ"]).sum() >= 10
    # the attribute is cleared by a call without the key
    assert _passes(monkeypatch)["none"]["target"].dataset_t0 is None


def _grid_inputs():
    """five nodes of a Gaussian prior of one cadence on dataset 1, two unequal nodes on dataset 0 (the dataset whose
    reduction carries the secondary-eclipse rule)"""
    a, b = _two_cadences()
    a = dict(a, t0_grid=[(-0.5 * CADENCE_0, 1.0), (0.75 * CADENCE_0, 3.0)])
    b = dict(b, t0_grid=t0_shift_grid(CADENCE_1, n=5, span=3.0))
    return [a, b]


def test_chunks_refined_posterior_and_fused_refusal(device_mode, monkeypatch):
    data = _grid_inputs()
    whole = _run(monkeypatch, data)
    assert whole["softmin_calls"] > 0 and np.isfinite(whole["lnZ"]).sum() >= 10
    assert whole["cells"] == whole["rows"] * (2 * 50 + 5 * 21)
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["softmin_calls"] >= whole["softmin_calls"] + 2 * 2 * sum(h.size >= 3 for h in whole["h"])
    assert _same_bits(whole, chunked)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(whole["h"], chunked["h"]))
    refined = _run(monkeypatch, data, refined=True)
    assert _same_bits(whole, refined)
    for x, y in zip(whole["target"].dataset_t0, refined["target"].dataset_t0):
        for l in (0, 1):
            assert np.array_equal(x[l]["weight"], y[l]["weight"], equal_nan=True)
    sampled = _run(monkeypatch, data, n_samples=64)
    assert _same_bits(whole, sampled)
    post = sampled["target"].posterior
    assert len(post) == whole["lnZ"].size and sum(p is not None for p in post) >= 10
    tg = _target()
    with pytest.raises(NotImplementedError, match="t0_grid"):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)
    # ... and where the evaluation is picked, for a caller that comes past the target's own check
    monkeypatch.setattr(Datasets, "has_t0_grids", property(lambda self: False))
    with pytest.raises(NotImplementedError, match="t0_grid dataset is not built: the nodes"):
        _target().calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_grid_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x, shift grids on both datasets: the model
    curves on the shifted stamps from the oracle, the reductions, the soft minimum and the evidence in numpy."""
    data = _grid_inputs()
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    sets = validate(data)
    ds = Datasets(sets, t0_grids(data, sets)).renorm(float(TARGET_SHARE))
    assert [None if g is None else g.shape for g in ds.t0_grids] == [(2, 2), (5, 2)]
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
            for l, (s, g) in enumerate(zip(ds.sets, ds.t0_grids)):
                nodes = []
                for shift in g[:, 0]:
                    grid, sec = O.flux_grid(model, s.time + shift, block, exptime=s.exptime, nsamples=s.nsamples)
                    r = s.flux - grid
                    hj = 0.5 * np.sum(r * r / s.flux_err ** 2, axis=1)
                    if l == 0 and model == O.MODEL_EB:
                        hj[sec >= 1.5 * ds.sigma_ref] = np.inf
                    nodes.append(hj)
                h += _numerics.t0_mix_halfchi2(np.stack(nodes), np.log(g[:, 1]))
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
    print("shift grids against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
    w = np.array([row[1]["weight"] for row, z in zip(tg.dataset_t0, tg.lnZ) if np.isfinite(z)])
    print("posterior weights of the five nodes of dataset 1 at the best draws:\n%s" % w)


def test_a_miscentred_dataset_is_recovered(device_mode, monkeypatch):
    """dataset 1 with time - d, d = 4 cadences of that dataset: its transit is centred at +d on the stamps given"""
    three = [(-DELTA, 1.0), (0.0, 1.0), (DELTA, 1.0)]
    grid = _run(monkeypatch, _inputs(shift=-DELTA, t0_grid=three))
    single = _run(monkeypatch, _inputs(shift=-DELTA, t0_grid=[(DELTA, 1.0)]))
    assert grid["rows"] == single["rows"] > 0
    fin = np.isfinite(single["lnZ"])
    assert fin.sum() >= 10 and np.isfinite(grid["lnZ"][fin]).all()
    for j in np.flatnonzero(fin):
        bar, _ = _bar(grid["h"][j], single["h"][j])
        slack = grid["lnZ"][j] - (single["lnZ"][j] - math.log(3.0))
        print("row %d: lnZ_grid %.6f, lnZ_single - ln 3 %.6f (bar %.3g)" % (j, grid["lnZ"][j], single["lnZ"][j] - math.log(3.0), bar))
        assert slack >= -bar, (j, slack, bar)
    top = int(np.nanargmax(grid["prob"]))
    row = grid["target"].dataset_t0[top][1]
    print("most probable scenario %d (prob %.4f): weights of the nodes (-d, 0, +d) at its best draw %s, mean shift %.5f "
          "(d = %.5f; not gated: no d was confirmed with the CPU oracle beforehand)"
          % (top, grid["prob"][top], row["weight"], row["mean"], DELTA))
    assert abs(math.fsum(row["weight"]) - 1.0) <= 8 * EPS * 3
