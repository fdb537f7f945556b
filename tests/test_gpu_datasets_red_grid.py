"""target.calc_probs_datasets with a grid of red-noise candidates per dataset (`red_grid`), end to end
on the fixtures of tests/test_gpu_datasets.py: TOI-465.01, two cadences, N = 20 000, set_sampling("device"), one seed for
every pass.

Bars, none of them chosen from results:
  no key / key = None: the same bits, and _lib.chi2_grid_ou_mix is never called;
  a grid of one candidate against the same pair as red_sigma / red_timescale: the same lnZ, prob and best-draw bits
        (lnc = 0, and the kernel's T is then h_1 bit for bit);
  linearity: exp(-T) = sum_j c_j exp(-h_j) per draw and the masks depend on sigma_bar alone, so from one seed
        lnZ{A, B} = logsumexp(lnc_A + lnZ_A, lnc_B + lnZ_B) per scenario row, lnc from ou_mix_system of the input;
        |d| <= 8 eps (1 + the largest finite h among the row's draws) + 1e-12: the h_j are the same bits in the three
        passes, so only the kernel's exp / log and the three log-mean-exp folds differ;
  an OU realisation added to dataset 1 and a grid that contains its pair, against the CPU oracle's model grid reduced with
        _numerics.ou_mix_halfchi2: |d lnZ| <= 1e-9, the bar of the other oracle checks of the datasets path;
  three chunks of the grid, and calc_probs_datasets_refined(n_adapt = 0): the same bits;
  .dataset_red_noise: weights >= 0, their sum 1 to 8 eps J, and equal to softmax_j(lnc_j - h_j) with the h_j of
        _lib.chi2_grid_ou on the best draw's model row, to 16 eps (1 + max_j h_j) (the softmax is 1-Lipschitz in the h_j up
        to its own rounding).
"""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from test_gpu_datasets_red_noise import CADENCE_1, COLS, SIGMA_1, _ou_inputs, _same_bits
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import Datasets, ou_mix_system, validate
from triceratops_amd.lightcurve import red_noise_grid

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
A = (2.0 * SIGMA_1, 20.0 * CADENCE_1)
B = (0.7 * SIGMA_1, 4.0 * CADENCE_1)
AB = [A + (0.3,), B + (0.7,)]


def _inputs(**keys):
    a, b = _two_cadences()
    return [a, dict(b, **keys)]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it; the calls of _lib.chi2_grid_ou_mix and
    _lib.chi2_grid_ou; and per evidence that had a draw, the best draw's re-evaluation of a red_grid dataset: its index, the
    dataset's device record and the one model row"""

    def __init__(self, monkeypatch):
        self.h, self.mix_calls, self.ou_calls, self.best = [], 0, 0, []
        real_z, real_mix, real_ou, real_half = (_lib.lnz_from_halfchi2, _lib.chi2_grid_ou_mix, _lib.chi2_grid_ou,
                                                fused._Dataset.halfchi2)
        spy = self

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def mix(*a, **k):
            spy.mix_calls += 1
            return real_mix(*a, **k)

        def ou(*a, **k):
            spy.ou_calls += 1
            return real_ou(*a, **k)

        def halfchi2(d, grid, *a, **k):
            if k.get("cand_out") is not None:
                spy.best.append((len(spy.h) - 1, d, grid.clone()))
            return real_half(d, grid, *a, **k)

        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "chi2_grid_ou_mix", mix)
        monkeypatch.setattr(_lib, "chi2_grid_ou", ou)
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
    rows = _lib.STATS["rows"]
    monkeypatch.undo()
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows,
            "best": np.stack([tg.probs[c].values for c in COLS]), "target": tg, "h": s.h, "mix_calls": s.mix_calls,
            "ou_calls": s.ou_calls, "best_rows": s.best}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["A"] = _run(monkeypatch, _inputs(red_grid=[A + (1.0,)]))
        _runs["B"] = _run(monkeypatch, _inputs(red_grid=[B + (5.0,)]))
        _runs["AB"] = _run(monkeypatch, _inputs(red_grid=AB))
    return _runs


def test_without_the_key_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(red_grid=None))
    assert np.isfinite(a["lnZ"]).sum() >= 10 and _same_bits(a, b)
    assert a["mix_calls"] == b["mix_calls"] == 0 and a["ou_calls"] == 0
    assert a["target"].dataset_red_noise is None and b["target"].dataset_red_noise is None
    assert _passes(monkeypatch)["AB"]["mix_calls"] > 0 and _passes(monkeypatch)["AB"]["ou_calls"] == 0


def test_one_candidate_is_red_sigma_and_red_timescale_in_bits(device_mode, monkeypatch):
    g = _passes(monkeypatch)["A"]
    p = _run(monkeypatch, _inputs(red_sigma=A[0], red_timescale=A[1]))
    assert g["mix_calls"] > 0 and g["ou_calls"] == 0 and p["mix_calls"] == 0 and p["ou_calls"] > 0
    assert np.isfinite(g["lnZ"]).sum() >= 10 and _same_bits(g, p)
    assert len(g["h"]) == len(p["h"]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(g["h"], p["h"]))
    # the noise model changes the evidence: the point of the feature
    fin = np.isfinite(g["lnZ"])
    assert np.abs(g["lnZ"][fin] - _passes(monkeypatch)["none"]["lnZ"][fin]).max() > 1e-3
    # one candidate: its weight is 1 wherever there is a best draw
    for row, lnz in zip(g["target"].dataset_red_noise, g["lnZ"]):
        assert row[0] is None and row[1]["grid"].shape == (1, 3) and row[1]["grid"][0, 2] == 1.0
        assert row[1]["weight"].shape == (1,) and (row[1]["weight"][0] == 1.0 if np.isfinite(lnz) else np.isnan(row[1]["weight"][0]))


def test_the_evidence_is_linear_in_the_candidates(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    a, b, m = r["A"], r["B"], r["AB"]
    lnc = ou_mix_system(validate(_inputs(red_grid=AB))[1])[3]
    assert lnc.shape == (2,) and np.isfinite(lnc).all()
    assert a["rows"] == b["rows"] == m["rows"] == r["none"]["rows"] > 0, "masked counts differ"
    assert len(a["h"]) == len(b["h"]) == len(m["h"]) == m["lnZ"].size
    fin = np.isfinite(m["lnZ"])
    assert np.array_equal(fin, np.isfinite(a["lnZ"])) and np.array_equal(fin, np.isfinite(b["lnZ"])) and fin.sum() >= 10
    worst = 0.0
    for j in np.flatnonzero(fin):
        assert a["h"][j].shape == b["h"][j].shape == m["h"][j].shape
        top = max(float(h[np.isfinite(h)].max()) for h in (a["h"][j], b["h"][j], m["h"][j]))
        bar = 8 * EPS * (1.0 + top) + 1e-12
        x, y = lnc[0] + a["lnZ"][j], lnc[1] + b["lnZ"][j]
        want = max(x, y) + math.log(math.fsum((math.exp(x - max(x, y)), math.exp(y - max(x, y)))))
        d = abs(m["lnZ"][j] - want)
        worst = max(worst, d / bar)
        print("row %d: lnZ_A %.6f lnZ_B %.6f lnZ_AB %.6f, |d| %.3g, bar %.3g (largest finite h %.4g)"
              % (j, a["lnZ"][j], b["lnZ"][j], m["lnZ"][j], d, bar, top))
        assert d <= bar, (j, d, bar)
        # per draw as well: T = -ln(c_A exp(-h_A) + c_B exp(-h_B)), to the kernel's own rounding
        ha, hb, t = a["h"][j], b["h"][j], m["h"][j]
        ok = np.isfinite(ha) & np.isfinite(hb)
        assert np.array_equal(ok, np.isfinite(t))
        ref = -np.logaddexp(lnc[0] - ha[ok], lnc[1] - hb[ok])
        assert (np.abs(t[ok] - np.maximum(ref, 0.0)) <= 8 * EPS * (1.0 + np.abs(t[ok]) + np.abs(lnc).max()) + 1e-12).all()
    print("linearity: lnc %s, max |d lnZ| / bar %.3g over %d finite rows" % (lnc, worst, fin.sum()))
    # the two candidates give different evidences, and both count somewhere
    assert np.abs(a["lnZ"][fin] - b["lnZ"][fin]).max() > 1e-3


def test_candidate_weights_at_the_best_draw(device_mode, monkeypatch):
    m = _passes(monkeypatch)["AB"]
    tg = m["target"]
    table = tg.dataset_red_noise
    given = validate(_inputs(red_grid=AB))[1].red_grid
    assert isinstance(table, list) and len(table) == m["lnZ"].size
    best = {k: (d, grid) for k, d, grid in m["best_rows"]}
    assert len(best) == len(m["best_rows"]), "one re-evaluation per evidence"
    checked = 0
    for j, (row, lnz) in enumerate(zip(table, m["lnZ"])):
        assert len(row) == 2 and row[0] is None
        assert np.array_equal(row[1]["grid"], given)
        w = row[1]["weight"]
        assert w.shape == (2,) and w.dtype == np.float64
        if not np.isfinite(lnz):
            assert np.isnan(w).all()
            continue
        assert (w >= 0).all() and abs(math.fsum(w) - 1.0) <= 8 * EPS * 2
        d, grid = best[j]
        alpha, beta, omega, lnc = d.term
        h = np.array([float(_lib.chi2_grid_ou(d.flux, grid, alpha[k], beta[k], omega[k]).cpu()[0]) for k in range(2)])
        x = lnc - h
        want = np.exp(x - x.max())
        want = want / want.sum()
        print("row %d: h %s, weights %s" % (j, h, w))
        assert (np.abs(w - want) <= 16 * EPS * (1.0 + h.max())).all()
        checked += 1
    assert checked == np.isfinite(m["lnZ"]).sum() >= 10
    # the attribute is cleared by a call without the key
    assert _passes(monkeypatch)["none"]["target"].dataset_red_noise is None


def _grid_inputs():
    """_ou_inputs() of tests/test_gpu_datasets_red_noise.py -- an OU realisation of (2 sigma_1, 20 cadences) on dataset 1
    -- with a 2 x 2 grid that contains the pair in place of the keys"""
    a, b = _ou_inputs()
    s_r, tau = b.pop("red_sigma"), b.pop("red_timescale")
    b["red_grid"] = red_noise_grid([0.5 * s_r, s_r], [0.25 * tau, tau], [[1.0, 2.0], [3.0, 2.0]])
    return [a, b]


def test_chunks_fused_refusal_and_refined(device_mode, monkeypatch):
    data = _grid_inputs()
    whole = _run(monkeypatch, data)
    assert whole["mix_calls"] > 0 and np.isfinite(whole["lnZ"]).sum() >= 10
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["mix_calls"] > whole["mix_calls"]
    assert chunked["mix_calls"] - len(chunked["best_rows"]) >= 3 * sum(h.size >= 3 for h in whole["h"])
    assert _same_bits(whole, chunked)
    refined = _run(monkeypatch, data, refined=True)
    assert _same_bits(whole, refined)
    for x, y in zip(whole["target"].dataset_red_noise, refined["target"].dataset_red_noise):
        assert np.array_equal(x[1]["weight"], y[1]["weight"], equal_nan=True)
    tg = _target()
    with pytest.raises(NotImplementedError, match="red_grid"):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_grid_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x, an OU realisation and a grid of four
    candidates on dataset 1: the model curves from the oracle, the recurrences, the soft minimum and the evidence in numpy."""
    data = _grid_inputs()
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
                r = s.flux - grid
                if s.red_grid is None:
                    h += 0.5 * np.sum(r * r / s.flux_err ** 2, axis=1)
                else:
                    h += _numerics.ou_mix_halfchi2(r, *ou_mix_system(s))
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
    assert ds.sets[0].red_grid is None and ds.sets[1].red_grid.shape == (4, 3)
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and np.isfinite(want).sum() >= 2
    fin = np.isfinite(want)
    print("red-grid dataset against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
    # the grid contains the pair the realisation was drawn with: the candidates with its amplitude carry the weight
    w = np.array([row[1]["weight"] for row, z in zip(tg.dataset_red_noise, tg.lnZ) if np.isfinite(z)])
    print("posterior weights of the four candidates at the best draws:\n%s" % w)
