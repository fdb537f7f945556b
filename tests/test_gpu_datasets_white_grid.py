"""target.calc_probs_datasets with a grid of white-noise candidates per dataset (`white_grid`: error scale and jitter;
DESIGN.md section 14), end to end on the fixtures of tests/test_gpu_datasets.py: TOI-465.01, two cadences, N = 20 000,
set_sampling("device"), one seed for every pass.

Bars, none of them chosen from results:
  no key / key = None: the same bits, and _lib.chi2_grid_white_mix is never called;
  the grid [(1, 0, 1)] on dataset 1 against no key: the same lnZ, prob and best-draw bits (the candidate's weights are the
        bits of 1 / flux_err^2, lnc = 0, and the kernel's T is then h_1 bit for bit);
  linearity: exp(-T) = sum_j c_j exp(-h_j) per draw and the masks depend on sigma_bar alone -- which ignores the key --, so
        from one seed lnZ{A, B} = logsumexp(lnc_A + lnZ_A, lnc_B + lnZ_B) per scenario row, lnc from white_mix_system of
        the input; |d| <= 8 eps (1 + the largest finite h among the row's draws) + 1e-12: the h_j are the same bits in the
        three passes, so only the kernel's exp / log and the three log-mean-exp folds differ; per draw to
        8 eps (1 + |T| + max |lnc|) + 1e-12;
  .dataset_white_noise: weights >= 0, their sum 1 to 8 eps J, and equal to softmax_j(lnc_j - h_j) with the h_j of
        _lib.chi2_grid_weighted on the best draw's model row, to 16 eps (1 + max_j h_j) (the softmax is 1-Lipschitz in the
        h_j up to its own rounding); on a dataset whose white noise is twice the stated error the candidate k = 2 of
        [1, 2, 4] carries the largest weight at every scenario's best draw;
  the same dataset with a grid that contains (2, 0), against the CPU oracle's model grid reduced with
        _numerics.white_mix_halfchi2: |d lnZ| <= 1e-9, the bar of the other oracle checks of the datasets path;
  three chunks of the grid, calc_probs_datasets_refined(n_adapt = 0) and a one-node t0_grid (0, 1): the same bits.
"""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from test_gpu_datasets_red_noise import COLS, SIGMA_1, _same_bits
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import Datasets, validate, white_grids, white_mix_system
from triceratops_amd.lightcurve import white_noise_grid

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
A = (1.5, 0.0)
B = (1.0, 2.0 * SIGMA_1)
AB = [A + (0.3,), B + (0.7,)]


def _inputs(**keys):
    a, b = _two_cadences()
    return [a, dict(b, **keys)]


NOISE = 10.0        # the stated error of _noisy_inputs' dataset 1, in units of the light curve's own sigma


def _noisy_inputs(**keys):
    """dataset 1 with one stated error e = NOISE sigma for all points and white noise of variance (2 e)^2 - sigma^2 injected
    on top of the light curve's own sigma^2 (a fixed seed; the injected values have mean 0 and that mean square exactly):
    the true white noise is twice the stated error.  e is ten times the light curve's sigma so that the noise decides the
    candidates' weights and not a scenario's misfit: with T = 21 points and chi^2 = sum (residual / e)^2, k = 2 beats k = 1
    while chi^2 > (8 / 3) T ln 2 = 38.8 and k = 4 while chi^2 < (32 / 3) T ln 4 = 155; the noise alone gives 4 T = 84.  With
    e = sigma the scenarios that cannot fit the transit (chi^2 of 240 ... 1100 on these 21 points) put the weight on k = 4
    -- rightly: under them the residuals are that large --; in units of e = 10 sigma their misfit adds at most 10."""
    a, b = _two_cadences()
    sigma = LC["sigma"]
    e = NOISE * sigma
    xi = np.random.default_rng(465).normal(size=b["time"].size)
    xi = xi - xi.mean()
    xi = xi / np.sqrt(np.mean(xi * xi))
    return [a, dict(b, flux=b["flux"] + math.sqrt(4.0 * e * e - sigma * sigma) * xi, flux_err=e, **keys)]


def _lnc(data):
    sets = validate(data)
    return white_mix_system(sets[1], white_grids(data, sets)[1])[1]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it; the calls of _lib.chi2_grid_white_mix and
    _lib.chi2_grid_weighted; and per evidence that had a draw, the best draw's re-evaluation of a white_grid dataset: its
    index, the dataset's device record and the one model row"""

    def __init__(self, monkeypatch):
        self.h, self.mix_calls, self.plain_calls, self.best = [], 0, 0, []
        real_z, real_mix, real_plain, real_half = (_lib.lnz_from_halfchi2, _lib.chi2_grid_white_mix,
                                                   _lib.chi2_grid_weighted, fused._Dataset.halfchi2)
        spy = self

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def mix(*a, **k):
            spy.mix_calls += 1
            return real_mix(*a, **k)

        def plain(*a, **k):
            spy.plain_calls += 1
            return real_plain(*a, **k)

        def halfchi2(d, grid, *a, **k):
            if k.get("cand_out") is not None:
                spy.best.append((len(spy.h) - 1, d, grid.clone()))
            return real_half(d, grid, *a, **k)

        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "chi2_grid_white_mix", mix)
        monkeypatch.setattr(_lib, "chi2_grid_weighted", plain)
        monkeypatch.setattr(fused._Dataset, "halfchi2", halfchi2)


def _run(monkeypatch, datasets, refined=None, **kw):
    tg = _target()
    s = _Spy(monkeypatch)
    torch.manual_seed(SEED)
    _lib.reset_stats()
    if refined is not None:
        tg.calc_probs_datasets_refined(datasets, LC["P_orb"], n_adapt=refined, **dict(KW, **kw))
    else:
        tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(KW, **kw))
    rows = _lib.STATS["rows"]
    monkeypatch.undo()
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows,
            "best": np.stack([tg.probs[c].values for c in COLS]), "target": tg, "h": s.h, "mix_calls": s.mix_calls,
            "plain_calls": s.plain_calls, "best_rows": s.best}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["A"] = _run(monkeypatch, _inputs(white_grid=[A + (1.0,)]))
        _runs["B"] = _run(monkeypatch, _inputs(white_grid=[B + (5.0,)]))
        _runs["AB"] = _run(monkeypatch, _inputs(white_grid=AB))
    return _runs


def test_without_the_key_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(white_grid=None))
    assert np.isfinite(a["lnZ"]).sum() >= 10 and _same_bits(a, b)
    assert a["mix_calls"] == b["mix_calls"] == 0 and a["plain_calls"] == b["plain_calls"] > 0
    assert a["target"].dataset_white_noise is None and b["target"].dataset_white_noise is None
    assert len(a["h"]) == len(b["h"]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["h"], b["h"]))
    m = _passes(monkeypatch)["AB"]
    assert m["mix_calls"] > 0 and 0 < m["plain_calls"] < a["plain_calls"]           # (dataset 0 keeps the plain reduction)


def test_the_unit_candidate_is_no_key_in_bits(device_mode, monkeypatch):
    p = _passes(monkeypatch)["none"]
    g = _run(monkeypatch, _inputs(white_grid=[(1.0, 0.0, 1.0)]))
    assert g["mix_calls"] > 0 and p["mix_calls"] == 0
    assert np.isfinite(g["lnZ"]).sum() >= 10 and _same_bits(g, p)
    assert len(g["h"]) == len(p["h"]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(g["h"], p["h"]))
    # a scaled error changes the evidence: the point of the feature
    a = _passes(monkeypatch)["A"]
    fin = np.isfinite(a["lnZ"])
    assert np.abs(a["lnZ"][fin] - p["lnZ"][fin]).max() > 1e-3
    # one candidate: its weight is 1 wherever there is a best draw
    for row, lnz in zip(g["target"].dataset_white_noise, g["lnZ"]):
        assert row[0] is None and row[1]["grid"].shape == (1, 3) and row[1]["grid"][0].tolist() == [1.0, 0.0, 1.0]
        assert row[1]["weight"].shape == (1,) and (row[1]["weight"][0] == 1.0 if np.isfinite(lnz) else np.isnan(row[1]["weight"][0]))


def test_the_evidence_is_linear_in_the_candidates(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    a, b, m = r["A"], r["B"], r["AB"]
    lnc = _lnc(_inputs(white_grid=AB))
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


def _check_weights(m, data):
    """.dataset_white_noise of a pass against the softmax of the candidates' chi^2/2 on the best draws' model rows; returns
    the [finite scenarios][J] weights"""
    tg = m["target"]
    table = tg.dataset_white_noise
    sets = validate(data)
    given = white_grids(data, sets)[1]
    J = given.shape[0]
    assert isinstance(table, list) and len(table) == m["lnZ"].size
    best = {k: (d, grid) for k, d, grid in m["best_rows"]}
    assert len(best) == len(m["best_rows"]), "one re-evaluation per evidence"
    out = []
    for j, (row, lnz) in enumerate(zip(table, m["lnZ"])):
        assert len(row) == 2 and row[0] is None
        assert np.array_equal(row[1]["grid"], given)
        w = row[1]["weight"]
        assert w.shape == (J,) and w.dtype == np.float64
        if not np.isfinite(lnz):
            assert np.isnan(w).all()
            continue
        assert (w >= 0).all() and abs(math.fsum(w) - 1.0) <= 8 * EPS * J
        d, grid = best[j]
        w_d, lnc = d.term
        h = np.array([float(_lib.chi2_grid_weighted(d.flux, w_d[k].contiguous(), grid).cpu()[0]) for k in range(J)])
        x = lnc - h
        want = np.exp(x - x.max())
        want = want / want.sum()
        print("row %d: h %s, weights %s" % (j, h, w))
        assert (np.abs(w - want) <= 16 * EPS * (1.0 + h.max())).all()
        out.append(w)
    assert len(out) == np.isfinite(m["lnZ"]).sum() >= 10
    return np.array(out)


def test_candidate_weights_at_the_best_draw(device_mode, monkeypatch):
    _check_weights(_passes(monkeypatch)["AB"], _inputs(white_grid=AB))
    # the attribute is cleared by a call without the key
    assert _passes(monkeypatch)["none"]["target"].dataset_white_noise is None


def test_understated_errors_put_the_weight_on_their_true_scale(device_mode, monkeypatch):
    data = _noisy_inputs(white_grid=white_noise_grid([1.0, 2.0, 4.0]))
    m = _run(monkeypatch, data)
    w = _check_weights(m, data)
    print("posterior weights of k = 1, 2, 4 at the best draws:\n%s" % w)
    assert (np.argmax(w, axis=1) == 1).all()


def test_chunks_refined_passes_a_single_node_and_the_fused_refusal(device_mode, monkeypatch):
    data = _inputs(white_grid=AB)
    whole = _passes(monkeypatch)["AB"]
    assert whole["mix_calls"] > 0 and np.isfinite(whole["lnZ"]).sum() >= 10
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["mix_calls"] > whole["mix_calls"]
    assert chunked["mix_calls"] - len(chunked["best_rows"]) >= 3 * sum(h.size >= 3 for h in whole["h"])
    assert _same_bits(whole, chunked)
    refined = _run(monkeypatch, data, refined=0)
    node = _run(monkeypatch, _inputs(white_grid=AB, t0_grid=[(0.0, 1.0)]))
    for other in (refined, node):
        assert _same_bits(whole, other)
        for x, y in zip(whole["target"].dataset_white_noise, other["target"].dataset_white_noise):
            assert np.array_equal(x[1]["weight"], y[1]["weight"], equal_nan=True)
    assert node["target"].dataset_t0 is not None and whole["target"].dataset_t0 is None
    # an adaptation pass skips the report, the final pass fills it
    adapted = _run(monkeypatch, data, refined=1)
    assert len(adapted["target"].refine_history) == 2
    assert 0 < len(adapted["best_rows"]) <= adapted["lnZ"].size           # (one re-evaluation per evidence: the final pass')
    table = adapted["target"].dataset_white_noise
    assert len(table) == adapted["lnZ"].size and np.isfinite(adapted["lnZ"]).sum() >= 10
    for row, lnz in zip(table, adapted["lnZ"]):
        w = row[1]["weight"]
        assert row[0] is None and w.shape == (2,)
        assert (abs(math.fsum(w) - 1.0) <= 8 * EPS * 2 and (w >= 0).all()) if np.isfinite(lnz) else np.isnan(w).all()
    tg = _target()
    with pytest.raises(NotImplementedError, match="white_grid"):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_grid_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x on dataset 0, understated by a factor 2 on
    dataset 1 with a grid of six candidates that contains (2, 0): the model curves from the oracle, the weighted sums, the
    soft minimum and the evidence in numpy."""
    data = _noisy_inputs(white_grid=white_noise_grid([1.0, 2.0, 3.0], [0.0, NOISE * LC["sigma"]],
                                                     [[1.0, 2.0], [3.0, 2.0], [1.0, 1.0]]))
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    sets = validate(data)
    ds = Datasets(sets, white_grids=white_grids(data, sets)).renorm(float(TARGET_SHARE))
    assert ds.white_grids[0] is None and ds.white_grids[1].shape == (6, 3) and [2.0, 0.0] in ds.white_grids[1][:, :2].tolist()
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
            for l, (s, g) in enumerate(zip(ds.sets, ds.white_grids)):
                grid, sec = O.flux_grid(model, s.time, block, exptime=s.exptime, nsamples=s.nsamples)
                r = s.flux - grid
                if g is None:
                    h += 0.5 * np.sum(r * r / s.flux_err ** 2, axis=1)
                else:
                    h += _numerics.white_mix_halfchi2(r, *white_mix_system(s, g))
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
    print("white-grid dataset against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
    w = np.array([row[1]["weight"] for row, z in zip(tg.dataset_white_noise, tg.lnZ) if np.isfinite(z)])
    print("posterior weights of the six candidates at the best draws:\n%s" % w)
