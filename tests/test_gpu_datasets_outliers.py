"""target.calc_probs_datasets with the outlier-tolerant likelihood on a dataset (`outlier_frac` / `outlier_scale`; DESIGN.md
section 14), end to end on the fixtures of tests/test_gpu_datasets.py: TOI-465.01, two cadences (50 + 21 points), N = 20 000,
set_sampling("device"), one seed for every pass.  The keys go on dataset 1: (eps, kappa) = (0.05, 10).

Bars, none of them chosen from results:
  no keys / keys = None: the same bits, and _lib.chi2_grid_robust is never called;
  TP, EB and EB-twin of the target star against the CPU oracle's model curves reduced with _numerics.robust_halfchi2, the
        evidence in numpy: |d lnZ| <= 1e-9, the bar of the same check in tests/test_gpu_datasets_t0_grid.py; the same masked
        counts, the same best draw (the smallest sum of the datasets' terms) per branch;
  per draw, h(keys on dataset 1) <= h(no keys) + T_1 c0 + bar: the first upper bound of the mixture on dataset 1, dataset 0's
        term being the same bits in both passes; bar = 1e-12 (71 + h) + 1e-12 at the robust value h -- the host statement's
        bar 1e-12 sum_t (1 + lo_t) + 1e-12 with sum_t lo_t <= h + T ln 2 over the 71 points of both datasets (the plain
        dataset's terms are their own lo).  The per-draw sums are those the evidence is formed from, taken where
        fused hands them to _lib.lnz_from_halfchi2 (fused.DUMP holds the draws, not their sums);
  three points of dataset 1 inside the transit window set to exactly 1 + 8 sigma_t: the model never exceeds 1 in a star's own
        normalisation and renorm_flux keeps (flux - 1) / sigma, so z_t >= 8 at every draw, a_t >= 32, and
        p_t >= 1 / (1 + exp(c1 - c0 - 32 (1 - k2))), less 1e-12 for the rounding of z in the renormalisation;
  three chunks of the grid, calc_probs_datasets_refined(n_adapt = 0), n_samples = 64: the same bits;
  a one-node t0_grid (d, 1) next to the keys: the bits of time + d with the keys.
"""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from test_gpu_datasets_red_noise import CADENCE_1, COLS, _same_bits
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import Datasets, outliers, robust_constants, t0_grids, validate

pytestmark = pytest.mark.gpu

PAIR = (0.05, 10.0)
KEYS = {"outlier_frac": PAIR[0], "outlier_scale": PAIR[1]}
C0, C1, K2 = robust_constants(*PAIR)
T0, T1 = 50, 21
DELTA = 4.0 * CADENCE_1


def _inputs(shift=0.0, glitch=False, **keys):
    a, b = _two_cadences()
    b = dict(b, time=b["time"] + shift, **keys)
    if glitch:
        flux = np.array(b["flux"], dtype=np.float64)
        err = np.broadcast_to(np.asarray(b["flux_err"], dtype=np.float64), flux.shape)
        flux[GLITCH] = 1.0 + 8.0 * err[GLITCH]
        b["flux"] = flux
    return [a, b]


# the three points of dataset 1 nearest the transit midpoint (time 0 of the folded light curve)
GLITCH = np.sort(np.argsort(np.abs(_two_cadences()[1]["time"]))[:3])


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it; and the calls of _lib.chi2_grid_robust"""

    def __init__(self, monkeypatch):
        self.h, self.robust_calls = [], 0
        real_z, real_r = _lib.lnz_from_halfchi2, _lib.chi2_grid_robust
        spy = self

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def robust(*a, **k):
            spy.robust_calls += 1
            return real_r(*a, **k)

        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "chi2_grid_robust", robust)


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
            "best": np.stack([tg.probs[c].values for c in COLS]), "target": tg, "h": s.h, "robust_calls": s.robust_calls}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["keys"] = _run(monkeypatch, _inputs(**KEYS))
    return _runs


def _same_outliers(x, y):
    assert len(x) == len(y)
    for u, v in zip(x, y):
        assert u[0] is None and v[0] is None
        assert (u[1]["frac"], u[1]["scale"]) == (v[1]["frac"], v[1]["scale"]) == PAIR
        assert u[1]["prob"].tobytes() == v[1]["prob"].tobytes()


def test_without_the_keys_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(outlier_frac=None, outlier_scale=None))
    assert np.isfinite(a["lnZ"]).sum() >= 10 and _same_bits(a, b)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["h"], b["h"]))
    assert a["robust_calls"] == b["robust_calls"] == 0
    assert a["cells"] == b["cells"] and a["launches"] == b["launches"]
    assert a["target"].dataset_outliers is None and b["target"].dataset_outliers is None
    k = _passes(monkeypatch)["keys"]
    assert k["robust_calls"] > 0 and k["rows"] == a["rows"] and k["cells"] == a["cells"]
    # the keys change the evidence: the point of the feature
    fin = np.isfinite(a["lnZ"])
    assert np.array_equal(fin, np.isfinite(k["lnZ"])) and np.abs(k["lnZ"][fin] - a["lnZ"][fin]).max() > 1e-3
    table = k["target"].dataset_outliers
    assert isinstance(table, list) and len(table) == k["lnZ"].size
    for row, lnz in zip(table, k["lnZ"]):
        assert len(row) == 2 and row[0] is None and (row[1]["frac"], row[1]["scale"]) == PAIR
        p = row[1]["prob"]
        assert p.shape == (T1,) and p.dtype == np.float64
        assert np.isnan(p).all() if not np.isfinite(lnz) else ((p >= 0) & (p <= 1)).all()


def test_every_draw_obeys_the_first_upper_bound(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    plain, keyed = r["none"]["h"], r["keys"]["h"]
    assert len(plain) == len(keyed) == r["keys"]["lnZ"].size
    worst, draws = -np.inf, 0
    for hp, hk in zip(plain, keyed):
        assert hp.shape == hk.shape
        assert np.array_equal(np.isposinf(hp), np.isposinf(hk)) and not np.isnan(hk).any()
        ok = np.isfinite(hk)
        bar = 1e-12 * ((T0 + T1) + hk[ok]) + 1e-12
        slack = hk[ok] - (hp[ok] + T1 * C0)
        if ok.any():
            worst = max(worst, float(np.max(slack / bar)))
        draws += int(ok.sum())
        assert (slack <= bar).all()
        assert (hk[ok] >= 0).all()
    print("h(keys) - h(no keys) - T_1 c0 over %d draws: at most %.3g bars" % (draws, worst))
    assert draws > 1000


def test_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x, the keys on dataset 1: the model curves from
    the oracle, the reductions and the evidence in numpy."""
    data = _inputs(**KEYS)
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    spy = _Spy(monkeypatch)
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    _lib.reset_stats()
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    masked = _lib.STATS["rows"]
    monkeypatch.undo()
    assert len(dump) == 2 and len(spy.h) == 3 and spy.robust_calls > 0
    sets = validate(data)
    ds = Datasets(sets, t0_grids(data, sets), outliers(data, sets)).renorm(float(TARGET_SHARE))
    assert ds.outliers == (None, PAIR)
    want, count, above = [], 0, 0.0
    for d in dump:
        cols = d["cols"].cpu().numpy()
        mask, mask2 = d["mask"].cpu().numpy(), None if d["mask_twin"] is None else d["mask_twin"].cpu().numpy()
        lnprior = None if d["lnprior"] is None else d["lnprior"].cpu().numpy()
        planet = mask2 is None
        branches = ((O.MODEL_TP, mask, False),) if planet else ((O.MODEL_EB, mask, False), (O.MODEL_EB_TWIN, mask2, True))
        for model, m, twin in branches:
            idx = np.flatnonzero(m)
            count += idx.size
            block = cols[:10 if planet else 11][:, idx].copy()
            if twin:
                block[2] *= 2.0
                block[4] = cols[11][idx]
            h = np.zeros(idx.size)
            for l, (s, o) in enumerate(zip(ds.sets, ds.outliers)):
                grid, sec = O.flux_grid(model, s.time, block, exptime=s.exptime, nsamples=s.nsamples)
                above = max(above, float(np.max(grid - 1.0))) if grid.size else above
                w = 1.0 / s.flux_err ** 2
                if o is None:
                    hl = 0.5 * np.sum(w * (s.flux - grid) ** 2, axis=1)
                else:
                    hl = _numerics.robust_halfchi2(s.flux - grid, w, *robust_constants(*o))
                if l == 0 and model == O.MODEL_EB:
                    hl[sec >= 1.5 * ds.sigma_ref] = np.inf
                h += hl
            got_h = spy.h[len(want)]
            assert got_h.shape == h.shape and np.array_equal(np.isposinf(got_h), np.isposinf(h))
            if np.isfinite(h).any():
                assert int(np.argmin(got_h)) == int(np.argmin(h)), "best draws differ"
            x = -0.5 * np.log(2 * np.pi) - np.log(ds.sigma_ref) - h
            if lnprior is not None:
                x = x + lnprior[idx]
            full = np.full(m.size, -np.inf)
            full[idx] = x
            want.append(O.log_mean_exp(full, m.size))
    assert count == masked > 0, "masked counts differ"
    print("largest model value above 1 on this fixture (oracle): %.3g" % above)
    want = np.array(want)
    got = tg.lnZ[:3]
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and np.isfinite(want).sum() >= 2
    fin = np.isfinite(want)
    print("the outlier mixture against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9


def test_a_glitch_is_recognised_at_every_best_draw(device_mode, monkeypatch):
    g = _run(monkeypatch, _inputs(glitch=True, **KEYS))
    floor = 1.0 / (1.0 + math.exp(C1 - C0 - 32.0 * (1.0 - K2))) - 1e-12
    table = g["target"].dataset_outliers
    checked = 0
    for row, lnz in zip(table, g["lnZ"]):
        assert row[0] is None
        p = row[1]["prob"]
        if not np.isfinite(lnz):
            assert np.isnan(p).all()
            continue
        print("lnZ %.4f: p at the three points %s, largest elsewhere %.3g" % (lnz, p[GLITCH], np.delete(p, GLITCH).max()))
        assert (p[GLITCH] >= floor).all(), (p[GLITCH], floor)
        checked += 1
    assert checked >= 10
    # without the keys the same three points cost every scenario about 96 units of log-weight
    plain = _run(monkeypatch, _inputs(glitch=True))
    fin = np.isfinite(g["lnZ"]) & np.isfinite(plain["lnZ"])
    assert fin.sum() >= 10 and (g["lnZ"][fin] > plain["lnZ"][fin] + 50.0).all()


def test_chunks_refined_posterior_and_fused_refusal(device_mode, monkeypatch):
    data = _inputs(**KEYS)
    whole = _passes(monkeypatch)["keys"]
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["robust_calls"] >= whole["robust_calls"] + 2 * sum(h.size >= 3 for h in whole["h"])
    assert _same_bits(whole, chunked)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(whole["h"], chunked["h"]))
    _same_outliers(whole["target"].dataset_outliers, chunked["target"].dataset_outliers)
    refined = _run(monkeypatch, data, refined=True)
    assert _same_bits(whole, refined)
    _same_outliers(whole["target"].dataset_outliers, refined["target"].dataset_outliers)
    sampled = _run(monkeypatch, data, n_samples=64)
    assert _same_bits(whole, sampled)
    post = sampled["target"].posterior
    assert len(post) == whole["lnZ"].size and sum(p is not None for p in post) >= 10
    tg = _target()
    with pytest.raises(NotImplementedError, match="outlier"):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)
    # ... and where the evaluation is picked, for a caller that comes past the target's own check
    monkeypatch.setattr(Datasets, "has_outliers", property(lambda self: False))
    with pytest.raises(NotImplementedError, match="outlier_frac dataset is not built: the fused kernel"):
        _target().calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_one_node_next_to_the_keys_is_the_shifted_stamps_in_bits(device_mode, monkeypatch):
    g = _run(monkeypatch, _inputs(t0_grid=[(DELTA, 1.0)], **KEYS))
    p = _run(monkeypatch, _inputs(shift=DELTA, **KEYS))
    assert g["robust_calls"] > 0 and p["robust_calls"] > 0
    assert np.isfinite(g["lnZ"]).sum() >= 10 and _same_bits(g, p)
    assert len(g["h"]) == len(p["h"]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(g["h"], p["h"]))
    _same_outliers(g["target"].dataset_outliers, p["target"].dataset_outliers)
    assert g["target"].dataset_t0 is not None and p["target"].dataset_t0 is None
    fin = np.isfinite(g["lnZ"])
    assert np.abs(g["lnZ"][fin] - _passes(monkeypatch)["keys"]["lnZ"][fin]).max() > 1e-3
