"""target.calc_probs_datasets with the kernel of a dataset's correlated noise chosen by `red_kernel` ("matern32", "ou2";
DESIGN.md section 14), end to end on the fixtures of tests/test_gpu_datasets.py: TOI-465.01, two cadences, N = 20 000,
set_sampling("device"), one seed for every pass.

Bars, none of them chosen from results:
  no key / red_kernel = "ou" / None: the same bits as without the key, and _lib.chi2_grid_ss2 is never called;
  "ou2" with tau_1 = tau_2 on dataset 1 against red_sigma = hypot(s_1, s_2) through chi2_grid_ou (the same covariance): the
        same masked counts; |d lnZ| <= the sum of the two kernels' bars on one draw's h, with the plain chi^2/2 of the
        pass's best draw in place of their sums as tests/test_gpu_datasets_red_noise.py does:
        1e-12 (1 + 1 / (1 - max alpha)) chi^2/2 + 1e-12 (tests/test_gpu_chi2_ou.py) plus 1e-12 (1 + Gamma) chi^2/2 + 1e-12
        (tests/test_gpu_chi2_ss2.py, Gamma the l1 gain of the dataset's predictor); the same best draw wherever the row's
        two smallest sums of h differ by more than that, and at most a quarter of the finite rows excused (a cap);
  a Matern-3/2 realisation added to dataset 1, the matching keys, against the CPU oracle's model grid reduced with
        _numerics.ss2_halfchi2: |d lnZ| <= 1e-9, the bar of the other oracle checks of this path;
  three chunks of the grid, calc_probs_datasets_refined(n_adapt = 0), and a one-node t0_grid (delta, 1) against
        time + delta (delta = 4 cadences): the same bits;
  evaluation = "fused": NotImplementedError.
Measured (one MI355X): cross-path the same lnZ in bits over 15 finite rows (1 + 1 / (1 - max alpha) = 2.858, 1 + Gamma = 1.909),
the same best draw in all 15, 1 row excused; against the oracle max |d lnZ| 1.2e-11.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_chi2_ss2 import gain
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import Datasets, ou_system, ss2_system, validate

pytestmark = pytest.mark.gpu

SIGMA_1 = Datasets(validate(_two_cadences()[1:])).sigma_ref        # sigma_bar of dataset 1 alone
CADENCE_1 = float(np.median(np.diff(_two_cadences()[1]["time"])))
COLS = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB")
S1, S2, TAU = 2.0 * SIGMA_1, 1.5 * SIGMA_1, 20.0 * CADENCE_1       # two exponential terms of one time scale ...
S_ONE = float(np.hypot(S1, S2))                                    # ... are one term of this amplitude


def _inputs(**keys):
    a, b = _two_cadences()
    return [a, dict(b, **keys)]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it and -- replay -- h with white noise (the same rows
    evaluated again with the plain reduction); and the calls of _lib.chi2_grid_ss2 and _lib.chi2_grid_ou"""

    def __init__(self, monkeypatch, replay):
        self.h, self.plain, self.ss2_calls, self.ou_calls = [], [], 0, 0
        real_h, real_z = fused._Scenario._datasets_halfchi2, _lib.lnz_from_halfchi2
        real_ss2, real_ou = _lib.chi2_grid_ss2, _lib.chi2_grid_ou
        spy = self

        def halfchi2(scen, model, flags, block):
            h = real_h(scen, model, flags, block)
            if replay:
                kept, scen.datasets = scen.datasets, [d._replace(term=None) for d in scen.datasets]
                try:
                    spy.plain.append(real_h(scen, model, flags, block).cpu().numpy())
                finally:
                    scen.datasets = kept
            return h

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def ss2(*a, **k):
            spy.ss2_calls += 1
            return real_ss2(*a, **k)

        def ou(*a, **k):
            spy.ou_calls += 1
            return real_ou(*a, **k)

        monkeypatch.setattr(fused._Scenario, "_datasets_halfchi2", halfchi2)
        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "chi2_grid_ss2", ss2)
        monkeypatch.setattr(_lib, "chi2_grid_ou", ou)


def _run(monkeypatch, datasets, replay=False, refined=False, **kw):
    tg = _target()
    s = _Spy(monkeypatch, replay)
    torch.manual_seed(SEED)
    _lib.reset_stats()
    if refined:
        tg.calc_probs_datasets_refined(datasets, LC["P_orb"], n_adapt=0, **dict(KW, **kw))
    else:
        tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(KW, **kw))
    rows = _lib.STATS["rows"]
    monkeypatch.undo()
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows // (2 if replay else 1),
            "best": np.stack([tg.probs[c].values for c in COLS]), "h": s.h, "plain": s.plain,
            "ss2_calls": s.ss2_calls, "ou_calls": s.ou_calls}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["ou"] = _run(monkeypatch, _inputs(red_sigma=S_ONE, red_timescale=TAU), replay=True)
        _runs["ou2"] = _run(monkeypatch, _inputs(red_kernel="ou2", red_sigma=(S1, S2), red_timescale=(TAU, TAU)), replay=True)
    return _runs


def _same_bits(a, b):
    return (a["lnZ"].tobytes() == b["lnZ"].tobytes() and a["prob"].tobytes() == b["prob"].tobytes()
            and a["best"].tobytes() == b["best"].tobytes() and a["rows"] == b["rows"] > 0)


def test_without_the_key_nothing_changes(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    assert np.isfinite(r["none"]["lnZ"]).sum() >= 10
    assert _same_bits(r["none"], _run(monkeypatch, _inputs(red_kernel=None)))
    assert _same_bits(r["none"], _run(monkeypatch, _inputs(red_kernel="ou")))
    named = _run(monkeypatch, _inputs(red_kernel="ou", red_sigma=S_ONE, red_timescale=TAU))
    assert _same_bits(r["ou"], named) and named["ou_calls"] == r["ou"]["ou_calls"] > 0
    assert r["none"]["ss2_calls"] == r["ou"]["ss2_calls"] == named["ss2_calls"] == 0
    assert r["ou2"]["ss2_calls"] > 0 and r["ou2"]["ou_calls"] == 0


def test_two_equal_time_scales_are_one_ou_term(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    u, s = r["ou"], r["ou2"]
    d_ou = validate(_inputs(red_sigma=S_ONE, red_timescale=TAU))[1]
    d_ss = validate(_inputs(red_kernel="ou2", red_sigma=(S1, S2), red_timescale=(TAU, TAU)))[1]
    A, g, _ = ss2_system(d_ss)
    # (alpha, A and g do not depend on the star's normalisation: Datasets.renorm)
    amp_ou, amp_ss = 1.0 + 1.0 / (1.0 - ou_system(d_ou)[0].max()), 1.0 + gain(A, g)
    assert len(s["h"]) == len(u["h"]) == len(s["plain"]) == s["lnZ"].size
    assert u["rows"] == s["rows"] == r["none"]["rows"] > 0, "masked counts differ"
    fin = np.isfinite(u["lnZ"])
    assert np.array_equal(fin, np.isfinite(s["lnZ"])) and fin.sum() >= 10
    n_sep = n_same = 0
    worst = 0.0
    for j in np.flatnonzero(fin):
        h = s["h"][j]
        best = int(np.argmin(h))
        bar = 1e-12 * (amp_ou + amp_ss) * s["plain"][j][best] + 2e-12
        d = abs(u["lnZ"][j] - s["lnZ"][j])
        worst = max(worst, d / bar)
        assert d <= bar, (j, d, bar)
        two = np.partition(h, 1)[:2] if h.size > 1 else np.array([h[0], np.inf])
        same = np.array_equal(u["best"][:, j], s["best"][:, j])
        if two[1] - two[0] > bar:
            n_sep += 1
            assert same, "row %d: best draws differ although the two smallest h are %g apart" % (j, two[1] - two[0])
        n_same += same
    print("ou2 with equal time scales against red_sigma = hypot: 1 + 1 / (1 - max alpha) = %.4g, 1 + Gamma = %.4g, max "
          "|d lnZ| / bar %.3g over %d finite rows; two smallest h further apart than the bar in %d rows, the same best draw "
          "in %d" % (amp_ou, amp_ss, worst, fin.sum(), n_sep, n_same))
    assert fin.sum() - n_sep <= 0.25 * fin.sum()
    # the keys change the evidence: the point of the feature
    assert np.abs(s["lnZ"][fin] - r["none"]["lnZ"][fin]).max() > 1e-3


def _matern_inputs():
    """dataset 1 with a Matern-3/2 realisation added (s = 2 sigma of dataset 1, l = 20 cadences; a fixed seed: the Cholesky
    factor of the kernel matrix on its stamps times unit normals) and its keys"""
    a, b = _two_cadences()
    s, ell = 2.0 * SIGMA_1, 20.0 * CADENCE_1
    t = b["time"]
    x = np.sqrt(3.0) * np.abs(t[:, None] - t[None, :]) / ell
    K = s * s * (1.0 + x) * np.exp(-x)
    wiggle = np.linalg.cholesky(K + 1e-12 * s * s * np.eye(t.size)) @ np.random.default_rng(465).normal(size=t.size)
    return [a, dict(b, flux=b["flux"] + wiggle, red_kernel="matern32", red_sigma=s, red_timescale=ell)]


def test_chunks_refined_shift_node_and_fused_refusal(device_mode, monkeypatch):
    data = _matern_inputs()
    whole = _run(monkeypatch, data)
    assert whole["ss2_calls"] > 0 and whole["ou_calls"] == 0 and np.isfinite(whole["lnZ"]).sum() >= 10
    fin = np.isfinite(whole["lnZ"])
    assert np.abs(whole["lnZ"][fin] - _run(monkeypatch, data[:1] + [dict(data[1], red_kernel="ou")])["lnZ"][fin]).max() > 1e-3
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["ss2_calls"] >= 3 * sum(h.size >= 3 for h in whole["h"]) and chunked["ss2_calls"] > whole["ss2_calls"]
    assert _same_bits(whole, chunked)
    assert _same_bits(whole, _run(monkeypatch, data, refined=True))
    # a one-node t0_grid (delta, 1) is the stamps time + delta (delta = 4 cadences, as tests/test_gpu_datasets_t0_grid.py:
    # the differences of the shifted stamps keep their bits, so the noise tables of the two inputs are the same)
    delta = 4.0 * CADENCE_1
    moved = dict(data[1], time=data[1]["time"] + delta)
    for u, v in zip(ss2_system(validate([moved])[0]), ss2_system(validate([data[1]])[0])):
        assert u.tobytes() == v.tobytes()
    a = _run(monkeypatch, [data[0], moved])
    b = _run(monkeypatch, [data[0], dict(data[1], t0_grid=[(delta, 1.0)])])
    assert _same_bits(a, b) and not _same_bits(a, whole)
    tg = _target()
    with pytest.raises(NotImplementedError):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_matern_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x, a Matern-3/2 realisation and its keys on
    dataset 1: the model curves from the oracle, the two-state recurrence and the evidence in numpy."""
    data = _matern_inputs()
    kw = dict(KW, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
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
                if s.red_kernel is None:
                    h += 0.5 * np.sum(r * r / s.flux_err ** 2, axis=1)
                else:
                    h += _numerics.ss2_halfchi2(r, *ss2_system(s))
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
    assert ds.sets[0].red_kernel is None and ds.sets[1].red_kernel == "matern32"
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and np.isfinite(want).sum() >= 2
    fin = np.isfinite(want)
    print("matern32 dataset against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
